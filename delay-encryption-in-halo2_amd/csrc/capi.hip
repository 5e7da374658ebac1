// capi.hip -- C ABI (include/dehalo.h) over the gfx950 kernels.  Host logic only: argument
// checks, HBM workspace, dispatch to the per-curve / per-field translation units
// (msm_*.hip, ntt_*.hip), HIP-event timing.  No CPU arithmetic path exists here: every field
// or group operation runs on the device, and context creation fails without one.
#include <algorithm>
#include <atomic>
#include <initializer_list>

#include <map>
#include <memory>

#include "evalh_types.hpp"
#include "hostfield.hpp"
#include "internal.hpp"
#include "msm_plan.hpp"      // the window rules: choose_window, choose_window_single, signed_windows, msm_table_fits

namespace {

// the op tables of the per-field / per-curve translation units (ntt_*.hip, msm_*.hip) by dehalo_field / dehalo_curve id; null for an unknown id
const FieldOps* field_ops(int field) {
    static const FieldOps* const ops[] = {&bn254_fr_field_ops(), &bn254_fq_field_ops(), &pasta_fp_field_ops(), &pasta_fq_field_ops()};
    static_assert(DEHALO_FIELD_BN254_FR == 0 && DEHALO_FIELD_BN254_FQ == 1 && DEHALO_FIELD_PASTA_FP == 2 && DEHALO_FIELD_PASTA_FQ == 3, "field ids");
    return field >= 0 && field < 4 ? ops[field] : nullptr;
}
const CurveOps* curve_ops(int curve) {
    static const CurveOps* const ops[] = {&bn254_curve_ops(), &pallas_curve_ops(), &vesta_curve_ops()};
    static_assert(DEHALO_CURVE_BN254_G1 == 0 && DEHALO_CURVE_PALLAS == 1 && DEHALO_CURVE_VESTA == 2, "curve ids");
    return curve >= 0 && curve < 3 ? ops[curve] : nullptr;
}
int unknown_field(dehalo_ctx* ctx) { return dh_fail(ctx, DEHALO_ERR_INVALID, "unknown field id"); }
int unknown_curve(dehalo_ctx* ctx) { return dh_fail(ctx, DEHALO_ERR_INVALID, "unknown curve id"); }

// Host-side compilation of upstream's GraphEvaluator into the device program: sources are
// resolved to table indices, and every intermediate gets a slot from a liveness scan (a slot is
// reused as soon as its value has been read for the last time; the first EVH_MAX_LDS_SLOTS slots
// live in LDS, the rest in an HBM scratch column).
int compile_graph(dehalo_ctx* ctx, dehalo_graph* g, const int32_t* rotations, uint32_t num_rotations, const dehalo_calculation* calcs, uint32_t num_calcs,
                  const dehalo_source* parts, uint32_t num_parts, uint32_t num_intermediates, std::vector<DevCalc>& out_calcs, std::vector<DevSrc>& out_parts,
                  bool propagate = true, const uint32_t* root_of = nullptr, std::vector<uint32_t>* out_root_of = nullptr) {
    // root_of (a checking program, dh_graph_create_roots): per calculation the root it is, or NEVER.  Such a calculation survives the copy
    // propagation, and out_root_of says where it went.
    const uint32_t NEVER = 0xffffffffu;
    if (propagate) {
        // Copy propagation.  Upstream's GraphEvaluator::add_expression wraps EVERY column query in Calculation::Store(source) so that its
        // CPU loop loads a cell once; on the device a Store is a calculation of its own (fetch, slot write) and every later use a slot
        // read, while reading the column directly costs the same fetch.  A Store of a non-intermediate source whose target is written
        // exactly once is therefore dropped and its uses read the source (MainGate's gate: 34 calculations / 7 slots -> 20 / 3; fewer
        // slots is more resident waves: the kernel's occupancy is bounded by its LDS slots).  The original program is validated first.
        {
            std::vector<DevCalc> tc;
            std::vector<DevSrc> tp;
            dehalo_graph probe{};      // (the validation reads the number of constants only)
            probe.num_constants = g->num_constants;
            TRY(compile_graph(ctx, &probe, rotations, num_rotations, calcs, num_calcs, parts, num_parts, num_intermediates, tc, tp, false));
        }
        std::vector<uint32_t> defs(num_intermediates, 0);
        for (uint32_t i = 0; i < num_calcs; i++) defs[calcs[i].target]++;
        std::vector<int> aliased(num_intermediates, 0);
        std::vector<dehalo_source> alias(num_intermediates);
        std::vector<dehalo_calculation> cc;
        std::vector<uint32_t> cc_root;
        std::vector<dehalo_source> pp(parts, parts + num_parts);
        auto sub = [&](dehalo_source s) { return (s.kind == DEHALO_SRC_INTERMEDIATE && aliased[s.index]) ? alias[s.index] : s; };
        for (uint32_t i = 0; i < num_calcs; i++) {
            dehalo_calculation c = calcs[i];
            c.a = sub(c.a);
            c.b = sub(c.b);
            if (c.op == DEHALO_CALC_HORNER)
                for (uint32_t k = 0; k < c.parts_len; k++) pp[c.parts_begin + k] = sub(pp[c.parts_begin + k]);
            const bool is_root = root_of && root_of[i] != NEVER;
            if (!is_root && c.op == DEHALO_CALC_STORE && c.a.kind != DEHALO_SRC_INTERMEDIATE && i + 1 != num_calcs && defs[c.target] == 1) {
                aliased[c.target] = 1;
                alias[c.target] = c.a;
                continue;
            }
            cc.push_back(c);
            if (root_of) cc_root.push_back(root_of[i]);
        }
        g->num_calcs = (uint32_t)cc.size();
        if (out_root_of) *out_root_of = cc_root;
        return compile_graph(ctx, g, rotations, num_rotations, cc.data(), (uint32_t)cc.size(), pp.data(), num_parts, num_intermediates, out_calcs, out_parts, false);
    }
    std::vector<uint32_t> last_use(num_intermediates, NEVER), first_def(num_intermediates, NEVER);
    auto check_src = [&](const dehalo_source& src, uint32_t at) -> int {
        switch (src.kind) {
            case DEHALO_SRC_CONSTANT: if (src.index >= g->num_constants) return dh_fail(ctx, DEHALO_ERR_INVALID, "graph: constant index out of range"); break;
            case DEHALO_SRC_INTERMEDIATE:
                if (src.index >= num_intermediates) return dh_fail(ctx, DEHALO_ERR_INVALID, "graph: intermediate index out of range");
                if (first_def[src.index] == NEVER || first_def[src.index] >= at) return dh_fail(ctx, DEHALO_ERR_INVALID, "graph: intermediate read before it is written");
                last_use[src.index] = at;
                break;
            case DEHALO_SRC_FIXED: case DEHALO_SRC_ADVICE: case DEHALO_SRC_INSTANCE:
                if (src.rotation >= num_rotations) return dh_fail(ctx, DEHALO_ERR_INVALID, "graph: rotation index out of range");
                break;
            case DEHALO_SRC_CHALLENGE: case DEHALO_SRC_BETA: case DEHALO_SRC_GAMMA: case DEHALO_SRC_THETA: case DEHALO_SRC_Y: case DEHALO_SRC_PREVIOUS: break;
            default: return dh_fail(ctx, DEHALO_ERR_INVALID, "graph: unknown value source kind");
        }
        return 0;
    };
    auto binary = [](uint32_t op) { return op == DEHALO_CALC_ADD || op == DEHALO_CALC_SUB || op == DEHALO_CALC_MUL || op == DEHALO_CALC_HORNER; };
    // pass 1: validation, definitions and last uses
    for (uint32_t i = 0; i < num_calcs; i++) {
        const dehalo_calculation& c = calcs[i];
        if (c.op > DEHALO_CALC_STORE) return dh_fail(ctx, DEHALO_ERR_INVALID, "graph: unknown calculation");
        if (c.target >= num_intermediates) return dh_fail(ctx, DEHALO_ERR_INVALID, "graph: target out of range");
        TRY(check_src(c.a, i));
        if (binary(c.op)) TRY(check_src(c.b, i));
        if (c.op == DEHALO_CALC_HORNER) {
            if ((uint64_t)c.parts_begin + c.parts_len > num_parts) return dh_fail(ctx, DEHALO_ERR_INVALID, "graph: horner parts out of range");
            for (uint32_t k = 0; k < c.parts_len; k++) TRY(check_src(parts[c.parts_begin + k], i));
        }
        if (first_def[c.target] == NEVER) first_def[c.target] = i;
    }
    if (num_calcs) last_use[calcs[num_calcs - 1].target] = num_calcs;   // the result stays live to the end
    // pass 2: slots
    std::vector<uint32_t> slot_of(num_intermediates, NEVER), free_slots;
    uint32_t next_slot = 0;
    auto conv = [&](const dehalo_source& src) {
        DevSrc d{EVS_SCALAR, 0, 0};
        switch (src.kind) {
            case DEHALO_SRC_BETA: d.index = 0; break;
            case DEHALO_SRC_GAMMA: d.index = 1; break;
            case DEHALO_SRC_THETA: d.index = 2; break;
            case DEHALO_SRC_Y: d.index = 3; break;
            case DEHALO_SRC_CONSTANT: d.index = 4 + src.index; break;
            case DEHALO_SRC_CHALLENGE: d.index = 4 + g->num_constants + src.index; g->max_challenge = std::max(g->max_challenge, src.index + 1); break;
            case DEHALO_SRC_INTERMEDIATE: {
                uint32_t sl = slot_of[src.index];
                d.kind = sl < EVH_MAX_LDS_SLOTS ? EVS_SLOT_LDS : EVS_SLOT_HBM;
                d.index = sl < EVH_MAX_LDS_SLOTS ? sl : sl - EVH_MAX_LDS_SLOTS;
            } break;
            case DEHALO_SRC_FIXED: d.kind = EVS_FIXED; d.index = src.index; d.rot = rotations[src.rotation]; g->max_fixed = std::max(g->max_fixed, src.index + 1); break;
            case DEHALO_SRC_ADVICE: d.kind = EVS_ADVICE; d.index = src.index; d.rot = rotations[src.rotation]; g->max_advice = std::max(g->max_advice, src.index + 1); break;
            case DEHALO_SRC_INSTANCE: d.kind = EVS_INSTANCE; d.index = src.index; d.rot = rotations[src.rotation]; g->max_instance = std::max(g->max_instance, src.index + 1); break;
            default: d.kind = EVS_PREVIOUS; g->uses_previous = true; break;
        }
        return d;
    };
    std::vector<std::vector<uint32_t>> dying(num_calcs + 1);
    for (uint32_t v = 0; v < num_intermediates; v++)
        if (last_use[v] != NEVER) dying[last_use[v]].push_back(v);
    out_calcs.resize(num_calcs);
    out_parts.resize(num_parts ? num_parts : 1);
    for (uint32_t i = 0; i < num_calcs; i++) {
        const dehalo_calculation& c = calcs[i];
        DevCalc d{};
        d.op = c.op;
        d.a = conv(c.a);
        if (binary(c.op)) d.b = conv(c.b);
        d.parts_begin = c.parts_begin; d.parts_len = c.op == DEHALO_CALC_HORNER ? c.parts_len : 0;
        for (uint32_t k = 0; k < d.parts_len; k++) out_parts[c.parts_begin + k] = conv(parts[c.parts_begin + k]);
        // operands are all read before the result is written: slots whose last use is this calculation are free for its target
        for (uint32_t v : dying[i])
            if (slot_of[v] != NEVER && v != c.target) { free_slots.push_back(slot_of[v]); slot_of[v] = NEVER; }
        if (slot_of[c.target] == NEVER) {
            if (!free_slots.empty()) {
                auto it = std::min_element(free_slots.begin(), free_slots.end());   // lowest slot first: LDS before HBM
                slot_of[c.target] = *it;
                free_slots.erase(it);
            } else slot_of[c.target] = next_slot++;
        }
        uint32_t sl = slot_of[c.target];
        d.target_kind = sl < EVH_MAX_LDS_SLOTS ? EVS_SLOT_LDS : EVS_SLOT_HBM;
        d.target_slot = sl < EVH_MAX_LDS_SLOTS ? sl : sl - EVH_MAX_LDS_SLOTS;
        if (last_use[c.target] == NEVER || last_use[c.target] <= i) { /* dead value: its slot is released at once */
            if (!(i + 1 == num_calcs)) { free_slots.push_back(sl); slot_of[c.target] = NEVER; }
        }
        out_calcs[i] = d;
    }
    g->lds_slots = std::min<uint32_t>(next_slot, EVH_MAX_LDS_SLOTS);
    g->hbm_slots = next_slot > EVH_MAX_LDS_SLOTS ? next_slot - EVH_MAX_LDS_SLOTS : 0;
    if (num_calcs) {
        dehalo_source r{DEHALO_SRC_INTERMEDIATE, calcs[num_calcs - 1].target, 0};
        g->result = conv(r);
    }
    return 0;
}

// The host-buffer forms: under the context's lock, each input is uploaded into its workspace buffer (a null host pointer only sizes the buffer),
// dev() runs the device form on the workspace copies, and the output is downloaded from out_buf, synchronously.  Every caller names the buffers it
// has always used: the device form it calls may use some of the others itself.
struct HostIn { DevBuf& buf; const void* p; size_t bytes; };
template <class Dev>
int with_host_io(dehalo_ctx* ctx, std::initializer_list<HostIn> ins, DevBuf& out_buf, void* out, size_t out_bytes, Dev&& dev) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    for (const HostIn& in : ins) TRY(dh_ensure(ctx, in.buf, std::max<size_t>(32, in.bytes)));
    TRY(dh_ensure(ctx, out_buf, std::max<size_t>(32, out_bytes)));
    for (const HostIn& in : ins)
        if (in.p) TRY(dh_h2d(ctx, in.buf.p, in.p, in.bytes, ctx->stream.get()));
    TRY(dev());
    TRY(dh_d2h(ctx, out, out_buf.p, out_bytes, ctx->stream.get()));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
    return 0;
}

// a device-form entry point over one field / curve: dh_device (internal.hpp) with its op table, "unknown field id" / "unknown curve id" without one
template <class Body>
int field_device(dehalo_ctx* ctx, int field, void* stream, Body&& body) {
    return dh_device(ctx, stream, [&](hipStream_t s) {
        const FieldOps* f = field_ops(field);
        return f ? body(*f, s) : unknown_field(ctx);
    });
}
template <class Body>
int curve_device(dehalo_ctx* ctx, int curve, void* stream, Body&& body) {
    return dh_device(ctx, stream, [&](hipStream_t s) {
        const CurveOps* cv = curve_ops(curve);
        return cv ? body(*cv, s) : unknown_curve(ctx);
    });
}

// the NTT family's host-buffer forms: ws_ntt_io in, ws_ntt_io2 out unless in place; dev(d_in, d_out)
template <class Dev>
int ntt_host_io(dehalo_ctx* ctx, const uint64_t* in, size_t in_elems, uint64_t* out, size_t out_elems, bool inplace, Dev&& dev) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!in || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "null buffer");
    return dh_guard(ctx, [&] {
        HostPin pin_in(in, in_elems * 32), pin_out(out == in ? nullptr : out, out_elems * 32);
        DevBuf& d_in = ctx->ws_ntt_io;
        DevBuf& d_out = inplace ? ctx->ws_ntt_io : ctx->ws_ntt_io2;
        return with_host_io(ctx, {{d_in, in, in_elems * 32}}, d_out, out, out_elems * 32, [&] { return dev((uint64_t*)d_in.p, (uint64_t*)d_out.p); });
    });
}

int register_impl(dehalo_ctx* ctx, int curve, const uint64_t* affine_xy, size_t n, size_t stride_bytes, int window_bits, int precompute,
                  BasesPtr& out, bool on_device) {
    if (!affine_xy || n == 0 || stride_bytes < 64 || n >= (1ull << 30)) return dh_fail(ctx, DEHALO_ERR_INVALID, "bases_register: bad argument");
    if (window_bits != 0 && (window_bits < (int)MSM_WINDOW_MIN || window_bits > (int)msm_window_max(precompute != 0)))
        return dh_fail(ctx, DEHALO_ERR_INVALID, "window_bits must be 0 or in [4, 16] (17 with precomputed rows)");
    const CurveOps* cv = curve_ops(curve);
    if (!cv) return unknown_curve(ctx);
    uint32_t c = window_bits ? (uint32_t)window_bits : (precompute ? choose_window(n) : choose_window_single(n));
    if (!window_bits && precompute) {      // DEHALO_WINDOW_BITS: tuning experiments (results never depend on the window)
        const char* e = DH_EXPERIMENT_ENV("DEHALO_WINDOW_BITS");
        if (e && atoi(e) >= (int)MSM_WINDOW_MIN && atoi(e) <= (int)msm_window_max(true)) c = (uint32_t)atoi(e);
    }
    c = std::max<uint32_t>(MSM_WINDOW_MIN, c);
    uint32_t W = signed_windows(cv->scalar_modulus, c);
    if (precompute && !msm_table_fits(n, W)) return dh_fail(ctx, DEHALO_ERR_INVALID, "precomputed table too large");      // 30-bit table indices in the sorted list (msm.cuh)
    // stage the caller's points (standard Montgomery form) on the device, then build the table
    if (!on_device) TRY(dh_ensure(ctx, ctx->ws_tmp_bases, n * sizeof(affine_t)));
    BasesPtr b(new dehalo_bases(), BasesFree{ctx});
    b->curve = curve; b->n = n; b->c = c; b->W = W; b->precomp = precompute ? 1 : 0;
    size_t rows = precompute ? W : 1;
    TRY(b->table.alloc(ctx, rows * n, false));
    // 64 MiB of SRS points at 2^20: DMA straight from the caller's pages -- only when these bytes are what is copied (host memory, contiguous points)
    HostPin pin_bases(on_device || stride_bytes != 64 ? nullptr : affine_xy, n * stride_bytes);
    // (contiguous points: a plain copy -- the 2-D path took 3 of the 4.1 ms of registering 2^20 points)
    std::vector<uint64_t> packed;      // (points with a trailing flag byte: gathered on the host, so that the upload is one contiguous copy)
    if (stride_bytes != 64 && !on_device) {
        packed.resize(n * 8);
        for (size_t i = 0; i < n; i++) memcpy(&packed[i * 8], (const char*)affine_xy + i * stride_bytes, 64);
    }
    if (!on_device) TRY(dh_h2d(ctx, ctx->ws_tmp_bases.p, stride_bytes == 64 ? (const void*)affine_xy : (const void*)packed.data(), n * 64, ctx->stream.get()));
    TRY(cv->build_table(ctx, b.get(), on_device ? (const affine_t*)affine_xy : (const affine_t*)ctx->ws_tmp_bases.p, ctx->stream.get()));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
    out = std::move(b);
    return 0;
}

// dehalo_bases_register / dehalo_bases_register_device: register_impl under the guard, the context's lock and its device; the handle crosses the ABI on success only
int register_entry(dehalo_ctx* ctx, int curve, const uint64_t* affine_xy, size_t n, size_t stride_bytes, int window_bits, int precompute, dehalo_bases** out,
                   bool on_device) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!curve_ops(curve)) return unknown_curve(ctx);
    if (!out) return dh_fail(ctx, DEHALO_ERR_INVALID, "bases_register: bad argument");
    return dh_guard(ctx, [&]() -> int {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        BasesPtr b;
        TRY(register_impl(ctx, curve, affine_xy, n, stride_bytes, window_bits, precompute, b, on_device));
        *out = b.release();
        return 0;
    });
}

}  // namespace

// ---- the point codec (gfft.cuh): GroupEncoding::to_bytes / from_bytes and the checked from_raw_bytes over vectors of points ----
namespace {
// the argument checks the three calls share; ops stays null when the call has nothing to launch (count = 0)
int points_codec_args(dehalo_ctx* ctx, const char* who, int curve, const void* d_affine, const void* d_bytes32, size_t count, const GfftOps** ops) {
    *ops = nullptr;
    const GfftOps* o = gfft_ops(curve);
    if (!o) return unknown_curve(ctx);
    if (count >= ((size_t)1 << 29)) return dh_fail(ctx, DEHALO_ERR_INVALID, std::string(who) + ": too many points");
    if (count == 0) return 0;
    if (!d_affine || ((uintptr_t)d_affine & 15)) return dh_fail(ctx, DEHALO_ERR_INVALID, std::string(who) + ": the points are null or not 16-byte aligned");
    if (d_bytes32 && ((uintptr_t)d_bytes32 & 3)) return dh_fail(ctx, DEHALO_ERR_INVALID, std::string(who) + ": the encodings are not 4-byte aligned");
    *ops = o;
    return 0;
}
// zero the context's status word on s, run `launch` with it, bring it to the host: the one host wait of a call that reports a status
template <class Launch>
int points_status(dehalo_ctx* ctx, uint32_t* status_out, hipStream_t s, Launch&& launch) {
    TRY(dh_ensure(ctx, ctx->ws_codec, 16));
    uint32_t* d_status = (uint32_t*)ctx->ws_codec.p;
    HIP_TRY(ctx, hipMemsetAsync(d_status, 0, 4, s));
    TRY(launch(d_status));
    return dh_d2h(ctx, status_out, d_status, 4, s);
}
// ---- the scalar codec's host half (scalar_codec.cuh) ----
// The context's codec words: status (u32) at byte 0, the lowest offending index (u64) at byte 8.  Both are reset on s (status 0, index all ones), `launch` runs
// with them, and one download brings them to the host: the one host wait of the call.  An index still all ones means no element was reported: count.
template <class Launch>
int scalars_status(dehalo_ctx* ctx, size_t count, uint32_t* status_out, uint64_t* first_bad_out, hipStream_t s, Launch&& launch) {
    TRY(dh_ensure(ctx, ctx->ws_codec, 16));
    uint8_t* d = (uint8_t*)ctx->ws_codec.p;
    HIP_TRY(ctx, hipMemsetAsync(d, 0, 8, s));
    HIP_TRY(ctx, hipMemsetAsync(d + 8, 0xff, 8, s));
    TRY(launch((uint32_t*)d, (uint64_t*)(d + 8)));
    uint64_t h[2] = {0, 0};
    TRY(dh_d2h(ctx, h, d, 16, s));
    *status_out = (uint32_t)h[0];
    *first_bad_out = h[1] == ~(uint64_t)0 ? (uint64_t)count : h[1];
    return 0;
}
int scalars_codec_args(dehalo_ctx* ctx, const char* who, int field, const void* d_words, size_t count, uint32_t* status_out, uint64_t* first_bad_out) {
    if (!field_ops(field)) return unknown_field(ctx);
    if (count >= ((size_t)1 << 29)) return dh_fail(ctx, DEHALO_ERR_INVALID, std::string(who) + ": too many elements");
    if (!status_out || !first_bad_out) return dh_fail(ctx, DEHALO_ERR_INVALID, std::string(who) + ": null status");
    *status_out = 0;
    *first_bad_out = 0;
    if (count && (!d_words || ((uintptr_t)d_words & 15))) return dh_fail(ctx, DEHALO_ERR_INVALID, std::string(who) + ": the elements are null or not 16-byte aligned");
    return 0;
}
}   // namespace

const IpaOps* ipa_ops(int curve) {
    if (curve == DEHALO_CURVE_PALLAS) return &pallas_ipa_ops();
    if (curve == DEHALO_CURVE_VESTA) return &vesta_ipa_ops();
    return nullptr;
}

const FieldOps* dh_field_ops(int field) { return field_ops(field); }

const GfftOps* gfft_ops(int curve) {
    static const GfftOps* const ops[] = {&bn254_gfft_ops(), &pallas_gfft_ops(), &vesta_gfft_ops()};
    return curve >= 0 && curve < 3 ? ops[curve] : nullptr;
}

int dh_bases_plain_alloc(dehalo_ctx* ctx, int curve, size_t cap, BasesPtr& out) {
    if (!curve_ops(curve) || cap == 0 || cap >= (1ull << 30)) return dh_fail(ctx, DEHALO_ERR_INVALID, "bases_plain_alloc: bad argument");
    BasesPtr b(new dehalo_bases(), BasesFree{ctx});
    b->curve = curve; b->n = 0; b->c = 4; b->W = 0; b->precomp = 0;
    TRY(b->table.alloc(ctx, cap, false));
    out = std::move(b);
    return 0;
}

int dh_bases_plain_rebuild(dehalo_ctx* ctx, dehalo_bases* b, const affine_t* d_points, size_t n, hipStream_t s) {
    const CurveOps* cv = curve_ops(b->curve);
    b->n = n;
    b->c = std::max<uint32_t>(MSM_WINDOW_MIN, choose_window_single(n));
    b->W = signed_windows(cv->scalar_modulus, b->c);
    return cv->build_table(ctx, b, d_points, s);
}

// the limit of a precomputed table registered with window_bits = 0: n x windows < 2^30 (30-bit table indices in the sorted list, msm.cuh)
bool dh_precomputed_table_fits(int curve, size_t n) {
    const CurveOps* cv = curve_ops(curve);
    return cv && msm_table_fits(n, signed_windows(cv->scalar_modulus, std::max<uint32_t>(MSM_WINDOW_MIN, choose_window(n))));
}

// ==========================================================================================
extern "C" {

const char* dehalo_version(void) { return "dehalo 0.2 gfx950"; }

int dehalo_ctx_create(int device, dehalo_ctx** out) { return dehalo_ctx_create_with_priority(device, 0, out); }

int dehalo_ctx_create_with_priority(int device, int priority, dehalo_ctx** out) {
    if (!out) return DEHALO_ERR_INVALID;
    *out = nullptr;
    return dh_guard(nullptr, [&]() -> int {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return DEHALO_ERR_NO_DEVICE;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) return DEHALO_ERR_NO_DEVICE;
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return DEHALO_ERR_NO_DEVICE;  // code objects are gfx950-only
        if (hipSetDevice(device) != hipSuccess) return DEHALO_ERR_NO_DEVICE;
        std::unique_ptr<dehalo_ctx> ctx(new dehalo_ctx());
        ctx->device = device;
        ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        {   // priority > 0: the device's highest stream priority (a context of small kernels beside another context's long ones), < 0: lowest
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            const int prio = priority > 0 ? greatest : (priority < 0 ? least : 0);
            // Experiment (DEHALO_CU_PARTITION = P, measurements only): the i-th context created by this process gets a stream that may only use the (i mod P)-th
            // P-th of the compute units (hipExtStreamCreateWithCUMask), so that the provers of a batch do not wait for each other's workgroups to leave a CU.
            static const int cu_parts = [] { const char* e = DH_EXPERIMENT_ENV("DEHALO_CU_PARTITION"); return e ? atoi(e) : 0; }();
            static std::atomic<int> cu_next{0};
            hipError_t e;
            hipStream_t st = nullptr;
            if (cu_parts > 1 && cu_parts <= 16) {
                const int part = cu_next.fetch_add(1) % cu_parts, ncu = ctx->num_cus, per = ncu / cu_parts;
                std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
                static const bool interleave = DH_EXPERIMENT_ENV("DEHALO_CU_PARTITION_INTERLEAVE") != nullptr;
                for (int cu = 0; cu < ncu; cu++) {
                    const bool mine = interleave ? (cu % cu_parts) == part : (cu / per) == part;
                    if (mine) mask[cu / 32] |= 1u << (cu % 32);
                }
                e = hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data());
                if (e == hipSuccess) ctx->num_cus = per;
            } else
            e = priority == 0 ? hipStreamCreateWithFlags(&st, hipStreamNonBlocking)
                              : hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio);
            if (e != hipSuccess) return DEHALO_ERR_HIP;
            ctx->stream.reset(st);
        }
        if (const char* e = DH_EXPERIMENT_ENV("DEHALO_MSM_ACC_MIN_LAYERS")) ctx->msm_acc_min_layers = std::max(1, std::min(4, atoi(e)));
        if (const char* e = DH_EXPERIMENT_ENV("DEHALO_HOST_SPIN_US")) ctx->host_wait_spin_us = std::max(0, std::min(1000000, atoi(e)));
        if (const char* e = DH_EXPERIMENT_ENV("DEHALO_MSM_ACC_BLOCK")) ctx->msm_acc_block = atoi(e) == 768 ? 768 : 128;                                      // launch geometry only
        if (const char* e = DH_EXPERIMENT_ENV("DEHALO_MSM_ACC_POINTS")) ctx->msm_acc_points = std::max(0, std::min(4096, atoi(e)));   // launch geometry only (dehalo_ctx_set_tuning)
        *out = ctx.release();
        return 0;
    });
}

void dehalo_ctx_destroy(dehalo_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    // (the context's members free what they hold, in reverse order of declaration: the stream goes last)
    delete ctx;
}

const char* dehalo_last_error(const dehalo_ctx* ctx) {
    if (!ctx) return "null context";
    // a copy per calling thread, taken under the lock: another thread's error path may replace ctx->err at any time
    static thread_local std::string copy;
    try {
        std::lock_guard<std::mutex> lk(const_cast<dehalo_ctx*>(ctx)->err_mu);
        copy = ctx->err;
    } catch (...) {
        return "out of host memory copying the last error";
    }
    return copy.c_str();
}

int dehalo_ctx_set_tuning(dehalo_ctx* ctx, const char* key, int value) {
    if (!ctx || !key) return DEHALO_ERR_INVALID;
    return dh_guard(ctx, [&]() -> int {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        if (!strcmp(key, "msm_acc_points")) {
            if (value < 0 || value > 4096) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm_acc_points must be in [0, 4096]");
            ctx->msm_acc_points = value;
            return 0;
        }
        if (!strcmp(key, "msm_acc_waves")) {
            if (value < 1 || value > 4) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm_acc_waves must be in [1, 4]");
            ctx->msm_acc_waves = value;
            return 0;
        }
        if (!strcmp(key, "host_wait_spin_us")) {
            if (value < 0 || value > 1000000) return dh_fail(ctx, DEHALO_ERR_INVALID, "host_wait_spin_us must be in [0, 1000000]");
            ctx->host_wait_spin_us = value;
            return 0;
        }
        if (!strcmp(key, "msm_sort_block")) {
            if (value != 512 && value != 1024) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm_sort_block must be 512 or 1024");
            ctx->msm_sort_block = value;
            return 0;
        }
        if (!strcmp(key, "msm_acc_block")) {
            if (value != 128 && value != 768) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm_acc_block must be 128 or 768");
            ctx->msm_acc_block = value;
            return 0;
        }
        if (!strcmp(key, "ntt_full_table_log")) {
            if (value < 0 || value > 30) return dh_fail(ctx, DEHALO_ERR_INVALID, "ntt_full_table_log must be in [0, 30]");
            ctx->ntt_full_table_log = value;
            return 0;
        }
        return dh_fail(ctx, DEHALO_ERR_INVALID, std::string("unknown tuning key: ") + key);
    });
}

void* dehalo_ctx_stream(dehalo_ctx* ctx) { return ctx ? (void*)ctx->stream.get() : nullptr; }

int dehalo_ctx_synchronize(dehalo_ctx* ctx) {
    if (!ctx) return DEHALO_ERR_INVALID;
    return dh_guard(ctx, [&]() -> int {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
        return 0;
    });
}

int dehalo_download(dehalo_ctx* ctx, const void* d_src, size_t bytes, void* host_dst) {
    if (!ctx) return DEHALO_ERR_INVALID;
    return dh_guard(ctx, [&]() -> int {
        if ((!d_src || !host_dst) && bytes) return dh_fail(ctx, DEHALO_ERR_INVALID, "download: null argument");
        (void)hipSetDevice(ctx->device);
        if (bytes) TRY(dh_d2h(ctx, host_dst, d_src, bytes, ctx->stream.get()));
        HIP_TRY(ctx, dh_stream_wait(ctx, ctx->stream.get()));
        return 0;
    });
}

int dehalo_upload(dehalo_ctx* ctx, const void* host_src, size_t bytes, void* d_dst) {
    if (!ctx) return DEHALO_ERR_INVALID;
    return dh_guard(ctx, [&]() -> int {
        if ((!host_src || !d_dst) && bytes) return dh_fail(ctx, DEHALO_ERR_INVALID, "upload: null argument");
        (void)hipSetDevice(ctx->device);
        {
            HostPin pin(host_src, bytes);      // 4 MiB and more: one DMA from the caller's pages, released below, after the stream has drained
            TRY(dh_h2d(ctx, d_dst, host_src, bytes, ctx->stream.get()));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
        }
        return 0;
    });
}

int dehalo_bases_register(dehalo_ctx* ctx, int curve, const uint64_t* affine_xy, size_t n, size_t stride_bytes, int window_bits, int precompute,
                          dehalo_bases** out) {
    return register_entry(ctx, curve, affine_xy, n, stride_bytes, window_bits, precompute, out, false);
}

int dehalo_bases_register_device(dehalo_ctx* ctx, int curve, const uint64_t* d_affine_xy, size_t n, int window_bits, int precompute, dehalo_bases** out) {
    return register_entry(ctx, curve, d_affine_xy, n, 64, window_bits, precompute, out, true);
}

int dehalo_bases_release(dehalo_ctx* ctx, dehalo_bases* bases) {
    if (!ctx || !bases) return DEHALO_ERR_INVALID;
    return dh_guard(ctx, [&] {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        (void)hipDeviceSynchronize();
        delete bases;
        return 0;
    });
}

size_t dehalo_bases_len(const dehalo_bases* bases) { return bases ? bases->n : 0; }

int dehalo_bases_info(const dehalo_bases* bases, uint32_t* window_bits, uint32_t* windows, int* precomputed) {
    if (!bases) return DEHALO_ERR_INVALID;
    if (window_bits) *window_bits = bases->c;
    if (windows) *windows = bases->W;
    if (precomputed) *precomputed = bases->precomp;
    return 0;
}

int dehalo_msm_device(dehalo_ctx* ctx, const dehalo_bases* bases, const uint64_t* d_scalars, size_t len, size_t batch, uint64_t* d_out_jacobian,
                      void* stream) {
    if (!bases || (!d_scalars && len) || !d_out_jacobian) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm: null argument");
    if (len > bases->n) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm: more scalars than registered bases");
    return curve_device(ctx, bases->curve, stream, [&](const CurveOps& cv, hipStream_t s) {
        return cv.run_msm(ctx, bases, (const fe*)d_scalars, len, batch, (jacobian_t*)d_out_jacobian, s);
    });
}

int dehalo_msm_device_affine(dehalo_ctx* ctx, const dehalo_bases* bases, const uint64_t* d_scalars, size_t len, size_t batch, uint64_t* d_out_jacobian,
                             uint64_t* d_out_affine, void* stream) {
    if (!bases || (!d_scalars && len) || !d_out_affine) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm: null argument");
    if (len > bases->n) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm: more scalars than registered bases");
    return dh_device(ctx, stream, [&](hipStream_t s) -> int {
        if (len == 0 || batch == 0) {   // the empty sum: identity = (0, 0)
            if (batch) HIP_TRY(ctx, hipMemsetAsync(d_out_affine, 0, batch * sizeof(affine_t), s));
            if (batch && d_out_jacobian) HIP_TRY(ctx, hipMemsetAsync(d_out_jacobian, 0, batch * sizeof(jacobian_t), s));
            return 0;
        }
        const CurveOps* cv = curve_ops(bases->curve);
        if (!cv) return unknown_curve(ctx);
        // (without a Jacobian destination the kernel skips that form; run_msm_t only passes the pointer on)
        struct AffineOut {      // set for this call only, also when it throws
            dehalo_ctx* ctx;
            ~AffineOut() { ctx->msm_affine_out = nullptr; }
        } reset{ctx};
        ctx->msm_affine_out = (affine_t*)d_out_affine;
        return cv->run_msm(ctx, bases, (const fe*)d_scalars, len, batch, (jacobian_t*)d_out_jacobian, s);
    });
}

int dehalo_msm_batch(dehalo_ctx* ctx, const dehalo_bases* bases, const uint64_t* const* scalars, size_t len, size_t batch, uint64_t* out_jacobian) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!bases || !scalars || !out_jacobian) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm: null argument");
    if (len > bases->n) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm: more scalars than registered bases");
    if (batch && len > (SIZE_MAX / 32) / batch) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm: batch * len overflows");
    for (size_t b = 0; b < batch; b++)
        if (!scalars[b] && len) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm: null scalar column");
    // (not with_host_io: the columns are separate host arrays, each pinned and copied on its own into one workspace buffer)
    return dh_guard(ctx, [&]() -> int {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);   // one critical section per host-buffer call: staging, kernels, download
        (void)hipSetDevice(ctx->device);
        TRY(dh_ensure(ctx, ctx->ws_scalars, std::max<size_t>(32, batch * len * 32)));
        TRY(dh_ensure(ctx, ctx->ws_out, std::max<size_t>(96, batch * 96)));
        for (size_t b = 0; b < batch && len; b++) {
            HostPin pin(scalars[b], len * 32);
            TRY(dh_h2d(ctx, (char*)ctx->ws_scalars.p + b * len * 32, scalars[b], len * 32, ctx->stream.get()));
            if (pin.p) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));      // the pin ends with this scope
        }
        TRY(dehalo_msm_device(ctx, bases, (const uint64_t*)ctx->ws_scalars.p, len, batch, (uint64_t*)ctx->ws_out.p, nullptr));
        TRY(dh_d2h(ctx, out_jacobian, ctx->ws_out.p, batch * 96, ctx->stream.get()));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
        return 0;
    });
}

int dehalo_msm(dehalo_ctx* ctx, const dehalo_bases* bases, const uint64_t* scalars, size_t len, uint64_t out_jacobian[12]) {
    const uint64_t* cols[1] = {scalars};
    return dehalo_msm_batch(ctx, bases, cols, len, 1, out_jacobian);
}

int dehalo_best_multiexp(dehalo_ctx* ctx, int curve, const uint64_t* scalars, const uint64_t* affine_xy, size_t len, uint64_t out_jacobian[12]) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!out_jacobian || ((!scalars || !affine_xy) && len)) return dh_fail(ctx, DEHALO_ERR_INVALID, "best_multiexp: null argument");
    if (!curve_ops(curve)) return unknown_curve(ctx);
    if (len == 0) { memset(out_jacobian, 0, 96); return 0; }
    return dh_guard(ctx, [&]() -> int {
        std::lock_guard<std::recursive_mutex> hold(ctx->mu);
        BasesPtr b;
        TRY(dehalo_bases_register(ctx, curve, affine_xy, len, 64, 0, 0, adopt(ctx, b)));
        return dehalo_msm(ctx, b.get(), scalars, len, out_jacobian);
    });
}

// ---- segmented sums (msm_segments.cuh): many short independent sums in one launch ----
static MsmSegmentsFn msm_segments_fn(int curve) {
    static const MsmSegmentsFn fns[] = {&msm_segments_bn254, &msm_segments_pallas, &msm_segments_vesta};
    return curve >= 0 && curve < 3 ? fns[curve] : nullptr;
}
// what both forms refuse before anything is read: 0 and *fn, or the error
static int msm_segments_args(dehalo_ctx* ctx, int curve, const void* offsets, uint32_t segments, const void* out, MsmSegmentsFn* fn) {
    *fn = msm_segments_fn(curve);
    if (!*fn) return unknown_curve(ctx);
    if (!offsets || (!out && segments)) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm_segments: null argument");
    if (segments > DEHALO_MSM_SEGMENTS_MAX) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm_segments: more than 2^24 segments");
    return 0;
}
// the offsets on the host: segments + 1 words that do not decrease and end within the limit; terms behind them need their scalars and points
static int msm_segments_offsets(dehalo_ctx* ctx, const uint32_t* offsets, uint32_t segments, const void* scalars, const void* points) {
    for (uint32_t s = 0; s < segments; s++)
        if (offsets[s + 1] < offsets[s]) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm_segments: the offsets decrease");
    if (offsets[segments] > DEHALO_MSM_SEGMENTS_MAX_TERMS) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm_segments: more than 2^30 terms");
    if (offsets[segments] > offsets[0] && (!scalars || !points)) return dh_fail(ctx, DEHALO_ERR_INVALID, "msm_segments: null argument");
    return 0;
}

int dehalo_msm_segments_device(dehalo_ctx* ctx, int curve, const uint64_t* d_scalars, const uint64_t* d_affine_xy, const uint32_t* d_offsets, uint32_t segments,
                               uint64_t* d_out_affine, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    MsmSegmentsFn fn;
    TRY(msm_segments_args(ctx, curve, d_offsets, segments, d_out_affine, &fn));
    if (segments == 0) return 0;
    return dh_device(ctx, stream, [&](hipStream_t s) -> int {
        // the offsets come back and are checked BEFORE the launch (one small copy and a wait for the stream): a block then walks its own segment or nothing
        std::vector<uint32_t> offsets((size_t)segments + 1);
        TRY(dh_d2h(ctx, offsets.data(), d_offsets, 4 * offsets.size(), s));
        TRY(msm_segments_offsets(ctx, offsets.data(), segments, d_scalars, d_affine_xy));
        return fn(ctx, (const fe*)d_scalars, (const affine_t*)d_affine_xy, d_offsets, segments, (affine_t*)d_out_affine, s);
    });
}

int dehalo_msm_segments(dehalo_ctx* ctx, int curve, const uint64_t* scalars, const uint64_t* affine_xy, const uint32_t* offsets, uint32_t segments, uint64_t* out_affine) {
    if (!ctx) return DEHALO_ERR_INVALID;
    MsmSegmentsFn fn;
    TRY(msm_segments_args(ctx, curve, offsets, segments, out_affine, &fn));
    if (segments == 0) return 0;
    TRY(msm_segments_offsets(ctx, offsets, segments, scalars, affine_xy));
    return dh_guard(ctx, [&] {
        // (the kernel indexes scalars and points by the offsets themselves: the copies start at term 0)
        const size_t terms = offsets[segments];
        DevBuf* w = ctx->ws_segments;
        return with_host_io(ctx, {{w[0], terms ? scalars : nullptr, terms * 32}, {w[1], terms ? affine_xy : nullptr, terms * 64}, {w[2], offsets, 4 * ((size_t)segments + 1)}},
                            w[3], out_affine, 64 * (size_t)segments, [&] {
            return fn(ctx, (const fe*)w[0].p, (const affine_t*)w[1].p, (const uint32_t*)w[2].p, segments, (affine_t*)w[3].p, ctx->stream.get());
        });
    });
}

int dehalo_point_sum_device(dehalo_ctx* ctx, int curve, const uint64_t* d_jacobian, size_t count, uint64_t* d_out_jacobian, void* stream) {
    if ((!d_jacobian && count) || !d_out_jacobian) return dh_fail(ctx, DEHALO_ERR_INVALID, "point_sum: null argument");
    if (count >= (1ull << 31)) return dh_fail(ctx, DEHALO_ERR_INVALID, "point_sum: too many points");
    return curve_device(ctx, curve, stream, [&](const CurveOps& cv, hipStream_t s) {
        return cv.point_sum(ctx, (const jacobian_t*)d_jacobian, (uint32_t)count, (jacobian_t*)d_out_jacobian, s);
    });
}

int dehalo_to_affine_device(dehalo_ctx* ctx, int curve, const uint64_t* d_jacobian, size_t count, uint64_t* d_affine_xy, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if ((!d_jacobian || !d_affine_xy) && count) return dh_fail(ctx, DEHALO_ERR_INVALID, "to_affine: null argument");
    if (count == 0) return 0;
    if (count >= (1ull << 31)) return dh_fail(ctx, DEHALO_ERR_INVALID, "to_affine: too many points");
    return curve_device(ctx, curve, stream, [&](const CurveOps& cv, hipStream_t s) {
        return cv.to_affine(ctx, (const jacobian_t*)d_jacobian, (affine_t*)d_affine_xy, (uint32_t)count, s);
    });
}

int dehalo_generator_collapse_device(dehalo_ctx* ctx, int curve, const uint64_t* d_affine_xy, size_t len, const uint64_t challenge[4], uint64_t* d_out_affine_xy,
                                     void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!curve_ops(curve)) return unknown_curve(ctx);
    const IpaOps* ops = ipa_ops(curve);
    if (!ops) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "generator_collapse: Pallas and Vesta only (IPA)");
    if (!challenge || ((!d_affine_xy || !d_out_affine_xy) && len)) return dh_fail(ctx, DEHALO_ERR_INVALID, "generator_collapse: null argument");
    if (len & 1) return dh_fail(ctx, DEHALO_ERR_INVALID, "generator_collapse: odd length");
    if (len >= (1ull << 31)) return dh_fail(ctx, DEHALO_ERR_INVALID, "generator_collapse: too many points");
    if (len == 0) return 0;
    const size_t half = len / 2;
    // out == the input is the in-place collapse; any other overlap with the input would be read after it is written
    const uintptr_t ia = (uintptr_t)d_affine_xy, ib = ia + 64 * len, oa = (uintptr_t)d_out_affine_xy, ob = oa + 64 * half;
    if (oa != ia && oa < ib && ia < ob) return dh_fail(ctx, DEHALO_ERR_INVALID, "generator_collapse: the output overlaps the input other than in place");
    const HostField* f = host_field(curve_scalar_field(curve));
    Fe u;
    memcpy(u.v, challenge, 32);
    const Fe uc = f->to_canonical(u);
    return dh_device(ctx, stream, [&](hipStream_t s) { return ops->collapse(ctx, (const affine_t*)d_affine_xy, half, uc.v, (affine_t*)d_out_affine_xy, s); });
}

int dehalo_ipa_s_device(dehalo_ctx* ctx, int curve, const uint64_t* d_challenges, const uint64_t* d_inits, size_t count, uint32_t k, uint64_t* d_out, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!curve_ops(curve)) return unknown_curve(ctx);
    const IpaOps* ops = ipa_ops(curve);
    if (!ops) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "ipa_s: Pallas and Vesta only (IPA)");
    if (!d_challenges || !d_inits || !d_out) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_s: null argument");
    if (k < 1 || k > 28) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_s: k out of range");
    if (count < 1 || count >= ((size_t)1 << 24)) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_s: count out of range");
    return dh_device(ctx, stream, [&](hipStream_t s) -> int {
        TRY(dh_ensure(ctx, ctx->ws_ipa_s, 32 * ipa_s_table_elems(k, count)));
        return ops->s_vector(ctx, (const fe*)d_challenges, (const fe*)d_inits, (uint32_t)count, k, (fe*)ctx->ws_ipa_s.p, (fe*)d_out, s);
    });
}

int dehalo_g_to_lagrange_device(dehalo_ctx* ctx, int curve, const uint64_t* d_g_affine_xy, uint32_t k, uint64_t* d_out_affine_xy, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    const GfftOps* ops = gfft_ops(curve);
    if (!ops) return unknown_curve(ctx);
    if (!d_g_affine_xy || !d_out_affine_xy) return dh_fail(ctx, DEHALO_ERR_INVALID, "g_to_lagrange: null argument");
    if (k > 28) return dh_fail(ctx, DEHALO_ERR_INVALID, "g_to_lagrange: k out of range");
    const size_t n = (size_t)1 << k;
    // out == the input is the in-place transform; any other overlap would be read after it is written
    const uintptr_t ia = (uintptr_t)d_g_affine_xy, ib = ia + 64 * n, oa = (uintptr_t)d_out_affine_xy, ob = oa + 64 * n;
    if (oa != ia && oa < ib && ia < ob) return dh_fail(ctx, DEHALO_ERR_INVALID, "g_to_lagrange: the output overlaps the input other than in place");
    // omega_inv = (ROOT_OF_UNITY^(2^(S - k)))^-1, n_inv = (2^k)^-1 [UPSTREAM halo2_proofs/src/poly/commitment.rs g_to_lagrange: ROOT_OF_UNITY_INV squared S - k times, TWO_INV^k]
    const HostField* f = host_field(curve_scalar_field(curve));
    if (k > f->two_adicity) return dh_fail(ctx, DEHALO_ERR_INVALID, "g_to_lagrange: k out of range");
    Fe omega = f->root_of_unity;
    for (uint32_t i = k; i < f->two_adicity; i++) omega = f->sqr(omega);
    const Fe omega_inv = f->invert(omega), n_inv = f->to_canonical(f->invert(f->from_u64((uint64_t)n)));
    return dh_device(ctx, stream, [&](hipStream_t s) -> int {
        if (k == 0) {      // one point: the transform is the identity map
            if (oa != ia) HIP_TRY(ctx, hipMemcpyAsync(d_out_affine_xy, d_g_affine_xy, 64, hipMemcpyDeviceToDevice, s));
            return 0;
        }
        return ops->g_to_lagrange(ctx, (const affine_t*)d_g_affine_xy, k, omega_inv.v, n_inv.v, (affine_t*)d_out_affine_xy, s);
    });
}

// ---- the point codec (gfft.cuh; its argument checks: points_codec_args above) ----
int dehalo_points_compress_device(dehalo_ctx* ctx, int curve, const uint64_t* d_affine_xy, size_t count, uint8_t* d_out32, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    const GfftOps* ops;
    TRY(points_codec_args(ctx, "points_compress", curve, d_affine_xy, d_out32, count, &ops));
    if (!ops) return 0;
    if (!d_out32) return dh_fail(ctx, DEHALO_ERR_INVALID, "points_compress: null output");
    return dh_device(ctx, stream, [&](hipStream_t s) { return ops->compress(ctx, (const affine_t*)d_affine_xy, d_out32, count, s); });
}

int dehalo_points_decompress_device(dehalo_ctx* ctx, int curve, const uint8_t* d_in32, size_t count, uint64_t* d_affine_xy, uint32_t* status_out, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    const GfftOps* ops;
    TRY(points_codec_args(ctx, "points_decompress", curve, d_affine_xy, d_in32, count, &ops));
    if (status_out) *status_out = 0;
    if (!ops) return 0;
    if (!d_in32 || !status_out) return dh_fail(ctx, DEHALO_ERR_INVALID, "points_decompress: null argument");
    return dh_device(ctx, stream, [&](hipStream_t s) {
        return points_status(ctx, status_out, s, [&](uint32_t* d_status) { return ops->decompress(ctx, d_in32, (affine_t*)d_affine_xy, count, d_status, s); });
    });
}

int dehalo_points_check_device(dehalo_ctx* ctx, int curve, const uint64_t* d_affine_xy, size_t count, uint32_t* status_out, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    const GfftOps* ops;
    TRY(points_codec_args(ctx, "points_check", curve, d_affine_xy, nullptr, count, &ops));
    if (status_out) *status_out = 0;
    if (!ops) return 0;
    if (!status_out) return dh_fail(ctx, DEHALO_ERR_INVALID, "points_check: null status");
    return dh_device(ctx, stream, [&](hipStream_t s) {
        return points_status(ctx, status_out, s, [&](uint32_t* d_status) { return ops->points_check(ctx, (const affine_t*)d_affine_xy, count, d_status, s); });
    });
}

// ---- generated points (gfft.cuh k_points_generate; the rule: include/dehalo.h) ----
int dehalo_points_generate_device(dehalo_ctx* ctx, int curve, const uint8_t* key32, uint64_t chacha_stream, uint64_t first_index, uint64_t* d_affine_xy, size_t count,
                                  void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    const GfftOps* ops;
    TRY(points_codec_args(ctx, "points_generate", curve, d_affine_xy, nullptr, count, &ops));
    const uint64_t index_end = (uint64_t)1 << 48;
    if (first_index > index_end || count > index_end - first_index) return dh_fail(ctx, DEHALO_ERR_INVALID, "points_generate: first_index + count > 2^48");
    if (!ops) return 0;
    uint32_t key[8];
    memcpy(key, key32 ? (const void*)key32 : (const void*)DEHALO_GENERATORS_DEFAULT_KEY, 32);
    uint32_t status = 0;
    TRY(dh_device(ctx, stream, [&](hipStream_t s) {
        return points_status(ctx, &status, s, [&](uint32_t* d_status) { return ops->points_generate(ctx, key, chacha_stream, first_index, (affine_t*)d_affine_xy, count, d_status, s); });
    }));
    if (status) return dh_fail(ctx, DEHALO_ERR_INVALID, "points_generate: an index found no point in 256 attempts (written as (0, 0))");
    return 0;
}

// ---- the scalar codec (scalar_codec.cuh): from_repr and the checked from_raw_bytes over vectors of field elements ----
int dehalo_scalars_from_repr_device(dehalo_ctx* ctx, int field, const uint8_t* d_in32, size_t count, uint64_t* d_out, uint32_t* status_out, uint64_t* first_bad_out,
                                    void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    TRY(scalars_codec_args(ctx, "scalars_from_repr", field, d_out, count, status_out, first_bad_out));
    if (count == 0) return 0;
    if (!d_in32 || ((uintptr_t)d_in32 & 3)) return dh_fail(ctx, DEHALO_ERR_INVALID, "scalars_from_repr: the encodings are null or not 4-byte aligned");
    const uintptr_t a = (uintptr_t)d_in32, b = (uintptr_t)d_out, bytes = (uintptr_t)count * 32;
    if (a != b && a < b + bytes && b < a + bytes) return dh_fail(ctx, DEHALO_ERR_INVALID, "scalars_from_repr: the output overlaps the input without being it");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) {
        return scalars_status(ctx, count, status_out, first_bad_out, s,
                              [&](uint32_t* d_status, uint64_t* d_first) { return f.scalars_from_repr(ctx, d_in32, (fe*)d_out, count, d_status, d_first, s); });
    });
}

int dehalo_scalars_check_device(dehalo_ctx* ctx, int field, const uint64_t* d_words, size_t count, uint32_t* status_out, uint64_t* first_bad_out, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    TRY(scalars_codec_args(ctx, "scalars_check", field, d_words, count, status_out, first_bad_out));
    if (count == 0) return 0;
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) {
        return scalars_status(ctx, count, status_out, first_bad_out, s,
                              [&](uint32_t* d_status, uint64_t* d_first) { return f.scalars_check(ctx, (const fe*)d_words, count, d_status, d_first, s); });
    });
}

int dehalo_blind_commitments_device(dehalo_ctx* ctx, int curve, uint64_t* d_jacobian, const uint64_t* d_blinds, size_t count, const uint64_t* d_w_affine_xy, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!curve_ops(curve)) return unknown_curve(ctx);
    const IpaOps* ops = ipa_ops(curve);
    if (!ops) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "blind_commitments: Pallas and Vesta only (IPA)");
    if (!d_w_affine_xy || ((!d_jacobian || !d_blinds) && count)) return dh_fail(ctx, DEHALO_ERR_INVALID, "blind_commitments: null argument");
    if (count >= (1ull << 29)) return dh_fail(ctx, DEHALO_ERR_INVALID, "blind_commitments: too many points");
    if (count == 0) return 0;
    return dh_device(ctx, stream, [&](hipStream_t s) { return ops->blind(ctx, (jacobian_t*)d_jacobian, (const fe*)d_blinds, (const affine_t*)d_w_affine_xy, count, s); });
}

// ---- fixed-base tables (fixed_base.cuh) ------------------------------------------------------
static const FixedBaseOps* fixed_base_ops(int curve) {
    static const FixedBaseOps* const ops[] = {&bn254_fixed_base_ops(), &pallas_fixed_base_ops(), &vesta_fixed_base_ops()};
    return curve >= 0 && curve < 3 ? ops[curve] : nullptr;
}

int dehalo_fixed_base_create(dehalo_ctx* ctx, int curve, const uint64_t affine_xy[8], dehalo_fixed_base** out) {
    if (!ctx) return DEHALO_ERR_INVALID;
    const FixedBaseOps* ops = fixed_base_ops(curve);
    if (!ops) return unknown_curve(ctx);
    if (!affine_xy || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "fixed_base_create: null argument");
    return dh_guard(ctx, [&]() -> int {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        FixedBasePtr fb(new dehalo_fixed_base(), FixedBaseFree{ctx});
        fb->curve = curve;
        TRY(fb->table.alloc(ctx, 32 * 256, false));
        DevArray<affine_t> tmp;      // the point, then its 32 window multiples
        TRY(tmp.alloc(ctx, 1 + 32, false));
        TRY(dh_h2d(ctx, tmp.p, affine_xy, 64, ctx->stream.get()));
        TRY(ops->build(ctx, tmp.at(0), tmp.at(1), fb->table.p, ctx->stream.get()));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));      // (tmp is freed on return: nothing may still read it)
        *out = fb.release();
        return 0;
    });
}

int dehalo_fixed_base_release(dehalo_ctx* ctx, dehalo_fixed_base* fb) {
    if (!ctx || !fb) return DEHALO_ERR_INVALID;
    return dh_guard(ctx, [&] {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        (void)hipDeviceSynchronize();
        delete fb;
        return 0;
    });
}

int dehalo_fixed_base_mul_device(dehalo_ctx* ctx, const dehalo_fixed_base* fb, const uint64_t* d_scalars, size_t count, uint64_t* d_out_affine_xy, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!fb || ((!d_scalars || !d_out_affine_xy) && count)) return dh_fail(ctx, DEHALO_ERR_INVALID, "fixed_base_mul: null argument");
    const FixedBaseOps* ops = fixed_base_ops(fb->curve);
    if (!ops) return unknown_curve(ctx);
    if (count >= (1ull << 29)) return dh_fail(ctx, DEHALO_ERR_INVALID, "fixed_base_mul: too many scalars");
    if (count == 0) return 0;
    return dh_device(ctx, stream, [&](hipStream_t s) { return ops->mul(ctx, fb->table.p, (const fe*)d_scalars, (affine_t*)d_out_affine_xy, count, s); });
}

int dehalo_fixed_base_blind_device(dehalo_ctx* ctx, const dehalo_fixed_base* fb, uint64_t* d_jacobian, const uint64_t* d_blinds, size_t count, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!fb || ((!d_jacobian || !d_blinds) && count)) return dh_fail(ctx, DEHALO_ERR_INVALID, "fixed_base_blind: null argument");
    const FixedBaseOps* ops = fixed_base_ops(fb->curve);
    if (!ops) return unknown_curve(ctx);
    if (count >= (1ull << 29)) return dh_fail(ctx, DEHALO_ERR_INVALID, "fixed_base_blind: too many points");
    if (count == 0) return 0;
    return dh_device(ctx, stream, [&](hipStream_t s) { return ops->blind(ctx, fb->table.p, (jacobian_t*)d_jacobian, (const fe*)d_blinds, count, s); });
}

int dehalo_to_affine(dehalo_ctx* ctx, int curve, const uint64_t* jacobian, size_t count, uint64_t* affine_xy) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if ((!jacobian || !affine_xy) && count) return dh_fail(ctx, DEHALO_ERR_INVALID, "to_affine: null argument");
    if (count == 0) return 0;
    if (count >= (1ull << 31)) return dh_fail(ctx, DEHALO_ERR_INVALID, "to_affine: too many points");
    return dh_guard(ctx, [&] {
        return with_host_io(ctx, {{ctx->ws_fop[0], jacobian, count * 96}}, ctx->ws_fop[1], affine_xy, count * 64, [&] {
            const CurveOps* cv = curve_ops(curve);
            return cv ? cv->to_affine(ctx, (const jacobian_t*)ctx->ws_fop[0].p, (affine_t*)ctx->ws_fop[1].p, (uint32_t)count, ctx->stream.get()) : unknown_curve(ctx);
        });
    });
}

// ---- NTT family -----------------------------------------------------------------------------
static int ntt_device_impl(dehalo_ctx* ctx, int field, const uint64_t* d_src, uint64_t src_len, uint64_t src_stride, uint64_t* d_dst,
                           uint64_t dst_stride, uint32_t log_n, const uint64_t omega[4], size_t batch, const NttScale& sc, void* stream) {
    if (!d_src || !d_dst || !omega) return dh_fail(ctx, DEHALO_ERR_INVALID, "ntt: null argument");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) {
        return f.run_ntt(ctx, (const fe*)d_src, src_len, src_stride, (fe*)d_dst, dst_stride, log_n, omega, batch, sc, s);
    });
}

int dehalo_ntt_device(dehalo_ctx* ctx, int field, uint64_t* d_a, uint32_t log_n, const uint64_t omega[4], size_t batch, void* stream) {
    NttScale sc;
    uint64_t N = 1ull << (log_n & 63);
    return ntt_device_impl(ctx, field, d_a, N, N, d_a, N, log_n, omega, batch, sc, stream);
}

int dehalo_intt_scaled_device(dehalo_ctx* ctx, int field, uint64_t* d_a, uint32_t log_n, const uint64_t omega_inv[4], const uint64_t n_inv[4],
                              size_t batch, void* stream) {
    if (!n_inv) return dh_fail(ctx, DEHALO_ERR_INVALID, "intt: null n_inv");
    NttScale sc;
    sc.post_mode = 1; sc.post0 = fe_from_u64(n_inv);
    uint64_t N = 1ull << (log_n & 63);
    return ntt_device_impl(ctx, field, d_a, N, N, d_a, N, log_n, omega_inv, batch, sc, stream);
}

int dehalo_lagrange_to_coeff_device(dehalo_ctx* ctx, int field, const uint64_t* d_values, uint64_t* d_coeffs, uint32_t log_n, const uint64_t omega_inv[4],
                                    const uint64_t n_inv[4], size_t batch, void* stream) {
    if (!n_inv) return dh_fail(ctx, DEHALO_ERR_INVALID, "lagrange_to_coeff: null n_inv");
    NttScale sc;
    sc.post_mode = 1; sc.post0 = fe_from_u64(n_inv);
    uint64_t N = 1ull << (log_n & 63);
    return ntt_device_impl(ctx, field, d_values, N, N, d_coeffs, N, log_n, omega_inv, batch, sc, stream);
}

static int form_shift_of(uint32_t flags) {   // OUT_INTERNAL: x 2^5; IN_INTERNAL: x 2^-5; both: no change of scale
    return (flags & DEHALO_FORM_OUT_INTERNAL ? 1 : 0) - (flags & DEHALO_FORM_IN_INTERNAL ? 1 : 0);
}

int dehalo_coset_ntt_device(dehalo_ctx* ctx, int field, const uint64_t* d_coeffs, uint32_t log_n, uint64_t* d_ext_out, uint32_t log_ext,
                            const uint64_t omega_ext[4], const uint64_t zeta[4], size_t batch, void* stream) {
    return dehalo_coset_ntt_form_device(ctx, field, d_coeffs, log_n, d_ext_out, log_ext, omega_ext, zeta, batch, 0, stream);
}

int dehalo_coset_ntt_form_device(dehalo_ctx* ctx, int field, const uint64_t* d_coeffs, uint32_t log_n, uint64_t* d_ext_out, uint32_t log_ext,
                                 const uint64_t omega_ext[4], const uint64_t zeta[4], size_t batch, uint32_t form_flags, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!zeta || log_ext < log_n) return dh_fail(ctx, DEHALO_ERR_INVALID, "coset_ntt: bad argument");
    if (d_coeffs == d_ext_out) return dh_fail(ctx, DEHALO_ERR_INVALID, "coset_ntt: coeffs and ext_out may not alias");
    NttScale sc;
    sc.form_shift = form_shift_of(form_flags);
    sc.pre_mode = 1; sc.pre_z = fe_from_u64(zeta);  // zeta^2 is formed inside the kernel
    uint64_t n = 1ull << (log_n & 63), N = 1ull << (log_ext & 63);
    return ntt_device_impl(ctx, field, d_coeffs, n, n, d_ext_out, N, log_ext, omega_ext, batch, sc, stream);
}

int dehalo_coset_intt_form_device(dehalo_ctx* ctx, int field, uint64_t* d_a, uint32_t log_ext, const uint64_t omega_ext_inv[4],
                                  const uint64_t ext_n_inv[4], const uint64_t zeta[4], size_t batch, uint32_t form_flags, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!zeta || !ext_n_inv) return dh_fail(ctx, DEHALO_ERR_INVALID, "coset_intt: null argument");
    NttScale sc;
    sc.post_mode = 2; sc.post0 = fe_from_u64(ext_n_inv); sc.post_z = fe_from_u64(zeta);
    sc.form_shift = form_shift_of(form_flags);
    uint64_t N = 1ull << (log_ext & 63);
    return ntt_device_impl(ctx, field, d_a, N, N, d_a, N, log_ext, omega_ext_inv, batch, sc, stream);
}

int dehalo_coset_intt_device(dehalo_ctx* ctx, int field, uint64_t* d_a, uint32_t log_ext, const uint64_t omega_ext_inv[4],
                             const uint64_t ext_n_inv[4], const uint64_t zeta[4], size_t batch, void* stream) {
    return dehalo_coset_intt_form_device(ctx, field, d_a, log_ext, omega_ext_inv, ext_n_inv, zeta, batch, 0, stream);
}

int dehalo_convert_form_device(dehalo_ctx* ctx, int field, const uint64_t* d_in, uint64_t* d_out, size_t n, int to_internal, void* stream) {
    if ((!d_in || !d_out) && n) return dh_fail(ctx, DEHALO_ERR_INVALID, "convert_form: null argument");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) { return f.convert_form(ctx, (const fe*)d_in, (fe*)d_out, n, to_internal, s); });
}

int dehalo_ntt(dehalo_ctx* ctx, int field, uint64_t* a, uint32_t log_n, const uint64_t omega[4]) {
    if (log_n > 30) return dh_fail(ctx, DEHALO_ERR_INVALID, "log_n > 30");
    size_t N = (size_t)1 << log_n;
    return ntt_host_io(ctx, a, N, a, N, true, [&](uint64_t* di, uint64_t*) { return dehalo_ntt_device(ctx, field, di, log_n, omega, 1, nullptr); });
}

int dehalo_intt_scaled(dehalo_ctx* ctx, int field, uint64_t* a, uint32_t log_n, const uint64_t omega_inv[4], const uint64_t n_inv[4]) {
    if (log_n > 30) return dh_fail(ctx, DEHALO_ERR_INVALID, "log_n > 30");
    size_t N = (size_t)1 << log_n;
    return ntt_host_io(ctx, a, N, a, N, true, [&](uint64_t* di, uint64_t*) { return dehalo_intt_scaled_device(ctx, field, di, log_n, omega_inv, n_inv, 1, nullptr); });
}

int dehalo_coset_ntt(dehalo_ctx* ctx, int field, const uint64_t* coeffs, uint32_t log_n, uint64_t* ext_out, uint32_t log_ext,
                     const uint64_t omega_ext[4], const uint64_t zeta[4]) {
    if (log_ext > 30 || log_ext < log_n) return dh_fail(ctx, DEHALO_ERR_INVALID, "coset_ntt: bad sizes");
    return ntt_host_io(ctx, coeffs, (size_t)1 << log_n, ext_out, (size_t)1 << log_ext, false, [&](uint64_t* di, uint64_t* dout) {
        return dehalo_coset_ntt_device(ctx, field, di, log_n, dout, log_ext, omega_ext, zeta, 1, nullptr);
    });
}

int dehalo_coset_intt(dehalo_ctx* ctx, int field, uint64_t* a, uint32_t log_ext, const uint64_t omega_ext_inv[4], const uint64_t ext_n_inv[4],
                      const uint64_t zeta[4]) {
    if (log_ext > 30) return dh_fail(ctx, DEHALO_ERR_INVALID, "log_ext > 30");
    size_t N = (size_t)1 << log_ext;
    return ntt_host_io(ctx, a, N, a, N, true, [&](uint64_t* di, uint64_t*) {
        return dehalo_coset_intt_device(ctx, field, di, log_ext, omega_ext_inv, ext_n_inv, zeta, 1, nullptr);
    });
}

int dehalo_field_op(dehalo_ctx* ctx, int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!a || !out || op < 0 || op > 6) return dh_fail(ctx, DEHALO_ERR_INVALID, "field_op: bad argument");
    if (n == 0) return 0;
    return dh_guard(ctx, [&] {
        DevBuf* w = ctx->ws_fop;
        return with_host_io(ctx, {{w[0], a, n * 32}, {w[1], b, n * 32}}, w[2], out, n * 32, [&] {
            const FieldOps* f = field_ops(field);
            return f ? f->field_op(ctx, op, (const fe*)w[0].p, b ? (const fe*)w[1].p : nullptr, (fe*)w[2].p, n, ctx->stream.get()) : unknown_field(ctx);
        });
    });
}

int dehalo_field_op_device(dehalo_ctx* ctx, int field, int op, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, size_t n, void* stream) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (((!d_a || !d_out) && n) || op < 0 || op > 6) return dh_fail(ctx, DEHALO_ERR_INVALID, "field_op: bad argument");
    if (n == 0) return 0;
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) { return f.field_op(ctx, op, (const fe*)d_a, (const fe*)d_b, (fe*)d_out, n, s); });
}

// ---- field-vector primitives (poly.cuh) ---------------------------------------------------------
int dehalo_eval_polynomial_device(dehalo_ctx* ctx, int field, const uint64_t* d_coeffs, size_t len, size_t stride_elems, size_t batch,
                                  const uint64_t point[4], uint64_t* d_out, void* stream) {
    if ((!d_coeffs && len) || !point || !d_out) return dh_fail(ctx, DEHALO_ERR_INVALID, "eval_polynomial: null argument");
    if (batch > 1 && stride_elems < len) return dh_fail(ctx, DEHALO_ERR_INVALID, "eval_polynomial: stride shorter than the polynomial");
    if (batch >= 65536) return dh_fail(ctx, DEHALO_ERR_INVALID, "eval_polynomial: batch too large");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) {
        return f.eval_poly(ctx, (const fe*)d_coeffs, len, stride_elems, batch, point, (fe*)d_out, s);
    });
}

int dehalo_eval_polynomial_multi_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_polys, size_t count, size_t len, const uint64_t* points,
                                        uint32_t num_points, uint64_t* d_out, void* stream) {
    return dehalo_eval_polynomial_multi_masked_device(ctx, field, d_polys, count, len, points, num_points, nullptr, d_out, stream);
}

int dehalo_eval_polynomial_multi_masked_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_polys, size_t count, size_t len, const uint64_t* points,
                                               uint32_t num_points, const uint8_t* wanted, uint64_t* d_out, void* stream) {
    if ((count && !d_polys) || !points || !d_out) return dh_fail(ctx, DEHALO_ERR_INVALID, "eval_polynomial_multi: null argument");
    for (size_t j = 0; j < count; j++)
        if (!d_polys[j] && len) return dh_fail(ctx, DEHALO_ERR_INVALID, "eval_polynomial_multi: null polynomial");
    if (num_points == 0 || num_points > 4) return dh_fail(ctx, DEHALO_ERR_INVALID, "eval_polynomial_multi: 1 to 4 points");
    if (count >= 65536) return dh_fail(ctx, DEHALO_ERR_INVALID, "eval_polynomial_multi: too many polynomials");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) {
        return f.eval_poly_multi(ctx, (const fe* const*)d_polys, count, len, points, num_points, (fe*)d_out, s, wanted);
    });
}

int dehalo_eval_polynomial_points_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_polys, size_t count, size_t len, const uint64_t* points,
                                         uint32_t num_points, const uint32_t* wanted, uint64_t* d_out, void* stream) {
    if ((count && !d_polys) || !points || !d_out) return dh_fail(ctx, DEHALO_ERR_INVALID, "eval_polynomial_points: null argument");
    for (size_t j = 0; j < count; j++)
        if (!d_polys[j] && len) return dh_fail(ctx, DEHALO_ERR_INVALID, "eval_polynomial_points: null polynomial");
    if (num_points == 0 || num_points > 32) return dh_fail(ctx, DEHALO_ERR_INVALID, "eval_polynomial_points: 1 to 32 points");
    if (count >= 65536) return dh_fail(ctx, DEHALO_ERR_INVALID, "eval_polynomial_points: too many polynomials");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) {
        return f.eval_poly_points(ctx, (const fe* const*)d_polys, count, len, points, num_points, (fe*)d_out, s, wanted);
    });
}

int dehalo_eval_polynomial(dehalo_ctx* ctx, int field, const uint64_t* coeffs, size_t len, const uint64_t point[4], uint64_t out[4]) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if ((!coeffs && len) || !point || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "eval_polynomial: null argument");
    return dh_guard(ctx, [&] {
        HostPin pin_c(coeffs, len * 32);
        DevBuf* w = ctx->ws_poly_io;
        return with_host_io(ctx, {{w[0], coeffs, len * 32}}, w[1], out, 32, [&] {
            return dehalo_eval_polynomial_device(ctx, field, (const uint64_t*)w[0].p, len, len, 1, point, (uint64_t*)w[1].p, nullptr);
        });
    });
}

int dehalo_batch_invert_device(dehalo_ctx* ctx, int field, uint64_t* d_values, size_t len, void* stream) {
    if (!d_values && len) return dh_fail(ctx, DEHALO_ERR_INVALID, "batch_invert: null argument");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) { return f.batch_invert(ctx, (fe*)d_values, len, s); });
}

int dehalo_batch_invert(dehalo_ctx* ctx, int field, uint64_t* values, size_t len) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!values && len) return dh_fail(ctx, DEHALO_ERR_INVALID, "batch_invert: null argument");
    return dh_guard(ctx, [&] {
        HostPin pin_v(values, len * 32);
        if (len == 0) return 0;
        DevBuf* w = ctx->ws_poly_io;
        return with_host_io(ctx, {{w[0], values, len * 32}}, w[0], values, len * 32, [&] {
            return dehalo_batch_invert_device(ctx, field, (uint64_t*)w[0].p, len, nullptr);
        });
    });
}

int dehalo_prefix_product_device(dehalo_ctx* ctx, int field, const uint64_t* d_in, size_t len, uint64_t* d_out, void* stream) {
    if ((!d_in || !d_out) && len) return dh_fail(ctx, DEHALO_ERR_INVALID, "prefix_product: null argument");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) { return f.prefix_product(ctx, (const fe*)d_in, len, (fe*)d_out, s); });
}

int dehalo_grand_product_batch_device(dehalo_ctx* ctx, int field, const uint64_t* d_num, const uint64_t* d_den, size_t len, size_t batch, size_t stride_elems,
                                      uint64_t* d_z, void* stream) {
    if ((!d_num || !d_den || !d_z) && len && batch) return dh_fail(ctx, DEHALO_ERR_INVALID, "grand_product: null argument");
    if (batch > 1 && stride_elems < len) return dh_fail(ctx, DEHALO_ERR_INVALID, "grand_product: stride shorter than the columns");
    if (batch >= 65536) return dh_fail(ctx, DEHALO_ERR_INVALID, "grand_product: batch too large");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) {
        return f.grand_product(ctx, (const fe*)d_num, (const fe*)d_den, len, batch, stride_elems, (fe*)d_z, s);
    });
}

int dehalo_grand_product_device(dehalo_ctx* ctx, int field, const uint64_t* d_num, const uint64_t* d_den, size_t len, uint64_t* d_z, void* stream) {
    return dehalo_grand_product_batch_device(ctx, field, d_num, d_den, len, 1, len, d_z, stream);
}

int dehalo_grand_product(dehalo_ctx* ctx, int field, const uint64_t* num, const uint64_t* den, size_t len, uint64_t* z) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if ((!num || !den || !z) && len) return dh_fail(ctx, DEHALO_ERR_INVALID, "grand_product: null argument");
    return dh_guard(ctx, [&] {
        HostPin pin_n(num, len * 32), pin_d(den, len * 32), pin_z(z, len * 32);
        if (len == 0) return 0;
        DevBuf* w = ctx->ws_poly_io;
        return with_host_io(ctx, {{w[0], num, len * 32}, {w[1], den, len * 32}}, w[2], z, len * 32, [&] {
            return dehalo_grand_product_device(ctx, field, (const uint64_t*)w[0].p, (const uint64_t*)w[1].p, len, (uint64_t*)w[2].p, nullptr);
        });
    });
}

int dehalo_lincomb_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_cols, const uint64_t* coefs, size_t count, size_t len, uint64_t* d_out,
                          const uint64_t* sub_const, void* stream) {
    if ((count && (!d_cols || !coefs)) || (!d_out && len)) return dh_fail(ctx, DEHALO_ERR_INVALID, "lincomb: null argument");
    for (size_t j = 0; j < count; j++)
        if (!d_cols[j] && len) return dh_fail(ctx, DEHALO_ERR_INVALID, "lincomb: null column");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) {
        return f.lincomb(ctx, (const fe* const*)d_cols, coefs, count, len, (fe*)d_out, sub_const, s);
    });
}

int dehalo_scale_device(dehalo_ctx* ctx, int field, uint64_t* d_a, size_t len, const uint64_t* pattern, uint32_t period, const uint64_t* d_factor, void* stream) {
    if ((!d_a && len) || (period && !pattern)) return dh_fail(ctx, DEHALO_ERR_INVALID, "scale: null argument");
    if (period > 8 || (period & (period - 1))) return dh_fail(ctx, DEHALO_ERR_INVALID, "scale: period must be 0, 1, 2, 4 or 8");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) { return f.scale(ctx, (fe*)d_a, len, pattern, period, (const fe*)d_factor, s); });
}

int dehalo_kate_division_device(dehalo_ctx* ctx, int field, const uint64_t* d_a, size_t len, const uint64_t point[4], uint64_t* d_q, void* stream) {
    if (((!d_a || !d_q) && len > 1) || !point) return dh_fail(ctx, DEHALO_ERR_INVALID, "kate_division: null argument");
    if (d_a == d_q) return dh_fail(ctx, DEHALO_ERR_INVALID, "kate_division: a and q may not alias");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) { return f.kate_division(ctx, (const fe*)d_a, len, point, (fe*)d_q, s); });
}

int dehalo_kate_division_batch_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_a, size_t len, const uint64_t* points, uint64_t* const* d_q,
                                      size_t count, void* stream) {
    if (count && (!d_a || !d_q || !points)) return dh_fail(ctx, DEHALO_ERR_INVALID, "kate_division_batch: null argument");
    if (count > 8) return dh_fail(ctx, DEHALO_ERR_INVALID, "kate_division_batch: at most 8 divisions per call");
    if (len > (1ull << 22)) return dh_fail(ctx, DEHALO_ERR_INVALID, "kate_division_batch: polynomials of at most 2^22 coefficients");
    for (size_t y = 0; y < count; y++) {
        if ((!d_a[y] || !d_q[y]) && len > 1) return dh_fail(ctx, DEHALO_ERR_INVALID, "kate_division_batch: null polynomial");
        if (d_a[y] == d_q[y]) return dh_fail(ctx, DEHALO_ERR_INVALID, "kate_division_batch: a and q may not alias");
    }
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) {
        return f.kate_division_batch(ctx, (const fe* const*)d_a, len, points, (fe* const*)d_q, count, s);
    });
}

int dehalo_vanishing_quotient_batch_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_a, size_t len, const uint64_t* const* points, const uint32_t* num_points,
                                           uint64_t* const* d_q, size_t count, void* stream) {
    // every check and the weights come before the first launch: a refused call leaves the outputs untouched
    if (count && (!d_a || !d_q || !points || !num_points)) return dh_fail(ctx, DEHALO_ERR_INVALID, "vanishing_quotient_batch: null argument");
    if (count > 8) return dh_fail(ctx, DEHALO_ERR_INVALID, "vanishing_quotient_batch: at most 8 polynomials per call");
    if (len > (1ull << 22)) return dh_fail(ctx, DEHALO_ERR_INVALID, "vanishing_quotient_batch: polynomials of at most 2^22 coefficients");
    const HostField* hf = host_field(field);
    if (!hf || !field_ops(field)) return unknown_field(ctx);
    size_t total = 0;
    for (size_t y = 0; y < count; y++) {
        if (num_points[y] == 0 || num_points[y] > 32) return dh_fail(ctx, DEHALO_ERR_INVALID, "vanishing_quotient_batch: 1 to 32 points per polynomial");
        if (!points[y] || ((!d_a[y] || !d_q[y]) && len)) return dh_fail(ctx, DEHALO_ERR_INVALID, "vanishing_quotient_batch: null polynomial or point set");
        if (d_a[y] == d_q[y]) return dh_fail(ctx, DEHALO_ERR_INVALID, "vanishing_quotient_batch: a and q may not alias");
        total += num_points[y];
    }
    return dh_guard(ctx, [&]() -> int {
        // per point {z, w, z^2048}: w_t = 1 / prod_{s != t} (z_t - z_s), every denominator of the call inverted together (Montgomery's trick)
        std::vector<Fe> tab(3 * total), pre(total);
        Fe acc = hf->one;
        size_t o = 0;
        for (size_t y = 0; y < count; y++) {
            const Fe* z = (const Fe*)points[y];
            for (uint32_t t = 0; t < num_points[y]; t++, o++) {
                Fe den = hf->one;
                for (uint32_t s2 = 0; s2 < num_points[y]; s2++)
                    if (s2 != t) den = hf->mul(den, hf->sub(z[t], z[s2]));
                if (den.is_zero()) return dh_fail(ctx, DEHALO_ERR_INVALID, "vanishing_quotient_batch: two equal points in one set");
                Fe z2048 = z[t];
                for (int q = 0; q < 11; q++) z2048 = hf->sqr(z2048);
                tab[3 * o] = z[t]; tab[3 * o + 1] = den; tab[3 * o + 2] = z2048;
                pre[o] = acc;
                acc = hf->mul(acc, den);
            }
        }
        Fe inv = hf->invert(acc);
        for (size_t i = total; i-- > 0;) {
            const Fe w = hf->mul(inv, pre[i]);
            inv = hf->mul(inv, tab[3 * i + 1]);
            tab[3 * i + 1] = w;
        }
        return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) {
            return f.vanishing_quotient_batch(ctx, (const fe* const*)d_a, len, tab.empty() ? nullptr : tab[0].v, num_points, (fe* const*)d_q, count, s);
        });
    });
}

int dehalo_kate_division(dehalo_ctx* ctx, int field, const uint64_t* a, size_t len, const uint64_t point[4], uint64_t* q) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (((!a || !q) && len > 1) || !point) return dh_fail(ctx, DEHALO_ERR_INVALID, "kate_division: null argument");
    return dh_guard(ctx, [&] {
        HostPin pin_a(a, len * 32), pin_q(q, (len - 1) * 32);
        if (len <= 1) return 0;
        DevBuf* w = ctx->ws_poly_io;      // (q: len - 1 coefficients in a buffer sized for len, as a)
        return with_host_io(ctx, {{w[0], a, len * 32}, {w[1], nullptr, len * 32}}, w[1], q, (len - 1) * 32, [&] {
            return dehalo_kate_division_device(ctx, field, (const uint64_t*)w[0].p, len, point, (uint64_t*)w[1].p, nullptr);
        });
    });
}

int dehalo_permute_expression_pair_batch_device(dehalo_ctx* ctx, int field, const uint64_t* d_inputs, const uint64_t* d_tables, size_t usable_rows, size_t batch,
                                                size_t stride_elems, uint64_t* d_permuted_inputs, uint64_t* d_permuted_tables, void* stream) {
    if ((!d_inputs || !d_tables || !d_permuted_inputs || !d_permuted_tables) && usable_rows && batch)
        return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair: null argument");
    if (d_permuted_inputs == d_inputs || d_permuted_tables == d_tables || d_permuted_inputs == d_tables || d_permuted_tables == d_inputs)
        return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair: outputs may not alias inputs");
    if (batch > 1 && stride_elems < usable_rows) return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair: stride shorter than the columns");
    if (batch >= 4096) return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair: batch too large");
    if (!field_ops(field)) return unknown_field(ctx);
    return dh_device(ctx, stream, [&](hipStream_t s) {
        return lookup_permute_impl(ctx, field, (const fe*)d_inputs, (const fe*)d_tables, usable_rows, batch, stride_elems, (fe*)d_permuted_inputs,
                                   (fe*)d_permuted_tables, s);
    });
}

static int permute_ptrs(dehalo_ctx* ctx, int field, const uint64_t* const* d_inputs, const uint64_t* const* d_tables, size_t usable_rows, size_t batch,
                        uint64_t* const* d_permuted_inputs, uint64_t* const* d_permuted_tables, int* d_status, void* stream, const LookupDistinct* distinct);
int dehalo_permute_expression_pair_ptrs_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_inputs, const uint64_t* const* d_tables, size_t usable_rows, size_t batch,
                                               uint64_t* const* d_permuted_inputs, uint64_t* const* d_permuted_tables, void* stream) {
    return permute_ptrs(ctx, field, d_inputs, d_tables, usable_rows, batch, d_permuted_inputs, d_permuted_tables, nullptr, stream, nullptr);
}
int dehalo_permute_expression_pair_ptrs_deferred_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_inputs, const uint64_t* const* d_tables, size_t usable_rows,
                                                        size_t batch, uint64_t* const* d_permuted_inputs, uint64_t* const* d_permuted_tables, int32_t* d_status, void* stream) {
    if (ctx && !d_status && batch) return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair: null status array");
    return permute_ptrs(ctx, field, d_inputs, d_tables, usable_rows, batch, d_permuted_inputs, d_permuted_tables, (int*)d_status, stream, nullptr);
}
static int permute_ptrs(dehalo_ctx* ctx, int field, const uint64_t* const* d_inputs, const uint64_t* const* d_tables, size_t usable_rows, size_t batch,
                        uint64_t* const* d_permuted_inputs, uint64_t* const* d_permuted_tables, int* d_status, void* stream, const LookupDistinct* distinct) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if ((!d_inputs || !d_tables || !d_permuted_inputs || !d_permuted_tables) && batch) return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair: null argument");
    if (batch >= 4096) return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair: batch too large");
    if (!field_ops(field)) return unknown_field(ctx);
    for (size_t y = 0; y < batch && usable_rows; y++) {
        if (!d_inputs[y] || !d_tables[y] || !d_permuted_inputs[y] || !d_permuted_tables[y]) return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair: null column");
        for (size_t z = 0; z < batch; z++)
            if (d_permuted_inputs[y] == d_inputs[z] || d_permuted_inputs[y] == d_tables[z] || d_permuted_tables[y] == d_inputs[z] || d_permuted_tables[y] == d_tables[z])
                return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair: outputs may not alias inputs");
    }
    return dh_device(ctx, stream, [&](hipStream_t s) {
        return lookup_permute_ptrs(ctx, field, (const fe* const*)d_inputs, (const fe* const*)d_tables, usable_rows, batch, (fe* const*)d_permuted_inputs,
                                   (fe* const*)d_permuted_tables, s, d_status, distinct);
    });
}
int dehalo_permute_expression_pair_distinct_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_inputs, const uint64_t* const* d_tables, size_t usable_rows, size_t batch,
                                                   uint64_t* const* d_permuted_inputs, uint64_t* const* d_permuted_tables, const uint32_t* const* d_rep_rows,
                                                   const uint32_t* const* d_multiplicities, const uint32_t* distinct_count, int32_t* d_status, void* stream) {
    if (ctx && batch && (!d_rep_rows || !d_multiplicities || !distinct_count)) return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair_distinct: null argument");
    return dh_guard(ctx, [&] {
        std::vector<LookupDistinct> dist(batch);
        for (size_t y = 0; y < batch; y++) {
            dist[y] = LookupDistinct{d_rep_rows[y], d_multiplicities[y], distinct_count[y]};
            if (distinct_count[y] && (!d_rep_rows[y] || !d_multiplicities[y])) return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair_distinct: null distinct-row array");
            if (distinct_count[y] > usable_rows) return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair_distinct: more distinct rows than usable rows");
            for (size_t z = 0; z < y; z++)      // lookups of one table must describe it alike
                if (d_tables && d_tables[z] == d_tables[y] && (d_rep_rows[z] != d_rep_rows[y] || d_multiplicities[z] != d_multiplicities[y] || distinct_count[z] != distinct_count[y]))
                    return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair_distinct: lookups that share a table must pass the same distinct-row arrays");
        }
        return permute_ptrs(ctx, field, d_inputs, d_tables, usable_rows, batch, d_permuted_inputs, d_permuted_tables, (int*)d_status, stream, dist.data());
    });
}

int dehalo_permute_expression_pair_device(dehalo_ctx* ctx, int field, const uint64_t* d_input, const uint64_t* d_table, size_t usable_rows,
                                          uint64_t* d_permuted_input, uint64_t* d_permuted_table, void* stream) {
    return dehalo_permute_expression_pair_batch_device(ctx, field, d_input, d_table, usable_rows, 1, usable_rows, d_permuted_input, d_permuted_table, stream);
}

int dehalo_permute_expression_pair(dehalo_ctx* ctx, int field, const uint64_t* input, const uint64_t* table, size_t usable_rows, uint64_t* permuted_input,
                                   uint64_t* permuted_table) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if ((!input || !table || !permuted_input || !permuted_table) && usable_rows) return dh_fail(ctx, DEHALO_ERR_INVALID, "permute_expression_pair: null argument");
    // (not with_host_io: two columns back to back in one workspace buffer each way)
    return dh_guard(ctx, [&] {
        HostPin pin_i(input, usable_rows * 32), pin_t(table, usable_rows * 32), pin_pi(permuted_input, usable_rows * 32), pin_pt(permuted_table, usable_rows * 32);
        if (usable_rows == 0) return 0;
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);   // one critical section per host-buffer call: staging, kernels, download
        (void)hipSetDevice(ctx->device);
        TRY(dh_ensure(ctx, ctx->ws_poly_io[0], usable_rows * 64));
        TRY(dh_ensure(ctx, ctx->ws_poly_io[1], usable_rows * 64));
        TRY(dh_h2d(ctx, ctx->ws_poly_io[0].p, input, usable_rows * 32, ctx->stream.get()));
        TRY(dh_h2d(ctx, (char*)ctx->ws_poly_io[0].p + usable_rows * 32, table, usable_rows * 32, ctx->stream.get()));
        uint64_t* d_in = (uint64_t*)ctx->ws_poly_io[0].p;
        uint64_t* d_out = (uint64_t*)ctx->ws_poly_io[1].p;
        TRY(dehalo_permute_expression_pair_device(ctx, field, d_in, d_in + usable_rows * 4, usable_rows, d_out, d_out + usable_rows * 4, nullptr));
        TRY(dh_d2h(ctx, permuted_input, d_out, usable_rows * 32, ctx->stream.get()));
        TRY(dh_d2h(ctx, permuted_table, d_out + usable_rows * 4, usable_rows * 32, ctx->stream.get()));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
        return 0;
    });
}

// ---- quotient numerator (evalh.cuh) -----------------------------------------------------------------
static int graph_create_impl(dehalo_ctx* ctx, int field, const uint64_t* constants, uint32_t num_constants, const int32_t* rotations, uint32_t num_rotations,
                             const dehalo_calculation* calcs, uint32_t num_calcs, const dehalo_source* horner_parts, uint32_t num_horner_parts,
                             uint32_t num_intermediates, const uint32_t* root_of, uint32_t num_roots, dehalo_graph** out) {
    if (!ctx) return DEHALO_ERR_INVALID;
    if (!out || (num_constants && !constants) || (num_rotations && !rotations) || (num_calcs && !calcs) || (num_horner_parts && !horner_parts))
        return dh_fail(ctx, DEHALO_ERR_INVALID, "graph_create: null argument");
    const FieldOps* f = field_ops(field);
    if (!f) return unknown_field(ctx);
    if (num_calcs > (1u << 20) || num_intermediates > (1u << 20)) return dh_fail(ctx, DEHALO_ERR_INVALID, "graph_create: program too large");
    return dh_guard(ctx, [&]() -> int {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        GraphPtr g(new dehalo_graph(), GraphFree{ctx});
        g->field = field; g->num_calcs = num_calcs; g->num_parts = num_horner_parts; g->num_constants = num_constants;
        std::vector<DevCalc> dc;
        std::vector<DevSrc> dp;
        std::vector<uint32_t> roots;
        TRY(compile_graph(ctx, g.get(), rotations, num_rotations, calcs, num_calcs, horner_parts, num_horner_parts, num_intermediates, dc, dp, true, root_of, &roots));
        TRY(g->d_calcs.alloc(ctx, std::max<size_t>(1, dc.size()), false));
        TRY(g->d_parts.alloc(ctx, dp.size(), false));
        TRY(g->d_constants.alloc(ctx, std::max<size_t>(1, num_constants), false));
        if (!dc.empty()) HIP_TRY(ctx, hipMemcpy(g->d_calcs.p, dc.data(), dc.size() * sizeof(DevCalc), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(g->d_parts.p, dp.data(), dp.size() * sizeof(DevSrc), hipMemcpyHostToDevice));
        if (root_of) {
            g->num_roots = num_roots;
            TRY(g->d_root_of.alloc(ctx, std::max<size_t>(1, roots.size()), false));
            if (!roots.empty()) HIP_TRY(ctx, hipMemcpy(g->d_root_of.p, roots.data(), roots.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        TRY(f->graph_upload(ctx, g.get(), constants, ctx->stream.get()));
        *out = g.release();
        return 0;
    });
}

int dehalo_graph_create(dehalo_ctx* ctx, int field, const uint64_t* constants, uint32_t num_constants, const int32_t* rotations, uint32_t num_rotations,
                        const dehalo_calculation* calcs, uint32_t num_calcs, const dehalo_source* horner_parts, uint32_t num_horner_parts,
                        uint32_t num_intermediates, dehalo_graph** out) {
    return graph_create_impl(ctx, field, constants, num_constants, rotations, num_rotations, calcs, num_calcs, horner_parts, num_horner_parts, num_intermediates, nullptr, 0, out);
}

int dehalo_graph_release(dehalo_ctx* ctx, dehalo_graph* g) {
    if (!ctx || !g) return DEHALO_ERR_INVALID;
    return dh_guard(ctx, [&] {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        (void)hipDeviceSynchronize();
        delete g;
        return 0;
    });
}

int dehalo_graph_evaluate_device(dehalo_ctx* ctx, const dehalo_graph* g, const dehalo_eval_inputs* in, uint32_t log_rows, uint32_t rot_scale,
                                 const uint64_t* d_previous, uint64_t* d_out, void* stream) {
    if (!g || !in || !d_out) return dh_fail(ctx, DEHALO_ERR_INVALID, "graph_evaluate: null argument");
    if (log_rows > 30) return dh_fail(ctx, DEHALO_ERR_INVALID, "graph_evaluate: log_rows > 30");
    if (in->num_fixed < g->max_fixed || in->num_advice < g->max_advice || in->num_instance < g->max_instance || in->num_challenges < g->max_challenge)
        return dh_fail(ctx, DEHALO_ERR_INVALID, "graph_evaluate: the program reads a column or challenge that was not supplied");
    if ((in->num_fixed && !in->fixed) || (in->num_advice && !in->advice) || (in->num_instance && !in->instance) || (in->num_challenges && !in->challenges))
        return dh_fail(ctx, DEHALO_ERR_INVALID, "graph_evaluate: null column table");
    return field_device(ctx, g->field, stream, [&](const FieldOps& f, hipStream_t s) {
        return f.graph_evaluate(ctx, g, in, log_rows, rot_scale, (const fe*)d_previous, (fe*)d_out, s);
    });
}

int dehalo_graph_evaluate_batch_device(dehalo_ctx* ctx, const dehalo_graph* const* graphs, uint32_t count, const dehalo_eval_inputs* in, uint32_t log_rows,
                                       uint32_t rot_scale, uint64_t* const* d_outs, void* stream) {
    if ((count && (!graphs || !d_outs)) || !in) return dh_fail(ctx, DEHALO_ERR_INVALID, "graph_evaluate_batch: null argument");
    return dh_device(ctx, stream, [&](hipStream_t s) -> int {
        // DEHALO_GRAPH_BATCH=0: one staging + one evaluation launch per program, as before round 4 (A/B measurements)
        static const bool batched = [] { const char* e = DH_EXPERIMENT_ENV("DEHALO_GRAPH_BATCH"); return !(e && e[0] == '0'); }();
        bool same_field = count >= 2 && log_rows <= 30;
        for (uint32_t i = 0; same_field && i < count; i++) {
            const dehalo_graph* g = graphs[i];
            same_field = g && d_outs[i] && g->field == graphs[0]->field && in->num_fixed >= g->max_fixed && in->num_advice >= g->max_advice && in->num_instance >= g->max_instance &&
                         in->num_challenges >= g->max_challenge;
        }
        if (same_field && ((in->num_fixed && !in->fixed) || (in->num_advice && !in->advice) || (in->num_instance && !in->instance) || (in->num_challenges && !in->challenges))) same_field = false;
        if (!batched || !same_field) {      // (the single-program entry point reports what is wrong with an argument)
            for (uint32_t i = 0; i < count; i++)
                TRY(dehalo_graph_evaluate_device(ctx, graphs[i], in, log_rows, rot_scale, nullptr, d_outs[i], stream));
            return 0;
        }
        const FieldOps* f = field_ops(graphs[0]->field);
        return f ? f->graph_evaluate_batch(ctx, graphs, count, in, log_rows, rot_scale, (fe* const*)d_outs, s) : unknown_field(ctx);
    });
}

int dehalo_permutation_h_device(dehalo_ctx* ctx, int field, const dehalo_perm_inputs* in, uint32_t log_rows, uint32_t rot_scale, uint64_t* d_values,
                                void* stream) {
    if (!in || !d_values || !in->l0 || !in->l_last || !in->l_active_row || !in->beta || !in->gamma || !in->y || !in->delta || !in->beta_zeta || !in->extended_omega)
        return dh_fail(ctx, DEHALO_ERR_INVALID, "permutation_h: null argument");
    if ((in->num_sets && !in->z) || (in->num_columns && (!in->columns || !in->sigma))) return dh_fail(ctx, DEHALO_ERR_INVALID, "permutation_h: null column table");
    if (log_rows == 0 || log_rows > 30 || in->chunk_len == 0 || (uint64_t)in->num_sets * in->chunk_len < in->num_columns)
        return dh_fail(ctx, DEHALO_ERR_INVALID, "permutation_h: sets * chunk_len must cover the columns");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) { return f.perm_h(ctx, in, log_rows, rot_scale, (fe*)d_values, s); });
}

int dehalo_lookup_h_device(dehalo_ctx* ctx, int field, const dehalo_lookup_inputs* in, uint32_t log_rows, uint32_t rot_scale, uint64_t* d_values,
                           void* stream) {
    if (!in || !d_values || !in->product_coset || !in->permuted_input_coset || !in->permuted_table_coset || !in->table_value || !in->l0 || !in->l_last ||
        !in->l_active_row || !in->beta || !in->gamma || !in->y)
        return dh_fail(ctx, DEHALO_ERR_INVALID, "lookup_h: null argument");
    if (log_rows > 30) return dh_fail(ctx, DEHALO_ERR_INVALID, "lookup_h: log_rows > 30");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) { return f.lookup_h(ctx, in, log_rows, rot_scale, (fe*)d_values, s); });
}

int dehalo_product_terms_device(dehalo_ctx* ctx, int field, const dehalo_product_inputs* in, size_t n, uint64_t* d_num, uint64_t* d_den, size_t stride_elems, void* stream) {
    if (!in || !d_num || !d_den || !in->beta || !in->gamma) return dh_fail(ctx, DEHALO_ERR_INVALID, "product_terms: null argument");
    if (in->num_columns && (!in->columns || !in->sigma || !in->omega_powers || !in->delta || !in->set_factors || in->chunk_len == 0))
        return dh_fail(ctx, DEHALO_ERR_INVALID, "product_terms: incomplete permutation inputs");
    if (in->num_lookups && (!in->compressed_input || !in->compressed_table || !in->permuted_input || !in->permuted_table))
        return dh_fail(ctx, DEHALO_ERR_INVALID, "product_terms: incomplete lookup inputs");
    if (in->num_columns > 256 || in->num_lookups > 256) return dh_fail(ctx, DEHALO_ERR_INVALID, "product_terms: too many columns");
    if (stride_elems < n) return dh_fail(ctx, DEHALO_ERR_INVALID, "product_terms: stride shorter than the columns");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) { return f.product_terms(ctx, in, n, (fe*)d_num, (fe*)d_den, stride_elems, s); });
}

int dehalo_lookup_h_batch_device(dehalo_ctx* ctx, int field, const dehalo_lookup_inputs* in, uint32_t count, uint32_t log_rows, uint32_t rot_scale,
                                 uint64_t* d_values, void* stream) {
    if (!in || !d_values || count == 0) return dh_fail(ctx, DEHALO_ERR_INVALID, "lookup_h_batch: null argument");
    if (count > 8) return dh_fail(ctx, DEHALO_ERR_INVALID, "lookup_h_batch: more than 8 lookups in one call");
    for (uint32_t l = 0; l < count; l++) {
        const dehalo_lookup_inputs& q = in[l];
        if (!q.product_coset || !q.permuted_input_coset || !q.permuted_table_coset || !q.table_value || !q.l0 || !q.l_last || !q.l_active_row || !q.beta ||
            !q.gamma || !q.y)
            return dh_fail(ctx, DEHALO_ERR_INVALID, "lookup_h_batch: null argument");
        if (q.l0 != in[0].l0 || q.l_last != in[0].l_last || q.l_active_row != in[0].l_active_row || q.form_flags != in[0].form_flags ||
            memcmp(q.beta, in[0].beta, 32) || memcmp(q.gamma, in[0].gamma, 32) || memcmp(q.y, in[0].y, 32))
            return dh_fail(ctx, DEHALO_ERR_INVALID, "lookup_h_batch: the lookups of one call share l0 / l_last / l_active_row, the challenges and the form flags");
    }
    if (log_rows > 30) return dh_fail(ctx, DEHALO_ERR_INVALID, "lookup_h: log_rows > 30");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) { return f.lookup_h_batch(ctx, in, count, log_rows, rot_scale, (fe*)d_values, s); });
}

int dehalo_shuffle_h_batch_device(dehalo_ctx* ctx, int field, const dehalo_shuffle_inputs* in, uint32_t count, uint32_t log_rows, uint32_t rot_scale,
                                  uint64_t* d_values, void* stream) {
    if (!in || !d_values || count == 0) return dh_fail(ctx, DEHALO_ERR_INVALID, "shuffle_h_batch: null argument");
    if (count > 8) return dh_fail(ctx, DEHALO_ERR_INVALID, "shuffle_h_batch: more than 8 shuffles in one call");
    for (uint32_t j = 0; j < count; j++) {
        const dehalo_shuffle_inputs& q = in[j];
        if (!q.product_coset || !q.input_value || !q.shuffle_value || !q.l0 || !q.l_last || !q.l_active_row || !q.y)
            return dh_fail(ctx, DEHALO_ERR_INVALID, "shuffle_h_batch: null argument");
        if (q.l0 != in[0].l0 || q.l_last != in[0].l_last || q.l_active_row != in[0].l_active_row || q.form_flags != in[0].form_flags || memcmp(q.y, in[0].y, 32))
            return dh_fail(ctx, DEHALO_ERR_INVALID, "shuffle_h_batch: the shuffles of one call share l0 / l_last / l_active_row, y and the form flags");
    }
    if (log_rows > 30) return dh_fail(ctx, DEHALO_ERR_INVALID, "shuffle_h_batch: log_rows > 30");
    return field_device(ctx, field, stream, [&](const FieldOps& f, hipStream_t s) { return f.shuffle_h_batch(ctx, in, count, log_rows, rot_scale, (fe*)d_values, s); });
}

// ---- measurement ------------------------------------------------------------------------------
int dehalo_timing_enable(dehalo_ctx* ctx, int on) {
    if (!ctx) return DEHALO_ERR_INVALID;
    return dh_guard(ctx, [&]() -> int {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        ctx->timing = on != 0;
        return 0;
    });
}

static int timing_collect(dehalo_ctx* ctx) {
    (void)hipSetDevice(ctx->device);
    for (auto& r : ctx->regions) {
        HIP_TRY(ctx, hipEventSynchronize(r.b.get()));
        float ms = 0;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, r.a.get(), r.b.get()));
        ctx->timing_ms[r.kernel_id] += ms;
        ctx->timing_cnt[r.kernel_id] += 1;
    }
    ctx->regions.clear();
    return 0;
}

int dehalo_timing_reset(dehalo_ctx* ctx) {
    if (!ctx) return DEHALO_ERR_INVALID;
    return dh_guard(ctx, [&]() -> int {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        TRY(timing_collect(ctx));
        for (int i = 0; i < DEHALO_K_COUNT; i++) { ctx->timing_ms[i] = 0; ctx->timing_cnt[i] = 0; }
        return 0;
    });
}

int dehalo_timing_get(dehalo_ctx* ctx, int kernel_id, double* total_ms, uint64_t* count) {
    if (!ctx || kernel_id < 0 || kernel_id >= DEHALO_K_COUNT || !total_ms || !count) return DEHALO_ERR_INVALID;
    return dh_guard(ctx, [&]() -> int {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        TRY(timing_collect(ctx));
        *total_ms = ctx->timing_ms[kernel_id];
        *count = ctx->timing_cnt[kernel_id];
        return 0;
    });
}

int dehalo_msm_last_shape(dehalo_ctx* ctx, uint32_t out[6]) {
    if (!ctx || !out) return DEHALO_ERR_INVALID;
    return dh_guard(ctx, [&]() -> int {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        memset(out, 0, 6 * sizeof(uint32_t));
        if (!ctx->ws_counters.p) return 0;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
        uint32_t raw[10];      // eight merge-class counters (k_msm_merge_classify2: 2 | 3-4 | 5-8 | 9-64 | 65-512 records, parts of heavy buckets, heavy buckets, unused), L0, M
        HIP_TRY(ctx, hipMemcpy(raw, ctx->ws_counters.p, sizeof(raw), hipMemcpyDeviceToHost));
        out[0] = raw[0] + raw[1] + raw[2]; out[1] = raw[3]; out[2] = raw[4]; out[3] = raw[6]; out[4] = raw[8]; out[5] = raw[9];      // light (2-8 records) | 9-64 | 65-512 | > 512
        return 0;
    });
}

}  // extern "C"

// A checking program (check.cuh k_graph_check): calculation i with root_of[i] != 0xffffffff is root root_of[i] -- its value is tested, not kept.
int dh_graph_create_roots(dehalo_ctx* ctx, int field, const uint64_t* constants, uint32_t num_constants, const int32_t* rotations, uint32_t num_rotations,
                          const dehalo_calculation* calcs, uint32_t num_calcs, const dehalo_source* horner_parts, uint32_t num_horner_parts, uint32_t num_intermediates,
                          const uint32_t* root_of, uint32_t num_roots, dehalo_graph** out) {
    if (ctx && num_calcs && !root_of) return dh_fail(ctx, DEHALO_ERR_INVALID, "graph_create: null root table");
    return graph_create_impl(ctx, field, constants, num_constants, rotations, num_rotations, calcs, num_calcs, horner_parts, num_horner_parts, num_intermediates, root_of,
                             num_roots, out);
}
