// internal.hpp -- host-side state shared by the translation units of libdehalo.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dehalo.h"
#include "ec.cuh"
#include "experiment_env.hpp"
#include "guard.hpp"
#include "owners.hpp"

using DevMem = DevArray<fe>;

// Two library-owned page-locked chunks per context: every byte that travels between CALLER memory and the device either goes through them (a host memcpy
// on one side, a DMA on the other) or moves by DMA from / to pages that are page-locked for the duration of the call (HostPin, or locked by the caller).
// The HIP runtime's own handling of large pageable transfers -- it pins the caller's pages in place and keeps the registration in a small cache keyed by
// (address, size) after the copy -- is never reached from this library: the device then never holds a mapping of caller memory whose lifetime the
// library does not control ("the memory fault").
struct HostStage {
    static constexpr size_t CHUNK = 4u << 20;
    static constexpr size_t DIRECT_MAX = 64u << 10;      // below this the runtime copies through its own staging buffer (a host memcpy): nothing is pinned
    std::mutex mu;
    Pinned<void> buf[2];
    Event ev[2];
    bool busy[2] = {false, false};
};

struct TwiddleEntry {
    int field;
    uint32_t log_n;
    int form;  // 0: standard Montgomery (R = 2^256)
    uint64_t omega[4];
    uint64_t len;   // powers held: N (full table) or N / 2
    DevMem tw;
};

struct TimedRegion {
    int kernel_id;
    Event a, b;
};

struct dehalo_ctx {
    int device = 0;
    int num_cus = 256;
    Stream stream;             // declared in front of everything that was used on it: members go in reverse order, so the stream is destroyed last
    std::string err;           // guarded by err_mu (written on error paths of any thread, with or without mu held)
    std::mutex err_mu;
    std::recursive_mutex mu;   // recursive: host-buffer entry points hold it across their device-form calls
    // workspace (grow-only)
    DevBuf ws_scalars, ws_out, ws_count, ws_counters, ws_off, ws_records, ws_merge_lists, ws_merge_parts, ws_bhist, ws_pcount, ws_pairs, ws_bsum, ws_idx, ws_partial0, ws_buckets,
        ws_contrib, ws_tree, ws_bred_cnt, ws_gsums, ws_ntt_scratch, ws_ntt_io, ws_ntt_io2, ws_fop[3], ws_tmp_bases, ws_poly[5], ws_poly_io[3], ws_evh[4], ws_lookup, ws_gfft, ws_check[3], ws_codec, ws_ipa_s, ws_verify[2], ws_segments[4];
    std::vector<TwiddleEntry> twiddles;
    affine_t* msm_affine_out = nullptr;   // set for the duration of dehalo_msm_device_affine (under mu): k_msm_final also writes affine points
    int msm_acc_points = 48; // > 0: the accumulation's grid is 4, 6, 8, ... layers of one wave per SIMD, the fewest that leave a lane <= this many
                             // points (2^20 x 16: 6 layers of 43; four dense 2^17 columns: 4 of 34, where whole rounds of 3 waves gave one round of 46
                             // on three quarters of the wave slots -- k = 17 proof 12.6 -> 12.05 ms); 0: rounds of msm_acc_waves waves per SIMD
    int msm_acc_waves = 3;   // sizes the accumulation's points per lane (dehalo_ctx_set_tuning): 3 -> 43 points per lane at 2^20 x 16, ~1.5
                             // rounds of the 4 waves per SIMD that are resident; measured best (one round of 86 points at 3 resident waves: 1.30 ms)
    int host_wait_spin_us = 400; // > 0: a host wait for this context's stream polls hipStreamQuery for up to this many microseconds before it blocks (dh_stream_wait;
                               // dehalo_ctx_set_tuning "host_wait_spin_us" / DEHALO_HOST_SPIN_US): the runtime's blocking wait wakes the thread ~15 us after the stream
                               // drained -- five waits of a K = 11 proof: 1.73 -> 1.65 ms; waits longer than this (a k = 17 commitment) block as before, where it was measured to make no difference
    int msm_acc_min_layers = 4; // the fewest layers of one wave per SIMD the accumulation's grid has (msm_acc_points > 0): 2 .. 4 (DEHALO_MSM_ACC_MIN_LAYERS)
    int msm_sort_block = 1024; // threads per workgroup of the sort's two scalar-decoding kernels: 1024 (128 / 115 KiB of LDS, a CU to itself) or 512 (64 / 58 KiB: shares a CU with an NTT
                               // tile / the tails of another context -- measured 2.3 % SLOWER in the step and equal in the proofs, profiles/r06_sort_block_ab.txt) (dehalo_ctx_set_tuning)
    int msm_acc_block = 128; // threads per block of k_msm_accum0: 128, or 768 = one 12-wave block per CU (3 waves per SIMD; dehalo_ctx_set_tuning / DEHALO_MSM_ACC_BLOCK)
    int ntt_full_table_log = 0;    // transforms up to this size keep all N twiddles (32 B x N; one load per inter-pass twiddle), larger ones N / 2 and a
                                   // negation.  Measured equal at 23 x 2^19 with warm clocks (1.19 ms either way: the negation hides behind the load), so
                                   // the default keeps the smaller table
    HostStage stage;
    bool timing = false;
    std::vector<TimedRegion> regions;
    double timing_ms[DEHALO_K_COUNT] = {};
    uint64_t timing_cnt[DEHALO_K_COUNT] = {};
};

struct dehalo_bases {
    int curve;
    size_t n;
    uint32_t c, W;
    int precomp;
    DevArray<affine_t> table;  // n * (precomp ? W : 1) affine points in HBM, internal (R' = 2^261) canonical form
};

struct dehalo_fixed_base {
    int curve;
    DevArray<affine_t> table;  // T[w][d] = [d 2^(8 w)] P: 32 x 256 affine points, internal (R' = 2^261) canonical form, all zero for d = 0 and for P the identity
};

// never throws, so that argument checks may run in front of an entry point's guard: a message that cannot be stored is dropped
inline int dh_fail(dehalo_ctx* ctx, int code, const char* msg) noexcept {
    if (ctx) try {
        std::lock_guard<std::mutex> lk(ctx->err_mu);
        ctx->err = msg;
    } catch (...) {}
    return code;
}
inline int dh_fail(dehalo_ctx* ctx, int code, const std::string& msg) noexcept { return dh_fail(ctx, code, msg.c_str()); }

// the guard of a C entry point (guard.hpp) with the context whose last error receives the message
template <class Body>
int dh_guard(dehalo_ctx* ctx, Body&& body) noexcept {
    return dh_guard_noting([ctx](const char* msg) { dh_fail(ctx, DEHALO_ERR_INVALID, msg); }, body);
}

inline hipStream_t pick_stream(dehalo_ctx* ctx, void* stream) { return stream ? (hipStream_t)stream : ctx->stream.get(); }
inline hipStream_t dh_ctx_stream(dehalo_ctx* ctx) { return ctx->stream.get(); }

// a device-form entry point: guarded, under the context's lock, on its device, body(stream) on the caller's stream or the context's
template <class Body>
int dh_device(dehalo_ctx* ctx, void* stream, Body&& body) noexcept {
    if (!ctx) return DEHALO_ERR_INVALID;
    return dh_guard(ctx, [&]() -> int {
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        return body(pick_stream(ctx, stream));
    });
}

// hipFuncAttributeMaxDynamicSharedMemorySize of a kernel on the context's device: set once per (device, kernel) and only ever raised --
// the call costs microseconds, and every MSM / NTT / graph launch used to make it
inline hipError_t dh_func_lds(dehalo_ctx* ctx, const void* fn, int bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, int> have;
    std::lock_guard<std::mutex> lk(mu);
    int& cur = have[std::make_pair(ctx->device, fn)];
    if (cur >= bytes) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) cur = bytes;
    return e;
}

inline int dh_ensure(dehalo_ctx* ctx, DevBuf& b, size_t bytes) { return b.ensure(ctx, bytes); }

inline bool dh_host_locked(const void* ptr, size_t bytes) {
    {
        HostPinRegistry& reg = host_pin_registry();
        std::lock_guard<std::mutex> lk(reg.mu);
        const uintptr_t a = (uintptr_t)ptr, b = a + bytes;
        for (auto& e : reg.entries)
            if (e.a <= a && b <= e.b) return true;
    }
    hipPointerAttribute_t at;      // page-locked by the caller (hipHostMalloc / hipHostRegister / torch's pin_memory)
    if (hipPointerGetAttributes(&at, ptr) == hipSuccess) return at.type == hipMemoryTypeHost;
    (void)hipGetLastError();       // an ordinary pageable pointer is reported as an error by some runtime versions
    return false;
}

inline int dh_stage_init(dehalo_ctx* ctx) {
    HostStage& st = ctx->stage;
    for (int i = 0; i < 2; i++) {
        if (!st.buf[i]) HIP_TRY(ctx, make_pinned(st.buf[i], HostStage::CHUNK));
        if (!st.ev[i]) HIP_TRY(ctx, make_event(st.ev[i], hipEventDisableTiming));
    }
    return 0;
}

// host -> device from CALLER memory, queued on `s`.  On return the source has been read in full unless it is page-locked (then the copy is an ordinary
// asynchronous DMA from it and the caller's pin / the caller itself keeps the pages until `s` has been synchronised, as before).
inline int dh_h2d(dehalo_ctx* ctx, void* d_dst, const void* h_src, size_t bytes, hipStream_t s) {
    if (!bytes) return 0;
    if (bytes <= HostStage::DIRECT_MAX || dh_host_locked(h_src, bytes)) {
        HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, s));
        return 0;
    }
    HostStage& st = ctx->stage;
    std::lock_guard<std::mutex> lk(st.mu);
    TRY(dh_stage_init(ctx));
    int i = 0;
    for (size_t off = 0; off < bytes; off += HostStage::CHUNK, i ^= 1) {
        const size_t len = std::min(HostStage::CHUNK, bytes - off);
        if (st.busy[i]) { HIP_TRY(ctx, hipEventSynchronize(st.ev[i].get())); st.busy[i] = false; }
        memcpy(st.buf[i].get(), (const char*)h_src + off, len);
        HIP_TRY(ctx, hipMemcpyAsync((char*)d_dst + off, st.buf[i].get(), len, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipEventRecord(st.ev[i].get(), s));
        st.busy[i] = true;
    }
    return 0;
}

// device -> host into CALLER memory, behind everything queued on `s`; synchronous: the data is in h_dst when this returns
// Host wait for a stream.  With host_wait_spin_us set the thread first polls (a transcript round trip of the prover: the few commitments of a phase come back and
// the next phase's launches wait for the challenge hashed from them -- five to seven such waits a proof), then blocks as hipStreamSynchronize always does.
inline hipError_t dh_stream_wait(dehalo_ctx* ctx, hipStream_t s) {
    if (ctx->host_wait_spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t q = hipStreamQuery(s);
            if (q != hipErrorNotReady) return q;
#if defined(__x86_64__) || defined(__i386__)
            for (int i = 0; i < 64; i++) __builtin_ia32_pause();
#else
            std::this_thread::yield();
#endif
            if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() >= ctx->host_wait_spin_us) break;
        }
    }
    return hipStreamSynchronize(s);
}

inline int dh_d2h(dehalo_ctx* ctx, void* h_dst, const void* d_src, size_t bytes, hipStream_t s) {
    if (!bytes) { HIP_TRY(ctx, dh_stream_wait(ctx, s)); return 0; }
    if (bytes <= HostStage::DIRECT_MAX || dh_host_locked(h_dst, bytes)) {
        HIP_TRY(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, dh_stream_wait(ctx, s));
        return 0;
    }
    HostStage& st = ctx->stage;
    std::lock_guard<std::mutex> lk(st.mu);
    TRY(dh_stage_init(ctx));
    for (int i = 0; i < 2; i++)
        if (st.busy[i]) { HIP_TRY(ctx, hipEventSynchronize(st.ev[i].get())); st.busy[i] = false; }
    int i = 0;
    size_t prev_off = 0, prev_len = 0;
    for (size_t off = 0; off < bytes; off += HostStage::CHUNK, i ^= 1) {
        const size_t len = std::min(HostStage::CHUNK, bytes - off);
        HIP_TRY(ctx, hipMemcpyAsync(st.buf[i].get(), (const char*)d_src + off, len, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipEventRecord(st.ev[i].get(), s));
        if (prev_len) {      // the previous chunk lands in the other buffer: hand it to the caller while this one is in flight
            HIP_TRY(ctx, hipEventSynchronize(st.ev[i ^ 1].get()));
            memcpy((char*)h_dst + prev_off, st.buf[i ^ 1].get(), prev_len);
        }
        prev_off = off; prev_len = len;
    }
    HIP_TRY(ctx, hipEventSynchronize(st.ev[i ^ 1].get()));
    memcpy((char*)h_dst + prev_off, st.buf[i ^ 1].get(), prev_len);
    return 0;
}

// the limit of a precomputed table registered with window_bits = 0: n x windows < 2^30 (capi.hip)
bool dh_precomputed_table_fits(int curve, size_t n);

// DEHALO_CO_LDS (bytes; experiments with co-resident contexts): every latency-bound kernel that is meant to run in the wave slot a
// 768-thread accumulation block leaves free asks for at least this much LDS per block in all (its own + unused padding), so that no two such blocks
// fit one compute unit (> 80 KB of the 160) and the accumulation's next block always finds its three waves per SIMD.  0 = off.
inline size_t dh_co_lds_pad(size_t own_static, size_t own_dynamic) {
    static const size_t want = [] { const char* e = DH_EXPERIMENT_ENV("DEHALO_CO_LDS"); return e ? (size_t)atol(e) : (size_t)0; }();
    if (want <= own_static + own_dynamic) return own_dynamic;
    return want - own_static;
}
inline int dh_co_lds_attr(dehalo_ctx* ctx, const void* fn, size_t dyn) {
    if (dyn > 48 * 1024) HIP_TRY(ctx, dh_func_lds(ctx, fn, (int)dyn));
    return 0;
}

struct ScopedTimer {
    dehalo_ctx* ctx;
    hipStream_t s;
    int id;
    Event a, b;
    ScopedTimer(dehalo_ctx* c, hipStream_t st, int kid) : ctx(c), s(st), id(kid) {
        if (ctx->timing && make_event(a, hipEventDefault) == hipSuccess && make_event(b, hipEventDefault) == hipSuccess) (void)hipEventRecord(a.get(), s);
    }
    ~ScopedTimer() {
        if (a && b) {
            (void)hipEventRecord(b.get(), s);
            ctx->regions.push_back({id, std::move(a), std::move(b)});
        }
    }
};

inline fe fe_from_u64(const uint64_t v[4]) {
    fe r;
    for (int i = 0; i < 4; i++) {
        r.v[2 * i] = (u32)v[i];
        r.v[2 * i + 1] = (u32)(v[i] >> 32);
    }
    return r;
}

struct NttScale {
    uint32_t pre_mode = 0, post_mode = 0;
    fe pre_z{}, post0{}, post_z{};
    int form_shift = 0;   // +1: emit the internal form (x * 2^261, canonical, packed); -1: the input is in it
};

// per-curve operations, one table per curve (msm_*.hip: make_curve_ops in msm.cuh)
struct CurveOps {
    int (*run_msm)(dehalo_ctx* ctx, const dehalo_bases* bases, const fe* d_scalars, size_t len, size_t batch, jacobian_t* d_out, hipStream_t s);
    int (*build_table)(dehalo_ctx* ctx, dehalo_bases* b, const affine_t* d_std_points, hipStream_t s);
    int (*to_affine)(dehalo_ctx* ctx, const jacobian_t* d_in, affine_t* d_out, uint32_t count, hipStream_t s);
    int (*point_sum)(dehalo_ctx* ctx, const jacobian_t* d_in, uint32_t count, jacobian_t* d_out, hipStream_t s);
    const uint32_t* scalar_modulus;   // r, eight 32-bit words, least significant first
};
// (functions rather than const objects: a const namespace-scope object would also be emitted into the device code, pointing at host functions)
const CurveOps& bn254_curve_ops();
const CurveOps& pallas_curve_ops();
const CurveOps& vesta_curve_ops();
// the IPA opening argument's kernels, one table per Pasta curve (ipa.cuh, instantiated in msm_pallas.hip / msm_vesta.hip)
struct IpaOps {
    // out[i] = g[i] + [u] g[half + i] for i < half; u canonical (4 x u64)
    int (*collapse)(dehalo_ctx* ctx, const affine_t* d_g, uint64_t half, const uint64_t u_canon[4], affine_t* d_out, hipStream_t s);
    // one round's scalar slots of the [G' | U | W] MSM (dehalo_ipa_open)
    int (*slots)(dehalo_ctx* ctx, const fe* d_evals, const uint64_t coef_l[4], const uint64_t coef_r[4], const fe* d_rands, fe* d_sl, fe* d_sr, hipStream_t s);
    // pts[i] <- pts[i] + [blinds[i]] W for i < m: Jacobian points as dehalo_msm_device leaves them, blinds standard Montgomery, all on the device
    int (*blind)(dehalo_ctx* ctx, jacobian_t* d_pts, const fe* d_blinds, const affine_t* d_w, uint64_t m, hipStream_t s);
    // the verifier's scalars over g: out[idx] = sum_i inits[i] prod_{bit j of idx} challenges[i k + k - 1 - j], idx < 2^k; d_tables: ipa_s_table_elems(k, count)
    // elements of workspace (ipa.cuh)
    int (*s_vector)(dehalo_ctx* ctx, const fe* d_challenges, const fe* d_inits, uint32_t count, uint32_t k, fe* d_tables, fe* d_out, hipStream_t s);
};
// the workspace of IpaOps::s_vector in elements, h = ceil(k / 2): count x (2^h + 2^(k - h))
inline size_t ipa_s_table_elems(uint32_t k, size_t count) { const uint32_t h = (k + 1) / 2; return count * (((size_t)1 << h) + ((size_t)1 << (k - h))); }
const IpaOps& pallas_ipa_ops();
const IpaOps& vesta_ipa_ops();
const IpaOps* ipa_ops(int curve);       // capi.hip: null unless Pallas / Vesta
// g_to_lagrange (the group FFT), the point codec (decompress, compress, check) and the generated points, one table per curve (gfft.cuh, instantiated in msm_*.hip)
struct GfftOps {
    // d_out = g_to_lagrange(d_g): 2^k affine points, 1 <= k; d_out == d_g or disjoint; omega_inv standard Montgomery, n_inv canonical (4 x u64 each)
    int (*g_to_lagrange)(dehalo_ctx* ctx, const affine_t* d_g, uint32_t k, const uint64_t omega_inv[4], const uint64_t n_inv_canon[4], affine_t* d_out, hipStream_t s);
    // GroupEncoding::from_bytes of `count` 32-byte encodings (4-byte aligned) into affine points; d_status[0] |= 1 (x >= p) | 2 (not on the curve) | 4 (x = 0, sign set)
    int (*decompress)(dehalo_ctx* ctx, const uint8_t* d_in, affine_t* d_out, uint64_t count, uint32_t* d_status, hipStream_t s);
    // GroupEncoding::to_bytes of `count` affine points into 32-byte encodings (4-byte aligned): the inverse of decompress
    int (*compress)(dehalo_ctx* ctx, const affine_t* d_in, uint8_t* d_out, uint64_t count, hipStream_t s);
    // a checked from_raw_bytes over `count` affine points, read only; d_status[0] |= 1 (a coordinate's word >= p) | 2 (neither on the curve nor (0, 0))
    int (*points_check)(dehalo_ctx* ctx, const affine_t* d_in, uint64_t count, uint32_t* d_status, hipStream_t s);
    // d_out[i] = the point named (curve, key, cha_stream, first + i) by the generated-points rule of include/dehalo.h, i < count; d_status[0] |= 1 (an index used up
    // its attempts and was written as (0, 0))
    int (*points_generate)(dehalo_ctx* ctx, const uint32_t key[8], uint64_t cha_stream, uint64_t first, affine_t* d_out, uint64_t count, uint32_t* d_status, hipStream_t s);
};
const GfftOps& bn254_gfft_ops();
const GfftOps& pallas_gfft_ops();
const GfftOps& vesta_gfft_ops();
const GfftOps* gfft_ops(int curve);     // capi.hip: null for an unknown curve
// fixed-base scalar multiplication over the window table of one point, one table of kernels per curve (fixed_base.cuh, instantiated in msm_*.hip)
struct FixedBaseOps {
    // d_table (32 x 256 entries, packed internal form) from d_base (one affine point, standard Montgomery); d_pows: 32 points of scratch
    int (*build)(dehalo_ctx* ctx, const affine_t* d_base, affine_t* d_pows, affine_t* d_table, hipStream_t s);
    // out[i] = [scalars[i]] P for i < m, affine
    int (*mul)(dehalo_ctx* ctx, const affine_t* d_table, const fe* d_scalars, affine_t* d_out, uint64_t m, hipStream_t s);
    // pts[i] <- pts[i] + [blinds[i]] P for i < m: IpaOps::blind over the table
    int (*blind)(dehalo_ctx* ctx, const affine_t* d_table, jacobian_t* d_pts, const fe* d_blinds, uint64_t m, hipStream_t s);
};
const FixedBaseOps& bn254_fixed_base_ops();
const FixedBaseOps& pallas_fixed_base_ops();
const FixedBaseOps& vesta_fixed_base_ops();
// out[s] = sum over d_offsets[s] <= i < d_offsets[s + 1] of [d_scalars[i]] d_points[i], affine, s < segments: one launch, one function per curve (msm_segments.cuh,
// instantiated in msm_*.hip).  d_offsets: segments + 1 words that do not decrease -- the caller has checked
typedef int (*MsmSegmentsFn)(dehalo_ctx* ctx, const fe* d_scalars, const affine_t* d_points, const uint32_t* d_offsets, uint32_t segments, affine_t* d_out, hipStream_t s);
int msm_segments_bn254(dehalo_ctx* ctx, const fe* d_scalars, const affine_t* d_points, const uint32_t* d_offsets, uint32_t segments, affine_t* d_out, hipStream_t s);
int msm_segments_pallas(dehalo_ctx* ctx, const fe* d_scalars, const affine_t* d_points, const uint32_t* d_offsets, uint32_t segments, affine_t* d_out, hipStream_t s);
int msm_segments_vesta(dehalo_ctx* ctx, const fe* d_scalars, const affine_t* d_points, const uint32_t* d_offsets, uint32_t segments, affine_t* d_out, hipStream_t s);
// A plain (precompute 0) registration whose points are replaced on the stream, without a host wait or an allocation (capi.hip): the IPA rounds'
// shrinking generator vector.  alloc: room for `cap` points, empty; rebuild: n <= cap points from d_points (standard Montgomery), the window
// chosen for n as dehalo_bases_register_device would; queued on s, so the caller may overwrite d_points once later work on s reads the table.
int dh_bases_plain_alloc(dehalo_ctx* ctx, int curve, size_t cap, BasesPtr& out);
int dh_bases_plain_rebuild(dehalo_ctx* ctx, dehalo_bases* b, const affine_t* d_points, size_t n, hipStream_t s);
// ParamsKZG::setup's device half (setup.cuh, instantiated in msm_bn254.hip): g[i] = [s^i] G, g_lagrange[i] = [L_i(s)] G into device memory
int kzg_setup_bn254(dehalo_ctx* ctx, uint32_t k, const uint64_t s[4], const uint64_t omega[4], const uint64_t cfac[4], affine_t* d_g, affine_t* d_gl, hipStream_t st);

// per-field operations, one table per field (ntt_*.hip: make_field_ops in evalh.cuh)
struct dehalo_graph;
struct FieldOps {
    // ntt.cuh
    int (*run_ntt)(dehalo_ctx* ctx, const fe* src, uint64_t src_len, uint64_t src_stride, fe* dst, uint64_t dst_stride, uint32_t log_n, const uint64_t omega[4],
                   size_t batch, const NttScale& sc, hipStream_t s);
    int (*field_op)(dehalo_ctx* ctx, int op, const fe* a, const fe* b, fe* out, uint64_t n, hipStream_t s);
    // field-vector primitives (poly.cuh)
    int (*eval_poly)(dehalo_ctx* ctx, const fe* c, uint64_t len, uint64_t stride, size_t batch, const uint64_t pt[4], fe* out, hipStream_t s);
    int (*eval_poly_multi)(dehalo_ctx* ctx, const fe* const* polys, size_t count, uint64_t len, const uint64_t* pts, uint32_t npts, fe* out, hipStream_t s,
                           const uint8_t* masks);
    int (*eval_poly_points)(dehalo_ctx* ctx, const fe* const* polys, size_t count, uint64_t len, const uint64_t* pts, uint32_t npts, fe* out, hipStream_t s,
                            const uint32_t* masks);
    int (*batch_invert)(dehalo_ctx* ctx, fe* v, uint64_t len, hipStream_t s);
    int (*prefix_product)(dehalo_ctx* ctx, const fe* in, uint64_t len, fe* out, hipStream_t s);
    int (*grand_product)(dehalo_ctx* ctx, const fe* num, const fe* den, uint64_t len, size_t batch, uint64_t stride, fe* z, hipStream_t s);
    int (*lincomb)(dehalo_ctx* ctx, const fe* const* cols, const uint64_t* coefs, size_t count, uint64_t len, fe* out, const uint64_t* sub0, hipStream_t s);
    int (*scale)(dehalo_ctx* ctx, fe* a, uint64_t len, const uint64_t* pattern, uint32_t period, const fe* d_factor, hipStream_t s);
    int (*kate_division)(dehalo_ctx* ctx, const fe* a, uint64_t len, const uint64_t pt[4], fe* q, hipStream_t s);
    int (*kate_division_batch)(dehalo_ctx* ctx, const fe* const* a, uint64_t len, const uint64_t* pts, fe* const* q, size_t count, hipStream_t s);
    // q[y] = a[y] div prod_t (X - z_t) over polynomial y's m[y] points; h_tab: {z, w, z^2048} per point, on the host (capi.hip: the weights w)
    int (*vanishing_quotient_batch)(dehalo_ctx* ctx, const fe* const* a, uint64_t len, const uint64_t* h_tab, const uint32_t* m, fe* const* q, size_t count, hipStream_t s);
    // quotient-numerator kernels (evalh.cuh)
    int (*convert_form)(dehalo_ctx* ctx, const fe* in, fe* out, uint64_t n, int to_internal, hipStream_t s);
    int (*graph_upload)(dehalo_ctx* ctx, dehalo_graph* g, const uint64_t* constants, hipStream_t s);
    int (*graph_evaluate)(dehalo_ctx* ctx, const dehalo_graph* g, const dehalo_eval_inputs* in, uint32_t log_rows, uint32_t rot_scale, const fe* prev, fe* out,
                          hipStream_t s);
    int (*graph_evaluate_batch)(dehalo_ctx* ctx, const dehalo_graph* const* graphs, uint32_t count, const dehalo_eval_inputs* in, uint32_t log_rows,
                                uint32_t rot_scale, fe* const* outs, hipStream_t s);
    int (*perm_h)(dehalo_ctx* ctx, const dehalo_perm_inputs* in, uint32_t log_rows, uint32_t rot_scale, fe* v, hipStream_t s);
    int (*lookup_h)(dehalo_ctx* ctx, const dehalo_lookup_inputs* in, uint32_t log_rows, uint32_t rot_scale, fe* v, hipStream_t s);
    int (*lookup_h_batch)(dehalo_ctx* ctx, const dehalo_lookup_inputs* in, uint32_t count, uint32_t log_rows, uint32_t rot_scale, fe* v, hipStream_t s);
    int (*product_terms)(dehalo_ctx* ctx, const dehalo_product_inputs* in, uint64_t n, fe* num, fe* den, uint64_t stride, hipStream_t s);
    // witness check (check.cuh): bitmap[root][row / 64] bit row % 64 = "root's value is non-zero at row", rows >= usable masked; words = 64-bit words per root
    int (*graph_check)(dehalo_ctx* ctx, const dehalo_graph* g, const dehalo_eval_inputs* in, uint32_t log_rows, uint64_t usable, uint64_t* bitmap, uint64_t words,
                       hipStream_t s);
    // bitmap[row / 64] bit row % 64 = "input[row] (standard form) is none of the n_keys sorted canonical keys", rows >= usable masked; every word of 2^log_rows rows written
    int (*check_member)(dehalo_ctx* ctx, const fe* input, const fe* sorted_keys, uint64_t n_keys, uint32_t log_rows, uint64_t usable, uint64_t* bitmap, hipStream_t s);
    // the shuffle arguments' terms of the quotient numerator (evalh.cuh), count <= 8
    int (*shuffle_h_batch)(dehalo_ctx* ctx, const dehalo_shuffle_inputs* in, uint32_t count, uint32_t log_rows, uint32_t rot_scale, fe* v, hipStream_t s);
    // witness check (check.cuh): bitmap[row / 64] bit row % 64 = "input[row] (standard form) occurs another number of times among the n_keys sorted canonical keys of the
    // inputs than among those of the shuffle side", rows >= usable masked; every word of 2^log_rows rows written
    int (*check_shuffle)(dehalo_ctx* ctx, const fe* input, const fe* sorted_inputs, const fe* sorted_side, uint64_t n_keys, uint32_t log_rows, uint64_t usable,
                         uint64_t* bitmap, hipStream_t s);
    // the scalar codec (scalar_codec.cuh).  from_repr: n 32-byte little-endian integers (4-byte aligned) -> Montgomery words, out == in or disjoint; an integer not
    // below p is written as 0, d_status[0] |= 1 and d_first_bad[0] = min(d_first_bad[0], its index).  check: the same report for stored words not below p; reads only
    int (*scalars_from_repr)(dehalo_ctx* ctx, const uint8_t* in, fe* out, uint64_t n, uint32_t* d_status, uint64_t* d_first_bad, hipStream_t s);
    int (*scalars_check)(dehalo_ctx* ctx, const fe* in, uint64_t n, uint32_t* d_status, uint64_t* d_first_bad, hipStream_t s);
};
const FieldOps* dh_field_ops(int field);      // capi.hip: null for an unknown field
// capi.hip: dehalo_graph_create for a checking program -- calculation i with root_of[i] != 0xffffffff computes root root_of[i] (kept by the copy propagation)
int dh_graph_create_roots(dehalo_ctx* ctx, int field, const uint64_t* constants, uint32_t num_constants, const int32_t* rotations, uint32_t num_rotations,
                          const dehalo_calculation* calcs, uint32_t num_calcs, const dehalo_source* horner_parts, uint32_t num_horner_parts, uint32_t num_intermediates,
                          const uint32_t* root_of, uint32_t num_roots, dehalo_graph** out);
const FieldOps& bn254_fr_field_ops();
const FieldOps& bn254_fq_field_ops();
const FieldOps& pasta_fp_field_ops();
const FieldOps& pasta_fq_field_ops();

// lookup_permute.hip
int lookup_permute_impl(dehalo_ctx* ctx, int field, const fe* d_inputs, const fe* d_tables, uint64_t n, size_t batch, uint64_t stride, fe* d_out_inputs,
                        fe* d_out_tables, hipStream_t s);

// per lookup of a call (null array: none): its table as distinct rows -- representative row indices and multiplicities on the device, their number (0 or more
// than 2048: the general path); lookups that share a table carry the same arrays
struct LookupDistinct { const uint32_t* d_rep_rows; const uint32_t* d_mult; uint32_t count; };
int lookup_permute_ptrs(dehalo_ctx* ctx, int field, const fe* const* d_inputs, const fe* const* d_tables, uint64_t n, size_t batch, fe* const* d_out_inputs,
                        fe* const* d_out_tables, hipStream_t s, int* d_status = nullptr, const LookupDistinct* distinct = nullptr);
// The first n values of `count` <= 16 table columns (standard form) as canonical keys sorted ascending (the tile sort and merge passes of the permutation), in the
// context's lookup workspace: column t at *d_sorted + t * *npad, padded to whole tiles with all-ones keys.  Valid until the next call that uses that workspace.
int lookup_sort_tables(dehalo_ctx* ctx, int field, const fe* const* d_tables, uint32_t count, uint64_t n, const fe** d_sorted, uint64_t* npad, hipStream_t s);
