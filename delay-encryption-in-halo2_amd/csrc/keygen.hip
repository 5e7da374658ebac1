// keygen.hip -- the keys behind the C ABI: keygen_vk / keygen_pk, ProvingKey / VerifyingKey RawBytes and the verifying key's transcript representation
// [UPSTREAM halo2_proofs @ v2023_04_20: plonk/keygen.rs, plonk.rs, plonk/permutation/keygen.rs] -- the calls the reference makes at
// benches/delay_enc.rs:84-115 (keys).
// C entry points run under dh_guard and the column work goes through the library's device entry points, as in prover.hip; the one kernel here is a gather.
#include <memory>

#include "key_format.hpp"
#include "whole_call.hpp"

namespace {

__global__ void k_gather_elems(const fe* __restrict__ src, const uint64_t* __restrict__ idx, fe* __restrict__ dst, uint64_t count) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = src[idx[i]];
}

// what the circuit fixes of a key's shape (key_format.hpp)
KeyShape key_shape(const dehalo_pk* pk) {
    KeyShape sh;
    sh.nf = pk->cs.num_fixed; sh.npc = pk->cs.perm_cols.size(); sh.nsel = pk->num_selectors; sh.ext_shift = pk->dom.extended_k - pk->dom.k;
    return sh;
}

int pk_common_init(dehalo_ctx* ctx, int curve, const dehalo_constraint_system* csd, uint32_t k, dehalo_pk* pk) {
    pk->ctx = ctx;
    pk->curve = curve;
    pk->k = k;
    pk->f = host_field(curve_scalar_field(curve));
    if (!pk->f) return dh_fail(ctx, DEHALO_ERR_INVALID, "unknown curve");
    const std::string err = pk->cs.load(csd);
    if (!err.empty()) return dh_fail(ctx, pk->cs.unsupported ? DEHALO_ERR_UNSUPPORTED : DEHALO_ERR_INVALID, err);
    if (k > 28 || !pk->dom.init(pk->f, pk->cs.degree(), k)) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "extended_k exceeds the field's two-adicity");
    if (pk->dom.n < (size_t)pk->cs.blinding_factors() + 3) return dh_fail(ctx, DEHALO_ERR_INVALID, "not enough rows available");      // Error::NotEnoughRowsAvailable
    return 0;
}

// values (cnt x n, standard form, device) -> polys (lagrange_to_coeff), cosets (coeff_to_extended, internal form), commitments to the host
int lagrange_to_all(dehalo_pk* pk, const dehalo_params* params, const fe* values, size_t cnt, fe* polys, fe* cosets, uint64_t* commitments_host) {
    dehalo_ctx* ctx = pk->ctx;
    if (!cnt) return 0;
    const HostDomain& d = pk->dom;
    DevMem aff, jac, bl;
    if (commitments_host) {
        TRY(aff.alloc(ctx, 2 * cnt, false));
        if (params->scheme == DEHALO_SCHEME_IPA) {      // commit_lagrange(values, Blind::default()): MSM + [default blind] W
            const Fe b = pk->f->from_u64(IPA_DEFAULT_BLIND);
            std::vector<Fe> bh(cnt, b);
            TRY(jac.alloc(ctx, 3 * cnt, false));
            TRY(bl.alloc(ctx, cnt, false));
            TRY(dehalo_upload(ctx, bh.data(), cnt * 32, bl.p));
            TRY(dehalo_msm_device(ctx, params->bases_gl.get(), (const uint64_t*)values, d.n, cnt, jac.u64(), nullptr));
            TRY(dehalo_fixed_base_blind_device(ctx, params->fb_w.get(), jac.u64(), bl.u64(), cnt, nullptr));
            TRY(dehalo_to_affine_device(ctx, params->curve, jac.u64(), cnt, aff.u64(), nullptr));
        } else TRY(dehalo_msm_device_affine(ctx, params->bases_gl.get(), (const uint64_t*)values, d.n, cnt, nullptr, aff.u64(), nullptr));
    }
    TRY(dehalo_lagrange_to_coeff_device(ctx, pk->f->id, (const uint64_t*)values, (uint64_t*)polys, d.k, d.omega_inv.v, d.ifft_divisor.v, cnt, nullptr));
    TRY(dehalo_coset_ntt_form_device(ctx, pk->f->id, (const uint64_t*)polys, d.k, (uint64_t*)cosets, d.extended_k, d.ext_omega.v, d.g_coset.v, cnt, DEHALO_FORM_OUT_INTERNAL,
                                     nullptr));
    if (commitments_host) TRY(dehalo_download(ctx, aff.p, cnt * 64, commitments_host));
    else TRY(dehalo_ctx_synchronize(ctx));
    return 0;
}

}   // namespace

// the RawBytes sizes are key_format.hpp's layout (0 only for a key without a domain)
size_t dehalo_pk::vk_size() const {
    KeyLayout L;
    return key_layout(DEHALO_SERDE_RAW_BYTES, k, key_shape(this), L) ? L.vk_size : 0;
}
void dehalo_pk::vk_write(uint8_t* o) const {
    key_put_u32_be(o, k);
    key_put_u32_be(o + 4, cs.num_fixed);
    o += 8;
    memcpy(o, fixed_commitments.data(), 64 * (size_t)cs.num_fixed);
    o += 64 * (size_t)cs.num_fixed;
    memcpy(o, perm_commitments.data(), 64 * cs.perm_cols.size());
    o += 64 * cs.perm_cols.size();
    for (auto& s : selectors) {
        memcpy(o, s.data(), s.size());
        o += s.size();
    }
}
size_t dehalo_pk::size() const {
    KeyLayout L;
    return key_layout(DEHALO_SERDE_RAW_BYTES, k, key_shape(this), L) ? L.pk_size : 0;
}
void dehalo_pk::default_transcript_repr() { transcript_repr = substitute_transcript_repr(f, k, cs, fixed_commitments, perm_commitments, selectors); }      // (plonk_host.hpp)
int dehalo_pk::compile_graphs() {
    TRY(custom_gates_graph(cs, f).compile(ctx, adopt(ctx, custom_gates)));
    for (auto& lk : cs.lookups) {
        GraphPtr g, gi, gt;
        TRY(lookup_table_value_graph(cs, lk, f).compile(ctx, adopt(ctx, g)));
        lookup_graphs.push_back(std::move(g));
        TRY(compress_graph(cs, lk.inputs, f).compile(ctx, adopt(ctx, gi)));
        TRY(compress_graph(cs, lk.tables, f).compile(ctx, adopt(ctx, gt)));
        compress_graphs.emplace_back(std::move(gi), std::move(gt));
    }
    for (auto& sf : cs.shuffles) {
        GraphPtr gi, gs;
        TRY(shuffle_side_graph(cs, sf.inputs, f).compile(ctx, adopt(ctx, gi)));
        TRY(shuffle_side_graph(cs, sf.tables, f).compile(ctx, adopt(ctx, gs)));
        shuffle_graphs.emplace_back(std::move(gi), std::move(gs));
    }
    const GateCheckProgram chk = gate_check_graph(cs, f);
    TRY(chk.g.compile(ctx, adopt(ctx, check_gates), &chk.root_of, (uint32_t)cs.gates.size()));
    return 0;
}

// (n, 4) device column of omega^i: the forward NTT of the unit vector e_1
int omega_powers(dehalo_ctx* ctx, const HostDomain& d, fe* col) {
    HIP_TRY(ctx, hipMemsetAsync(col, 0, d.n * sizeof(fe), ctx->stream.get()));
    TRY(dh_h2d(ctx, col + (d.n > 1 ? 1 : 0), d.f->one.v, 32, ctx->stream.get()));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));      // (the source is a host object: copied before returning)
    if (d.n > 1) TRY(dehalo_ntt_device(ctx, d.f->id, (uint64_t*)col, d.k, d.omega.v, 1, nullptr));
    return 0;
}

namespace {

// what a verifying key that already exists gives keygen_pk: its commitments (Montgomery affine, validated as its format asked) and its packed selectors
struct VkParts {
    std::vector<uint64_t> fixed_commitments, perm_commitments;
    std::vector<std::vector<uint8_t>> selectors;
};

// keygen_vk + keygen_pk (vk null: the commitments are computed, the selectors packed from the caller's), or keygen_pk under `vk` (the commitments and the packed
// selectors are the vk's; no MSM is launched); pk comes initialised (pk_common_init)
int keygen_body(dehalo_ctx* ctx, const dehalo_params* params, const uint64_t* fixed, const uint64_t* mapping, const uint8_t* const* selectors, uint32_t num_selectors,
                uint32_t flags, VkParts* vk, std::unique_ptr<dehalo_pk>& pk) {
    const HostCS& cs = pk->cs;
    const HostDomain& d = pk->dom;
    const size_t n = d.n, m = d.m, nf = cs.num_fixed, npc = cs.perm_cols.size();
    if ((nf && !fixed) || (npc && !mapping) || (!vk && num_selectors && !selectors)) return dh_fail(ctx, DEHALO_ERR_INVALID, "keygen: null column data");
    const int fid = pk->f->id;
    // fixed columns
    TRY(pk->fixed_values.alloc(ctx, nf * n, false));
    TRY(pk->fixed_polys.alloc(ctx, nf * n, false));
    TRY(pk->fixed_cosets.alloc(ctx, nf * m, false));
    pk->fixed_commitments.assign(8 * nf, 0);
    if (nf) {
        HostPin pin_fixed(fixed, nf * n * 32);
        TRY(dh_h2d(ctx, pk->fixed_values.p, fixed, nf * n * 32, ctx->stream.get()));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
        if (flags & DEHALO_KEYGEN_FIXED_CANONICAL) TRY(dehalo_field_op_device(ctx, fid, 4, pk->fixed_values.u64(), nullptr, pk->fixed_values.u64(), nf * n, nullptr));
        TRY(lagrange_to_all(pk.get(), params, pk->fixed_values.p, nf, pk->fixed_polys.p, pk->fixed_cosets.p, vk ? nullptr : pk->fixed_commitments.data()));
    }
    // permutation: sigma_j(omega^i) = delta^(column of the mapped cell) * omega^(its row)  [permutation::keygen::Assembly::build_pk]
    TRY(pk->perm_values.alloc(ctx, npc * n, false));
    TRY(pk->perm_polys.alloc(ctx, npc * n, false));
    TRY(pk->perm_cosets.alloc(ctx, npc * m, false));
    pk->perm_commitments.assign(8 * npc, 0);
    if (npc) {
        for (size_t i = 0; i < npc * n; i++)
            if (mapping[i] >= npc * n) return dh_fail(ctx, DEHALO_ERR_INVALID, "keygen: permutation mapping points outside the permutation's columns");
        DevMem ident, w;
        DevArray<uint64_t> d_map;
        TRY(ident.alloc(ctx, npc * n, false));
        TRY(w.alloc(ctx, n, false));
        TRY(omega_powers(ctx, d, w.p));
        Fe dj = pk->f->one;
        for (size_t j = 0; j < npc; j++) {
            HIP_TRY(ctx, hipMemcpyAsync(ident.at(j * n), w.p, n * sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream.get()));
            if (j) TRY(dehalo_scale_device(ctx, fid, ident.u64(j * n), n, dj.v, 1, nullptr, nullptr));
            dj = pk->f->mul(dj, pk->f->delta);
        }
        TRY(d_map.alloc(ctx, npc * n, false));
        HostPin pin_map(mapping, npc * n * 8);
        TRY(dh_h2d(ctx, d_map.p, mapping, npc * n * 8, ctx->stream.get()));
        k_gather_elems<<<(unsigned)((npc * n + 255) / 256), 256, 0, ctx->stream.get()>>>(ident.p, d_map.p, pk->perm_values.p, npc * n);
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
        TRY(lagrange_to_all(pk.get(), params, pk->perm_values.p, npc, pk->perm_polys.p, pk->perm_cosets.p, vk ? nullptr : pk->perm_commitments.data()));
    }
    // l0, l_last, l_active_row = 1 - (l_last + l_blind) over the extended domain
    {
        const size_t u = n - (cs.blinding_factors() + 1);
        std::vector<Fe> lag(3 * n, Fe{{0, 0, 0, 0}});
        lag[0] = pk->f->one;
        lag[n + u] = pk->f->one;
        for (size_t i = 0; i < u; i++) lag[2 * n + i] = pk->f->one;
        DevMem vals, polys;
        TRY(vals.alloc(ctx, 3 * n, false));
        TRY(polys.alloc(ctx, 3 * n, false));
        TRY(pk->l_ext.alloc(ctx, 3 * m, false));
        HostPin pin_lag(lag.data(), 3 * n * 32);
        TRY(dh_h2d(ctx, vals.p, lag.data(), 3 * n * 32, ctx->stream.get()));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
        TRY(lagrange_to_all(pk.get(), params, vals.p, 3, polys.p, pk->l_ext.p, nullptr));
    }
    pk->num_selectors = num_selectors;
    if (vk) {
        pk->fixed_commitments = std::move(vk->fixed_commitments);
        pk->perm_commitments = std::move(vk->perm_commitments);
        pk->selectors = std::move(vk->selectors);
    } else
        for (uint32_t s = 0; s < num_selectors; s++) {
            if (!selectors[s]) return dh_fail(ctx, DEHALO_ERR_INVALID, "keygen: null selector");
            std::vector<uint8_t> packed((n + 7) / 8, 0);
            for (size_t i = 0; i < n; i++)
                if (selectors[s][i]) packed[i >> 3] |= (uint8_t)(1u << (i & 7));
            pk->selectors.push_back(std::move(packed));
        }
    pk->default_transcript_repr();
    TRY(pk->compile_graphs());
    TRY(dehalo_ctx_synchronize(ctx));
    return 0;
}

}   // namespace

extern "C" int dehalo_keygen(dehalo_ctx* ctx, const dehalo_params* params, const dehalo_constraint_system* csd, const uint64_t* fixed, const uint64_t* mapping,
                             const uint8_t* const* selectors, uint32_t num_selectors, uint32_t flags, dehalo_pk** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !params || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "keygen: null argument");
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        std::unique_ptr<dehalo_pk> pk(new dehalo_pk);
        TRY(pk_common_init(ctx, params->curve, csd, params->k, pk.get()));
        TRY(keygen_body(ctx, params, fixed, mapping, selectors, num_selectors, flags, nullptr, pk));
        *out = pk.release();
        return 0;
    });
}

extern "C" size_t dehalo_pk_size(const dehalo_pk* pk) { return pk ? pk->size() : 0; }
extern "C" size_t dehalo_vk_size(const dehalo_pk* pk) { return pk ? pk->vk_size() : 0; }
extern "C" int dehalo_vk_write(const dehalo_pk* pk, uint8_t* out, size_t cap) {
    return dh_guard(pk ? pk->ctx : nullptr, [&]() -> int {
        if (!pk || !out) return DEHALO_ERR_INVALID;
        if (cap < pk->vk_size()) return dh_fail(pk->ctx, DEHALO_ERR_INVALID, "vk_write: buffer too small");
        pk->vk_write(out);
        return 0;
    });
}

extern "C" int dehalo_pk_write(dehalo_ctx* ctx, const dehalo_pk* pk, uint8_t* out, size_t cap) {
    return dh_guard(ctx ? ctx : pk ? pk->ctx : nullptr, [&]() -> int {
        if (!pk || !out) return DEHALO_ERR_INVALID;
        if (!ctx) ctx = pk->ctx;
        if (cap < pk->size()) return dh_fail(ctx, DEHALO_ERR_INVALID, "pk_write: buffer too small");
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        const size_t n = pk->dom.n, m = pk->dom.m, nf = pk->cs.num_fixed, npc = pk->cs.perm_cols.size();
        pk->vk_write(out);
        uint8_t* o = out + pk->vk_size();
        DevMem tmp;      // extended-domain columns leave in upstream's standard form
        TRY(tmp.alloc(ctx, m, false));
        auto poly = [&](const fe* src, size_t len, bool internal) -> int {
            key_put_u32_be(o, (uint32_t)len);
            o += 4;
            if (internal) {
                TRY(dehalo_convert_form_device(ctx, pk->f->id, (const uint64_t*)src, tmp.u64(), len, 0, nullptr));
                src = tmp.p;
            }
            TRY(dehalo_download(ctx, src, len * 32, o));
            o += len * 32;
            return 0;
        };
        auto slice = [&](const DevMem& mem, size_t cnt, size_t len, bool internal) -> int {
            key_put_u32_be(o, (uint32_t)cnt);
            o += 4;
            for (size_t i = 0; i < cnt; i++) TRY(poly(mem.at(i * len), len, internal));
            return 0;
        };
        for (int i = 0; i < 3; i++) TRY(poly(pk->l_ext.at((size_t)i * m), m, true));
        TRY(slice(pk->fixed_values, nf, n, false));
        TRY(slice(pk->fixed_polys, nf, n, false));
        TRY(slice(pk->fixed_cosets, nf, m, true));
        TRY(slice(pk->perm_values, npc, n, false));
        TRY(slice(pk->perm_polys, npc, n, false));
        TRY(slice(pk->perm_cosets, npc, m, true));
        return 0;
    });
}

extern "C" int dehalo_pk_read(dehalo_ctx* ctx, int curve, const dehalo_constraint_system* csd, const uint8_t* bytes, size_t len, uint32_t num_selectors, dehalo_pk** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !bytes || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "pk_read: null argument");
        if (len < 8) return dh_fail(ctx, DEHALO_ERR_INVALID, "pk_read: unexpected end of input");
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        const uint32_t k = key_u32_be(bytes), nf_file = key_u32_be(bytes + 4);
        std::unique_ptr<dehalo_pk> pk(new dehalo_pk);
        TRY(pk_common_init(ctx, curve, csd, k, pk.get()));
        const size_t n = pk->dom.n, m = pk->dom.m, nf = pk->cs.num_fixed, npc = pk->cs.perm_cols.size();
        if (nf_file != nf) return dh_fail(ctx, DEHALO_ERR_INVALID, "pk_read: the key's number of fixed commitments differs from the circuit's fixed columns");
        pk->num_selectors = num_selectors;
        if (len != pk->size()) return dh_fail(ctx, DEHALO_ERR_INVALID, "pk_read: length does not match the circuit (unexpected end of input or trailing bytes)");
        HostPin pin_blob(bytes, len);      // every polynomial below is copied straight out of the caller's blob
        const uint8_t* p = bytes + 8;
        pk->fixed_commitments.resize(8 * nf);
        memcpy(pk->fixed_commitments.data(), p, 64 * nf);
        p += 64 * nf;
        pk->perm_commitments.resize(8 * npc);
        memcpy(pk->perm_commitments.data(), p, 64 * npc);
        p += 64 * npc;
        for (uint32_t s = 0; s < num_selectors; s++) {
            pk->selectors.emplace_back(p, p + (n + 7) / 8);
            p += (n + 7) / 8;
        }
        const int fid = pk->f->id;
        auto poly = [&](fe* dst, size_t want, bool to_internal) -> int {
            if (key_u32_be(p) != want) return dh_fail(ctx, DEHALO_ERR_INVALID, "pk_read: polynomial length differs from the domain's");
            p += 4;
            TRY(dh_h2d(ctx, dst, p, want * 32, ctx->stream.get()));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
            p += want * 32;
            if (to_internal) TRY(dehalo_convert_form_device(ctx, fid, (const uint64_t*)dst, (uint64_t*)dst, want, 1, nullptr));
            return 0;
        };
        auto slice = [&](DevMem& mem, size_t cnt, size_t ln, bool to_internal) -> int {
            if (key_u32_be(p) != cnt) return dh_fail(ctx, DEHALO_ERR_INVALID, "pk_read: polynomial count differs from the circuit's");
            p += 4;
            TRY(mem.alloc(ctx, cnt * ln, false));
            for (size_t i = 0; i < cnt; i++) TRY(poly(mem.at(i * ln), ln, to_internal));
            return 0;
        };
        TRY(pk->l_ext.alloc(ctx, 3 * m, false));
        for (int i = 0; i < 3; i++) TRY(poly(pk->l_ext.at((size_t)i * m), m, true));
        TRY(slice(pk->fixed_values, nf, n, false));
        TRY(slice(pk->fixed_polys, nf, n, false));
        TRY(slice(pk->fixed_cosets, nf, m, true));
        TRY(slice(pk->perm_values, npc, n, false));
        TRY(slice(pk->perm_polys, npc, n, false));
        TRY(slice(pk->perm_cosets, npc, m, true));
        pk->default_transcript_repr();
        TRY(pk->compile_graphs());
        TRY(dehalo_ctx_synchronize(ctx));
        *out = pk.release();
        return 0;
    });
}

extern "C" int dehalo_pk_set_transcript_repr(dehalo_pk* pk, const uint64_t repr[4]) {
    return dh_guard(pk ? pk->ctx : nullptr, [&]() -> int {
        if (!pk || !repr) return DEHALO_ERR_INVALID;
        memcpy(pk->transcript_repr.v, repr, 32);
        return 0;
    });
}
extern "C" int dehalo_pk_get_transcript_repr(const dehalo_pk* pk, uint64_t repr[4]) {
    return dh_guard(pk ? pk->ctx : nullptr, [&]() -> int {
        if (!pk || !repr) return DEHALO_ERR_INVALID;
        memcpy(repr, pk->transcript_repr.v, 32);
        return 0;
    });
}
extern "C" int dehalo_pk_release(dehalo_ctx* ctx, dehalo_pk* pk) {
    return dh_guard(ctx ? ctx : pk ? pk->ctx : nullptr, [&]() -> int {
        if (!pk) return 0;
        dehalo_ctx* c = ctx ? ctx : pk->ctx;
        std::lock_guard<std::recursive_mutex> lk(c->mu);
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream.get());
        delete pk;
        return 0;
    });
}

extern "C" int dehalo_pk_phases(const dehalo_pk* pk, uint32_t out[2]) {
    return dh_guard(pk ? pk->ctx : nullptr, [&]() -> int {
        if (!pk || !out) return DEHALO_ERR_INVALID;
        out[0] = pk->cs.num_phases;
        out[1] = (uint32_t)pk->cs.challenge_phase.size();
        return 0;
    });
}

extern "C" int dehalo_pk_info(const dehalo_pk* pk, uint32_t out[8]) {
    return dh_guard(pk ? pk->ctx : nullptr, [&]() -> int {
        if (!pk || !out) return DEHALO_ERR_INVALID;
        const HostCS& cs = pk->cs;
        const uint32_t L = (uint32_t)cs.lookups.size(), S = cs.num_sets();
        out[0] = pk->k;
        out[1] = pk->dom.extended_k;
        out[2] = cs.blinding_factors();
        out[3] = cs.degree();
        out[4] = S;
        out[5] = cs.num_advice + 2 * L + S + L + (uint32_t)cs.shuffles.size() + 1 + (cs.degree() - 1);
        out[6] = (uint32_t)(cs.advice_q.size() + cs.fixed_q.size() + 1 + cs.perm_cols.size() + (S ? 3 * S - 1 : 0) + 5 * L + 2 * cs.shuffles.size());
        std::vector<int32_t> rs = {0, 1, -(int32_t)(cs.blinding_factors() + 1)};
        if (L) rs.push_back(-1);
        for (auto& q : cs.advice_q) rs.push_back(q.rotation);
        for (auto& q : cs.fixed_q) rs.push_back(q.rotation);
        std::sort(rs.begin(), rs.end());
        out[7] = (uint32_t)(std::unique(rs.begin(), rs.end()) - rs.begin());
        return 0;
    });
}

// ================================================================================================ keys in every SerdeFormat
// [UPSTREAM halo2_proofs/src/plonk.rs VerifyingKey / ProvingKey::{write, read}(.., SerdeFormat), plonk/keygen.rs keygen_pk].  Layout and the validation of the
// header, the length and every count / length word: key_format.hpp, on the host.  The commitments go through the point codec and the polynomials through its
// scalar twin (capi.hip), one launch per slice.  Both raw formats write dehalo_pk_write's / dehalo_vk_write's bytes, and the unchecked read IS dehalo_pk_read.
namespace {

int key_fail(dehalo_ctx* ctx, const char* who, const std::string& what) { return dh_fail(ctx, DEHALO_ERR_INVALID, std::string(who) + ": " + what); }

// the vk's commitments and selectors out of bytes whose header passed (key_parse_header): each commitment list is uploaded as it lies, decompressed (Processed) or
// checked (RawBytes) on the device, and comes back as affine points
int vk_parse(dehalo_ctx* ctx, const char* who, int curve, const uint8_t* bytes, int format, const KeyShape& sh, const KeyLayout& L, VkParts& vk) {
    const bool enc = format == DEHALO_SERDE_PROCESSED;
    std::vector<uint64_t>* dst[2] = {&vk.fixed_commitments, &vk.perm_commitments};
    const size_t cnt[2] = {sh.nf, sh.npc}, off[2] = {L.off_fixed_c, L.off_perm_c};
    DevMem pts, in;
    TRY(pts.alloc(ctx, 2 * std::max<size_t>(1, std::max(sh.nf, sh.npc)), false));
    if (enc) TRY(in.alloc(ctx, std::max<size_t>(1, std::max(sh.nf, sh.npc)), false));
    for (int v = 0; v < 2; v++) {
        dst[v]->assign(8 * cnt[v], 0);
        if (!cnt[v]) continue;
        uint32_t status = 0;
        if (enc) {
            TRY(dehalo_upload(ctx, bytes + off[v], 32 * cnt[v], in.p));
            TRY(dehalo_points_decompress_device(ctx, curve, (const uint8_t*)in.p, cnt[v], pts.u64(), &status, nullptr));
        } else {
            TRY(dehalo_upload(ctx, bytes + off[v], 64 * cnt[v], pts.p));
            if (format == DEHALO_SERDE_RAW_BYTES) TRY(dehalo_points_check_device(ctx, curve, pts.u64(), cnt[v], &status, nullptr));
        }
        if (status) return key_fail(ctx, who, std::string(point_status_text(status, enc)) + ": " + key_section_name(v == 0 ? KEY_FIXED_COMMITMENTS : KEY_PERM_COMMITMENTS));
        TRY(dehalo_download(ctx, pts.p, 64 * cnt[v], dst[v]->data()));
    }
    const uint8_t* p = bytes + L.off_selectors;
    for (size_t s = 0; s < sh.nsel; s++, p += L.sel_bytes) vk.selectors.emplace_back(p, p + L.sel_bytes);
    return 0;
}

// the commitments of `pk` as the format writes them, at out + L.off_fixed_c and out + L.off_perm_c (Processed: compressed on the device)
int vk_write_formatted(dehalo_ctx* ctx, const dehalo_pk* pk, const KeyLayout& L, uint8_t* out) {
    key_put_u32_be(out, pk->k);
    key_put_u32_be(out + 4, pk->cs.num_fixed);
    const std::vector<uint64_t>* src[2] = {&pk->fixed_commitments, &pk->perm_commitments};
    const size_t cnt[2] = {(size_t)pk->cs.num_fixed, pk->cs.perm_cols.size()}, off[2] = {L.off_fixed_c, L.off_perm_c};
    DevMem pts, enc;
    TRY(pts.alloc(ctx, 2 * std::max<size_t>(1, std::max(cnt[0], cnt[1])), false));
    TRY(enc.alloc(ctx, std::max<size_t>(1, std::max(cnt[0], cnt[1])), false));
    for (int v = 0; v < 2; v++) {
        if (!cnt[v]) continue;
        TRY(dehalo_upload(ctx, src[v]->data(), 64 * cnt[v], pts.p));
        TRY(dehalo_points_compress_device(ctx, pk->curve, pts.u64(), cnt[v], (uint8_t*)enc.p, nullptr));
        TRY(dehalo_download(ctx, enc.p, 32 * cnt[v], out + off[v]));
    }
    uint8_t* o = out + L.off_selectors;
    for (auto& s : pk->selectors) {
        memcpy(o, s.data(), s.size());
        o += s.size();
    }
    return 0;
}

}   // namespace

extern "C" size_t dehalo_vk_size_custom(const dehalo_pk* pk, int format) {
    KeyLayout L;
    return pk && key_layout(format, pk->k, key_shape(pk), L) ? L.vk_size : 0;
}
extern "C" size_t dehalo_pk_size_custom(const dehalo_pk* pk, int format) {
    KeyLayout L;
    return pk && key_layout(format, pk->k, key_shape(pk), L) ? L.pk_size : 0;
}

extern "C" int dehalo_vk_write_custom(dehalo_ctx* ctx, const dehalo_pk* pk, int format, uint8_t* out, size_t cap) {
    return dh_guard(ctx ? ctx : pk ? pk->ctx : nullptr, [&]() -> int {
        if (!pk || !out) return DEHALO_ERR_INVALID;
        if (!ctx) ctx = pk->ctx;
        KeyLayout L;
        if (!key_layout(format, pk->k, key_shape(pk), L)) return key_fail(ctx, "vk_write_custom", "unknown format");
        if (cap < L.vk_size) return key_fail(ctx, "vk_write_custom", "buffer too small");
        if (format != DEHALO_SERDE_PROCESSED) return dehalo_vk_write(pk, out, cap);      // both raw formats: the same bytes
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        return vk_write_formatted(ctx, pk, L, out);
    });
}

extern "C" int dehalo_pk_write_custom(dehalo_ctx* ctx, const dehalo_pk* pk, int format, uint8_t* out, size_t cap) {
    return dh_guard(ctx ? ctx : pk ? pk->ctx : nullptr, [&]() -> int {
        if (!pk || !out) return DEHALO_ERR_INVALID;
        if (!ctx) ctx = pk->ctx;
        KeyLayout L;
        if (!key_layout(format, pk->k, key_shape(pk), L)) return key_fail(ctx, "pk_write_custom", "unknown format");
        if (cap < L.pk_size) return key_fail(ctx, "pk_write_custom", "buffer too small");
        if (format != DEHALO_SERDE_PROCESSED) return dehalo_pk_write(ctx, pk, out, cap);      // both raw formats: the same bytes
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        TRY(vk_write_formatted(ctx, pk, L, out));
        // One section at a time: out of the internal form where it is in it (dehalo_convert_form_device), then to_repr (dehalo_field_op_device op 5), each one
        // launch over the whole section, then down polynomial by polynomial between the length words.
        const DevMem* mem[KEY_SECTIONS] = {nullptr, nullptr, &pk->l_ext, &pk->l_ext, &pk->l_ext, &pk->fixed_values, &pk->fixed_polys, &pk->fixed_cosets,
                                           &pk->perm_values, &pk->perm_polys, &pk->perm_cosets};
        size_t most = 1;
        for (int s = KEY_L0; s < KEY_SECTIONS; s++) most = std::max(most, L.polys[s].count * L.polys[s].len);
        DevMem tmp;
        TRY(tmp.alloc(ctx, most, false));
        const int fid = pk->f->id;
        for (int s = KEY_L0; s < KEY_SECTIONS; s++) {
            const KeyPolys& P = L.polys[s];
            if (P.slice) key_put_u32_be(out + P.off, (uint32_t)P.count);
            const size_t elems = P.count * P.len;
            if (!elems) continue;
            const fe* src = s <= KEY_L_ACTIVE_ROW ? mem[s]->at((size_t)(s - KEY_L0) * L.m) : mem[s]->p;
            if (key_section_extended(s)) {      // the extended-domain columns
                TRY(dehalo_convert_form_device(ctx, fid, (const uint64_t*)src, tmp.u64(), elems, 0, nullptr));
                src = tmp.p;
            }
            TRY(dehalo_field_op_device(ctx, fid, 5, (const uint64_t*)src, nullptr, tmp.u64(), elems, nullptr));
            for (size_t i = 0; i < P.count; i++) {
                key_put_u32_be(out + P.poly_off(i), (uint32_t)P.len);
                TRY(dehalo_download(ctx, tmp.at(i * P.len), P.len * 32, out + P.poly_off(i) + 4));
            }
        }
        return 0;
    });
}

extern "C" int dehalo_pk_read_custom(dehalo_ctx* ctx, int curve, const dehalo_constraint_system* csd, const uint8_t* bytes, size_t len, int format, uint32_t num_selectors,
                                     dehalo_pk** out) {
    if (ctx && format == DEHALO_SERDE_RAW_BYTES_UNCHECKED) return dehalo_pk_read(ctx, curve, csd, bytes, len, num_selectors, out);      // the same path: an equal key
    return dh_guard(ctx, [&]() -> int {
        const char* who = "pk_read_custom";
        if (!ctx || !bytes || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "pk_read_custom: null argument");
        uint32_t k = 0;
        KeyHeaderError he = key_peek_k(bytes, len, format, k);
        if (he != KEY_HEADER_OK) return key_fail(ctx, who, key_header_error_text(he));
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        std::unique_ptr<dehalo_pk> pk(new dehalo_pk);
        TRY(pk_common_init(ctx, curve, csd, k, pk.get()));
        pk->num_selectors = num_selectors;
        const KeyShape sh = key_shape(pk.get());
        KeyLayout L;
        he = key_parse_header(bytes, len, format, sh, DEHALO_KEEP_K, true, L);
        if (he != KEY_HEADER_OK) return key_fail(ctx, who, key_header_error_text(he));
        int bad_section = -1;
        he = key_check_poly_words(bytes, L, bad_section);
        if (he != KEY_HEADER_OK) return key_fail(ctx, who, std::string(key_header_error_text(he)) + ": " + key_section_name(bad_section));
        const bool enc = format == DEHALO_SERDE_PROCESSED;
        VkParts vk;
        TRY(vk_parse(ctx, who, curve, bytes, format, sh, L, vk));
        pk->fixed_commitments = std::move(vk.fixed_commitments);
        pk->perm_commitments = std::move(vk.perm_commitments);
        pk->selectors = std::move(vk.selectors);
        HostPin pin_blob(bytes, len);      // every polynomial below is copied straight out of the caller's blob
        const int fid = pk->f->id;
        hipStream_t st = ctx->stream.get();
        // One group of adjacent polynomials at a time (l0 | l_last | l_active_row, then each slice): every polynomial goes up to its place, then ONE launch converts
        // (Processed: from_repr, in place) or checks (RawBytes) the whole group, and one more takes an extended-domain group into the internal form.
        auto group = [&](DevMem& mem, int first, int sections) -> int {
            const KeyPolys& P0 = L.polys[first];
            const size_t per = P0.count * P0.len, elems = per * (size_t)sections;
            TRY(mem.alloc(ctx, elems, false));
            if (!elems) return 0;
            for (int s = 0; s < sections; s++)
                for (size_t i = 0; i < P0.count; i++)
                    TRY(dh_h2d(ctx, mem.at((size_t)s * per + i * P0.len), bytes + L.polys[first + s].poly_off(i) + 4, P0.len * 32, st));
            // (the codec takes fewer than 2^29 elements a call: a larger group goes in pieces, in order, so the first piece that objects holds the lowest index)
            for (size_t at = 0; at < elems; at += KEY_CODEC_MOST) {
                const size_t piece = std::min(KEY_CODEC_MOST, elems - at);
                uint32_t status = 0;
                uint64_t first_bad = 0;
                if (enc) TRY(dehalo_scalars_from_repr_device(ctx, fid, (const uint8_t*)mem.at(at), piece, mem.u64(at), &status, &first_bad, nullptr));
                else TRY(dehalo_scalars_check_device(ctx, fid, mem.u64(at), piece, &status, &first_bad, nullptr));
                if (status) return key_fail(ctx, who, key_element_error_text(enc, first + (int)((at + first_bad) / per), (at + first_bad) % per));
            }
            if (key_section_extended(first)) TRY(dehalo_convert_form_device(ctx, fid, mem.u64(), mem.u64(), elems, 1, nullptr));
            return 0;
        };
        TRY(group(pk->l_ext, KEY_L0, 3));
        TRY(group(pk->fixed_values, KEY_FIXED_VALUES, 1));
        TRY(group(pk->fixed_polys, KEY_FIXED_POLYS, 1));
        TRY(group(pk->fixed_cosets, KEY_FIXED_COSETS, 1));
        TRY(group(pk->perm_values, KEY_PERM_VALUES, 1));
        TRY(group(pk->perm_polys, KEY_PERM_POLYS, 1));
        TRY(group(pk->perm_cosets, KEY_PERM_COSETS, 1));
        pk->default_transcript_repr();
        TRY(pk->compile_graphs());
        TRY(dehalo_ctx_synchronize(ctx));
        *out = pk.release();
        return 0;
    });
}

extern "C" int dehalo_keygen_pk(dehalo_ctx* ctx, const dehalo_params* params, const dehalo_constraint_system* csd, const uint8_t* vk_bytes, size_t vk_len, int vk_format,
                                uint32_t num_selectors, const uint64_t* fixed, const uint64_t* mapping, uint32_t flags, dehalo_pk** out) {
    return dh_guard(ctx, [&]() -> int {
        const char* who = "keygen_pk";
        if (!ctx || !params || !vk_bytes || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "keygen_pk: null argument");
        uint32_t k = 0;
        KeyHeaderError he = key_peek_k(vk_bytes, vk_len, vk_format, k);
        if (he == KEY_HEADER_OK && k != params->k) he = KEY_HEADER_K_DIFFERS;
        if (he != KEY_HEADER_OK) return key_fail(ctx, who, key_header_error_text(he));
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        std::unique_ptr<dehalo_pk> pk(new dehalo_pk);
        TRY(pk_common_init(ctx, params->curve, csd, params->k, pk.get()));
        pk->num_selectors = num_selectors;
        const KeyShape sh = key_shape(pk.get());
        KeyLayout L;
        he = key_parse_header(vk_bytes, vk_len, vk_format, sh, params->k, false, L);
        if (he != KEY_HEADER_OK) return key_fail(ctx, who, key_header_error_text(he));
        VkParts vk;
        TRY(vk_parse(ctx, who, params->curve, vk_bytes, vk_format, sh, L, vk));
        TRY(keygen_body(ctx, params, fixed, mapping, nullptr, num_selectors, flags, &vk, pk));
        *out = pk.release();
        return 0;
    });
}
