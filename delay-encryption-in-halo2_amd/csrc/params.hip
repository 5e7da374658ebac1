// params.hip -- the commitment schemes' parameters behind the C ABI: ParamsKZG (setup / read / write, the three SerdeFormats, from_g, downsize) and ParamsIPA
// (create, from_g, generate, read / write, downsize) [UPSTREAM halo2_proofs @ v2023_04_20: poly/kzg/commitment.rs, poly/ipa/commitment.rs] -- the calls the
// reference makes at benches/delay_enc.rs:41-54.  Every constructor checks its arguments, gets g and g_lagrange onto the device and ends in ONE tail,
// params_from_device.  C entry points run under dh_guard, as in prover.hip; no kernel is defined here (transcript and draws: transcript.hip; opening: ipa_open.hip).
#include <memory>

#include "params_format.hpp"
#include "whole_call.hpp"

namespace {

// what a constructor hands the tail beside the two device vectors
struct ParamsParts {
    int curve = 0;
    uint32_t k = 0;
    const uint8_t *g2 = nullptr, *s_g2 = nullptr;      // ParamsKZG's two G2 points (128 raw bytes each), or null
    const uint64_t *w = nullptr, *u = nullptr;         // on the host; non-null: ParamsIPA
    std::vector<uint64_t> g, g_lagrange;               // host copies the constructor already owns (8 x 2^k words each), moved in; empty: downloaded
};

// The one constructor tail: the params over g and g_lagrange as they stand on the device (2^k affine points each, standard Montgomery).  Both resident MSM
// tables are registered from there and the host copies taken or downloaded; ParamsIPA also gets g | u | w as plain points on the device, the [U | W]
// registration and W's fixed-base table.
int params_from_device(dehalo_ctx* ctx, ParamsParts&& in, const uint64_t* d_g, const uint64_t* d_gl, dehalo_params** out) {
    const size_t n = (size_t)1 << in.k;
    std::unique_ptr<dehalo_params> p(new dehalo_params);
    p->ctx = ctx; p->curve = in.curve; p->k = in.k; p->n = n;
    if (in.g2) memcpy(p->g2, in.g2, 128);
    if (in.s_g2) memcpy(p->s_g2, in.s_g2, 128);
    TRY(dehalo_bases_register_device(ctx, in.curve, d_g, n, 0, 1, adopt(ctx, p->bases_g)));
    TRY(dehalo_bases_register_device(ctx, in.curve, d_gl, n, 0, 1, adopt(ctx, p->bases_gl)));
    p->g = std::move(in.g);
    p->g_lagrange = std::move(in.g_lagrange);
    if (p->g.empty()) { p->g.resize(8 * n); TRY(dehalo_download(ctx, d_g, 64 * n, p->g.data())); }
    if (p->g_lagrange.empty()) { p->g_lagrange.resize(8 * n); TRY(dehalo_download(ctx, d_gl, 64 * n, p->g_lagrange.data())); }
    if (in.w) {
        p->scheme = DEHALO_SCHEME_IPA;
        memcpy(p->w, in.w, 64);
        memcpy(p->u, in.u, 64);
        TRY(p->d_guw.alloc(ctx, 2 * (n + 2), false));
        HIP_TRY(ctx, hipMemcpyAsync(p->d_guw.p, d_g, 64 * n, hipMemcpyDeviceToDevice, ctx->stream.get()));
        TRY(dh_h2d(ctx, p->d_guw.at(2 * n), p->u, 64, ctx->stream.get()));
        TRY(dh_h2d(ctx, p->d_guw.at(2 * n + 2), p->w, 64, ctx->stream.get()));
        TRY(dehalo_bases_register_device(ctx, in.curve, p->d_guw.u64(2 * n), 2, 0, 0, adopt(ctx, p->bases_uw)));
        TRY(dehalo_fixed_base_create(ctx, in.curve, p->w, adopt(ctx, p->fb_w)));
    }
    *out = p.release();
    return 0;
}

// The constructors whose points are host words, the caller's or another params' (create, read, from_g, downsize and their IPA twins): in.g holds g verbatim and
// goes up as it is (or, given d_g_src, g comes across on this device); g_lagrange goes up when in.g_lagrange holds it and is the group FFT of g where it
// lies (g_to_lagrange, gfft.cuh) when not; then the tail
int params_from_g(dehalo_ctx* ctx, ParamsParts&& in, const uint64_t* d_g_src, dehalo_params** out) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    const size_t n = (size_t)1 << in.k;
    const hipStream_t s = ctx->stream.get();
    DevMem dg, dgl;
    TRY(dg.alloc(ctx, 2 * n, false));
    TRY(dgl.alloc(ctx, 2 * n, false));
    if (d_g_src) HIP_TRY(ctx, hipMemcpyAsync(dg.p, d_g_src, 64 * n, hipMemcpyDeviceToDevice, s));
    else TRY(dh_h2d(ctx, dg.p, in.g.data(), 64 * n, s));
    if (in.g_lagrange.empty()) TRY(dehalo_g_to_lagrange_device(ctx, in.curve, dg.u64(), in.k, dgl.u64(), s));
    else TRY(dh_h2d(ctx, dgl.p, in.g_lagrange.data(), 64 * n, s));
    return params_from_device(ctx, std::move(in), dg.u64(), dgl.u64(), out);
}

// the range checks of a ParamsKZG built here, before any device work: the two precomputed tables must fit (as dehalo_params_setup checks)
int kzg_params_check(dehalo_ctx* ctx, const std::string& who, int curve, uint32_t k) {
    const HostField* f = host_field(curve_scalar_field(curve));
    if (!f) return dh_fail(ctx, DEHALO_ERR_INVALID, who + ": unknown curve");
    if (k > PARAMS_MAX_K || k > f->two_adicity) return dh_fail(ctx, DEHALO_ERR_INVALID, who + ": k out of range");
    if (!dh_precomputed_table_fits(curve, (size_t)1 << k)) return dh_fail(ctx, DEHALO_ERR_INVALID, who + ": 2^k x windows >= 2^30: precomputed table too large");
    return 0;
}

// the range checks of a ParamsIPA under construction (null arguments are the caller's to report)
int ipa_params_check(dehalo_ctx* ctx, const std::string& who, int curve, uint32_t k) {
    if (curve != DEHALO_CURVE_PALLAS && curve != DEHALO_CURVE_VESTA) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, who + ": IPA over Pallas / Vesta only");
    if (k < 1 || k > 28) return dh_fail(ctx, DEHALO_ERR_INVALID, who + ": k out of range");
    if (!dh_precomputed_table_fits(curve, (size_t)1 << k)) return dh_fail(ctx, DEHALO_ERR_INVALID, who + ": 2^k x windows >= 2^30: precomputed table too large");
    return 0;
}

// one G2 point of a file into the 128 raw bytes the params keep, validated as the format asks
int g2_read(dehalo_ctx* ctx, const G2Host& g2, int format, const uint8_t* in, uint8_t raw[128]) {
    int status = 0;
    if (format == DEHALO_SERDE_PROCESSED) status = g2.decompress_raw(in, raw);
    else {
        memcpy(raw, in, 128);
        G2Host::Pt P;
        if (format == DEHALO_SERDE_RAW_BYTES) status = g2.from_raw_checked(raw, P);
    }
    if (status) return dh_fail(ctx, DEHALO_ERR_INVALID, std::string("params_read_custom: G2: ") + point_status_text((uint32_t)status, format == DEHALO_SERDE_PROCESSED));
    return 0;
}

}   // namespace

// ================================================================================================ ParamsKZG
// (no table-fits check of its own: a table that is too large is refused by the registration)
extern "C" int dehalo_params_create(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, const uint8_t* g2, const uint8_t* s_g2,
                                    dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !out || !g || !g_lagrange) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_create: null argument");
        if (k > 28 || curve_scalar_field(curve) < 0) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_create: k or curve out of range");
        ParamsParts in{curve, k, g2, s_g2};
        in.g.assign(g, g + ((size_t)8 << k));
        in.g_lagrange.assign(g_lagrange, g_lagrange + ((size_t)8 << k));
        return params_from_g(ctx, std::move(in), nullptr, out);
    });
}

// ---- ParamsKZG::setup: the two G2 points on the host (O(1): one 254-bit scalar multiplication over Fq2 = Fq[i] / (i^2 + 1); G2Host and the generator: params_format.hpp) ----
extern "C" int dehalo_params_setup(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t s[4], dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !out || !s) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_setup: null argument");
        if (curve != DEHALO_CURVE_BN254_G1) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "params_setup: ParamsKZG needs a pairing: BN254 only");
        const HostField* f = host_field(curve_scalar_field(curve));
        if (k > f->two_adicity) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_setup: k out of range");
        if (k > 25) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_setup: k > 25: the SRS tables would be too large (include/dehalo.h)");      // (2 x 15 x 2^26 x 64 B = 128 GB at k = 26: fits the index and the card, never exercised)
        // checked BEFORE the 2^(k+1) fixed-base multiplications: the tables this call registers must fit (BN254: k <= 25, include/dehalo.h)
        if (!dh_precomputed_table_fits(curve, (size_t)1 << k)) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_setup: 2^k x windows >= 2^30: precomputed table too large");
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        Fe sm;
        memcpy(sm.v, s, 32);
        const size_t n = (size_t)1 << k;
        // omega = ROOT_OF_UNITY^(2^(S - k));  (s^n - 1) / n
        Fe omega = f->root_of_unity;
        for (uint32_t i = k; i < f->two_adicity; i++) omega = f->sqr(omega);
        Fe sn = sm;
        for (uint32_t i = 0; i < k; i++) sn = f->sqr(sn);
        const Fe cfac = f->mul(f->sub(sn, f->one), f->invert(f->from_u64((uint64_t)n)));
        DevMem dg, dgl;
        TRY(dg.alloc(ctx, 2 * n, false));
        TRY(dgl.alloc(ctx, 2 * n, false));
        TRY(kzg_setup_bn254(ctx, k, sm.v, omega.v, cfac.v, (affine_t*)dg.p, (affine_t*)dgl.p, ctx->stream.get()));
        uint8_t g2raw[128], sg2raw[128];
        {   // g2 = the generator, s_g2 = [s] g2
            const HostField* q = host_field(curve_base_field(curve));
            G2Host g2(q);
            const G2Host::Pt G = bn254_g2_generator(q);
            const Fe sc = f->to_canonical(sm);
            g2.to_raw(G, g2raw);
            g2.to_raw(g2.scalar_mul(sc.v, G), sg2raw);
        }
        return params_from_device(ctx, {curve, k, g2raw, sg2raw}, dg.u64(), dgl.u64(), out);
    });
}

extern "C" int dehalo_params_read(dehalo_ctx* ctx, int curve, const uint8_t* bytes, size_t len, dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !bytes || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_read: null argument");
        if (len < 4) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_read: unexpected end of input");
        const uint32_t k = params_u32_le(bytes);
        if (k > 28) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_read: k out of range");
        const size_t n = (size_t)1 << k;
        if (len != 4 + 2 * 64 * n + 256) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_read: length does not match k");
        if (curve_scalar_field(curve) < 0) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_create: k or curve out of range");      // (worded as dehalo_params_create refuses it: the text callers know)
        // (the points are 8-byte aligned only if the caller's buffer is: copied once, into the aligned vectors the params keep)
        ParamsParts in{curve, k, bytes + 4 + 128 * n, bytes + 4 + 128 * n + 128};
        in.g.resize(8 * n); in.g_lagrange.resize(8 * n);
        memcpy(in.g.data(), bytes + 4, 64 * n);
        memcpy(in.g_lagrange.data(), bytes + 4 + 64 * n, 64 * n);
        return params_from_g(ctx, std::move(in), nullptr, out);
    });
}

extern "C" size_t dehalo_params_size(const dehalo_params* p) { return p && p->scheme == DEHALO_SCHEME_KZG ? 4 + 2 * 64 * p->n + 256 : 0; }

extern "C" int dehalo_params_write(const dehalo_params* p, uint8_t* out, size_t cap) {
    return dh_guard(p ? p->ctx : nullptr, [&]() -> int {
        if (!p || !out) return DEHALO_ERR_INVALID;
        if (p->scheme != DEHALO_SCHEME_KZG) return dh_fail(p->ctx, DEHALO_ERR_UNSUPPORTED, "params_write: ParamsIPA::write is not implemented");
        if (cap < dehalo_params_size(p)) return dh_fail(p->ctx, DEHALO_ERR_INVALID, "params_write: buffer too small");
        for (int i = 0; i < 4; i++) out[i] = (uint8_t)(p->k >> (8 * i));
        memcpy(out + 4, p->g.data(), 64 * p->n);
        memcpy(out + 4 + 64 * p->n, p->g_lagrange.data(), 64 * p->n);
        memcpy(out + 4 + 128 * p->n, p->g2, 128);
        memcpy(out + 4 + 128 * p->n + 128, p->s_g2, 128);
        return 0;
    });
}

extern "C" int dehalo_params_release(dehalo_ctx* ctx, dehalo_params* p) {
    return dh_guard(ctx, [&]() -> int {
        delete p;      // (its bases release themselves, each as dehalo_bases_release does, on the context the params were made on)
        return 0;
    });
}

extern "C" int dehalo_params_commit_device(dehalo_ctx* ctx, const dehalo_params* p, const uint64_t* d_polys, size_t batch, int lagrange, uint64_t* d_out_affine,
                                           void* stream) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !p) return DEHALO_ERR_INVALID;
        return dehalo_msm_device_affine(ctx, (lagrange ? p->bases_gl : p->bases_g).get(), d_polys, p->n, batch, nullptr, d_out_affine, stream);
    });
}

extern "C" int dehalo_params_scheme(const dehalo_params* p) { return p ? p->scheme : DEHALO_ERR_INVALID; }
extern "C" const dehalo_fixed_base* dehalo_params_fixed_base(const dehalo_params* p) { return p ? p->fb_w.get() : nullptr; }

// ================================================================================================ ParamsIPA
extern "C" int dehalo_params_ipa_create(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, const uint64_t w[8],
                                        const uint64_t u[8], dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !out || !g || !g_lagrange || !w || !u) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_create: null argument");
        TRY(ipa_params_check(ctx, "params_ipa_create", curve, k));
        ParamsParts in{curve, k, nullptr, nullptr, w, u};
        in.g.assign(g, g + ((size_t)8 << k));
        in.g_lagrange.assign(g_lagrange, g_lagrange + ((size_t)8 << k));
        return params_from_g(ctx, std::move(in), nullptr, out);
    });
}

// ParamsIPA from g alone: g_lagrange = g_to_lagrange(g) on the device (gfft.cuh)
extern "C" int dehalo_params_ipa_from_g(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t* g, const uint64_t w[8], const uint64_t u[8], dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !out || !g || !w || !u) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_from_g: null argument");
        TRY(ipa_params_check(ctx, "params_ipa_from_g", curve, k));
        ParamsParts in{curve, k, nullptr, nullptr, w, u};
        in.g.assign(g, g + ((size_t)8 << k));
        return params_from_g(ctx, std::move(in), nullptr, out);
    });
}

// ParamsIPA without a file: g | W | U are generated points (gfft.cuh k_points_generate; the rule: include/dehalo.h), g_lagrange the group FFT of g where it lies
extern "C" int dehalo_params_ipa_generate(dehalo_ctx* ctx, int curve, uint32_t k, const uint8_t* key32, dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_generate: null argument");
        TRY(ipa_params_check(ctx, "params_ipa_generate", curve, k));
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        const size_t n = (size_t)1 << k;
        uint32_t key[8];
        memcpy(key, key32 ? (const void*)key32 : (const void*)DEHALO_GENERATORS_DEFAULT_KEY, 32);
        DevMem dg, dwu, dgl, status;
        TRY(dg.alloc(ctx, 2 * n, false));
        TRY(dwu.alloc(ctx, 4, false));
        TRY(dgl.alloc(ctx, 2 * n, false));
        TRY(status.alloc(ctx, 1, true));
        hipStream_t s = ctx->stream.get();
        TRY(gfft_ops(curve)->points_generate(ctx, key, /* stream */ 0, 0, (affine_t*)dg.p, n, (uint32_t*)status.p, s));
        TRY(gfft_ops(curve)->points_generate(ctx, key, /* stream */ 1, 0, (affine_t*)dwu.p, 2, (uint32_t*)status.p, s));
        TRY(dehalo_g_to_lagrange_device(ctx, curve, dg.u64(), k, dgl.u64(), s));
        uint32_t bad[8];
        TRY(dehalo_download(ctx, status.p, 32, bad));
        if (bad[0]) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_generate: an index found no point in 256 attempts");
        uint64_t wu[16];
        TRY(dehalo_download(ctx, dwu.p, 128, wu));
        return params_from_device(ctx, {curve, k, nullptr, nullptr, wu, wu + 8}, dg.u64(), dgl.u64(), out);
    });
}

// ---- ParamsIPA::{write, read} [UPSTREAM halo2_proofs/src/poly/ipa/commitment.rs]: k: u32 LE | g | g_lagrange | w | u, every point GroupEncoding::to_bytes
// (g1_compress_host, g1_host.hpp: what dehalo_transcript::write_point appends to a proof)
extern "C" size_t dehalo_params_ipa_size(const dehalo_params* p) { return p && p->scheme == DEHALO_SCHEME_IPA ? 4 + 2 * 32 * p->n + 64 : 0; }

extern "C" int dehalo_params_ipa_write(const dehalo_params* p, uint8_t* out, size_t cap) {
    return dh_guard(p ? p->ctx : nullptr, [&]() -> int {
        if (!p || !out) return DEHALO_ERR_INVALID;
        if (p->scheme != DEHALO_SCHEME_IPA) return dh_fail(p->ctx, DEHALO_ERR_UNSUPPORTED, "params_ipa_write: not ParamsIPA (ParamsKZG: dehalo_params_write)");
        if (cap < dehalo_params_ipa_size(p)) return dh_fail(p->ctx, DEHALO_ERR_INVALID, "params_ipa_write: buffer too small");
        const HostField* fq = host_field(curve_base_field(p->curve));
        for (int i = 0; i < 4; i++) out[i] = (uint8_t)(p->k >> (8 * i));
        uint8_t* o = out + 4;
        for (size_t i = 0; i < p->n; i++, o += 32) g1_compress_host(fq, &p->g[8 * i], o);
        for (size_t i = 0; i < p->n; i++, o += 32) g1_compress_host(fq, &p->g_lagrange[8 * i], o);
        g1_compress_host(fq, p->w, o);
        g1_compress_host(fq, p->u, o + 32);
        return 0;
    });
}

extern "C" int dehalo_params_ipa_read(dehalo_ctx* ctx, int curve, const uint8_t* bytes, size_t len, dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !bytes || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_read: null argument");
        if (len < 4) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_read: unexpected end of input");
        const uint32_t k = params_u32_le(bytes);
        TRY(ipa_params_check(ctx, "params_ipa_read", curve, k));
        const size_t n = (size_t)1 << k, count = 2 * n + 2;
        if (len != 4 + 32 * count) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_read: length does not match k");
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        // the encodings go up as they are and become affine points where they lie: one lane per point takes the square root (k_decompress, gfft.cuh)
        DevMem enc, pts, status;
        TRY(enc.alloc(ctx, count, false));
        TRY(pts.alloc(ctx, 2 * count, false));
        TRY(status.alloc(ctx, 1, true));
        TRY(dh_h2d(ctx, enc.p, bytes + 4, 32 * count, ctx->stream.get()));
        TRY(gfft_ops(curve)->decompress(ctx, (const uint8_t*)enc.p, (affine_t*)pts.p, count, (uint32_t*)status.p, ctx->stream.get()));
        uint32_t bad[8];
        TRY(dehalo_download(ctx, status.p, 32, bad));
        if (bad[0]) return dh_fail(ctx, DEHALO_ERR_INVALID, std::string("params_ipa_read: ") + point_status_text(bad[0], true));
        uint64_t wu[16];
        TRY(dehalo_download(ctx, pts.at(4 * n), 128, wu));
        return params_from_device(ctx, {curve, k, nullptr, nullptr, wu, wu + 8}, pts.u64(), pts.u64(2 * n), out);
    });
}

// ================================================================================================ ParamsKZG from any SRS
// SerdeFormat read / write, ParamsKZG from g alone, Params::downsize [UPSTREAM halo2_proofs/src/poly/kzg/commitment.rs: write_custom, read_custom, from_parts,
// downsize; poly/ipa/commitment.rs: downsize].  Layout, header and the two G2 points: params_format.hpp, on the host; the G1 vectors: the point codec and the
// group FFT, on the device (gfft.cuh).
extern "C" size_t dehalo_params_size_custom(const dehalo_params* p, int format) {
    ParamsLayout L;
    return p && p->scheme == DEHALO_SCHEME_KZG && params_layout(format, p->k, L) ? L.size : 0;
}

extern "C" int dehalo_params_write_custom(const dehalo_params* p, int format, uint8_t* out, size_t cap) {
    return dh_guard(p ? p->ctx : nullptr, [&]() -> int {
        if (!p || !out) return DEHALO_ERR_INVALID;
        dehalo_ctx* ctx = p->ctx;
        if (p->scheme != DEHALO_SCHEME_KZG) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "params_write_custom: ParamsIPA has one format (dehalo_params_ipa_write)");
        ParamsLayout L;
        if (!params_layout(format, p->k, L)) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_write_custom: unknown format");
        if (cap < L.size) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_write_custom: buffer too small");
        if (format != DEHALO_SERDE_PROCESSED) return dehalo_params_write(p, out, cap);      // both raw formats: the same bytes
        if (curve_base_field(p->curve) != DEHALO_FIELD_BN254_FQ) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "params_write_custom: the G2 encoding is BN254's");
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        for (int i = 0; i < 4; i++) out[i] = (uint8_t)(p->k >> (8 * i));
        // one vector at a time: up as the host copy, compressed by one lane per point, down at 32 B per point
        DevMem pts, enc;
        TRY(pts.alloc(ctx, 2 * L.n, false));
        TRY(enc.alloc(ctx, L.n, false));
        const std::vector<uint64_t>* vec[2] = {&p->g, &p->g_lagrange};
        const size_t off[2] = {L.off_g, L.off_gl};
        for (int v = 0; v < 2; v++) {
            TRY(dh_h2d(ctx, pts.p, vec[v]->data(), 64 * L.n, ctx->stream.get()));
            TRY(dehalo_points_compress_device(ctx, p->curve, pts.u64(), L.n, (uint8_t*)enc.p, ctx->stream.get()));
            TRY(dehalo_download(ctx, enc.p, 32 * L.n, out + off[v]));
        }
        const G2Host g2(host_field(DEHALO_FIELD_BN254_FQ));
        g2.compress_raw(p->g2, out + L.off_g2);
        g2.compress_raw(p->s_g2, out + L.off_sg2);
        return 0;
    });
}

extern "C" int dehalo_params_read_custom(dehalo_ctx* ctx, int curve, const uint8_t* bytes, size_t len, int format, uint32_t downsize_k, dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !bytes || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_read_custom: null argument");
        ParamsLayout L;
        const ParamsHeaderError he = params_parse_header(bytes, len, format, L);
        if (he != PARAMS_HEADER_OK) return dh_fail(ctx, DEHALO_ERR_INVALID, std::string("params_read_custom: ") + params_header_error_text(he));
        const bool keep = downsize_k == DEHALO_KEEP_K;
        if (!keep && downsize_k > L.k) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_read_custom: downsize_k is above the file's k");
        if (keep && format == DEHALO_SERDE_RAW_BYTES_UNCHECKED) return dehalo_params_read(ctx, curve, bytes, len, out);
        const uint32_t k = keep ? L.k : downsize_k;
        TRY(kzg_params_check(ctx, "params_read_custom", curve, k));
        if (curve_base_field(curve) != DEHALO_FIELD_BN254_FQ && format != DEHALO_SERDE_RAW_BYTES_UNCHECKED)
            return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "params_read_custom: the G2 encoding and its curve are BN254's");
        // the two G2 points, on the host
        uint8_t g2raw[128], sg2raw[128];
        {
            const G2Host g2(host_field(DEHALO_FIELD_BN254_FQ));
            TRY(g2_read(ctx, g2, format, bytes + L.off_g2, g2raw));
            TRY(g2_read(ctx, g2, format, bytes + L.off_sg2, sg2raw));
        }
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        // the G1 points that are kept: g | g_lagrange (adjacent in the file), or the first 2^k of g alone -- the rest of the file is never read
        const size_t n = (size_t)1 << k, count = keep ? 2 * n : n;
        DevMem pts, enc, gl;
        TRY(pts.alloc(ctx, 2 * count, false));
        uint32_t status = 0;
        if (format == DEHALO_SERDE_PROCESSED) {
            TRY(enc.alloc(ctx, count, false));
            TRY(dh_h2d(ctx, enc.p, bytes + L.off_g, 32 * count, ctx->stream.get()));
            TRY(dehalo_points_decompress_device(ctx, curve, (const uint8_t*)enc.p, count, pts.u64(), &status, ctx->stream.get()));
        } else {
            TRY(dh_h2d(ctx, pts.p, bytes + L.off_g, 64 * count, ctx->stream.get()));
            if (format == DEHALO_SERDE_RAW_BYTES) TRY(dehalo_points_check_device(ctx, curve, pts.u64(), count, &status, ctx->stream.get()));
        }
        if (status) return dh_fail(ctx, DEHALO_ERR_INVALID, std::string("params_read_custom: ") + point_status_text(status, format == DEHALO_SERDE_PROCESSED));
        const uint64_t* d_gl = pts.u64(2 * n);
        if (!keep) {
            TRY(gl.alloc(ctx, 2 * n, false));
            TRY(dehalo_g_to_lagrange_device(ctx, curve, pts.u64(), k, gl.u64(), ctx->stream.get()));
            d_gl = gl.u64();
        }
        return params_from_device(ctx, {curve, k, g2raw, sg2raw}, pts.u64(), d_gl, out);
    });
}

extern "C" int dehalo_params_from_g(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t* g, const uint8_t* g2, const uint8_t* s_g2, dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !out || !g) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_from_g: null argument");
        TRY(kzg_params_check(ctx, "params_from_g", curve, k));
        ParamsParts in{curve, k, g2, s_g2};
        in.g.assign(g, g + ((size_t)8 << k));
        return params_from_g(ctx, std::move(in), nullptr, out);
    });
}

extern "C" int dehalo_params_downsize(dehalo_ctx* ctx, const dehalo_params* p, uint32_t k, dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !p || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_downsize: null argument");
        if (k > p->k) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_downsize: k is above the params'");
        const bool ipa = p->scheme == DEHALO_SCHEME_IPA;
        if (ipa) TRY(ipa_params_check(ctx, "params_downsize", p->curve, k));
        else TRY(kzg_params_check(ctx, "params_downsize", p->curve, k));
        ParamsParts in = ipa ? ParamsParts{p->curve, k, nullptr, nullptr, p->w, p->u} : ParamsParts{p->curve, k, p->g2, p->s_g2};
        in.g.assign(p->g.begin(), p->g.begin() + ((size_t)8 << k));
        // the first 2^k of g: from the plain points ParamsIPA keeps on the device (when it is this context's device), else from the host copy
        return params_from_g(ctx, std::move(in), ipa && p->d_guw.p && p->ctx && p->ctx->device == ctx->device ? p->d_guw.u64() : nullptr, out);
    });
}
