// params.hip -- the commitment schemes' parameters, the transcript and the IPA opening argument behind the C ABI: ParamsKZG (setup / read / write,
// the three SerdeFormats, from_g, downsize), ParamsIPA, Blake2bWrite, commitment::create_proof of ParamsIPA and the scalar draws [UPSTREAM halo2_proofs @ v2023_04_20: poly/kzg/commitment.rs,
// poly/ipa/commitment.rs, poly/ipa/commitment/prover.rs, transcript.rs] -- the calls the reference makes at benches/delay_enc.rs:41-54 (params) and,
// through create_proof, :120-134 (the Blake2bWrite transcript).
// C entry points run under dh_guard and the column work goes through the library's device entry points, as in prover.hip; the one kernel here is the ChaCha20 draw.
#include <memory>

#include "pairing_host.hpp"
#include "params_format.hpp"
#include "whole_call.hpp"

namespace {

// The ChaCha20 kinds (DEHALO_RNG_OS, DEHALO_RNG_CHACHA20), the vanishing argument's random polynomial (n scalars: 4 MiB at k = 17): generated ON THE DEVICE from
// the proof's ChaCha20 key (32 bytes of operating-system entropy, or the caller's) instead of being drawn on a host thread and uploaded.  Scalar i = the first of
// ChaCha20 blocks (counter low = i, counter high = attempt 0, 1, ...), nonce = the helper's stream, whose first 256 bits masked to the modulus' length are < p
// (chacha_accept, hostrng.hpp): uniform over the field.  The schedule of all draws: include/dehalo.h, dehalo_rng_kind.
// (the block function: chacha_indexed_block, hostrng.hpp, shared with the generator kernel of gfft.cuh)
__global__ void k_chacha_scalars(ChaKey key, u64 stream, fe p, u32 bits, fe* out, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (u32 attempt = 0;; attempt++) {
        fe v;
        chacha_indexed_block(key.k, stream, i, attempt, v.v);
        if (chacha_accept(v.v, p.v, bits)) {
            out[i] = v;
            return;
        }
    }
}

}   // namespace

// the ChaCha20 kinds' indexed draw: key from the proof's generator, modulus and bit length of its field
int chacha_scalars_device(dehalo_ctx* ctx, const HostRng& rng, uint64_t cha_stream, fe* out, size_t n, hipStream_t s) {
    const HostField* f = rng.f;
    ChaKey ck;
    memcpy(ck.k, rng.key, 32);
    fe pw;
    for (int i = 0; i < 4; i++) { pw.v[2 * i] = (u32)f->p[i]; pw.v[2 * i + 1] = (u32)(f->p[i] >> 32); }
    k_chacha_scalars<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(ck, /* stream of the fork */ cha_stream, pw, f->bits, out, n);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ================================================================================================ ParamsKZG
extern "C" int dehalo_params_create(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, const uint8_t* g2, const uint8_t* s_g2,
                                    dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !out || !g || !g_lagrange) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_create: null argument");
        if (k > 28 || curve_scalar_field(curve) < 0) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_create: k or curve out of range");
        std::unique_ptr<dehalo_params> p(new dehalo_params);
        p->ctx = ctx; p->curve = curve; p->k = k; p->n = (size_t)1 << k;
        p->g.assign(g, g + 8 * p->n);
        p->g_lagrange.assign(g_lagrange, g_lagrange + 8 * p->n);
        if (g2) memcpy(p->g2, g2, 128);
        if (s_g2) memcpy(p->s_g2, s_g2, 128);
        TRY(dehalo_bases_register(ctx, curve, g, p->n, 64, 0, 1, adopt(ctx, p->bases_g)));
        TRY(dehalo_bases_register(ctx, curve, g_lagrange, p->n, 64, 0, 1, adopt(ctx, p->bases_gl)));
        *out = p.release();
        return 0;
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
        std::unique_ptr<dehalo_params> p(new dehalo_params);
        p->ctx = ctx; p->curve = curve; p->k = k; p->n = n;
        DevMem dg, dgl;
        TRY(dg.alloc(ctx, 2 * n, false));
        TRY(dgl.alloc(ctx, 2 * n, false));
        TRY(kzg_setup_bn254(ctx, k, sm.v, omega.v, cfac.v, (affine_t*)dg.p, (affine_t*)dgl.p, ctx->stream.get()));
        TRY(dehalo_bases_register_device(ctx, curve, dg.u64(), n, 0, 1, adopt(ctx, p->bases_g)));
        TRY(dehalo_bases_register_device(ctx, curve, dgl.u64(), n, 0, 1, adopt(ctx, p->bases_gl)));
        p->g.resize(8 * n); p->g_lagrange.resize(8 * n);
        TRY(dehalo_download(ctx, dg.p, 64 * n, p->g.data()));
        TRY(dehalo_download(ctx, dgl.p, 64 * n, p->g_lagrange.data()));
        {   // g2 = the generator, s_g2 = [s] g2
            const HostField* q = host_field(curve_base_field(curve));
            G2Host g2(q);
            const G2Host::Pt G = bn254_g2_generator(q);
            const Fe sc = f->to_canonical(sm);
            g2.to_raw(G, p->g2);
            g2.to_raw(g2.scalar_mul(sc.v, G), p->s_g2);
        }
        *out = p.release();
        return 0;
    });
}

extern "C" int dehalo_params_read(dehalo_ctx* ctx, int curve, const uint8_t* bytes, size_t len, dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !bytes || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_read: null argument");
        if (len < 4) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_read: unexpected end of input");
        const uint32_t k = (uint32_t)bytes[0] | ((uint32_t)bytes[1] << 8) | ((uint32_t)bytes[2] << 16) | ((uint32_t)bytes[3] << 24);      // u32 LE
        if (k > 28) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_read: k out of range");
        const size_t n = (size_t)1 << k;
        if (len != 4 + 2 * 64 * n + 256) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_read: length does not match k");
        // (the points are 8-byte aligned only if the caller's buffer is: copy through aligned vectors)
        std::vector<uint64_t> g(8 * n), gl(8 * n);
        memcpy(g.data(), bytes + 4, 64 * n);
        memcpy(gl.data(), bytes + 4 + 64 * n, 64 * n);
        return dehalo_params_create(ctx, curve, k, g.data(), gl.data(), bytes + 4 + 128 * n, bytes + 4 + 128 * n + 128, out);
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

// ================================================================================================ transcript
extern "C" int dehalo_transcript_create(int curve, dehalo_transcript** out) {
    return dh_guard(nullptr, [&]() -> int {
        if (!out || curve_scalar_field(curve) < 0) return DEHALO_ERR_INVALID;
        dehalo_transcript* t = new dehalo_transcript;
        t->init(curve);
        *out = t;
        return 0;
    });
}
extern "C" int dehalo_transcript_common_scalar(dehalo_transcript* t, const uint64_t s[4]) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || !s) return DEHALO_ERR_INVALID;
        Fe v;
        memcpy(v.v, s, 32);
        t->common_scalar(v);
        return 0;
    });
}
extern "C" int dehalo_transcript_write_scalar(dehalo_transcript* t, const uint64_t s[4]) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || !s || t->reader) return DEHALO_ERR_INVALID;
        Fe v;
        memcpy(v.v, s, 32);
        t->write_scalar(v);
        return 0;
    });
}
extern "C" int dehalo_transcript_write_point(dehalo_transcript* t, const uint64_t xy[8]) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || !xy || t->reader) return DEHALO_ERR_INVALID;
        return t->write_point(xy) ? 0 : DEHALO_ERR_INVALID;
    });
}
extern "C" int dehalo_transcript_squeeze_challenge(dehalo_transcript* t, uint64_t out[4]) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || !out) return DEHALO_ERR_INVALID;
        const Fe c = t->squeeze();
        memcpy(out, c.v, 32);
        return 0;
    });
}
extern "C" size_t dehalo_transcript_len(const dehalo_transcript* t) { return t ? t->proof.size() : 0; }
extern "C" int dehalo_transcript_finalize(const dehalo_transcript* t, uint8_t* out, size_t cap) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || (!out && !t->proof.empty())) return DEHALO_ERR_INVALID;
        if (cap < t->proof.size()) return DEHALO_ERR_INVALID;
        if (!t->proof.empty()) memcpy(out, t->proof.data(), t->proof.size());
        return 0;
    });
}
extern "C" void dehalo_transcript_release(dehalo_transcript* t) { delete t; }

// ---- Blake2bRead: the same object over a proof's bytes (copied: the caller's buffer is not retained)
extern "C" int dehalo_transcript_create_read(int curve, const uint8_t* proof, size_t len, dehalo_transcript** out) {
    return dh_guard(nullptr, [&]() -> int {
        if (!out || (!proof && len) || curve_scalar_field(curve) < 0) return DEHALO_ERR_INVALID;
        std::unique_ptr<dehalo_transcript> t(new dehalo_transcript);
        t->init_read(curve, proof, len);
        *out = t.release();
        return 0;
    });
}
extern "C" int dehalo_transcript_read_point(dehalo_transcript* t, uint64_t affine_xy[8]) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || !affine_xy || !t->reader) return DEHALO_ERR_INVALID;
        uint64_t xy[8];
        if (!t->read_point(xy)) return DEHALO_ERR_INVALID;
        memcpy(affine_xy, xy, 64);
        return 0;
    });
}
extern "C" int dehalo_transcript_read_scalar(dehalo_transcript* t, uint64_t s[4]) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || !s || !t->reader) return DEHALO_ERR_INVALID;
        Fe v;
        if (!t->read_scalar(v)) return DEHALO_ERR_INVALID;
        memcpy(s, v.v, 32);
        return 0;
    });
}
extern "C" size_t dehalo_transcript_remaining(const dehalo_transcript* t) { return t && t->reader ? t->remaining() : 0; }

// ================================================================================================ the pairing check (pairing_host.hpp; host only)
extern "C" int dehalo_pairing_check(int curve, const uint64_t* g1_affine_xy, const uint8_t* g2_raw, size_t count, int* is_one) {
    return dh_guard(nullptr, [&]() -> int {
        if (curve_scalar_field(curve) < 0 || !is_one || (count && (!g1_affine_xy || !g2_raw))) return DEHALO_ERR_INVALID;
        const PairingHost* ph = pairing_host(curve);
        if (!ph) return DEHALO_ERR_UNSUPPORTED;      // Pallas and Vesta have no pairing
        return ph->check(g1_affine_xy, g2_raw, count, is_one);
    });
}

// ================================================================================================ ParamsIPA and the IPA opening argument
namespace {

// what dehalo_params_ipa_create and dehalo_params_ipa_from_g share once g_lagrange is known: the two resident MSM tables, g | u | w as plain points on the
// device, the [U | W] registration and W's fixed-base table
int ipa_params_finish(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, const uint64_t w[8], const uint64_t u[8],
                      dehalo_params** out) {
    const size_t n = (size_t)1 << k;
    dehalo_params* raw = nullptr;
    TRY(dehalo_params_create(ctx, curve, k, g, g_lagrange, nullptr, nullptr, &raw));
    std::unique_ptr<dehalo_params> p(raw);
    p->scheme = DEHALO_SCHEME_IPA;
    memcpy(p->w, w, 64);
    memcpy(p->u, u, 64);
    TRY(p->d_guw.alloc(ctx, 2 * (n + 2), false));
    TRY(dh_h2d(ctx, p->d_guw.p, g, 64 * n, ctx->stream.get()));
    TRY(dh_h2d(ctx, p->d_guw.at(2 * n), u, 64, ctx->stream.get()));
    TRY(dh_h2d(ctx, p->d_guw.at(2 * n + 2), w, 64, ctx->stream.get()));
    TRY(dehalo_bases_register_device(ctx, curve, p->d_guw.u64(2 * n), 2, 0, 0, adopt(ctx, p->bases_uw)));
    TRY(dehalo_fixed_base_create(ctx, curve, w, adopt(ctx, p->fb_w)));
    *out = p.release();
    return 0;
}

// the range checks of a ParamsIPA under construction (null arguments are the caller's to report)
int ipa_params_check(dehalo_ctx* ctx, const std::string& who, int curve, uint32_t k) {
    if (curve != DEHALO_CURVE_PALLAS && curve != DEHALO_CURVE_VESTA) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, who + ": IPA over Pallas / Vesta only");
    if (k < 1 || k > 28) return dh_fail(ctx, DEHALO_ERR_INVALID, who + ": k out of range");
    if (!dh_precomputed_table_fits(curve, (size_t)1 << k)) return dh_fail(ctx, DEHALO_ERR_INVALID, who + ": 2^k x windows >= 2^30: precomputed table too large");
    return 0;
}

}   // namespace

extern "C" int dehalo_params_ipa_create(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, const uint64_t w[8],
                                        const uint64_t u[8], dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !out || !g || !g_lagrange || !w || !u) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_create: null argument");
        TRY(ipa_params_check(ctx, "params_ipa_create", curve, k));
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        return ipa_params_finish(ctx, curve, k, g, g_lagrange, w, u, out);
    });
}

// ParamsIPA from g alone: g_lagrange = g_to_lagrange(g) on the device (gfft.cuh), then as dehalo_params_ipa_create
extern "C" int dehalo_params_ipa_from_g(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t* g, const uint64_t w[8], const uint64_t u[8], dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !out || !g || !w || !u) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_from_g: null argument");
        TRY(ipa_params_check(ctx, "params_ipa_from_g", curve, k));
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        const size_t n = (size_t)1 << k;
        DevMem dg, dgl;
        TRY(dg.alloc(ctx, 2 * n, false));
        TRY(dgl.alloc(ctx, 2 * n, false));
        TRY(dh_h2d(ctx, dg.p, g, 64 * n, ctx->stream.get()));
        TRY(dehalo_g_to_lagrange_device(ctx, curve, dg.u64(), k, dgl.u64(), ctx->stream.get()));
        std::vector<uint64_t> gl(8 * n);
        TRY(dehalo_download(ctx, dgl.p, 64 * n, gl.data()));
        return ipa_params_finish(ctx, curve, k, g, gl.data(), w, u, out);
    });
}

// ParamsIPA without a file: g | W | U are generated points (gfft.cuh k_points_generate; the rule: include/dehalo.h), g_lagrange the group FFT of g where it lies,
// then as dehalo_params_ipa_from_g
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
        std::vector<uint64_t> g(8 * n), gl(8 * n), wu(16);
        TRY(dehalo_download(ctx, dg.p, 64 * n, g.data()));
        TRY(dehalo_download(ctx, dgl.p, 64 * n, gl.data()));
        TRY(dehalo_download(ctx, dwu.p, 128, wu.data()));
        return ipa_params_finish(ctx, curve, k, g.data(), gl.data(), wu.data(), wu.data() + 8, out);
    });
}

// ---- ParamsIPA::{write, read} [UPSTREAM halo2_proofs/src/poly/ipa/commitment.rs]: k: u32 LE | g | g_lagrange | w | u, every point GroupEncoding::to_bytes
// (x little-endian canonical, bit 255 = y is odd, the identity all zero: what dehalo_transcript::write_point appends to a proof)
namespace {
void ipa_compress(const HostField* fq, const uint64_t xy[8], uint8_t out[32]) {
    Fe x, y;
    memcpy(x.v, xy, 32);
    memcpy(y.v, xy + 4, 32);
    if (x.is_zero() && y.is_zero()) { memset(out, 0, 32); return; }
    uint8_t yb[32];
    fq->to_bytes(x, out);
    fq->to_bytes(y, yb);
    out[31] |= (uint8_t)((yb[0] & 1) << 7);
}
}   // namespace

extern "C" size_t dehalo_params_ipa_size(const dehalo_params* p) { return p && p->scheme == DEHALO_SCHEME_IPA ? 4 + 2 * 32 * p->n + 64 : 0; }

extern "C" int dehalo_params_ipa_write(const dehalo_params* p, uint8_t* out, size_t cap) {
    return dh_guard(p ? p->ctx : nullptr, [&]() -> int {
        if (!p || !out) return DEHALO_ERR_INVALID;
        if (p->scheme != DEHALO_SCHEME_IPA) return dh_fail(p->ctx, DEHALO_ERR_UNSUPPORTED, "params_ipa_write: not ParamsIPA (ParamsKZG: dehalo_params_write)");
        if (cap < dehalo_params_ipa_size(p)) return dh_fail(p->ctx, DEHALO_ERR_INVALID, "params_ipa_write: buffer too small");
        const HostField* fq = host_field(curve_base_field(p->curve));
        for (int i = 0; i < 4; i++) out[i] = (uint8_t)(p->k >> (8 * i));
        uint8_t* o = out + 4;
        for (size_t i = 0; i < p->n; i++, o += 32) ipa_compress(fq, &p->g[8 * i], o);
        for (size_t i = 0; i < p->n; i++, o += 32) ipa_compress(fq, &p->g_lagrange[8 * i], o);
        ipa_compress(fq, p->w, o);
        ipa_compress(fq, p->u, o + 32);
        return 0;
    });
}

extern "C" int dehalo_params_ipa_read(dehalo_ctx* ctx, int curve, const uint8_t* bytes, size_t len, dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !bytes || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_read: null argument");
        if (len < 4) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_read: unexpected end of input");
        const uint32_t k = (uint32_t)bytes[0] | ((uint32_t)bytes[1] << 8) | ((uint32_t)bytes[2] << 16) | ((uint32_t)bytes[3] << 24);      // u32 LE
        TRY(ipa_params_check(ctx, "params_ipa_read", curve, k));
        const size_t n = (size_t)1 << k, count = 2 * n + 2;
        if (len != 4 + 32 * count) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_read: length does not match k");
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        // the encodings go up as they are and come back as affine points: one lane per point takes the square root (k_decompress, gfft.cuh)
        DevMem enc, pts, status;
        TRY(enc.alloc(ctx, count, false));
        TRY(pts.alloc(ctx, 2 * count, false));
        TRY(status.alloc(ctx, 1, true));
        TRY(dh_h2d(ctx, enc.p, bytes + 4, 32 * count, ctx->stream.get()));
        TRY(gfft_ops(curve)->decompress(ctx, (const uint8_t*)enc.p, (affine_t*)pts.p, count, (uint32_t*)status.p, ctx->stream.get()));
        uint32_t bad[8];
        TRY(dehalo_download(ctx, status.p, 32, bad));
        if (bad[0] & 1u) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_read: an x coordinate is not below the modulus");
        if (bad[0] & 4u) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_read: x = 0 with the sign bit set is not an encoding");
        if (bad[0] & 2u) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_ipa_read: an x coordinate is not on the curve");
        std::vector<uint64_t> host(8 * count);
        TRY(dehalo_download(ctx, pts.p, 64 * count, host.data()));
        return ipa_params_finish(ctx, curve, k, host.data(), host.data() + 8 * n, host.data() + 16 * n, host.data() + 16 * n + 8, out);
    });
}

// ================================================================================================ ParamsKZG from any SRS
// SerdeFormat read / write, ParamsKZG from g alone, Params::downsize [UPSTREAM halo2_proofs/src/poly/kzg/commitment.rs: write_custom, read_custom, from_parts,
// downsize; poly/ipa/commitment.rs: downsize].  Layout, header and the two G2 points: params_format.hpp, on the host; the G1 vectors: the point codec and the
// group FFT, on the device (gfft.cuh).
namespace {

// ParamsKZG over g and g_lagrange as they stand on the device (2^k affine points each, standard Montgomery): both tables registered from there, the
// host copies downloaded -- what dehalo_params_setup does with its own two vectors
int kzg_from_device(dehalo_ctx* ctx, int curve, uint32_t k, const affine_t* d_g, const affine_t* d_gl, const uint8_t* g2, const uint8_t* s_g2, dehalo_params** out) {
    const size_t n = (size_t)1 << k;
    std::unique_ptr<dehalo_params> p(new dehalo_params);
    p->ctx = ctx; p->curve = curve; p->k = k; p->n = n;
    if (g2) memcpy(p->g2, g2, 128);
    if (s_g2) memcpy(p->s_g2, s_g2, 128);
    TRY(dehalo_bases_register_device(ctx, curve, (const uint64_t*)d_g, n, 0, 1, adopt(ctx, p->bases_g)));
    TRY(dehalo_bases_register_device(ctx, curve, (const uint64_t*)d_gl, n, 0, 1, adopt(ctx, p->bases_gl)));
    p->g.resize(8 * n); p->g_lagrange.resize(8 * n);
    TRY(dehalo_download(ctx, d_g, 64 * n, p->g.data()));
    TRY(dehalo_download(ctx, d_gl, 64 * n, p->g_lagrange.data()));
    *out = p.release();
    return 0;
}

// the range checks of a ParamsKZG built here, before any device work: the two precomputed tables must fit (as dehalo_params_setup checks)
int kzg_params_check(dehalo_ctx* ctx, const std::string& who, int curve, uint32_t k) {
    const HostField* f = host_field(curve_scalar_field(curve));
    if (!f) return dh_fail(ctx, DEHALO_ERR_INVALID, who + ": unknown curve");
    if (k > PARAMS_MAX_K || k > f->two_adicity) return dh_fail(ctx, DEHALO_ERR_INVALID, who + ": k out of range");
    if (!dh_precomputed_table_fits(curve, (size_t)1 << k)) return dh_fail(ctx, DEHALO_ERR_INVALID, who + ": 2^k x windows >= 2^30: precomputed table too large");
    return 0;
}

const char* point_status_text(uint32_t status, bool encodings) {
    if (status & POINT_NOT_BELOW_P) return encodings ? "an x coordinate is not below the modulus" : "a coordinate's stored word is not below the modulus";
    if (status & POINT_ZERO_X_SIGNED) return "x = 0 with the sign bit set is not an encoding";
    if (status & POINT_NOT_ON_CURVE) return encodings ? "an x coordinate is not on the curve" : "a point is neither on the curve nor the identity";
    return "";
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
        const affine_t* d_gl = (const affine_t*)pts.at(2 * n);
        if (!keep) {
            TRY(gl.alloc(ctx, 2 * n, false));
            TRY(dehalo_g_to_lagrange_device(ctx, curve, pts.u64(), k, gl.u64(), ctx->stream.get()));
            d_gl = (const affine_t*)gl.p;
        }
        return kzg_from_device(ctx, curve, k, (const affine_t*)pts.p, d_gl, g2raw, sg2raw, out);
    });
}

extern "C" int dehalo_params_from_g(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t* g, const uint8_t* g2, const uint8_t* s_g2, dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !out || !g) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_from_g: null argument");
        TRY(kzg_params_check(ctx, "params_from_g", curve, k));
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        const size_t n = (size_t)1 << k;
        DevMem dg, dgl;
        TRY(dg.alloc(ctx, 2 * n, false));
        TRY(dgl.alloc(ctx, 2 * n, false));
        TRY(dh_h2d(ctx, dg.p, g, 64 * n, ctx->stream.get()));
        TRY(dehalo_g_to_lagrange_device(ctx, curve, dg.u64(), k, dgl.u64(), ctx->stream.get()));
        return kzg_from_device(ctx, curve, k, (const affine_t*)dg.p, (const affine_t*)dgl.p, g2, s_g2, out);
    });
}

extern "C" int dehalo_params_downsize(dehalo_ctx* ctx, const dehalo_params* p, uint32_t k, dehalo_params** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !p || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_downsize: null argument");
        if (k > p->k) return dh_fail(ctx, DEHALO_ERR_INVALID, "params_downsize: k is above the params'");
        const bool ipa = p->scheme == DEHALO_SCHEME_IPA;
        if (ipa) TRY(ipa_params_check(ctx, "params_downsize", p->curve, k));
        else TRY(kzg_params_check(ctx, "params_downsize", p->curve, k));
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        const size_t n = (size_t)1 << k;
        DevMem dg, dgl;
        TRY(dg.alloc(ctx, 2 * n, false));
        TRY(dgl.alloc(ctx, 2 * n, false));
        // the first 2^k of g: from the plain points ParamsIPA keeps on the device (when it is this context's device), else from the host copy
        if (ipa && p->d_guw.p && p->ctx && p->ctx->device == ctx->device) HIP_TRY(ctx, hipMemcpyAsync(dg.p, p->d_guw.p, 64 * n, hipMemcpyDeviceToDevice, ctx->stream.get()));
        else TRY(dh_h2d(ctx, dg.p, p->g.data(), 64 * n, ctx->stream.get()));
        TRY(dehalo_g_to_lagrange_device(ctx, p->curve, dg.u64(), k, dgl.u64(), ctx->stream.get()));
        if (!ipa) return kzg_from_device(ctx, p->curve, k, (const affine_t*)dg.p, (const affine_t*)dgl.p, p->g2, p->s_g2, out);
        std::vector<uint64_t> gl(8 * n);
        TRY(dehalo_download(ctx, dgl.p, 64 * n, gl.data()));
        return ipa_params_finish(ctx, p->curve, k, p->g.data(), gl.data(), p->w, p->u, out);
    });
}

extern "C" int dehalo_params_scheme(const dehalo_params* p) { return p ? p->scheme : DEHALO_ERR_INVALID; }
extern "C" const dehalo_fixed_base* dehalo_params_fixed_base(const dehalo_params* p) { return p ? p->fb_w.get() : nullptr; }

namespace {

// commit(poly, blind) of ParamsIPA = MSM(poly, g) + [blind] W, affine into d_pts[0 .. 8) (d_pts: 8 field elements of scratch = 32 u64; the Jacobian
// result sits in [8, 20), the blind in [20, 24)): the MSM, [blind] W from W's table on top of it, one normalisation -- all on the stream
int ipa_commit_blinded(dehalo_ctx* ctx, const dehalo_params* p, const uint64_t* d_poly, const Fe& blind, uint64_t* d_pts, hipStream_t s) {
    TRY(dh_h2d(ctx, d_pts + 20, blind.v, 32, s));
    TRY(dehalo_msm_device(ctx, p->bases_g.get(), d_poly, p->n, 1, d_pts + 8, s));
    TRY(dehalo_fixed_base_blind_device(ctx, p->fb_w.get(), d_pts + 8, d_pts + 20, 1, s));
    return dehalo_to_affine_device(ctx, p->curve, d_pts + 8, 1, d_pts, s);
}

}   // namespace

// commitment::create_proof on `rng` as it stands (dehalo_ipa_open: a fresh generator; a whole proof: the proof's generator, right behind f's blind).
// cha_stream: the ChaCha20 stream of the n-scalar draw under the ChaCha20 kinds -- within one proof it must differ from the random polynomial's (1).
int ipa_open_body(dehalo_ctx* ctx, const dehalo_params* p, const uint64_t* d_poly, const Fe& blind, const Fe& x3, HostRng& rng, uint64_t cha_stream, dehalo_transcript* t) {
        const hipStream_t s = ctx->stream.get();
        const int fid = curve_scalar_field(p->curve);
        const HostField* f = host_field(fid);
        const IpaOps* ops = ipa_ops(p->curve);
        const size_t n = p->n;
        const uint32_t k = p->k;
        DevMem s_poly, s_adj, pa, pb, guw, sc, ev, rr, pts, uwsc;
        TRY(s_poly.alloc(ctx, n, false));
        TRY(s_adj.alloc(ctx, n, false));
        TRY(pa.alloc(ctx, n, false));
        TRY(pb.alloc(ctx, n, false));
        TRY(guw.alloc(ctx, n + 4, false));           // G' of rounds 2.., then U, W: n / 2 + 2 points of 2 elements
        TRY(sc.alloc(ctx, 2 * n, false));
        TRY(ev.alloc(ctx, 2, false));
        TRY(rr.alloc(ctx, 2 * (size_t)k, false));
        TRY(pts.alloc(ctx, 8, false));
        TRY(uwsc.alloc(ctx, 4, false));
        // ---- draws, in upstream's order: s_poly (n), s_poly_blind, (l_rand, r_rand) per round.  The n scalars are the proof's large draw and come, as
        // the prover's random polynomial does, from the generator forked at their position: for the ChaCha20 kinds a ChaCha20 kernel under the call's key
        // (stream 1); for PCG64 / a callback the fork yields exactly the scalars a serial draw would, drawn on the host and uploaded.
        HostRng rng_poly = rng.fork(0, cha_stream);
        rng.skip(n);
        Fe s_blind;
        std::vector<uint64_t> rands(8 * (size_t)k);
        TRY(rng.scalars(s_blind.v, 1));
        TRY(rng.scalars(rands.data(), 2 * (size_t)k));
        if (rng.chacha()) TRY(chacha_scalars_device(ctx, rng, cha_stream, s_poly.p, n, s));
        else {
            std::vector<uint64_t> s_host(4 * n);
            TRY(rng_poly.scalars(s_host.data(), n));
            TRY(dh_h2d(ctx, s_poly.p, s_host.data(), 32 * n, s));
        }
        TRY(dh_h2d(ctx, rr.p, rands.data(), 64 * (size_t)k, s));
        // ---- s(x3) and p(x3); s_poly[0] -= s(x3)
        TRY(dehalo_eval_polynomial_device(ctx, fid, s_poly.u64(), n, n, 1, x3.v, ev.u64(0), s));
        TRY(dehalo_eval_polynomial_device(ctx, fid, d_poly, n, n, 1, x3.v, ev.u64(1), s));
        Fe at[2];
        TRY(dehalo_download(ctx, ev.p, 64, at));
        const uint64_t* one_col[1] = {s_poly.u64()};
        TRY(dehalo_lincomb_device(ctx, fid, one_col, f->one.v, 1, n, s_adj.u64(), at[0].v, s));
        // ---- S = commit(s_poly, s_poly_blind)
        TRY(ipa_commit_blinded(ctx, p, s_adj.u64(), s_blind, pts.u64(), s));
        uint64_t S[8];
        TRY(dehalo_download(ctx, pts.p, 64, S));
        if (!t->write_point(S)) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_open: s_poly commitment at infinity");
        const Fe xi = t->squeeze();
        const Fe z = t->squeeze();
        // ---- p' = p + xi s, p'[0] -= p'(x3) (= p(x3): s(x3) = 0 now); f = s_poly_blind xi + blind
        {
            const uint64_t* cols[2] = {d_poly, s_adj.u64()};
            Fe coefs[2] = {f->one, xi};
            TRY(dehalo_lincomb_device(ctx, fid, cols, coefs[0].v, 2, n, pa.u64(), at[1].v, s));
        }
        Fe fsum = f->add(f->mul(s_blind, xi), blind);
        // ---- k rounds; b stays geometric: b^(j)[i] = c_j x3^i.  Round 1 runs over the resident precomputed table of g (its [U | W] terms over
        // bases_uw, added by a collapse with u = 1); rounds 2.. over one plain registration of [G' | U | W], rebuilt on the stream each round.
        BasesPtr breg;
        TRY(dh_bases_plain_alloc(ctx, p->curve, n / 2 + 2, breg));
        std::vector<Fe> x3_pow(k + 1);           // x3^(2^i)
        x3_pow[0] = x3;
        for (uint32_t i = 1; i <= k; i++) x3_pow[i] = f->sqr(x3_pow[i - 1]);
        Fe c = f->one;
        DevMem* cur = &pa;
        DevMem* nxt = &pb;
        for (uint32_t j = 0; j < k; j++) {
            const size_t nj = n >> j, half = nj / 2, m = j == 0 ? nj : nj + 2;
            const Fe x3h = x3_pow[k - 1 - j];                  // x3^half
            // scalars: L = [p'_hi | 0 | z value_l | l_rand], R = [0 | p'_lo | z value_r | r_rand] (round 1: the [U | W] slots in uwsc)
            fe* sl = sc.at(0);
            fe* sr = sc.at(m);
            HIP_TRY(ctx, hipMemcpyAsync(sl, cur->at(half), 32 * half, hipMemcpyDeviceToDevice, s));
            HIP_TRY(ctx, hipMemsetAsync(sl + half, 0, 32 * half, s));
            HIP_TRY(ctx, hipMemsetAsync(sr, 0, 32 * half, s));
            HIP_TRY(ctx, hipMemcpyAsync(sr + half, cur->p, 32 * half, hipMemcpyDeviceToDevice, s));
            TRY(dehalo_eval_polynomial_device(ctx, fid, cur->u64(), half, half, 2, x3.v, ev.u64(), s));      // p'_lo(x3), p'_hi(x3)
            const Fe zc = f->mul(z, c), zch = f->mul(zc, x3h);
            if (j == 0) {
                TRY(ops->slots(ctx, ev.p, zc.v, zch.v, rr.at(0), uwsc.at(0), uwsc.at(2), s));
                TRY(dehalo_msm_device_affine(ctx, p->bases_g.get(), sc.u64(), n, 2, nullptr, pts.u64(0), s));       // L_g, R_g
                TRY(dehalo_msm_device_affine(ctx, p->bases_uw.get(), uwsc.u64(), 2, 2, nullptr, pts.u64(4), s));    // L_uw, R_uw (points 2, 3)
                const uint64_t one_m[4] = {f->one.v[0], f->one.v[1], f->one.v[2], f->one.v[3]};
                TRY(dehalo_generator_collapse_device(ctx, p->curve, pts.u64(), 4, one_m, pts.u64(), s));      // [L_g + L_uw, R_g + R_uw]
            } else {
                TRY(ops->slots(ctx, ev.p, zc.v, zch.v, rr.at(2 * j), sl + nj, sr + nj, s));
                HIP_TRY(ctx, hipMemcpyAsync(guw.at(2 * nj), p->d_guw.at(2 * n), 128, hipMemcpyDeviceToDevice, s));     // U, W behind G'
                TRY(dh_bases_plain_rebuild(ctx, breg.get(), (const affine_t*)guw.p, m, s));
                TRY(dehalo_msm_device_affine(ctx, breg.get(), sc.u64(), m, 2, nullptr, pts.u64(), s));
            }
            uint64_t LR[16];
            TRY(dehalo_download(ctx, pts.p, 128, LR));      // the round's one host wait
            if (!t->write_point(LR) || !t->write_point(LR + 8)) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_open: L_j or R_j at infinity");
            const Fe u = t->squeeze();
            const Fe u_inv = f->invert(u);
            Fe lr, rrnd;
            memcpy(lr.v, &rands[8 * j], 32);
            memcpy(rrnd.v, &rands[8 * j + 4], 32);
            fsum = f->add(fsum, f->add(f->mul(lr, u_inv), f->mul(rrnd, u)));
            c = f->mul(c, f->add(f->one, f->mul(u, x3h)));
            // p' <- p'_lo + u^-1 p'_hi (into the other buffer: lincomb's out may alias no column); G' <- G'_lo + [u] G'_hi (round 1 reads g, later
            // rounds collapse in place; the last round's G' would never be read)
            const uint64_t* cols[2] = {cur->u64(), cur->u64(half)};
            Fe coefs[2] = {f->one, u_inv};
            TRY(dehalo_lincomb_device(ctx, fid, cols, coefs[0].v, 2, half, nxt->u64(), nullptr, s));
            if (j + 1 < k) TRY(dehalo_generator_collapse_device(ctx, p->curve, j == 0 ? p->d_guw.u64() : guw.u64(), nj, u.v, guw.u64(), s));
            std::swap(cur, nxt);
        }
        Fe cfin;
        TRY(dehalo_download(ctx, cur->p, 32, cfin.v));
        t->write_scalar(cfin);
        t->write_scalar(fsum);
        return 0;
}

extern "C" int dehalo_ipa_open(dehalo_ctx* ctx, const dehalo_params* p, const uint64_t* d_poly, const uint64_t blind_in[4], const uint64_t x3_in[4], dehalo_rng* rng_in,
                               dehalo_transcript* t) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !p || !d_poly || !blind_in || !x3_in || !t) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_open: null argument");
        if (p->scheme != DEHALO_SCHEME_IPA) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_open: needs ParamsIPA (dehalo_params_ipa_create)");
        if (t->curve != p->curve) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_open: transcript and params disagree on the curve");
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        Fe blind, x3;
        memcpy(blind.v, blind_in, 32);
        memcpy(x3.v, x3_in, 32);
        HostRng rng;
        TRY(rng.init(rng_in, host_field(curve_scalar_field(p->curve))));
        TRY(ipa_open_body(ctx, p, d_poly, blind, x3, rng, 1, t));
        rng.write_back(rng_in);
        return 0;
    });
}

extern "C" int dehalo_field_info(int field, uint64_t out[24]) {
    return dh_guard(nullptr, [&]() -> int {
        const HostField* f = host_field(field);
        if (!f || !out) return DEHALO_ERR_INVALID;
        memcpy(out, f->p, 32);
        memcpy(out + 4, f->one.v, 32);
        memcpy(out + 8, f->root_of_unity.v, 32);
        memcpy(out + 12, f->zeta.v, 32);
        memcpy(out + 16, f->delta.v, 32);
        memcpy(out + 20, f->gen.v, 32);
        return 0;
    });
}

extern "C" int dehalo_rng_scalars(dehalo_rng* rng, int field, uint64_t skip, uint64_t* out, size_t count) {
    return dh_guard(nullptr, [&]() -> int {
        const HostField* f = host_field(field);
        if (!f || (!out && count)) return DEHALO_ERR_INVALID;
        HostRng r;
        TRY(r.init(rng, f));
        r.skip(skip);
        return r.scalars(out, count);
    });
}

extern "C" int dehalo_rng_scalars_device(dehalo_ctx* ctx, dehalo_rng* rng, int field, uint64_t cha_stream, uint64_t* d_out, size_t n, void* stream) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx) return DEHALO_ERR_INVALID;
        const HostField* f = host_field(field);
        if (!f) return dh_fail(ctx, DEHALO_ERR_INVALID, "rng_scalars_device: unknown field");
        if (!rng || rng->kind != DEHALO_RNG_CHACHA20) return dh_fail(ctx, DEHALO_ERR_INVALID, "rng_scalars_device: needs a keyed ChaCha20 generator (kind 3)");
        if (n >= ((size_t)1 << 29)) return dh_fail(ctx, DEHALO_ERR_INVALID, "rng_scalars_device: too many scalars");
        if (n == 0) return 0;
        if (!d_out) return dh_fail(ctx, DEHALO_ERR_INVALID, "rng_scalars_device: null output");
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        HostRng r;
        TRY(r.init(rng, f));
        return chacha_scalars_device(ctx, r, cha_stream, (fe*)d_out, n, pick_stream(ctx, stream));
    });
}
