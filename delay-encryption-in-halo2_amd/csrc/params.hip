// params.hip -- the commitment schemes' parameters, the transcript and the IPA opening argument behind the C ABI: ParamsKZG (setup / read / write),
// ParamsIPA, Blake2bWrite, commitment::create_proof of ParamsIPA and the scalar draws [UPSTREAM halo2_proofs @ v2023_04_20: poly/kzg/commitment.rs,
// poly/ipa/commitment.rs, poly/ipa/commitment/prover.rs, transcript.rs] -- the calls the reference makes at benches/delay_enc.rs:41-54 (params) and,
// through create_proof, :120-134 (the Blake2bWrite transcript).
// C entry points run under dh_guard and the column work goes through the library's device entry points, as in prover.hip; the one kernel here is the ChaCha20 draw.
#include <memory>

#include "whole_call.hpp"

namespace {

// The ChaCha20 kinds (DEHALO_RNG_OS, DEHALO_RNG_CHACHA20), the vanishing argument's random polynomial (n scalars: 4 MiB at k = 17): generated ON THE DEVICE from
// the proof's ChaCha20 key (32 bytes of operating-system entropy, or the caller's) instead of being drawn on a host thread and uploaded.  Scalar i = the first of
// ChaCha20 blocks (counter low = i, counter high = attempt 0, 1, ...), nonce = the helper's stream, whose first 256 bits masked to the modulus' length are < p
// (chacha_accept, hostrng.hpp): uniform over the field.  The schedule of all draws: include/dehalo.h, dehalo_rng_kind.
struct ChaKey { u32 k[8]; };
__device__ __forceinline__ u32 cha_rotl(u32 x, int n) { return (x << n) | (x >> (32 - n)); }
__global__ void k_chacha_scalars(ChaKey key, u64 stream, fe p, u32 bits, fe* out, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (u32 attempt = 0;; attempt++) {
        u32 st[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key.k[0], key.k[1], key.k[2], key.k[3], key.k[4], key.k[5], key.k[6], key.k[7],
                      (u32)i, ((u32)(i >> 32) & 0xffffu) | (attempt << 16), (u32)stream, (u32)(stream >> 32)};
        u32 x[16];
#pragma unroll
        for (int j = 0; j < 16; j++) x[j] = st[j];
#define CHA_QR(a, b, c, d)                                                                                         \
    x[a] += x[b]; x[d] = cha_rotl(x[d] ^ x[a], 16); x[c] += x[d]; x[b] = cha_rotl(x[b] ^ x[c], 12);                \
    x[a] += x[b]; x[d] = cha_rotl(x[d] ^ x[a], 8);  x[c] += x[d]; x[b] = cha_rotl(x[b] ^ x[c], 7);
        for (int r = 0; r < 10; r++) {
            CHA_QR(0, 4, 8, 12) CHA_QR(1, 5, 9, 13) CHA_QR(2, 6, 10, 14) CHA_QR(3, 7, 11, 15)
            CHA_QR(0, 5, 10, 15) CHA_QR(1, 6, 11, 12) CHA_QR(2, 7, 8, 13) CHA_QR(3, 4, 9, 14)
        }
#undef CHA_QR
        fe v;
#pragma unroll
        for (int j = 0; j < 8; j++) v.v[j] = x[j] + st[j];
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

// ---- ParamsKZG::setup: the two G2 points on the host (O(1): one 254-bit scalar multiplication over Fq2 = Fq[i] / (i^2 + 1)) -------------------
namespace {
struct Fq2 { Fe a, b; };
struct G2Host {
    const HostField* q;
    explicit G2Host(const HostField* f) : q(f) {}
    Fq2 add(const Fq2& x, const Fq2& y) const { return {q->add(x.a, y.a), q->add(x.b, y.b)}; }
    Fq2 sub(const Fq2& x, const Fq2& y) const { return {q->sub(x.a, y.a), q->sub(x.b, y.b)}; }
    Fq2 mul(const Fq2& x, const Fq2& y) const { return {q->sub(q->mul(x.a, y.a), q->mul(x.b, y.b)), q->add(q->mul(x.a, y.b), q->mul(x.b, y.a))}; }
    Fq2 inv(const Fq2& x) const {
        const Fe d = q->invert(q->add(q->sqr(x.a), q->sqr(x.b)));
        return {q->mul(x.a, d), q->neg(q->mul(x.b, d))};
    }
    bool is_zero(const Fq2& x) const { return x.a.is_zero() && x.b.is_zero(); }
    struct Pt { Fq2 x, y; bool inf; };
    Pt padd(const Pt& P, const Pt& Q) const {      // affine chord-and-tangent (a = 0): 381 inversions for one scalar multiplication are nothing here
        if (P.inf) return Q;
        if (Q.inf) return P;
        Fq2 lam;
        if (is_zero(sub(P.x, Q.x))) {
            if (is_zero(add(P.y, Q.y))) return Pt{{}, {}, true};
            const Fq2 xx = mul(P.x, P.x);
            lam = mul(add(add(xx, xx), xx), inv(add(P.y, P.y)));
        } else lam = mul(sub(Q.y, P.y), inv(sub(Q.x, P.x)));
        Pt R;
        R.inf = false;
        R.x = sub(sub(mul(lam, lam), P.x), Q.x);
        R.y = sub(mul(lam, sub(P.x, R.x)), P.y);
        return R;
    }
    Pt scalar_mul(const uint64_t k_canonical[4], Pt P) const {
        Pt acc{{}, {}, true};
        for (int i = 0; i < 256; i++) {
            if ((k_canonical[i >> 6] >> (i & 63)) & 1) acc = padd(acc, P);
            P = padd(P, P);
        }
        return acc;
    }
    void to_raw(const Pt& P, uint8_t out[128]) const {      // G2Affine RawBytes: x.c0 | x.c1 | y.c0 | y.c1, Montgomery limbs; all zero = identity
        memset(out, 0, 128);
        if (P.inf) return;
        memcpy(out, P.x.a.v, 32); memcpy(out + 32, P.x.b.v, 32); memcpy(out + 64, P.y.a.v, 32); memcpy(out + 96, P.y.b.v, 32);
    }
};
// the generator of BN254's G2 (halo2curves bn256::G2Affine::generator(); canonical limbs)
const uint64_t BN254_G2_GEN[4][4] = {{0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull},
                                     {0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull},
                                     {0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull},
                                     {0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull}};
}   // namespace

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
            G2Host::Pt G;
            G.inf = false;
            Fe c[4];
            for (int i = 0; i < 4; i++) { memcpy(c[i].v, BN254_G2_GEN[i], 32); c[i] = q->from_canonical(c[i]); }
            G.x = {c[0], c[1]}; G.y = {c[2], c[3]};
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
        if (!t || !s) return DEHALO_ERR_INVALID;
        Fe v;
        memcpy(v.v, s, 32);
        t->write_scalar(v);
        return 0;
    });
}
extern "C" int dehalo_transcript_write_point(dehalo_transcript* t, const uint64_t xy[8]) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || !xy) return DEHALO_ERR_INVALID;
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
