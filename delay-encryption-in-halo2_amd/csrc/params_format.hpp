// params_format.hpp -- ParamsKZG on disk in upstream's three SerdeFormats [UPSTREAM halo2_proofs/src/poly/kzg/commitment.rs write_custom / read_custom,
// halo2curves 0.3.x serde.rs and the curves' GroupEncoding]: the layout of  k: u32 LE | g | g_lagrange | g2 | s_g2  per format, the validation of a
// file's length against its k, and the G2 codec over Fq2 = Fq[i] / (i^2 + 1) on the host (two points per file: nothing for the device).  The G1 vectors
// are the device's (gfft.cuh: k_decompress, k_compress, k_points_check).
// Host only, no HIP header: params.hip includes it, and tests/native_host/params_format_check.cpp drives it on the CPU against the Python mirror
// (keygen.py) -- this is the parser of untrusted bytes.
// The formats restate halo2curves 0.3.x from memory, as the other formats here do.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/dehalo.h"
#include "g1_host.hpp"      // the point codec's status bits (POINT_*), serde_format_known
#include "hostfield.hpp"

// ---- layout -------------------------------------------------------------------------------------------------------------------------------------
// G1: 32 B compressed (Processed) or 64 B raw; G2: 64 B compressed or 128 B raw.  Processed is 4 + 64 n + 128 bytes, both raw formats 4 + 128 n + 256.
struct ParamsLayout {
    uint32_t k = 0;
    size_t n = 0, g1 = 0, g2 = 0;                        // points per vector, bytes per G1 / G2 point
    size_t off_g = 0, off_gl = 0, off_g2 = 0, off_sg2 = 0, size = 0;
};
constexpr uint32_t PARAMS_MAX_K = 28;

// false for an unknown format or k > 28 (at k = 28 the largest size is 4 + 2^35 + 256: far inside 64 bits; size_t narrower than that is refused)
inline bool params_layout(int format, uint32_t k, ParamsLayout& L) {
    if (!serde_format_known(format) || k > PARAMS_MAX_K) return false;
    const uint64_t n = (uint64_t)1 << k, g1 = format == DEHALO_SERDE_PROCESSED ? 32 : 64, g2 = 2 * g1;
    const uint64_t size = 4 + 2 * g1 * n + 2 * g2;
    if (size > (uint64_t)SIZE_MAX) return false;
    L.k = k; L.n = (size_t)n; L.g1 = (size_t)g1; L.g2 = (size_t)g2;
    L.off_g = 4; L.off_gl = (size_t)(4 + g1 * n); L.off_g2 = (size_t)(4 + 2 * g1 * n); L.off_sg2 = L.off_g2 + L.g2; L.size = (size_t)size;
    return true;
}

enum ParamsHeaderError { PARAMS_HEADER_OK = 0, PARAMS_HEADER_FORMAT, PARAMS_HEADER_SHORT, PARAMS_HEADER_K, PARAMS_HEADER_LENGTH };
inline const char* params_header_error_text(int e) {
    static const char* const text[] = {"", "unknown format", "unexpected end of input", "k out of range", "length does not match k"};
    return e >= 0 && e <= PARAMS_HEADER_LENGTH ? text[e] : "";
}
// k: u32 LE, the first word of every params file (ParamsKZG in each format, ParamsIPA)
inline uint32_t params_u32_le(const uint8_t* b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24); }
// The header of `len` bytes in `format`: reads bytes[0 .. 4) only, and only when len >= 4; the length must be exactly the layout's.
inline ParamsHeaderError params_parse_header(const uint8_t* bytes, size_t len, int format, ParamsLayout& L) {
    if (!serde_format_known(format)) return PARAMS_HEADER_FORMAT;
    if (len < 4) return PARAMS_HEADER_SHORT;
    const uint32_t k = params_u32_le(bytes);
    if (!params_layout(format, k, L)) return PARAMS_HEADER_K;
    if (len != L.size) return PARAMS_HEADER_LENGTH;
    return PARAMS_HEADER_OK;
}

// ---- G2 on the host ---------------------------------------------------------------------------------------------------------------------------
struct Fq2 { Fe a, b; };      // a + b i, Montgomery

struct G2Host {
    const HostField* q;
    explicit G2Host(const HostField* f) : q(f) {}
    Fq2 add(const Fq2& x, const Fq2& y) const { return {q->add(x.a, y.a), q->add(x.b, y.b)}; }
    Fq2 sub(const Fq2& x, const Fq2& y) const { return {q->sub(x.a, y.a), q->sub(x.b, y.b)}; }
    Fq2 neg(const Fq2& x) const { return {q->neg(x.a), q->neg(x.b)}; }
    Fq2 mul(const Fq2& x, const Fq2& y) const { return {q->sub(q->mul(x.a, y.a), q->mul(x.b, y.b)), q->add(q->mul(x.a, y.b), q->mul(x.b, y.a))}; }
    Fq2 inv(const Fq2& x) const {
        const Fe d = q->invert(q->add(q->sqr(x.a), q->sqr(x.b)));
        return {q->mul(x.a, d), q->neg(q->mul(x.b, d))};
    }
    bool is_zero(const Fq2& x) const { return x.a.is_zero() && x.b.is_zero(); }
    bool eq(const Fq2& x, const Fq2& y) const { return x.a == y.a && x.b == y.b; }
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

    // ---- the curve: y^2 = x^3 + b', b' = 3 / (9 + i) (the sextic twist; computed here, not typed)
    Fq2 twist_b() const { return mul({q->from_u64(3), Fe{}}, inv({q->from_u64(9), q->one})); }
    bool on_curve(const Pt& P) const { return P.inf || eq(mul(P.y, P.y), add(mul(mul(P.x, P.x), P.x), twist_b())); }

    // ---- square roots; q = 3 (mod 4) [BN254's base field]
    bool fq_sqrt(const Fe& a, Fe& r) const {      // r = a^((q + 1) / 4); true when r^2 = a
        uint64_t e[4];
        const uint64_t one[4] = {1, 0, 0, 0};
        HostField::add_limbs(e, q->p, one);      // q + 1 < 2^256
        for (int i = 0; i < 3; i++) e[i] = (e[i] >> 2) | (e[i + 1] << 62);
        e[3] >>= 2;
        r = q->pow(a, e);
        return q->sqr(r) == a;
    }
    // a = a0 + a1 i.  a1 = 0: sqrt(a0), or i sqrt(-a0) when a0 is a non-residue (one of the two always is a square).  Otherwise through the norm:
    // with n = sqrt(a0^2 + a1^2), x0^2 = (a0 + n) / 2 or (a0 - n) / 2, whichever is a square, and x1 = a1 / (2 x0).  False: a is not a square.
    bool fq2_sqrt(const Fq2& a, Fq2& r) const {
        Fe s;
        if (a.b.is_zero()) {
            if (fq_sqrt(a.a, s)) { r = {s, Fe{}}; return true; }
            if (fq_sqrt(q->neg(a.a), s)) { r = {Fe{}, s}; return true; }
            return false;
        }
        Fe n;
        if (!fq_sqrt(q->add(q->sqr(a.a), q->sqr(a.b)), n)) return false;
        const Fe half = q->invert(q->from_u64(2));
        Fe x0;
        if (!fq_sqrt(q->mul(q->add(a.a, n), half), x0) && !fq_sqrt(q->mul(q->sub(a.a, n), half), x0)) return false;
        if (x0.is_zero()) return false;
        r = {x0, q->mul(a.b, q->invert(q->add(x0, x0)))};
        return eq(mul(r, r), a);
    }

    // ---- the two encodings of a point, on the raw bytes a ParamsKZG keeps (to_raw's)
    static bool below_p(const HostField* f, const Fe& a) { return !HostField::geq(a.v, f->p); }
    static Fe load(const uint8_t* b) { Fe r; memcpy(r.v, b, 32); return r; }
    // 0, or POINT_NOT_BELOW_P (a stored coordinate word is not below q) / POINT_NOT_ON_CURVE (neither on the curve nor all zero); P is set when 0
    int from_raw_checked(const uint8_t raw[128], Pt& P) const {
        const Fe c[4] = {load(raw), load(raw + 32), load(raw + 64), load(raw + 96)};
        for (int i = 0; i < 4; i++)
            if (!below_p(q, c[i])) return POINT_NOT_BELOW_P;
        P.x = {c[0], c[1]}; P.y = {c[2], c[3]};
        P.inf = is_zero(P.x) && is_zero(P.y);
        return on_curve(P) ? 0 : POINT_NOT_ON_CURVE;
    }
    // GroupEncoding::to_bytes: x.c0 | x.c1, 32 B little-endian canonical each; bit 7 of byte 63 = y.c0 is odd; the identity all zero
    void compress_raw(const uint8_t raw[128], uint8_t out[64]) const {
        const Fe c[3] = {load(raw), load(raw + 32), load(raw + 64)};
        memset(out, 0, 64);
        if (c[0].is_zero() && c[1].is_zero() && c[2].is_zero() && load(raw + 96).is_zero()) return;
        q->to_bytes(c[0], out);
        q->to_bytes(c[1], out + 32);
        uint8_t y0[32];
        q->to_bytes(c[2], y0);
        out[63] |= (uint8_t)((y0[0] & 1) << 7);
    }
    // GroupEncoding::from_bytes into raw bytes: 0, or POINT_NOT_BELOW_P (x.c0 or x.c1 not canonical) / POINT_NOT_ON_CURVE (x^3 + b' is not a square) /
    // POINT_ZERO_X_SIGNED (x = 0 with the sign bit set)
    int decompress_raw(const uint8_t in[64], uint8_t raw[128]) const {
        memset(raw, 0, 128);
        Fe x0 = load(in), x1 = load(in + 32);
        const unsigned sign = (unsigned)(x1.v[3] >> 63);
        x1.v[3] &= ~((uint64_t)1 << 63);
        if (!below_p(q, x0) || !below_p(q, x1)) return POINT_NOT_BELOW_P;
        if (x0.is_zero() && x1.is_zero()) return sign ? POINT_ZERO_X_SIGNED : 0;
        Pt P;
        P.inf = false;
        P.x = {q->from_canonical(x0), q->from_canonical(x1)};
        if (!fq2_sqrt(add(mul(mul(P.x, P.x), P.x), twist_b()), P.y)) return POINT_NOT_ON_CURVE;
        if ((unsigned)(q->to_canonical(P.y.a).v[0] & 1) != sign) P.y = neg(P.y);
        to_raw(P, raw);
        return 0;
    }
};

// the generator of BN254's G2 (halo2curves bn256::G2Affine::generator(); canonical limbs: x.c0, x.c1, y.c0, y.c1)
constexpr uint64_t BN254_G2_GEN[4][4] = {{0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull},
                                         {0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull},
                                         {0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull},
                                         {0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull}};
inline G2Host::Pt bn254_g2_generator(const HostField* q) {
    Fe c[4];
    for (int i = 0; i < 4; i++) { memcpy(c[i].v, BN254_G2_GEN[i], 32); c[i] = q->from_canonical(c[i]); }
    G2Host::Pt G;
    G.inf = false;
    G.x = {c[0], c[1]}; G.y = {c[2], c[3]};
    return G;
}
