// g1_host.hpp -- G1 points on the host: the status bits of the point codec and their text, the curve constant, GroupEncoding::to_bytes / from_bytes of one
// point [UPSTREAM halo2curves 0.3.x: the curves' GroupEncoding] and the group law.  The one host home of these: the transcript (transcript_host.hpp), the params'
// files (params.hip, params_format.hpp), the keys' (keygen.hip, key_format.hpp) and the host verifier (verify_host.hpp) all come here.  Vectors of points are the
// device's (gfft.cuh: k_decompress, k_compress, k_points_check).
// Host only, no HIP header: tests/native_host/g1_host_check.cpp drives it on the CPU under ASan + UBSan.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/dehalo.h"
#include "hostfield.hpp"

// the three SerdeFormats of params and keys on disk
inline bool serde_format_known(int format) { return format == DEHALO_SERDE_PROCESSED || format == DEHALO_SERDE_RAW_BYTES || format == DEHALO_SERDE_RAW_BYTES_UNCHECKED; }

// the status bits of a point codec, host and device alike (include/dehalo.h, dehalo_points_decompress_device / dehalo_points_check_device)
enum { POINT_NOT_BELOW_P = 1, POINT_NOT_ON_CURVE = 2, POINT_ZERO_X_SIGNED = 4 };
// the bits as the kind of failure; encodings: the compressed (Processed) form, else stored Montgomery words
inline const char* point_status_text(uint32_t status, bool encodings) {
    if (status & POINT_NOT_BELOW_P) return encodings ? "an x coordinate is not below the modulus" : "a coordinate's stored word is not below the modulus";
    if (status & POINT_ZERO_X_SIGNED) return "x = 0 with the sign bit set is not an encoding";
    if (status & POINT_NOT_ON_CURVE) return encodings ? "an x coordinate is not on the curve" : "a point is neither on the curve nor the identity";
    return "";
}

// y^2 = x^3 + b: 3 on BN254's G1, 5 on Pallas and Vesta
inline uint64_t curve_b_host(int curve) { return curve == DEHALO_CURVE_BN254_G1 ? 3 : 5; }

// an affine {x, y} whose eight words are zero: the identity, and what a decoder writes for a point it refuses
inline bool g1_affine_is_zero(const uint64_t xy[8]) { return (xy[0] | xy[1] | xy[2] | xy[3] | xy[4] | xy[5] | xy[6] | xy[7]) == 0; }

// GroupEncoding::from_bytes on the host, with the device codec's verdicts (dehalo_points_decompress_device): 0, or POINT_NOT_BELOW_P / POINT_NOT_ON_CURVE /
// POINT_ZERO_X_SIGNED; a refused point and the all-zero identity are written as (0, 0).  The one host decoder: the reading transcript, the host verifier and
// the verifying key's Processed commitments go through it.  (Upstream sends x = 0 with the sign bit set to the square root like every other x; b is no square
// on any of the three curves -- a group of prime order has no point of order 3 -- so that path refuses it too.)
inline uint32_t g1_decompress_host(const HostField* q, const Fe& b, const uint8_t in[32], uint64_t xy[8]) {
    memset(xy, 0, 64);
    Fe c;
    memcpy(c.v, in, 32);
    const unsigned sign = (unsigned)(c.v[3] >> 63);
    c.v[3] &= ~((uint64_t)1 << 63);
    if (HostField::geq(c.v, q->p)) return POINT_NOT_BELOW_P;
    if (c.is_zero()) return sign ? POINT_ZERO_X_SIGNED : 0;
    const Fe x = q->from_canonical(c);
    Fe y;
    if (!q->sqrt(q->add(q->mul(q->sqr(x), x), b), y)) return POINT_NOT_ON_CURVE;
    if ((unsigned)(q->to_canonical(y).v[0] & 1) != sign) y = q->neg(y);
    memcpy(xy, x.v, 32);
    memcpy(xy + 4, y.v, 32);
    return 0;
}

// GroupEncoding::to_bytes on the host, of affine {x, y} Montgomery: x little-endian canonical, bit 255 = y is odd, the identity (0, 0) all zero.  The one host
// encoder: a proof's points (dehalo_transcript::write_point) and ParamsIPA's file (dehalo_params_ipa_write).
inline void g1_compress_host(const HostField* fq, const uint64_t xy[8], uint8_t out[32]) {
    Fe x, y;
    memcpy(x.v, xy, 32);
    memcpy(y.v, xy + 4, 32);
    if (x.is_zero() && y.is_zero()) { memset(out, 0, 32); return; }
    uint8_t yb[32];
    fq->to_bytes(x, out);
    fq->to_bytes(y, yb);
    out[31] |= (uint8_t)((yb[0] & 1) << 7);
}

// ---- G1 on the host: y^2 = x^3 + b, Jacobian accumulator, affine addends ((0, 0) = the identity)
struct G1Host {
    const HostField* q;
    Fe b;
    struct Jac { Fe x, y, z; };
    G1Host(const HostField* fq, uint64_t curve_b) : q(fq), b(fq->from_u64(curve_b)) {}
    Jac identity() const { return Jac{q->one, q->one, Fe{}}; }
    Jac dbl(const Jac& P) const {
        if (P.z.is_zero() || P.y.is_zero()) return identity();
        const Fe A = q->sqr(P.x), B = q->sqr(P.y), C = q->sqr(B);
        Fe D = q->sub(q->sub(q->sqr(q->add(P.x, B)), A), C);
        D = q->add(D, D);
        const Fe E = q->add(q->add(A, A), A), F = q->sqr(E);
        Jac R;
        R.x = q->sub(F, q->add(D, D));
        Fe C8 = q->add(C, C);
        C8 = q->add(C8, C8);
        C8 = q->add(C8, C8);
        R.y = q->sub(q->mul(E, q->sub(D, R.x)), C8);
        R.z = q->mul(q->add(P.y, P.y), P.z);
        return R;
    }
    Jac add_affine(const Jac& P, const Fe& x2, const Fe& y2) const {
        if (x2.is_zero() && y2.is_zero()) return P;
        if (P.z.is_zero()) return Jac{x2, y2, q->one};
        const Fe zz = q->sqr(P.z), u2 = q->mul(x2, zz), s2 = q->mul(q->mul(y2, P.z), zz);
        if (u2 == P.x) return s2 == P.y ? dbl(P) : identity();
        const Fe h = q->sub(u2, P.x), hh = q->sqr(h), hhh = q->mul(h, hh), r = q->sub(s2, P.y), v = q->mul(P.x, hh);
        Jac R;
        R.x = q->sub(q->sub(q->sqr(r), hhh), q->add(v, v));
        R.y = q->sub(q->mul(r, q->sub(v, R.x)), q->mul(P.y, hhh));
        R.z = q->mul(P.z, h);
        return R;
    }
    void to_affine(const Jac& P, uint64_t xy[8]) const {
        memset(xy, 0, 64);
        if (P.z.is_zero()) return;
        const Fe zi = q->invert(P.z), zi2 = q->sqr(zi), x = q->mul(P.x, zi2), y = q->mul(P.y, q->mul(zi2, zi));
        memcpy(xy, x.v, 32);
        memcpy(xy + 4, y.v, 32);
    }
    // sum_i [s_i] P_i, s canonical integers: one accumulator, 256 doublings, one mixed addition per set bit (a verifier's sums have about 10^2 terms)
    void msm(const Fe* canonical_scalars, const uint64_t* xy, size_t len, uint64_t out_affine[8]) const {
        Jac acc = identity();
        for (int bit = 255; bit >= 0; bit--) {
            acc = dbl(acc);
            for (size_t i = 0; i < len; i++)
                if ((canonical_scalars[i].v[bit >> 6] >> (bit & 63)) & 1) {
                    Fe x, y;
                    memcpy(x.v, xy + 8 * i, 32);
                    memcpy(y.v, xy + 8 * i + 4, 32);
                    acc = add_affine(acc, x, y);
                }
        }
        to_affine(acc, out_affine);
    }
    bool on_curve(const Fe& x, const Fe& y) const { return q->sqr(y) == q->add(q->mul(q->sqr(x), x), b); }
    // stored Montgomery words {x, y}: 0, POINT_NOT_BELOW_P, or POINT_NOT_ON_CURVE -- that for (0, 0) too: who takes the identity asks g1_affine_is_zero
    uint32_t check_stored(const uint64_t xy[8]) const {
        Fe x, y;
        memcpy(x.v, xy, 32);
        memcpy(y.v, xy + 4, 32);
        if (HostField::geq(x.v, q->p) || HostField::geq(y.v, q->p)) return POINT_NOT_BELOW_P;
        return on_curve(x, y) ? 0 : POINT_NOT_ON_CURVE;
    }
    // GroupEncoding::from_bytes with the device codec's verdicts (dehalo_points_decompress_device): 0, or POINT_NOT_BELOW_P / POINT_NOT_ON_CURVE /
    // POINT_ZERO_X_SIGNED; a refused point and the all-zero identity are written as (0, 0)
    uint32_t decompress(const uint8_t in[32], uint64_t xy[8]) const { return g1_decompress_host(q, b, in, xy); }
};
