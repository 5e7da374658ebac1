// pairing.cuh -- many independent BN254 pairing checks against FIXED G2 points in ONE launch (dehalo_pairing_checks*, include/dehalo.h):
//     gt[c] = (prod_j miller(P[c][j], Q_j)) ^ ((q^12 - 1) / r),    status[c] = (gt[c] == 1),    c < checks, j < pairs.
// What it is for: dehalo_verify_proofs_each in device mode -- every live proof's (L_i, -R_i) against the verifier's (s_g2, g2), each proof its own check, so
// that the cost no longer depends on how many proofs are invalid and no search over subsets is needed.
//
// What is left for the device.  All the Miller loop does on the twist depends on Q alone: the host walks it once (PairingHost::line_table, pairing_host.hpp)
// and keeps, per step, lam and mu = lam xt - yt.  A check is then arithmetic in Fq12 on the check's own P: per step the line  yp - lam xp w + mu w^3,  one
// squaring of f per tangent step shared by all pairs, and the host's final exponentiation: f^(q^6 - 1), ^(q^2 + 1), then the exact hard exponent
// (q^4 - q^2 + 1) / r by square-and-multiply.  No G2 arithmetic, no inversion in the loop, no branch on a coordinate's value.
//
// Shape: one wave per check, PAIRING_WAVES waves a block, nothing shared between the waves of a block (no __syncthreads: a wave whose check is off the curve
// or past `checks` leaves alone).  Fq12 is taken as Fq2[w] / (w^6 - xi), xi = 9 + i: six Fq2 coefficients c_0 .. c_5 of w^0 .. w^5 (the tower's a.a, b.a, a.b,
// b.b, a.c, b.c).  A value lives in the wave's LDS as 12 x 9 limbs (fp29.cuh's internal form, limbs normalized, every coefficient below 2 q).  One product:
//   phase A  lane 6 i + j < 36 multiplies a_i b_j in Fq2 -- two f29_mul2, (ar br + ai (-bi)) and (ar bi + ai br), one reduction each -- into the wave's 36 slots;
//   phase B  lane 2 k + part < 12 sums its coefficient's slots: c_k = sum_{i + j = k} + xi sum_{i + j = k + 6}, xi (x + y i) = (9 x - y) + (9 y + x) i, limb
//            sums in 32 bits, the combination through one signed 64-bit carry chain with 8 q added (the value stays positive and below 70 q < 2^260), and
//            one multiplication by 2^261 mod q brings it back below 2 q.
// Squarings, sparse lines and dense products all take this one routine: the lanes of a wave run side by side, so fewer Fq2 products would not be fewer steps.
// LDS operations of one wave complete in order; __builtin_amdgcn_wave_barrier() keeps the compiler from moving them across the phases (as in msm_bred.cuh).
//
// The one inversion of the final exponentiation needs no Fq6 code: with N = f conj(f) in Fq6 and s the q^2-power Frobenius (which fixes Fq2 and is a
// coefficient-wise multiplication), N' = s(N) s^2(N) and M = N N' is N's norm, in Fq2; f^-1 = conj(f) N' M^-1, and M^-1 = conj(M) / (a^2 + b^2) is lane 0's, with
// f29_inv_safegcd.  The values are the host's bit for bit: both compute exact field elements, and gt is stored canonical.
//
// Bounds.  Wave c reads g1[c * pairs .. (c + 1) * pairs), the tables' pairs x 102 steps, the 12 + 4 constants, and writes status[c] and gt[12 c .. 12 c + 12):
// nothing outside [0, checks).  No workspace, no scratch memory.
#pragma once
#include "fp29.cuh"

#define PAIRING_WAVES 4      // checks a block holds
#define PAIRING_BLOCK (64 * PAIRING_WAVES)
#define PAIRING_STEPS 102    // PairingHost::LINE_STEPS
#define PAIRING_MAX_PAIRS 8  // DEHALO_PAIRING_MAX_PAIRS

typedef Bn254Fq29 PF;

struct p12 { u32 c[12][9]; };      // c[2 k] + c[2 k + 1] i: the coefficient of w^k
struct pairing_wave {
    p12 f, t0, t1, t2, t3;
    u32 prod[36][2][9];            // phase A's a_i b_j
    u32 xy[PAIRING_MAX_PAIRS][2][9];      // the check's P_j, internal form
};

FP_DEV f29 p_get(const u32* p) {
    f29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = p[i];
    return r;
}
FP_DEV void p_put(u32* p, const f29& a) {
#pragma unroll
    for (int i = 0; i < 9; i++) p[i] = a.v[i];
}
FP_DEV void p_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// -a of a normalized a < 3 q: normalized, < 4 q
FP_DEV f29 p_neg(const f29& a) { return f29_norm(f29_sub(f29_zero(), a, PF::KM)); }
// (ar + ai i)(br + bi i), operands normalized and below 2 q: both parts < (4 + 8) q^2 / 2^261 + q < 1.1 q
FP_DEV void p_mul2(const f29& ar, const f29& ai, const f29& br, const f29& bi, f29& re, f29& im) {
    const f29 nbi = p_neg(bi);
    re = f29_mul2<PF>(ar, br, ai, nbi);
    im = f29_mul2<PF>(ar, bi, ai, br);
}

// dst = a b; dst may be a or b
FP_DEV void p12_mul(pairing_wave* w, p12* dst, const p12* a, const p12* b, u32 lane) {
    if (lane < 36) {
        const u32 i = lane / 6, j = lane - 6 * i;
        f29 re, im;
        p_mul2(p_get(a->c[2 * i]), p_get(a->c[2 * i + 1]), p_get(b->c[2 * j]), p_get(b->c[2 * j + 1]), re, im);
        p_put(w->prod[lane][0], re);
        p_put(w->prod[lane][1], im);
    }
    p_sync();
    if (lane < 12) {
        const u32 k = lane >> 1, part = lane & 1;
        u32 lo[9], hs[9], ho[9];
#pragma unroll
        for (int l = 0; l < 9; l++) lo[l] = hs[l] = ho[l] = 0;
        for (u32 i = 0; i < 6; i++) {
            const u32 j = k - i, j2 = k + 6 - i;      // (j wraps above 5 when i > k)
            if (j < 6) {
                const u32* s = w->prod[6 * i + j][part];
#pragma unroll
                for (int l = 0; l < 9; l++) lo[l] += s[l];
            }
            if (j2 < 6) {
                const u32* s = w->prod[6 * i + j2][part];
                const u32* o = w->prod[6 * i + j2][part ^ 1];
#pragma unroll
                for (int l = 0; l < 9; l++) { hs[l] += s[l]; ho[l] += o[l]; }
            }
        }
        // lo + 9 hs -+ ho + 8 q: at most 6 + 45 + 5 + 8 values of 1.1 q, at least 8 q - 5.5 q
        f29 r;
        int64_t c = 0;
#pragma unroll
        for (int l = 0; l < 9; l++) {
            const int64_t o = (int64_t)ho[l];
            const int64_t t = (int64_t)lo[l] + 9 * (int64_t)hs[l] + (part ? o : -o) + (int64_t)PF::P8[l] + c;
            if (l < 8) { r.v[l] = (u32)t & F29_MASK; c = t >> F29_BITS; }
            else r.v[l] = (u32)t;
        }
        p_put(dst->c[lane], f29_mul<PF>(r, f29_one<PF>()));      // < 70 q q / 2^261 + q < 1.6 q
    }
    p_sync();
}

// dst = src^(q^2): coefficient k times g[k] = conj(frob[k]) frob[k] (Fq2 as a | b, standard Montgomery words); dst may be src
FP_DEV void p12_frob2(p12* dst, const p12* src, const fe* g, u32 lane) {
    f29 re = f29_zero(), im = f29_zero();
    if (lane < 6) p_mul2(p_get(src->c[2 * lane]), p_get(src->c[2 * lane + 1]), f29_from_std<PF>(f_load(&g[2 * lane])), f29_from_std<PF>(f_load(&g[2 * lane + 1])), re, im);
    p_sync();
    if (lane < 6) {
        p_put(dst->c[2 * lane], re);
        p_put(dst->c[2 * lane + 1], im);
    }
    p_sync();
}
// dst = conj(src), the q^6-power Frobenius: the odd powers of w change sign; dst may be src
FP_DEV void p12_conj(p12* dst, const p12* src, u32 lane) {
    if (lane < 12) {
        f29 v = p_get(src->c[lane]);
        if (lane & 2) v = f29_mul<PF>(p_neg(v), f29_one<PF>());      // back below 2 q
        p_put(dst->c[lane], v);
    }
    p_sync();
}
FP_DEV void p12_one(p12* dst, u32 lane) {
    if (lane < 12) p_put(dst->c[lane], lane == 0 ? f29_one<PF>() : f29_zero());
    p_sync();
}

// lines:  pairs x 102 x {lam.a, lam.b, mu.a, mu.b}        one_mask: bit j = Q_j is the identity
// consts: 12 words of g (p12_frob2), then the hard exponent as 32 u32, hard_bits long        loop: the low 64 bits of 6x + 2 (bit 64 is T = Q)
__global__ __launch_bounds__(PAIRING_BLOCK) void k_pairing_checks(const fe* __restrict__ lines, u32 pairs, u32 one_mask, const fe* __restrict__ consts, u32 hard_bits,
                                                                  u64 loop, const fe* __restrict__ g1, u32 checks, uint8_t* status, fe* gt) {
    __shared__ pairing_wave sh[PAIRING_WAVES];
    const u32 lane = threadIdx.x & 63;
    const u32 check = blockIdx.x * PAIRING_WAVES + (threadIdx.x >> 6);
    if (check >= checks) return;      // (the whole wave)
    pairing_wave* w = &sh[threadIdx.x >> 6];

    // ---- the check's points: lane j < pairs loads P_j, tests the curve equation and leaves the internal form in LDS
    bool inf = false, off = false;
    if (lane < pairs) {
        const fe* p = g1 + 2 * ((size_t)check * pairs + lane);
        const fe xw = f_load(p), yw = f_load(p + 1);
        u32 any = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) any |= xw.v[i] | yw.v[i];
        inf = any == 0;
        const f29 x = f29_from_std<PF>(xw), y = f29_from_std<PF>(yw);      // a word not below q stands for its residue
        const f29 one = f29_one<PF>();
        const f29 rhs = f29_norm(f29_add(f29_add(f29_mul<PF>(f29_sqr<PF>(x), x), one), f29_add(one, one)));      // x^3 + 3 < 4.1 q
        off = !inf && !f29_is_zero_slow<PF>(f29_sub(f29_sqr<PF>(y), rhs, PF::KA));
        p_put(w->xy[lane][0], x);
        p_put(w->xy[lane][1], y);
    }
    const u64 off_mask = __ballot(off), inf_mask = __ballot(inf);
    if (off_mask) {
        if (lane == 0) status[check] = 2;      // DEHALO_PAIRING_OFF_CURVE
        if (gt && lane < 12) {
            fe z;
#pragma unroll
            for (int i = 0; i < 8; i++) z.v[i] = 0;
            f_store(&gt[12 * (size_t)check + lane], z);
        }
        return;
    }
    const u32 live = ~(u32)inf_mask & ~one_mask & ((1u << pairs) - 1u);
    p12_one(&w->f, lane);

    // ---- the Miller loop, in the order the tables were made: for i = 63 .. 0 the tangent (after f <- f^2), the addition where bit i of 6x + 2 is set; then pi(Q), -pi^2(Q)
    int bit = 63;
    bool addition = false;
    for (u32 s = 0; s < PAIRING_STEPS; s++) {
        const bool tangent = s < PAIRING_STEPS - 2 && !addition;
        if (tangent && live) p12_mul(w, &w->f, &w->f, &w->f, lane);
        for (u32 j = 0; j < pairs; j++) {
            if (!((live >> j) & 1u)) continue;
            // yp - lam xp w + mu w^3
            if (lane < 12) {
                const fe* ln = lines + 4 * ((size_t)j * PAIRING_STEPS + s);
                f29 v = f29_zero();
                if (lane == 0) v = p_get(w->xy[j][1]);
                else if (lane == 2 || lane == 3) v = f29_mul<PF>(p_neg(f29_from_std<PF>(f_load(&ln[lane & 1]))), p_get(w->xy[j][0]));
                else if (lane == 6 || lane == 7) v = f29_from_std<PF>(f_load(&ln[2 + (lane & 1)]));
                p_put(w->t0.c[lane], v);
            }
            p_sync();
            p12_mul(w, &w->f, &w->f, &w->t0, lane);
        }
        if (s < PAIRING_STEPS - 2) {
            if (tangent) addition = (loop >> bit) & 1;
            else addition = false;
            if (!addition) bit--;
        }
    }

    // ---- f^(q^6 - 1) = conj(f)^2 / (f conj(f))
    p12_conj(&w->t0, &w->f, lane);
    p12_mul(w, &w->t1, &w->f, &w->t0, lane);            // N, in Fq6
    p12_frob2(&w->t2, &w->t1, consts, lane);
    p12_frob2(&w->t3, &w->t2, consts, lane);
    p12_mul(w, &w->t2, &w->t2, &w->t3, lane);           // N' = s(N) s^2(N)
    p12_mul(w, &w->t1, &w->t1, &w->t2, lane);           // M = N N', in Fq2
    {
        f29 re = f29_zero(), im = f29_zero();
        if (lane == 0) {
            const f29 a = p_get(w->t1.c[0]), b = p_get(w->t1.c[1]);
            const f29 n = f29_inv_safegcd<PF>(f29_mul2<PF>(a, a, b, b));
            re = f29_mul<PF>(a, n);
            im = f29_mul<PF>(p_neg(b), n);
        }
        p_sync();
        if (lane == 0) {
            p_put(w->t1.c[0], re);
            p_put(w->t1.c[1], im);
        } else if (lane < 11) p_put(w->t1.c[lane + 1], f29_zero());
        p_sync();
    }
    p12_mul(w, &w->t2, &w->t2, &w->t1, lane);           // 1 / N
    p12_mul(w, &w->t3, &w->t0, &w->t0, lane);
    p12_mul(w, &w->f, &w->t3, &w->t2, lane);
    // ---- ^(q^2 + 1)
    p12_frob2(&w->t0, &w->f, consts, lane);
    p12_mul(w, &w->f, &w->t0, &w->f, lane);
    // ---- ^((q^4 - q^2 + 1) / r), from the exponent's top bit
    const u32* hard = reinterpret_cast<const u32*>(consts + 12);
    if (lane < 12) p_put(w->t1.c[lane], p_get(w->f.c[lane]));
    p_sync();
    for (int b = (int)hard_bits - 2; b >= 0; b--) {
        p12_mul(w, &w->t1, &w->t1, &w->t1, lane);
        if ((hard[b >> 5] >> (b & 31)) & 1u) p12_mul(w, &w->t1, &w->t1, &w->f, lane);
    }

    // ---- canonical words out, and the comparison with 1
    bool differs = false;
    if (lane < 12) {
        const fe v = f29_to_std<PF>(p_get(w->t1.c[lane]));
        const fe one = f29_to_std<PF>(f29_one<PF>());
        u32 d = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) d |= v.v[i] ^ (lane == 0 ? one.v[i] : 0u);
        differs = d != 0;
        if (gt) f_store(&gt[12 * (size_t)check + lane], v);
    }
    const u64 diff_mask = __ballot(differs);
    if (lane == 0) status[check] = diff_mask ? 0 : 1;      // DEHALO_PAIRING_NOT_ONE, _ONE
}
