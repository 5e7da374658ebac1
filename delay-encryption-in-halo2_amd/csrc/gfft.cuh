// gfft.cuh -- g_to_lagrange on the device: the group FFT that takes a commitment key g to its Lagrange basis [UPSTREAM halo2_proofs/src/poly/commitment.rs,
// poly/ipa/commitment.rs @ v2023_04_20: best_fft(&mut g, omega_inv, k); g[i] *= n_inv; batch_normalize]:
//     g_lagrange[i] = [n^-1] sum_j [omega^(-i j)] g[j],      omega the 2^k-th root of unity of the curve's scalar field.
// The output is canonical affine points, so the evaluation order is free.  Instantiated per curve in msm_*.hip (all three: the code is curve-generic).
//
// Shape: radix-2 decimation in time over 64-byte affine points (standard Montgomery, identity = (0, 0)), every stage one plain launch that reads and
// writes affine points in place -- no XYZZ workspace; the normalisation per point is one safegcd inversion against a ~340-operation scalar
// multiplication.
//   1. k_gfft_permute: out[i] = [n^-1] g[bitrev(i)].  The transform is linear, so the scaling is applied to the input, where it rides on the
//      permutation launch; n^-1 is one scalar for the whole vector, recoded once on the host (IpaNaf, ipa.cuh): wave-uniform digit branches.  A quad
//      owns the pair (i, bitrev(i)), i <= bitrev(i), so the same kernel is correct in place and out of place.
//   2. k_gfft_stage, s = 1 .. k: (a, b) -> (a + [t] b, a - [t] b) over blocks of 2^s points, t = omega^(-j 2^(k - s)) for position j in the block.
// Four lanes (a DPP quad) share one butterfly (x29_double_quad / x29_add_quad), as in the generator collapse.  The twiddle differs per butterfly:
// quads are numbered TWIDDLE-MAJOR (quad q -> j = q >> (k - s), block = q & (2^(k - s) - 1)), so while a stage has at least 16 blocks the 16 quads of
// a wave share j and walk one digit sequence -- the digit branches are uniform in fact.  The last four stages (fewer than 16 blocks) mix twiddles in
// a wave: the doublings still run in lock-step (one trip count for the wave) and only the additions branch per quad, with ONE addition site for
// both signs of the digit so that a wave never pays two.  Twiddles come from a table of omega^(-j), j < n / 2 (k_gfft_twiddles: 32 B x n / 2 of
// workspace); each quad takes its canonical bits with f_from_mont and recodes them into the non-adjacent form itself (3x against x, a few dozen
// word operations).  j = 0 (all of stage 1, half of stage 2) has t = 1: no scalar multiplication.
// Exceptional group-law cases (identity inputs, a = +-[t] b: a constant g collapses to one non-zero output) pass through the quad operations'
// own exceptional paths.  No scratch memory.
#pragma once
#include "hostrng.hpp"      // chacha_indexed_block: the block function k_points_generate shares with k_chacha_scalars (params.hip)
#include "ipa.cuh"

// tw[j] = base^j (standard Montgomery), j < count
template <class FS>
__global__ __launch_bounds__(256) void k_gfft_twiddles(fe* tw, fe base, u32 count) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    fe acc = f_one<FS>(), b = base;
    for (u32 e = j; e; e >>= 1) {
        if (e & 1) acc = f_mul<FS>(acc, b);
        b = f_sqr<FS>(b);
    }
    f_store(&tw[j], acc);
}

// p as an affine point in standard form; negate: -p
template <class CV, class F>
FP_DEV void gfft_emit(const xyzz29& p, bool negate, affine_t* out) {
    affine_t a;
    if (f29_is_zero_slow<F>(p.zz)) { a.x = f_zero(); a.y = f_zero(); }
    else {
        f29 ti = f29_inv_safegcd<F>(f29_mul<F>(p.zz, p.zzz));
        a.x = f29_to_std<F>(f29_mul<F>(p.x, f29_mul<F>(ti, p.zzz)));
        a.y = f29_to_std<F>(f29_mul<F>(p.y, f29_mul<F>(ti, p.zz)));
        if (negate) a.y = f_neg<typename CV::Base>(a.y);
    }
    aff_store(out, a);
}

// [naf] q, quad-cooperative; the digit sequence is the launch's (uniform)
template <class F>
FP_DEV xyzz29 gfft_mul_uniform(const aff29& qa, bool q_id, const IpaNaf& naf) {
    const xyzz29 q = x29_from_affine<F>(qa, q_id);
    xyzz29 qn = q;
    if (!q_id) qn.y = f29_norm(f29_sub(f29_zero(), q.y, F::KN));
    xyzz29 acc = x29_identity();
    if (naf.top >= 0) {
        acc = q;
        for (int b = naf.top - 1; b >= 0; b--) {
            acc = x29_double_quad<F>(acc);
            if (naf_bit(naf.pos, b)) acc = x29_add_quad<F>(acc, q);
            else if (naf_bit(naf.neg, b)) acc = x29_add_quad<F>(acc, qn);
        }
    }
    return acc;
}

FP_DEV u32 gfft_bitrev(u32 i, u32 k) { return k ? __brev(i) >> (32 - k) : 0; }

// out[i] = [n^-1] g[bitrev(i)]: quad i handles i and r = bitrev(i) when i <= r (out may be g itself: the pair is read before either is written)
template <class CV>
__global__ __launch_bounds__(256) void k_gfft_permute(const affine_t* g, u32 k, IpaNaf naf, affine_t* out) {
    typedef f29_lat<typename f29_of<typename CV::Base>::type> F;
    const u32 i = (u32)(((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 2);
    const u32 role = threadIdx.x & 3;
    if (i >= (1u << k)) return;               // (a quad is live or not as a whole)
    const u32 r = gfft_bitrev(i, k);
    if (i > r) return;
    bool a_id, b_id;
    const aff29 a = ipa_load_affine<F>(&g[i], a_id);
    const aff29 b = ipa_load_affine<F>(&g[r], b_id);
    const xyzz29 sb = gfft_mul_uniform<F>(b, b_id, naf);
    if (role == 0) gfft_emit<CV, F>(sb, false, &out[i]);
    if (i != r) {
        const xyzz29 sa = gfft_mul_uniform<F>(a, a_id, naf);
        if (role == 0) gfft_emit<CV, F>(sa, false, &out[r]);
    }
}

FP_DEV f29 f29_pick(const f29& a, const f29& b, bool take_b) {
    f29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = take_b ? b.v[i] : a.v[i];
    return r;
}

// stage s of k, in place: quad q -> position j = q >> (k - s) of block q & (2^(k - s) - 1); (a, b) = (p[i0], p[i0 + 2^(s-1)]) -> (a + [t] b, a - [t] b),
// t = tw[j << (k - s)]
template <class CV>
__global__ __launch_bounds__(256) void k_gfft_stage(affine_t* p, const fe* __restrict__ tw, u32 k, u32 s) {
    typedef f29_lat<typename f29_of<typename CV::Base>::type> F;
    typedef typename CV::Scalar FS;
    const u32 q = (u32)(((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 2);
    const u32 role = threadIdx.x & 3;
    if (q >= (1u << (k - 1))) return;         // (a quad is live or not as a whole)
    const u32 ls = k - s, half = 1u << (s - 1);
    const u32 j = q >> ls, blk = q & ((1u << ls) - 1);
    const u32 i0 = (blk << s) + j, i1 = i0 + half;
    bool b_id;
    const aff29 ba = ipa_load_affine<F>(&p[i1], b_id);
    xyzz29 t = x29_from_affine<F>(ba, b_id);  // identity: literal zeros, which the quad operations pass through
    if (j != 0) {
        // the twiddle's non-adjacent form: digit i = bit i + 1 of 3x minus bit i + 1 of x; nz = the non-zero digits, ng = the negative ones
        const fe x = f_from_mont<FS>(f_load(&tw[(u64)j << ls]));
        u32 nz[8], ng[8];
        {
            u32 x3[9];
            u64 c = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                c += (u64)x.v[i] + (((u64)x.v[i] << 1) & 0xffffffffu) + (i ? x.v[i - 1] >> 31 : 0);
                x3[i] = (u32)c;
                c >>= 32;
            }
            x3[8] = (u32)c + (x.v[7] >> 31);
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const u32 d = x3[i] ^ x.v[i], dn = x3[i + 1] ^ (i < 7 ? x.v[i + 1] : 0);
                const u32 m = x.v[i] & ~x3[i], mn = (i < 7 ? x.v[i + 1] : 0) & ~x3[i + 1];
                nz[i] = (d >> 1) | (dn << 31);
                ng[i] = (m >> 1) | (mn << 31);
            }
        }
        const xyzz29 b = t;
        const f29 by_neg = b_id ? b.y : f29_norm(f29_sub(f29_zero(), b.y, F::KN));
        xyzz29 acc = x29_identity();          // doubling the identity returns at once: the digits above a twiddle's top cost a branch each
        for (int w = 7; w >= 0; w--) {        // (the word index is uniform: the digit words are selected, never indexed per lane)
            u32 wz = 0, wn = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                wz = w == i ? nz[i] : wz;
                wn = w == i ? ng[i] : wn;
            }
            for (int bit = 31; bit >= 0; bit--) {
                acc = x29_double_quad<F>(acc);
                if ((wz >> bit) & 1u) {       // one addition site for both signs: a wave of mixed twiddles pays one addition per digit position
                    xyzz29 o = b;
                    o.y = f29_pick(b.y, by_neg, (wn >> bit) & 1u);
                    acc = x29_add_quad<F>(acc, o);
                }
            }
        }
        t = acc;
    }
    bool a_id;
    const aff29 aa = ipa_load_affine<F>(&p[i0], a_id);
    xyzz29 a = x29_from_affine<F>(aa, a_id);
    const xyzz29 sum = x29_add_quad<F>(a, t);                         // a + T
    if (!a_id) a.y = f29_norm(f29_sub(f29_zero(), a.y, F::KN));
    const xyzz29 dif = x29_add_quad<F>(a, t);                         // -a + T = -(a - T): negated on the way out
    // lane 0 normalises the sum, lane 1 the difference: one pass through the inversion for both
    xyzz29 mine;
    mine.x = f29_pick(sum.x, dif.x, role == 1);
    mine.y = f29_pick(sum.y, dif.y, role == 1);
    mine.zz = f29_pick(sum.zz, dif.zz, role == 1);
    mine.zzz = f29_pick(sum.zzz, dif.zzz, role == 1);
    if (role < 2) gfft_emit<CV, F>(mine, role == 1, &p[role == 1 ? i1 : i0]);
}

// d_out = g_to_lagrange(d_g), 2^k points, 1 <= k <= 28 (d_out == d_g or disjoint).  omega_inv, n_inv: standard Montgomery (omega_inv), canonical (n_inv).
template <class CV>
int gfft_t(dehalo_ctx* ctx, const affine_t* d_g, uint32_t k, const uint64_t omega_inv[4], const uint64_t n_inv_canon[4], affine_t* d_out, hipStream_t s) {
    typedef typename CV::Scalar FS;
    const uint64_t n = 1ull << k;
    const uint32_t ntw = k >= 2 ? (uint32_t)(n / 2) : 1;
    TRY(dh_ensure(ctx, ctx->ws_gfft, (size_t)ntw * sizeof(fe)));
    fe* tw = (fe*)ctx->ws_gfft.p;
    k_gfft_twiddles<FS><<<(ntw + 255) / 256, 256, 0, s>>>(tw, fe_from_u64(omega_inv), ntw);
    k_gfft_permute<CV><<<(u32)((4 * n + 255) / 256), 256, 0, s>>>(d_g, k, ipa_naf(n_inv_canon), d_out);
    for (uint32_t st = 1; st <= k; st++) k_gfft_stage<CV><<<(u32)((2 * n + 255) / 256), 256, 0, s>>>(d_out, tw, k, st);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// r = a square root of a (standard Montgomery, below p), false when a is a non-residue (r is then meaningless); a = 0 gives r = 0.  Which of the two roots
// is the caller's to choose.  t_exp = (p - 1) / 2^S, canonical (sqrt_t_exp below).  Shared by k_decompress and k_points_generate.
template <class F>
FP_DEV bool f_sqrt_ts(const fe& a, const fe& t_exp, fe& r) {
    // Tonelli-Shanks: p - 1 = t 2^S.  w = a^((t - 1) / 2); r = a w (a^((t + 1) / 2)); tt = r w (a^t); c = ROOT_OF_UNITY (a generator of the 2^S-th roots)
    fe e = t_exp;                                                                     // (t - 1) / 2: t is odd
#pragma unroll
    for (int j = 0; j < 8; j++) e.v[j] = (e.v[j] >> 1) | (j < 7 ? e.v[j + 1] << 31 : 0);
    fe w = f_one<F>();
    for (int bit = 0; bit < 256; bit++) {                                             // (the exponent is shifted through its top bit: no indexed register)
        w = f_sqr<F>(w);
        if (e.v[7] >> 31) w = f_mul<F>(w, a);
#pragma unroll
        for (int j = 7; j >= 0; j--) e.v[j] = (e.v[j] << 1) | (j ? e.v[j - 1] >> 31 : 0);
    }
    r = f_mul<F>(a, w);
    fe tt = f_mul<F>(r, w), c = f_const<F>(F::ROOT_OF_UNITY_M);
    const fe one = f_one<F>();
    if (f_is_zero(a)) { r = f_zero(); tt = one; }
    u32 m = F::TWO_ADICITY;
    while (!f_eq(tt, one)) {
        u32 l = 0;
        fe t2 = tt;
        while (!f_eq(t2, one) && l < m) { t2 = f_sqr<F>(t2); l++; }
        if (l >= m) return false;                                                     // the order of a^t is 2^S: a is a non-residue
        fe bb = c;
        for (u32 z = 0; z + l + 1 < m; z++) bb = f_sqr<F>(bb);
        m = l;
        c = f_sqr<F>(bb);
        tt = f_mul<F>(tt, c);
        r = f_mul<F>(r, bb);
    }
    return true;
}

// ---- GroupEncoding::from_bytes for a vector of points (ParamsIPA::read): in = 32 B per point (x little-endian, bit 255 = y is odd, all zero = the
// identity), out = affine standard Montgomery.  One lane per point, plain fp.cuh arithmetic: y = sqrt(x^3 + b) by Tonelli-Shanks with the field's
// 2-adicity S (read from the field's constants); not throughput-critical.  status[0] |= 1: an x not below p; 2: not on the curve; 4: x = 0 with the
// sign bit set.
template <class CV>
__global__ __launch_bounds__(128) void k_decompress(const u32* __restrict__ in, affine_t* out, u32 count, fe t_exp /* (p - 1) / 2^S, canonical */, u32* status) {
    typedef typename CV::Base F;
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    fe x;
#pragma unroll
    for (int j = 0; j < 8; j++) x.v[j] = in[(u64)i * 8 + j];
    const u32 sign = x.v[7] >> 31;
    x.v[7] &= 0x7fffffffu;
    affine_t o;
    o.x = f_zero(); o.y = f_zero();
    bool below = false, decided = false;
#pragma unroll
    for (int j = 7; j >= 0; j--)
        if (!decided && x.v[j] != F::P[j]) { below = x.v[j] < F::P[j]; decided = true; }
    if (!below) { atomicOr(status, 1u); aff_store(&out[i], o); return; }
    if (f_is_zero(x)) {
        if (sign) atomicOr(status, 4u);
        aff_store(&out[i], o);
        return;
    }
    const fe xm = f_to_mont<F>(x);
    const fe a = f_add<F>(f_mul<F>(f_sqr<F>(xm), xm), f_const<F>(CV::B_M));        // x^3 + b
    fe r;
    const bool ok = f_sqrt_ts<F>(a, t_exp, r);
    if (!ok) { atomicOr(status, 2u); aff_store(&out[i], o); return; }
    if ((f_from_mont<F>(r).v[0] & 1u) != sign) r = f_neg<F>(r);
    o.x = xm; o.y = r;
    aff_store(&out[i], o);
}

// f_sqrt_ts's exponent, on the host: (p - 1) >> S
template <class F>
fe sqrt_t_exp() {
    fe t;
    for (int i = 0; i < 8; i++) t.v[i] = F::P[i];
    t.v[0] -= 1;                                                                      // p is odd
    for (int sh = 0; sh < F::TWO_ADICITY; sh++)
        for (int i = 0; i < 8; i++) t.v[i] = (t.v[i] >> 1) | (i < 7 ? t.v[i + 1] << 31 : 0);
    return t;
}

template <class CV>
int decompress_t(dehalo_ctx* ctx, const uint8_t* d_in, affine_t* d_out, uint64_t count, uint32_t* d_status, hipStream_t s) {
    typedef typename CV::Base F;
    if (count == 0) return 0;
    k_decompress<CV><<<(u32)((count + 127) / 128), 128, 0, s>>>((const u32*)d_in, d_out, (u32)count, sqrt_t_exp<F>(), d_status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ---- GroupEncoding::to_bytes for a vector of points, the inverse of k_decompress: in = affine standard Montgomery, out = 32 B per point (x little-endian
// canonical, bit 255 = y is odd, (0, 0) -> all zero).  One lane per point: two f_from_mont (reduction rows only, no multiplication), no scratch.
template <class CV>
__global__ __launch_bounds__(128) void k_compress(const affine_t* __restrict__ in, u32* __restrict__ out, u32 count) {
    typedef typename CV::Base F;
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const affine_t a = aff_load(&in[i]);
    fe x = f_zero();
    if (!aff_is_identity(a)) {
        x = f_from_mont<F>(a.x);
        x.v[7] |= (f_from_mont<F>(a.y).v[0] & 1u) << 31;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) out[(u64)i * 8 + j] = x.v[j];
}

template <class CV>
int compress_t(dehalo_ctx* ctx, const affine_t* d_in, uint8_t* d_out, uint64_t count, hipStream_t s) {
    if (count == 0) return 0;
    k_compress<CV><<<(u32)((count + 127) / 128), 128, 0, s>>>(d_in, (u32*)d_out, (u32)count);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ---- what a checked from_raw_bytes does per point [UPSTREAM halo2curves SerdeObject::from_raw_bytes: each coordinate's stored word below the modulus,
// then is_on_curve, which the identity passes]: in = affine standard Montgomery as it arrived, read only.  status[0] |= 1: a coordinate's stored word is
// not below p; 2: neither on y^2 = x^3 + b nor (0, 0).  One lane per point, three multiplications (a lane with status 1 makes none: f_mul wants operands
// below p), no scratch.
template <class F>
FP_DEV bool f_below_p(const fe& a) {
    bool below = false, decided = false;
#pragma unroll
    for (int j = 7; j >= 0; j--)
        if (!decided && a.v[j] != F::P[j]) { below = a.v[j] < F::P[j]; decided = true; }
    return below;
}

template <class CV>
__global__ __launch_bounds__(128) void k_points_check(const affine_t* __restrict__ in, u32 count, u32* status) {
    typedef typename CV::Base F;
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const affine_t a = aff_load(&in[i]);
    if (!f_below_p<F>(a.x) || !f_below_p<F>(a.y)) { atomicOr(status, 1u); return; }
    if (aff_is_identity(a)) return;
    const fe rhs = f_add<F>(f_mul<F>(f_sqr<F>(a.x), a.x), f_const<F>(CV::B_M));
    if (!f_eq(f_sqr<F>(a.y), rhs)) atomicOr(status, 2u);
}

template <class CV>
int points_check_t(dehalo_ctx* ctx, const affine_t* d_in, uint64_t count, uint32_t* d_status, hipStream_t s) {
    if (count == 0) return 0;
    k_points_check<CV><<<(u32)((count + 127) / 128), 128, 0, s>>>(d_in, (u32)count, d_status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ---- points by a public rule (include/dehalo.h, "Generated points"): out[i] = the point named (curve, key, stream, first + i) -- the first ChaCha20 block
// (indexed schedule, attempt = 0, 1, ...) whose first 32 bytes k_decompress's rules decode to a point other than the identity.  One lane per index, plain
// fp.cuh arithmetic, no scratch.  Two loops, so that a wave pays a square root only for candidates that can be a point: the inner one draws blocks until
// 0 < x < p (word compares, no field arithmetic: half of all Pasta candidates end here) and the lanes of a wave meet again in front of f_sqrt_ts, which then
// runs once per outer trip for every lane still searching.  A wave makes as many trips as its slowest lane (about 7 where a lane needs 2 on Pasta:
// DESIGN.md section 4 for what that costs and why it was left).  Both loops are bounded by DEHALO_GENERATORS_MAX_ATTEMPTS blocks per index; an index that
// uses them up is written as (0, 0) and raises status[0] |= 1.  That path cannot be reached with a real key ((3/4)^256) and is not tested.
template <class CV>
__global__ __launch_bounds__(128) void k_points_generate(ChaKey key, u64 stream, u64 first, affine_t* out, u32 count, fe t_exp, u32* status) {
    typedef typename CV::Base F;
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u64 index = first + i;
    affine_t o;
    o.x = f_zero(); o.y = f_zero();
    bool found = false;
    u32 attempt = 0;
    while (attempt < DEHALO_GENERATORS_MAX_ATTEMPTS) {
        fe x;
        u32 sign = 0;
        bool in_range = false;
        while (attempt < DEHALO_GENERATORS_MAX_ATTEMPTS && !in_range) {
            chacha_indexed_block(key.k, stream, index, attempt, x.v);
            attempt++;
            sign = x.v[7] >> 31;
            x.v[7] &= 0x7fffffffu;
            in_range = f_below_p<F>(x) && !f_is_zero(x);
        }
        if (!in_range) break;
        const fe xm = f_to_mont<F>(x);
        const fe a = f_add<F>(f_mul<F>(f_sqr<F>(xm), xm), f_const<F>(CV::B_M));    // x^3 + b
        fe r;
        if (f_sqrt_ts<F>(a, t_exp, r) && !f_is_zero(a)) {
            if ((f_from_mont<F>(r).v[0] & 1u) != sign) r = f_neg<F>(r);
            o.x = xm; o.y = r;
            found = true;
            break;
        }
    }
    if (!found) atomicOr(status, 1u);
    aff_store(&out[i], o);
}

template <class CV>
int points_generate_t(dehalo_ctx* ctx, const uint32_t key[8], uint64_t cha_stream, uint64_t first, affine_t* d_out, uint64_t count, uint32_t* d_status, hipStream_t s) {
    typedef typename CV::Base F;
    if (count == 0) return 0;
    ChaKey ck;
    memcpy(ck.k, key, 32);
    k_points_generate<CV><<<(u32)((count + 127) / 128), 128, 0, s>>>(ck, cha_stream, first, d_out, (u32)count, sqrt_t_exp<F>(), d_status);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

template <class CV>
constexpr GfftOps make_gfft_ops() {
    return {&gfft_t<CV>, &decompress_t<CV>, &compress_t<CV>, &points_check_t<CV>, &points_generate_t<CV>};
}
