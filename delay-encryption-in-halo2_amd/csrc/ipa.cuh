// ipa.cuh -- the device half of the IPA opening argument [UPSTREAM halo2_proofs/src/poly/ipa/commitment/prover.rs @ v2023_04_20:
// create_proof's round loop and parallel_generator_collapse].  Instantiated per Pasta curve in msm_pallas.hip / msm_vesta.hip.
//
// Generator collapse: G'[i] <- G'[i] + [u] G'[i + half] for i < half, one challenge u for the whole vector.  Over the k rounds of an opening
// that is n - 1 variable-base scalar multiplications, all by scalars the host knows, so the scalar is recoded ONCE on the host into its
// non-adjacent form (signed binary digits, no two adjacent non-zero: ~255 doublings and ~85 additions) and handed to the kernel as two bit
// masks.  Every lane of the grid walks the same digit sequence: the branches on the digits are uniform (scalar branches, no divergence).
//
// Four lanes (a DPP quad) share one point and split each group operation's products (x29_double_quad / x29_add_quad, ec29.cuh): the chain
// of ~340 dependent group operations is ~3x shorter, at four times the lanes.  The halves an opening meets are small (round 1 at k = 17 is
// 2^16 points: one wave per SIMD with one lane per point), so lanes are what is plentiful.  A one-lane-per-point variant (mixed XYZZ + affine
// additions) needs more than 128 VGPRs for the doubling, the addition and its exceptional path together and spilled at every register budget
// tried (128 VGPRs: 532 B of scratch per lane), so it is not kept.  The result leaves as the affine point (standard Montgomery, identity =
// (0, 0)) with one safegcd inversion (msm_emit): the form that the next round's MSM registration and the host's transcript read.  No scratch
// memory, no workspace.
#pragma once
#include "msm.cuh"

// the challenge's non-adjacent form: digit i is +1 when bit i of pos is set, -1 when bit i of neg is set; `top` = index of the highest
// non-zero digit (always +1), -1 for u = 0
struct IpaNaf {
    u32 pos[9], neg[9];
    int top;
};

template <class F>
FP_DEV aff29 ipa_load_affine(const affine_t* p, bool& is_id) {
    const affine_t a = aff_load(p);
    is_id = aff_is_identity(a);
    aff29 r;
    r.x = f29_canon<F>(f29_from_std<F>(a.x));
    r.y = f29_canon<F>(f29_from_std<F>(a.y));
    return r;
}

FP_DEV bool naf_bit(const u32* w, int i) { return (w[i >> 5] >> (i & 31)) & 1u; }

// four lanes (a DPP quad) per output point: the quad's lanes hold the same operands and split every group operation's products
template <class CV>
__global__ __launch_bounds__(256) void k_ipa_collapse(const affine_t* __restrict__ g, u32 half, IpaNaf naf, affine_t* out) {
    typedef f29_lat<typename f29_of<typename CV::Base>::type> F;   // short dependent chains at low occupancy: latency schedule
    const u32 i = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const u32 role = threadIdx.x & 3;
    const bool live = i < half;                // a quad is live or not as a whole (blockDim is a multiple of 4): the quad operations see four active lanes
    if (!live) return;
    bool q_id, p_id;
    const aff29 qa = ipa_load_affine<F>(&g[(u64)half + i], q_id);
    const aff29 pa = ipa_load_affine<F>(&g[i], p_id);
    const xyzz29 q = x29_from_affine<F>(qa, q_id);   // identity: literal zeros, which x29_add_quad / x29_double_quad pass through
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
    acc = x29_add_quad<F>(acc, x29_from_affine<F>(pa, p_id));
    if (role == 0) msm_emit<F>(acc, nullptr, &out[i]);
}

// host: the challenge (canonical, 4 x u64) -> its non-adjacent form
inline IpaNaf ipa_naf(const uint64_t canon[4]) {
    IpaNaf r;
    memset(&r, 0, sizeof(r));
    r.top = -1;
    // k as a 5-word little-endian integer (room for the carry of the recoding)
    uint64_t k[5] = {canon[0], canon[1], canon[2], canon[3], 0};
    auto is_zero = [&] { return !(k[0] | k[1] | k[2] | k[3] | k[4]); };
    auto shr1 = [&] { for (int j = 0; j < 5; j++) k[j] = (k[j] >> 1) | (j < 4 ? k[j + 1] << 63 : 0); };
    for (int i = 0; !is_zero(); i++) {
        if (k[0] & 1) {
            if ((k[0] & 3) == 1) {          // digit +1: k -= 1
                r.pos[i >> 5] |= 1u << (i & 31);
                k[0] &= ~(uint64_t)1;
            } else {                         // digit -1: k += 1
                r.neg[i >> 5] |= 1u << (i & 31);
                for (int j = 0; j < 5 && ++k[j] == 0; j++) {}
            }
            r.top = i;
        }
        shr1();
    }
    return r;
}

// out[i] = g[i] + [u] g[half + i], i < half (out may be g itself: element i reads only i and half + i and writes i)
template <class CV>
int ipa_collapse_t(dehalo_ctx* ctx, const affine_t* d_g, uint64_t half, const uint64_t u_canon[4], affine_t* d_out, hipStream_t s) {
    if (half == 0) return 0;
    const IpaNaf naf = ipa_naf(u_canon);
    const uint64_t threads = 4 * half;
    k_ipa_collapse<CV><<<(u32)((threads + 255) / 256), 256, 0, s>>>(d_g, (u32)half, naf, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// Blinded commitments: C_i <- C_i + [b_i] W for the m results of one batched MSM (ParamsIPA::commit / commit_lagrange = MSM + [blind] W, [UPSTREAM
// halo2_proofs/src/poly/ipa/commitment.rs]).  One shared base, a different scalar per point, both on the device: the scalars are a proof's blinds,
// drawn before the MSM was queued, so the launch follows the MSM on its stream and the points reach the host blinded -- no host wait in between.
// The points are read and written where the MSM leaves them (Jacobian {x, y, z}, standard Montgomery, 96 B; z = 0: the identity).  Four lanes per
// point as in the collapse; every quad walks all 255 bits of its own scalar (plain double-and-add: the scalars differ per quad, so the trip count is
// kept uniform across the wave and only the additions branch, quad-uniformly).  m is a few dozen at most: one workgroup is typical.  No scratch.
template <class CV>
__global__ __launch_bounds__(256) void k_ipa_blind(jacobian_t* pts, const fe* __restrict__ blinds, const affine_t* __restrict__ w, u32 m) {
    typedef f29_lat<typename f29_of<typename CV::Base>::type> F;
    typedef typename CV::Scalar FS;
    const u32 i = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const u32 role = threadIdx.x & 3;
    if (i >= m) return;                       // (a quad is live or not as a whole)
    const fe b = f_from_mont<FS>(f_load(&blinds[i]));      // canonical: bit j of the scalar is bit j & 31 of word j >> 5
    bool w_id;
    const aff29 wa = ipa_load_affine<F>(w, w_id);
    const xyzz29 wp = x29_from_affine<F>(wa, w_id);
    xyzz29 acc = x29_identity();
    for (int j = 254; j >= 0; j--) {
        acc = x29_double_quad<F>(acc);
        if ((b.v[j >> 5] >> (j & 31)) & 1u) acc = x29_add_quad<F>(acc, wp);
    }
    // the MSM's point: {X, Y, Z} with x = X / Z^2, y = Y / Z^3 -> XYZZ (X, Y, Z^2, Z^3)
    const fe z = f_load(&pts[i].z);
    xyzz29 c = x29_identity();
    if (!f_is_zero(z)) {
        const f29 z9 = f29_from_std<F>(z);
        c.x = f29_canon<F>(f29_from_std<F>(f_load(&pts[i].x)));
        c.y = f29_canon<F>(f29_from_std<F>(f_load(&pts[i].y)));
        c.zz = f29_sqr<F>(z9);
        c.zzz = f29_mul<F>(c.zz, z9);
    }
    acc = x29_add_quad<F>(acc, c);
    if (role == 0) msm_emit<F>(acc, &pts[i], nullptr);
}

template <class CV>
int ipa_blind_t(dehalo_ctx* ctx, jacobian_t* d_pts, const fe* d_blinds, const affine_t* d_w, uint64_t m, hipStream_t s) {
    if (m == 0) return 0;
    k_ipa_blind<CV><<<(u32)((4 * m + 255) / 256), 256, 0, s>>>(d_pts, d_blinds, d_w, (u32)m);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// The scalar slots of one round's batch-2 MSM over [G' | U | W] (dehalo_ipa_open): L's column gets z c_j p'_hi(x3) and l_rand, R's column
// z c_j x3^half p'_lo(x3) and r_rand.  evals = {p'_lo(x3), p'_hi(x3)}; coef = {z c_j, z c_j x3^half}; rands = {l_rand, r_rand}; all standard
// Montgomery.  One thread.
template <class CV>
__global__ void k_ipa_slots(const fe* __restrict__ evals, fe coef_l, fe coef_r, const fe* __restrict__ rands, fe* sl, fe* sr) {
    typedef typename CV::Scalar FS;
    if (threadIdx.x != 0) return;
    sl[0] = f_mul<FS>(coef_l, evals[1]);
    sl[1] = rands[0];
    sr[0] = f_mul<FS>(coef_r, evals[0]);
    sr[1] = rands[1];
}

template <class CV>
int ipa_slots_t(dehalo_ctx* ctx, const fe* d_evals, const uint64_t coef_l[4], const uint64_t coef_r[4], const fe* d_rands, fe* d_sl, fe* d_sr, hipStream_t s) {
    k_ipa_slots<CV><<<1, 64, 0, s>>>(d_evals, fe_from_u64(coef_l), fe_from_u64(coef_r), d_rands, d_sl, d_sr);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// The verifier's scalar vector over g [UPSTREAM halo2_proofs/src/poly/ipa/strategy.rs @ v2023_04_20: GuardIPA::compute_s, and the accumulation of the
// guards' s vectors under random weights]: for `count` proofs with round challenges u_{i, 0 .. k} and one scalar init_i each,
//     out[idx] = sum_i init_i prod_{j < k, bit j of idx set} u_{i, k - 1 - j},    idx < 2^k.
// With idx = hi 2^h + lo, h = ceil(k / 2), a term is  (init_i H_i[hi]) L_i[lo]:  k_ipa_s_tables writes, per proof, the 2^h low products and the 2^(k - h)
// high products (those carry init_i), every entry as the product over its own set bits (at most h multiplications an entry; the tables are
// count x (2^h + 2^(k - h)) entries, a 2^-(k / 2) fraction of the second pass), and k_ipa_s_sum spends ONE multiplication per proof and output: the
// high entry -- one address per wave once 2^h >= 64 -- times the low entry, read coalesced.  The high table is kept in the multiplier's internal form
// (x 2^261, canonical, packed), the low table in the standard form, so that their product is the standard form of the term as it stands (the trick of
// k_lincomb, poly.cuh); the sum is brought below 16 p every 8 terms and leaves canonical.  Field type and multiplier are poly.cuh's (f29 over the curve's
// scalar field, product scanning).  No LDS beyond the k converted challenges, no scratch memory.
#define IPA_S_THREADS 256
#define IPA_S_MAX_K 28
template <class CV>
__global__ __launch_bounds__(IPA_S_THREADS) void k_ipa_s_tables(const fe* __restrict__ challenges, const fe* __restrict__ inits, u32 k, u32 h, u32 blocks_per_proof, fe* lo_tab,
                                                                    fe* hi_tab) {
    typedef typename f29_of<typename CV::Scalar>::type F9;
    __shared__ f29 us[IPA_S_MAX_K];      // us[j] = the challenge bit j of an index selects: u_{i, k - 1 - j}
    const u32 proof = blockIdx.x / blocks_per_proof, t = threadIdx.x;
    if (t < k) us[t] = f29_from_std<F9>(f_load(&challenges[(u64)proof * k + (k - 1 - t)]));
    __syncthreads();
    const u32 n_lo = 1u << h, n_hi = 1u << (k - h);
    const u32 e = (blockIdx.x % blocks_per_proof) * IPA_S_THREADS + t;      // entry of [low table | high table]
    if (e >= n_lo + n_hi) return;
    const bool high = e >= n_lo;
    const u32 bits = high ? e - n_lo : e, first = high ? h : 0, nbits = high ? k - h : h;
    f29 acc = high ? f29_from_std<F9>(f_load(&inits[proof])) : f29_one<F9>();      // < 2p; every product below is < 4 p^2 / 2^261 + p < 2p
    for (u32 j = 0; j < nbits; j++)
        if ((bits >> j) & 1u) acc = f29_mul<F9>(acc, us[first + j]);
    if (high) f_store(&hi_tab[(u64)proof * n_hi + bits], f29_to_packed_canon<F9>(acc));
    else f_store(&lo_tab[(u64)proof * n_lo + bits], f29_to_std<F9>(acc));
}

template <class CV>
__global__ __launch_bounds__(IPA_S_THREADS) void k_ipa_s_sum(const fe* __restrict__ lo_tab, const fe* __restrict__ hi_tab, u32 count, u32 k, u32 h, fe* out) {
    typedef typename f29_of<typename CV::Scalar>::type F9;
    const u64 idx = (u64)blockIdx.x * IPA_S_THREADS + threadIdx.x;
    if (idx >= ((u64)1 << k)) return;
    const u32 n_lo = 1u << h, n_hi = 1u << (k - h);
    const fe* lo = lo_tab + (idx & (n_lo - 1));
    const fe* hi = hi_tab + (idx >> h);
    f29 acc = f29_zero();
    for (u32 i = 0; i < count; i++) {
        // (x 2^261, < p) (y 2^256, < p) / 2^261 + p: the term's standard form, < 1.04 p
        const f29 term = f29_mul<F9>(f29_unpack(f_load(&hi[(u64)i * n_hi])), f29_unpack(f_load(&lo[(u64)i * n_lo])));
        acc = f29_norm(f29_add(acc, term));
        if ((i & 7u) == 7u) acc = f29_canon<F9>(acc);      // < p + 8 x 1.04 p < 16 p
    }
    f_store(&out[idx], f29_pack(f29_canon<F9>(acc)));
}

// d_tables: ipa_s_table_elems(k, count) elements of workspace (internal.hpp): [every proof's low table | every proof's high table]
inline uint32_t ipa_s_split(uint32_t k) { return (k + 1) / 2; }
template <class CV>
int ipa_s_t(dehalo_ctx* ctx, const fe* d_challenges, const fe* d_inits, uint32_t count, uint32_t k, fe* d_tables, fe* d_out, hipStream_t s) {
    const uint32_t h = ipa_s_split(k);
    const size_t n_lo = (size_t)1 << h, n_hi = (size_t)1 << (k - h);
    fe* lo_tab = d_tables;
    fe* hi_tab = d_tables + count * n_lo;
    const u32 blocks_per_proof = (u32)((n_lo + n_hi + IPA_S_THREADS - 1) / IPA_S_THREADS);      // <= 128; count < 2^24 (the caller's check)
    k_ipa_s_tables<CV><<<blocks_per_proof * count, IPA_S_THREADS, 0, s>>>(d_challenges, d_inits, k, h, blocks_per_proof, lo_tab, hi_tab);
    HIP_TRY(ctx, hipGetLastError());
    k_ipa_s_sum<CV><<<(u32)((((size_t)1 << k) + IPA_S_THREADS - 1) / IPA_S_THREADS), IPA_S_THREADS, 0, s>>>(lo_tab, hi_tab, count, k, h, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

template <class CV>
constexpr IpaOps make_ipa_ops() {
    return {&ipa_collapse_t<CV>, &ipa_slots_t<CV>, &ipa_blind_t<CV>, &ipa_s_t<CV>};
}
