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

template <class CV>
constexpr IpaOps make_ipa_ops() {
    return {&ipa_collapse_t<CV>, &ipa_slots_t<CV>, &ipa_blind_t<CV>};
}
