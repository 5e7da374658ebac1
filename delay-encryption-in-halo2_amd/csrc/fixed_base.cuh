// fixed_base.cuh -- fixed-base scalar multiplication over a resident window table of ANY point P (dehalo_fixed_base_*, include/dehalo.h): [s_i] P for
// many scalars and C_i + [b_i] P for the results of a batched MSM (ParamsIPA's [blind] W).  Instantiated per curve in msm_bn254.hip / msm_pallas.hip /
// msm_vesta.hip.
//
// The table is the one ParamsKZG::setup builds for the generator (k_fb_table, setup.cuh): T[w][d] = [d 2^(8 w)] P, 32 byte-windows x 256 entries, affine, in
// the kernels' packed internal form, d = 0 and every entry of an identity base all zero -- 512 KB, L2-resident.  A canonical scalar s < r is then the sum
// of at most 32 table entries and no doubling is left.
//
// Counts are a few dozen (the commitments of one proof phase), so lanes are plentiful and the dependent chain is the whole cost: ONE WAVE per scalar.  Quad
// q of the wave (16 DPP quads) loads the two entries of byte-windows 2 q and 2 q + 1 and adds them, the 16 partial sums fold in four levels
// (x29_group_reduce_quad) and, for the blinding form, quad 0 adds the MSM's point last: 6 dependent group additions, each quad-cooperative (4 multiplication
// rounds, ec29.cuh), against the 255 doublings and ~127 additions k_ipa_blind walks per point.
//
// Group-law cases: for s < r on a prime-order curve the partial sums of distinct windows are never equal or opposite, so inside the table part only "an
// operand is the identity" occurs (digit 0, identity base: literal zeros, which x29_add_quad passes through).  The final + C meets all three exceptional cases
// (C the identity, C = [b] P, C = -[b] P); x29_add_quad resolves them through x29_add.  No scratch memory, no workspace.
#pragma once
#include "ipa.cuh"

#define FBT_WINDOWS 32
#define FBT_ENTRIES (FBT_WINDOWS * 256)
#define FBT_BLOCK 256      // four waves = four scalars per block

// ---- table build (one-time per point): a doubling pass, then a fill pass ----
// pows[w] = [2^(8 w)] P, affine, standard Montgomery ((0, 0) for an identity base); thread w walks its own 8 w doublings
template <class CV>
__global__ __launch_bounds__(64) void k_fbt_pows(const affine_t* __restrict__ base, affine_t* pows) {
    typedef f29_lat<typename f29_of<typename CV::Base>::type> F;
    const u32 w = threadIdx.x;
    if (w >= FBT_WINDOWS) return;
    bool p_id;
    const aff29 pa = ipa_load_affine<F>(base, p_id);
    xyzz29 q = x29_from_affine<F>(pa, p_id);
    for (u32 i = 0; i < 8 * w; i++) q = x29_double<F>(q);
    msm_emit<F>(q, nullptr, &pows[w]);
}

// T[w][d] = [d] pows[w] by double-and-add from d's top bit (d < 256 < r: no exceptional case), one inversion per entry
template <class CV>
__global__ __launch_bounds__(64) void k_fbt_fill(const affine_t* __restrict__ pows, affine_t* table) {
    typedef f29_lat<typename f29_of<typename CV::Base>::type> F;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= FBT_ENTRIES) return;
    const u32 w = t >> 8, d = t & 255;
    affine_t o;
    o.x = f_zero(); o.y = f_zero();
    bool q_id;
    const aff29 q = ipa_load_affine<F>(&pows[w], q_id);
    if (d && !q_id) {
        xyzz29 acc = x29_from_affine<F>(q, false);
        for (int bit = 30 - __clz(d); bit >= 0; bit--) {
            acc = x29_double<F>(acc);
            if ((d >> bit) & 1) acc = x29_add_mixed<F>(acc, q);
        }
        const f29 ti = f29_inv_safegcd<F>(f29_mul<F>(acc.zz, acc.zzz));
        o.x = f29_to_packed_canon<F>(f29_mul<F>(acc.x, f29_mul<F>(ti, acc.zzz)));
        o.y = f29_to_packed_canon<F>(f29_mul<F>(acc.y, f29_mul<F>(ti, acc.zz)));
    }
    aff_store(&table[t], o);
}

// ---- [s] P: one wave per scalar; quad 0 of the wave returns with the sum (replicated over its four lanes), the other quads with partial sums ----
template <class F, class FS>
FP_DEV xyzz29 fbt_wave_mul(const affine_t* __restrict__ table, const fe* __restrict__ scalar) {
    const u32 quad = (threadIdx.x & 63) >> 2;
    const fe s = f_from_mont<FS>(f_load(scalar));      // canonical: byte-window w is byte w & 3 of word w >> 2
    u32 word = 0;                                      // (a select chain: a register array indexed by the lane would live in scratch)
#pragma unroll
    for (u32 j = 0; j < 8; j++) word = (quad >> 1) == j ? s.v[j] : word;
    const u32 d0 = (word >> (16 * (quad & 1))) & 255u, d1 = (word >> (16 * (quad & 1) + 8)) & 255u;
    // both loads are issued before either is used; digit 0 reads the all-zero entry of its window
    const affine_t e0 = aff_load(&table[(2 * quad) * 256 + d0]);
    const affine_t e1 = aff_load(&table[(2 * quad + 1) * 256 + d1]);
    const xyzz29 p0 = x29_from_affine<F>(a29_from_packed(e0), aff_is_identity(e0));
    const xyzz29 p1 = x29_from_affine<F>(a29_from_packed(e1), aff_is_identity(e1));
    return x29_group_reduce_quad<F, 64>(x29_add_quad<F>(p0, p1));
}

// out[i] = [scalars[i]] P, affine, standard Montgomery, (0, 0) for the identity
template <class CV>
__global__ __launch_bounds__(FBT_BLOCK) void k_fbt_mul(const affine_t* __restrict__ table, const fe* __restrict__ scalars, affine_t* out, u32 m) {
    typedef f29_lat<typename f29_of<typename CV::Base>::type> F;
    const u32 i = blockIdx.x * (FBT_BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= m) return;                       // (a wave is live or not as a whole)
    const xyzz29 acc = fbt_wave_mul<F, typename CV::Scalar>(table, &scalars[i]);
    if ((threadIdx.x & 63) == 0) msm_emit<F>(acc, nullptr, &out[i]);
}

// pts[i] <- pts[i] + [blinds[i]] P, in place: the contract of k_ipa_blind (ipa.cuh), Jacobian {x, y, z} as the MSM leaves it, z = 0 the identity
template <class CV>
__global__ __launch_bounds__(FBT_BLOCK) void k_fbt_blind(const affine_t* __restrict__ table, jacobian_t* pts, const fe* __restrict__ blinds, u32 m) {
    typedef f29_lat<typename f29_of<typename CV::Base>::type> F;
    const u32 i = blockIdx.x * (FBT_BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= m) return;
    xyzz29 acc = fbt_wave_mul<F, typename CV::Scalar>(table, &blinds[i]);
    if ((threadIdx.x & 63) >= 4) return;      // quad 0 (whole) adds the MSM's point: {X, Y, Z} with x = X / Z^2, y = Y / Z^3 -> XYZZ (X, Y, Z^2, Z^3)
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
    if ((threadIdx.x & 3) == 0) msm_emit<F>(acc, &pts[i], nullptr);
}

// d_base: one affine point (standard Montgomery, device); d_pows: FBT_WINDOWS points of scratch; d_table: FBT_ENTRIES entries
template <class CV>
int fbt_build_t(dehalo_ctx* ctx, const affine_t* d_base, affine_t* d_pows, affine_t* d_table, hipStream_t s) {
    k_fbt_pows<CV><<<1, 64, 0, s>>>(d_base, d_pows);
    k_fbt_fill<CV><<<FBT_ENTRIES / 64, 64, 0, s>>>(d_pows, d_table);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

template <class CV>
int fbt_mul_t(dehalo_ctx* ctx, const affine_t* d_table, const fe* d_scalars, affine_t* d_out, uint64_t m, hipStream_t s) {
    if (m == 0) return 0;
    k_fbt_mul<CV><<<(u32)((m + FBT_BLOCK / 64 - 1) / (FBT_BLOCK / 64)), FBT_BLOCK, 0, s>>>(d_table, d_scalars, d_out, (u32)m);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

template <class CV>
int fbt_blind_t(dehalo_ctx* ctx, const affine_t* d_table, jacobian_t* d_pts, const fe* d_blinds, uint64_t m, hipStream_t s) {
    if (m == 0) return 0;
    k_fbt_blind<CV><<<(u32)((m + FBT_BLOCK / 64 - 1) / (FBT_BLOCK / 64)), FBT_BLOCK, 0, s>>>(d_table, d_pts, d_blinds, (u32)m);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

template <class CV>
constexpr FixedBaseOps make_fixed_base_ops() {
    return {&fbt_build_t<CV>, &fbt_mul_t<CV>, &fbt_blind_t<CV>};
}
