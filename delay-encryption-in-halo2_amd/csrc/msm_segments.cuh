// msm_segments.cuh -- many short independent sums in ONE launch (dehalo_msm_segments*, include/dehalo.h):
//     out[s] = sum over offsets[s] <= i < offsets[s + 1] of [scalars[i]] points[i],    s < segments.
// Instantiated per curve in msm_bn254.hip / msm_pallas.hip / msm_vesta.hip.
//
// What it is for: the per-proof sums of dehalo_verify_proofs_each -- 10^2 terms a segment, 10^2 segments a call.  The Pippenger path (msm.cuh) is planned for
// 2^17 and more points, and on 10^2 terms its sort, accumulation, reduction and final launches are launch latency; one such call per segment would be 10^2 of them.
//
// Shape: one workgroup per segment, one DPP quad per term.  A quad walks the 255 bits of its term's scalar by double-and-add (x29_double_quad / x29_add_quad,
// ec29.cuh: the four lanes split each group operation's products), as k_ipa_blind (ipa.cuh) does; the block's 128 quads stride over the segment's terms, so a
// segment of up to 128 terms is one walk deep.  The scalars differ per quad: every quad runs the same 255 steps (a doubling of the identity returns at once)
// and only the additions branch, quad-uniformly.  The quads' sums fold inside a wave through register shuffles (x29_group_reduce_quad, four levels), the eight
// waves' sums through LDS and three more levels in wave 0, and lane 0 writes the affine point with one safegcd inversion (msm_emit).
//
// Group law.  The points are a caller's -- a proof's, so an adversary's: nothing may be assumed about them beyond "on the curve or (0, 0)".  x29_add_quad takes
// every exceptional case (an identity operand, equal operands, opposite operands) to x29_add, which decides them exactly, so a segment that lists one point
// several times, under equal scalars or opposite ones, sums to what the group law says.  A zero scalar leaves its quad's product the identity (literal zeros,
// which the additions pass through); a (0, 0) point likewise.  A scalar is any 256-bit word and stands for its residue: f_from_mont leaves the canonical
// integer whatever multiple of r the word carried.
//
// Bounds.  The kernel reads offsets[blockIdx.x] and [blockIdx.x + 1], and scalars / points at indices inside [offsets[s], offsets[s + 1]) only; the entry
// points (capi.hip) have checked on the host that the offsets do not decrease before the launch, so a block's loop runs over its own segment or not at all.
// No workspace, no scratch memory; 8 x 144 B of LDS.
#pragma once
#include "ipa.cuh"

#define MSEG_BLOCK 512      // 128 quads: eight waves, two a SIMD

template <class CV>
__global__ __launch_bounds__(MSEG_BLOCK) void k_msm_segments(const fe* __restrict__ scalars, const affine_t* __restrict__ points, const u32* __restrict__ offsets,
                                                             affine_t* out) {
    typedef f29_lat<typename f29_of<typename CV::Base>::type> F;      // dependent chains at low occupancy: latency schedule
    typedef typename CV::Scalar FS;
    __shared__ xyzz29_rec sh[MSEG_BLOCK / 64];
    const u32 seg = blockIdx.x;
    const u32 lo = offsets[seg], hi = offsets[seg + 1];
    const u32 quad = threadIdx.x >> 2;
    xyzz29 sum = x29_identity();
    for (u64 i = (u64)lo + quad; i < hi; i += MSEG_BLOCK / 4) {      // (a quad is in the loop or out of it as a whole)
        bool p_id;
        const aff29 pa = ipa_load_affine<F>(&points[i], p_id);
        if (p_id) continue;      // [s] O = O.  (Known to be no identity, p's ZZ and ZZZ are the constant one and hold no registers)
        const xyzz29 p = x29_from_affine<F>(pa, false);
        const fe b = f_from_mont<FS>(f_load(&scalars[i]));      // canonical: bit j of the scalar is bit j & 31 of word j >> 5
        xyzz29 acc = x29_identity();
        for (int w = 7; w >= 0; w--) {
            u32 word = 0;      // (a select chain: a register array indexed by the loop would live in scratch)
#pragma unroll
            for (int j = 0; j < 8; j++) word = w == j ? b.v[j] : word;
            for (int bit = 31; bit >= 0; bit--) {
                acc = x29_double_quad<F>(acc);
                if ((word >> bit) & 1u) acc = x29_add_quad<F>(acc, p);
            }
        }
        sum = x29_add_quad<F>(sum, acc);
    }
    // every lane of the block is here: the wave's 16 quads fold into its quad 0, the eight waves' sums into wave 0's
    sum = x29_group_reduce_quad<F, 64>(sum);
    if ((threadIdx.x & 63) == 0) x29_store(&sh[threadIdx.x >> 6], sum);
    __syncthreads();
    if (threadIdx.x >= 64) return;
    sum = quad < MSEG_BLOCK / 64 ? x29_load(&sh[quad]) : x29_identity();
    sum = x29_group_reduce_quad<F, 32>(sum);
    if (threadIdx.x == 0) msm_emit<F>(sum, nullptr, &out[seg]);
}

// d_offsets: segments + 1 words that do not decrease (the caller has checked); segments >= 1
template <class CV>
int msm_segments_t(dehalo_ctx* ctx, const fe* d_scalars, const affine_t* d_points, const u32* d_offsets, uint32_t segments, affine_t* d_out, hipStream_t s) {
    k_msm_segments<CV><<<segments, MSEG_BLOCK, 0, s>>>(d_scalars, d_points, d_offsets, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
