// MSM kernels + driver instantiated for CurveBn254 (one translation unit per curve: parallel builds); ParamsKZG::setup's kernels (BN254 is the pairing curve); the group FFT; the fixed-base tables; the segmented sums.
#include "msm.cuh"
#include "setup.cuh"
#include "gfft.cuh"
#include "fixed_base.cuh"
#include "msm_segments.cuh"
const CurveOps& bn254_curve_ops() { static constexpr CurveOps ops = make_curve_ops<CurveBn254>(); return ops; }
int kzg_setup_bn254(dehalo_ctx* ctx, uint32_t k, const uint64_t s[4], const uint64_t omega[4], const uint64_t cfac[4], affine_t* d_g, affine_t* d_gl, hipStream_t st) {
    return kzg_setup_t<CurveBn254>(ctx, k, s, omega, cfac, d_g, d_gl, st);
}
const GfftOps& bn254_gfft_ops() { static constexpr GfftOps ops = make_gfft_ops<CurveBn254>(); return ops; }
const FixedBaseOps& bn254_fixed_base_ops() { static constexpr FixedBaseOps ops = make_fixed_base_ops<CurveBn254>(); return ops; }
int msm_segments_bn254(dehalo_ctx* ctx, const fe* d_scalars, const affine_t* d_points, const uint32_t* d_offsets, uint32_t segments, affine_t* d_out, hipStream_t s) {
    return msm_segments_t<CurveBn254>(ctx, d_scalars, d_points, d_offsets, segments, d_out, s);
}
