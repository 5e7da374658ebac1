// MSM kernels + driver, the IPA opening's kernels, the group FFT, the fixed-base tables and the segmented sums instantiated for CurveVesta (one translation unit per curve: parallel builds).
#include "msm.cuh"
#include "ipa.cuh"
#include "gfft.cuh"
#include "fixed_base.cuh"
#include "msm_segments.cuh"
const CurveOps& vesta_curve_ops() { static constexpr CurveOps ops = make_curve_ops<CurveVesta>(); return ops; }
const IpaOps& vesta_ipa_ops() { static constexpr IpaOps ops = make_ipa_ops<CurveVesta>(); return ops; }
const GfftOps& vesta_gfft_ops() { static constexpr GfftOps ops = make_gfft_ops<CurveVesta>(); return ops; }
const FixedBaseOps& vesta_fixed_base_ops() { static constexpr FixedBaseOps ops = make_fixed_base_ops<CurveVesta>(); return ops; }
int msm_segments_vesta(dehalo_ctx* ctx, const fe* d_scalars, const affine_t* d_points, const uint32_t* d_offsets, uint32_t segments, affine_t* d_out, hipStream_t s) {
    return msm_segments_t<CurveVesta>(ctx, d_scalars, d_points, d_offsets, segments, d_out, s);
}
