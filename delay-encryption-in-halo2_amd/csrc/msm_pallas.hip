// MSM kernels + driver, the IPA opening's kernels, the group FFT and the fixed-base tables instantiated for CurvePallas (one translation unit per curve: parallel builds).
#include "msm.cuh"
#include "ipa.cuh"
#include "gfft.cuh"
#include "fixed_base.cuh"
const CurveOps& pallas_curve_ops() { static constexpr CurveOps ops = make_curve_ops<CurvePallas>(); return ops; }
const IpaOps& pallas_ipa_ops() { static constexpr IpaOps ops = make_ipa_ops<CurvePallas>(); return ops; }
const GfftOps& pallas_gfft_ops() { static constexpr GfftOps ops = make_gfft_ops<CurvePallas>(); return ops; }
const FixedBaseOps& pallas_fixed_base_ops() { static constexpr FixedBaseOps ops = make_fixed_base_ops<CurvePallas>(); return ops; }
