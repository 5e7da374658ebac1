// MSM kernels + driver, the IPA opening's kernels, the group FFT and the fixed-base tables instantiated for CurveVesta (one translation unit per curve: parallel builds).
#include "msm.cuh"
#include "ipa.cuh"
#include "gfft.cuh"
#include "fixed_base.cuh"
const CurveOps& vesta_curve_ops() { static constexpr CurveOps ops = make_curve_ops<CurveVesta>(); return ops; }
const IpaOps& vesta_ipa_ops() { static constexpr IpaOps ops = make_ipa_ops<CurveVesta>(); return ops; }
const GfftOps& vesta_gfft_ops() { static constexpr GfftOps ops = make_gfft_ops<CurveVesta>(); return ops; }
const FixedBaseOps& vesta_fixed_base_ops() { static constexpr FixedBaseOps ops = make_fixed_base_ops<CurveVesta>(); return ops; }
