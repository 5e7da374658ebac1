// MSM kernels + driver and the IPA opening's kernels instantiated for CurvePallas (one translation unit per curve: parallel builds).
#include "msm.cuh"
#include "ipa.cuh"
const CurveOps& pallas_curve_ops() { static constexpr CurveOps ops = make_curve_ops<CurvePallas>(); return ops; }
const IpaOps& pallas_ipa_ops() { static constexpr IpaOps ops = make_ipa_ops<CurvePallas>(); return ops; }
