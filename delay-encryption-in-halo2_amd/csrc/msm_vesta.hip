// MSM kernels + driver and the IPA opening's kernels instantiated for CurveVesta (one translation unit per curve: parallel builds).
#include "msm.cuh"
#include "ipa.cuh"
const CurveOps& vesta_curve_ops() { static constexpr CurveOps ops = make_curve_ops<CurveVesta>(); return ops; }
const IpaOps& vesta_ipa_ops() { static constexpr IpaOps ops = make_ipa_ops<CurveVesta>(); return ops; }
