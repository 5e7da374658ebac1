// MSM kernels + driver instantiated for CurveVesta (one translation unit per curve: parallel builds).
#include "msm.cuh"
const CurveOps& vesta_curve_ops() { static constexpr CurveOps ops = make_curve_ops<CurveVesta>(); return ops; }
