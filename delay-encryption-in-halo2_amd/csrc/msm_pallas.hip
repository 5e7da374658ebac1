// MSM kernels + driver instantiated for CurvePallas (one translation unit per curve: parallel builds).
#include "msm.cuh"
const CurveOps& pallas_curve_ops() { static constexpr CurveOps ops = make_curve_ops<CurvePallas>(); return ops; }
