// NTT / field-op / field-vector / quotient-numerator kernels + drivers instantiated for PastaFp.
#include "ntt.cuh"
#include "poly.cuh"
#include "evalh.cuh"
const FieldOps& pasta_fp_field_ops() { static constexpr FieldOps ops = make_field_ops<PastaFp>(); return ops; }
