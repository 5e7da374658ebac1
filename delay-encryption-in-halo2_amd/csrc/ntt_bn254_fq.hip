// NTT / field-op / field-vector / quotient-numerator kernels + drivers instantiated for Bn254Fq.
#include "ntt.cuh"
#include "poly.cuh"
#include "evalh.cuh"
const FieldOps& bn254_fq_field_ops() { static constexpr FieldOps ops = make_field_ops<Bn254Fq>(); return ops; }
