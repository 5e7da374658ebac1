// NTT / field-op / field-vector / quotient-numerator kernels + drivers instantiated for Bn254Fr.
#include "ntt.cuh"
#include "poly.cuh"
#include "evalh.cuh"
const FieldOps& bn254_fr_field_ops() { static constexpr FieldOps ops = make_field_ops<Bn254Fr>(); return ops; }
