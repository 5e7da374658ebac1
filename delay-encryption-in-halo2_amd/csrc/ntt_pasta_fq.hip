// NTT / field-op / field-vector / quotient-numerator kernels + drivers instantiated for PastaFq.
#include "ntt.cuh"
#include "poly.cuh"
#include "evalh.cuh"
const FieldOps& pasta_fq_field_ops() { static constexpr FieldOps ops = make_field_ops<PastaFq>(); return ops; }
