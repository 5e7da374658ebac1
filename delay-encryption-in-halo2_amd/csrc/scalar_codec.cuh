// scalar_codec.cuh -- the scalar twin of the point codec (gfft.cuh): vectors of field elements between their in-memory form (4 x u64 Montgomery limbs) and
// the two forms they take in a key on disk [UPSTREAM halo2curves 0.3.x PrimeField::from_repr, SerdeObject::from_raw_bytes; restated from memory].
//   k_scalars_from_repr  32-byte little-endian canonical integers -> Montgomery words; an integer not below p is written as 0 and reported
//   k_scalars_check      what a checked from_raw_bytes does per element: the stored Montgomery word must be below p; reads only
// Streaming maps, one lane per element.  A wave reports through its lowest offending lane alone (lane order is index order, so that lane holds the wave's
// minimum): one atomicOr on the status word and one atomicMin on the index per wave that saw a bad element, none otherwise.
// The other direction, to_repr, is k_field_op's op 5 (ntt.cuh).
#pragma once
#include "fp.cuh"
#include "internal.hpp"

// a >= p, both as 256-bit integers
template <class F>
FP_DEV bool f_word_geq_p(const fe& a) {
    u64 br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        u64 x = (u64)a.v[i] - F::P[i] - br;
        br = (x >> 32) & 1;
    }
    return br == 0;
}

// status |= 1 and first_bad = min(first_bad, i) for every lane with `bad` set, one pair of atomics per wave
FP_DEV void scalar_codec_report(bool bad, u64 i, u32* status, unsigned long long* first_bad) {
    const unsigned long long m = __ballot(bad);
    if (m && (u32)__lane_id() == (u32)(__ffsll((long long)m) - 1)) {
        atomicOr(status, 1u);
        atomicMin(first_bad, (unsigned long long)i);
    }
}

// in: 8 x u32 per element, 4-byte aligned (16-byte aligned input takes the two-vector load); out may be `in` itself: a lane reads its own 32 bytes in full
// before it writes them
template <class F>
__global__ void k_scalars_from_repr(const u32* in, fe* out, u64 n, bool aligned16, u32* status, unsigned long long* first_bad) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) {
        fe x;
        if (aligned16) x = f_load(reinterpret_cast<const fe*>(in) + i);
        else {
#pragma unroll
            for (int j = 0; j < 8; j++) x.v[j] = in[8 * i + j];
        }
        bad = f_word_geq_p<F>(x);
        f_store(&out[i], bad ? f_zero() : f_to_mont<F>(x));
    }
    scalar_codec_report(bad, i, status, first_bad);
}

template <class F>
__global__ void k_scalars_check(const fe* in, u64 n, u32* status, unsigned long long* first_bad) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool bad = i < n && f_word_geq_p<F>(f_load(&in[i]));
    scalar_codec_report(bad, i, status, first_bad);
}

template <class F>
int scalars_from_repr_t(dehalo_ctx* ctx, const uint8_t* in, fe* out, uint64_t n, uint32_t* d_status, uint64_t* d_first_bad, hipStream_t s) {
    if (n) k_scalars_from_repr<F><<<(u32)((n + 255) / 256), 256, 0, s>>>((const u32*)in, out, n, ((uintptr_t)in & 15) == 0, d_status, (unsigned long long*)d_first_bad);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

template <class F>
int scalars_check_t(dehalo_ctx* ctx, const fe* in, uint64_t n, uint32_t* d_status, uint64_t* d_first_bad, hipStream_t s) {
    if (n) k_scalars_check<F><<<(u32)((n + 255) / 256), 256, 0, s>>>(in, n, d_status, (unsigned long long*)d_first_bad);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
