// check.cuh -- the per-field kernels of dehalo_check_witness (check.hip): MockProver::verify's row loops [UPSTREAM halo2_proofs/src/dev.rs] on the device.
//
//   k_graph_check    every gate polynomial on every row of the ORIGINAL domain.  A sibling of graph_eval_body (evalh.cuh) over the same DevCalc programs: the
//                    key's checking program has one ROOT per gate polynomial (plonk_host.hpp gate_check_graph; subexpressions shared between gates, no y).
//                    At a root the lane reduces the value fully, decides "zero or not", the wave ballots and one lane stores the 64-bit word:
//                    one bit per (polynomial, row) where k_graph_eval writes 32 bytes per row.
//   k_check_member   one lane per row: is the lookup's compressed input a key of its sorted table (binary search, full 256-bit compare)?
//   k_check_shuffle  one lane per row: does the shuffle's compressed input occur as often among the sorted inputs as among the sorted shuffle side (two binary
//                    searches in each)?  Both lists hold the same number of values, so no row fails exactly when the two multisets are equal.
//
// Both write whole bitmap words with ordinary stores, every word of their region exactly once: no atomics, nothing depends on the order of the launches' waves.
// Included by evalh.cuh (instantiated per field in ntt_*.hip through FieldOps).
#pragma once

struct ChkArgs {
    EvhArgs e;
    const u32* root_of;           // per calculation: the root it computes, or 0xffffffff
    u64* bitmap;                  // [root][words]
    u64 words, usable;
};

template <class F>
__global__ __launch_bounds__(EVH_THREADS) void k_graph_check(ChkArgs C) {
    typedef typename f29_of<F>::type F9;
    extern __shared__ u32 evh_lds[];
    const EvhArgs& A = C.e;
    EvhLds L{evh_lds};
    const u64 row = (u64)blockIdx.x * EVH_THREADS + threadIdx.x;
    if (row >= A.rows) return;                  // (2^k rows: a wave is inside the domain or outside it, except below 64 rows, where lane 0 is inside)
    for (u32 ci = 0; ci < A.num_calcs; ci++) {
        const DevCalc c = A.calcs[ci];
        f29 a = evh_fetch<F9>(A, L, c.a, row);
        f29 r;
        switch (c.op) {
            case DEHALO_CALC_ADD: r = evh_add<F9>(a, evh_fetch<F9>(A, L, c.b, row)); break;
            case DEHALO_CALC_SUB: r = evh_sub<F9>(a, evh_fetch<F9>(A, L, c.b, row)); break;
            case DEHALO_CALC_MUL: r = f29_mul<F9>(a, evh_fetch<F9>(A, L, c.b, row)); break;
            case DEHALO_CALC_SQUARE: r = f29_sqr<F9>(a); break;
            case DEHALO_CALC_DOUBLE: r = evh_add<F9>(a, a); break;
            case DEHALO_CALC_NEGATE: r = evh_neg<F9>(a); break;
            case DEHALO_CALC_HORNER: {
                const f29 factor = evh_fetch<F9>(A, L, c.b, row);
                r = a;
                for (u32 k = 0; k < c.parts_len; k++)
                    r = evh_add<F9>(f29_mul<F9>(r, factor), evh_fetch<F9>(A, L, A.parts[c.parts_begin + k], row));
            } break;
            default: r = a; break;              // STORE
        }
        const u32 root = C.root_of[ci];         // uniform: the program is
        if (root != 0xffffffffu) {
            // a slot value is < 2p: 0 and p both stand for zero.  The canonical form (< p) is zero exactly when the value is.
            const fe canon = f29_to_packed_canon<F9>(r);
            u32 any = 0;
#pragma unroll
            for (int w = 0; w < 8; w++) any |= canon.v[w];
            const u64 mask = __ballot(any != 0 && row < C.usable);
            if ((threadIdx.x & 63) == 0) C.bitmap[(u64)root * C.words + (row >> 6)] = mask;
            continue;                           // a root's value is read by nothing
        }
        if (c.target_kind == EVS_SLOT_LDS) L.store(c.target_slot, r);
        else f_store(&A.spill[(u64)c.target_slot * A.rows + row], f29_to_packed_canon<F9>(r));
    }
}

FP_DEV int chk_cmp(const fe& a, const fe& b) {          // canonical integers, most significant word first
    int cmp = 0;
#pragma unroll
    for (int w = 7; w >= 0; w--) {
        const int d = a.v[w] < b.v[w] ? -1 : (a.v[w] > b.v[w] ? 1 : 0);
        cmp = cmp ? cmp : d;
    }
    return cmp;
}

#define CHK_THREADS 256
template <class F>
__global__ __launch_bounds__(CHK_THREADS) void k_check_member(const fe* __restrict__ input, const fe* __restrict__ keys, u64 n_keys, u64 rows, u64 usable,
                                                              u64* __restrict__ bitmap) {
    const u64 row = (u64)blockIdx.x * CHK_THREADS + threadIdx.x;
    if (row >= rows) return;
    bool miss = false;
    if (row < usable) {
        const fe a = f_from_mont<F>(f_load(&input[row]));
        u64 lo = 0;
        for (u64 len = n_keys; len > 1;) {                   // invariant: the lower bound lies in [lo, lo + len]
            const u64 half = len >> 1;
            if (chk_cmp(f_load(&keys[lo + half - 1]), a) < 0) lo += half;
            len -= half;
        }
        if (chk_cmp(f_load(&keys[lo]), a) < 0) lo++;         // the one remaining candidate
        miss = !(lo < n_keys && chk_cmp(f_load(&keys[lo]), a) == 0);
    }
    const u64 mask = __ballot(miss);
    if ((threadIdx.x & 63) == 0) bitmap[row >> 6] = mask;
}

// the number of keys below `a` (upper: not above `a`) among n sorted canonical keys
FP_DEV u64 chk_bound(const fe* __restrict__ keys, u64 n, const fe& a, bool upper) {
    u64 lo = 0;
    for (u64 len = n; len > 0;) {                            // invariant: the bound lies in [lo, lo + len]
        const u64 half = len >> 1;
        const int c = chk_cmp(f_load(&keys[lo + half]), a);
        if (c < 0 || (upper && c == 0)) { lo += half + 1; len -= half + 1; }
        else len = half;
    }
    return lo;
}
template <class F>
__global__ __launch_bounds__(CHK_THREADS) void k_check_shuffle(const fe* __restrict__ input, const fe* __restrict__ keys_in, const fe* __restrict__ keys_side, u64 n_keys,
                                                               u64 rows, u64 usable, u64* __restrict__ bitmap) {
    const u64 row = (u64)blockIdx.x * CHK_THREADS + threadIdx.x;
    if (row >= rows) return;
    bool miss = false;
    if (row < usable) {
        const fe a = f_from_mont<F>(f_load(&input[row]));
        const u64 m_in = chk_bound(keys_in, n_keys, a, true) - chk_bound(keys_in, n_keys, a, false);
        const u64 m_side = chk_bound(keys_side, n_keys, a, true) - chk_bound(keys_side, n_keys, a, false);
        miss = m_in != m_side;
    }
    const u64 mask = __ballot(miss);
    if ((threadIdx.x & 63) == 0) bitmap[row >> 6] = mask;
}

template <class F>
int graph_check_t(dehalo_ctx* ctx, const dehalo_graph* g, const dehalo_eval_inputs* in, uint32_t log_rows, uint64_t usable, uint64_t* bitmap, uint64_t words,
                  hipStream_t s) {
    const u64 rows = 1ull << log_rows;
    if (!g->num_roots || !g->num_calcs) return 0;
    if (words < (rows + 63) / 64) return dh_fail(ctx, DEHALO_ERR_INVALID, "graph_check: bitmap row shorter than the domain");
    ScopedTimer timer(ctx, s, DEHALO_K_EVAL_H);
    ChkArgs C{};
    TRY(evh_prepare<F>(ctx, g, in, log_rows, 1, s, C.e));
    C.root_of = g->d_root_of.p; C.bitmap = (u64*)bitmap; C.words = words; C.usable = usable;
    const size_t lds = (size_t)std::max<u32>(1, g->lds_slots) * EVH_SLOT_BYTES;
    if (lds > 48 * 1024) HIP_TRY(ctx, dh_func_lds(ctx, (const void*)k_graph_check<F>, EVH_LDS_BYTES));
    k_graph_check<F><<<(u32)((rows + EVH_THREADS - 1) / EVH_THREADS), EVH_THREADS, lds, s>>>(C);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

template <class F>
int check_member_t(dehalo_ctx* ctx, const fe* input, const fe* sorted_keys, uint64_t n_keys, uint32_t log_rows, uint64_t usable, uint64_t* bitmap, hipStream_t s) {
    const u64 rows = 1ull << log_rows;
    if (!n_keys || usable > rows) return dh_fail(ctx, DEHALO_ERR_INVALID, "check_member: bad shape");
    k_check_member<F><<<(u32)((rows + CHK_THREADS - 1) / CHK_THREADS), CHK_THREADS, 0, s>>>(input, sorted_keys, n_keys, rows, usable, (u64*)bitmap);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

template <class F>
int check_shuffle_t(dehalo_ctx* ctx, const fe* input, const fe* sorted_inputs, const fe* sorted_side, uint64_t n_keys, uint32_t log_rows, uint64_t usable, uint64_t* bitmap,
                    hipStream_t s) {
    const u64 rows = 1ull << log_rows;
    if (!n_keys || usable > rows || usable > n_keys) return dh_fail(ctx, DEHALO_ERR_INVALID, "check_shuffle: bad shape");
    k_check_shuffle<F><<<(u32)((rows + CHK_THREADS - 1) / CHK_THREADS), CHK_THREADS, 0, s>>>(input, sorted_inputs, sorted_side, n_keys, rows, usable, (u64*)bitmap);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
