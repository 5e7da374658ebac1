// check.hip -- dehalo_check_witness: MockProver::verify over a proving key [UPSTREAM halo2_proofs/src/dev.rs @ v2023_04_20 MockProver::verify], on the device.
//
// Given a key (the constraint system as data, the fixed values, the compiled programs) and a witness, say WHERE the witness breaks the circuit:
//   gates    k_graph_check (check.cuh) runs the key's checking program -- every gate polynomial a root of its own -- over the original domain: one bit per
//            (polynomial, row);
//   lookups  the key's compress programs evaluate every lookup's input and table expressions with a theta fixed per key, the usable rows' table values are sorted
//            (lookup_permute.hip: tile sort + merge), k_check_member (check.cuh) searches every usable input row: one bit per (lookup, row);
//   copies   k_check_copy compares every permutation cell with the cell the mapping sends it to: one bit per (column, row).
// The three regions are ONE bitmap in (kind, index, row) order, so the report is a popcount per word, an exclusive scan and the emission of the first `cap` set
// bits: deterministic, no atomics, nothing depends on the order in which waves run.  Everything is queued on the context's stream; one host wait at the end.
#include <memory>

#include "whole_call.hpp"

namespace {

constexpr uint32_t CK_THREADS = 256;      // words of the bitmap per block of the count / emit kernels: a tile

// every entry of the mapping must name a cell of the permutation's columns: flag <- 1 otherwise.  Reads the mapping, writes the flag, nothing else.
__global__ void k_check_range(const uint64_t* __restrict__ map, uint64_t cells, uint32_t* flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cells && map[i] >= cells) *flag = 1u;
}

struct CopyArgs {
    const uint64_t* map;
    const fe* const* cols;      // the permutation's columns, in cs.permutation_columns order
    uint64_t n, words;
    uint32_t log_n;
    const uint32_t* flag;       // k_check_range's: set = the mapping is not followed at all
    uint64_t* bitmap;           // [column][words]
    uint64_t p[4];              // the field's modulus
};
// a - b as 4 x u64 -> the borrow
__device__ __forceinline__ uint64_t ck_sub4(uint64_t (&r)[4], const uint64_t (&a)[4], const uint64_t (&b)[4]) {
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t d = a[i] - b[i], d2 = d - borrow;
        borrow = (a[i] < b[i]) | (d < borrow);
        r[i] = d2;
    }
    return borrow;
}
// do two stored words stand for the same element?  A witness word is any 256-bit integer and stands for its residue (dehalo.h "Non-canonical words"): the
// larger minus the smaller is a multiple of p below 2^256, one of 0, p, .., 5p
__device__ bool ck_same_residue(const fe& a, const fe& b, const uint64_t (&p)[4]) {
    uint64_t x[4], y[4], d[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { x[i] = (uint64_t)a.v[2 * i] | (uint64_t)a.v[2 * i + 1] << 32; y[i] = (uint64_t)b.v[2 * i] | (uint64_t)b.v[2 * i + 1] << 32; }
    if (ck_sub4(d, x, y)) ck_sub4(d, y, x);
    for (int k = 0; k < 6; k++) {
        if (!(d[0] | d[1] | d[2] | d[3])) return true;
        uint64_t e[4];
        if (ck_sub4(e, d, p)) return false;
#pragma unroll
        for (int i = 0; i < 4; i++) d[i] = e[i];
    }
    return false;
}
// one lane per cell (column blockIdx.y, row): bit = "the cell the mapping sends it to holds another value"
__global__ __launch_bounds__(CK_THREADS) void k_check_copy(CopyArgs A) {
    const uint64_t row = (uint64_t)blockIdx.x * CK_THREADS + threadIdx.x;
    const uint32_t j = blockIdx.y;
    if (row >= A.n || *A.flag) return;
    const uint64_t cell = (uint64_t)j * A.n + row, m = A.map[cell];
    bool bad = false;
    if (m != cell) {
        const fe a = f_load(&A.cols[j][row]), b = f_load(&A.cols[m >> A.log_n][m & (A.n - 1)]);
        uint32_t d = 0;
#pragma unroll
        for (int w = 0; w < 8; w++) d |= a.v[w] ^ b.v[w];
        bad = d != 0 && !ck_same_residue(a, b, A.p);      // (equal words, the case of every witness halo2curves writes, decide at once)
    }
    const uint64_t mask = __ballot(bad);
    if ((threadIdx.x & 63) == 0) A.bitmap[(uint64_t)j * A.words + (row >> 6)] = mask;
}

// set bits per tile of CK_THREADS words
__global__ __launch_bounds__(CK_THREADS) void k_check_count(const uint64_t* __restrict__ bitmap, uint64_t W, uint32_t* tile_sums) {
    __shared__ uint32_t part[CK_THREADS / 64];
    const uint64_t w = (uint64_t)blockIdx.x * CK_THREADS + threadIdx.x;
    uint32_t c = w < W ? (uint32_t)__popcll(bitmap[w]) : 0u;
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t i = 0; i < CK_THREADS / 64; i++) t += part[i];
        tile_sums[blockIdx.x] = t;
    }
}
// exclusive scan of the tile sums (one block; 64-bit running total)
__global__ __launch_bounds__(1024) void k_check_scan(const uint32_t* __restrict__ tile_sums, uint64_t tiles, uint64_t* tile_prefix) {
    __shared__ uint32_t wave_sums[16];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < tiles; base += 1024) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < tiles ? tile_sums[i] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t x = __shfl_up(incl, d); if ((int)lane >= d) incl += x; }
        if (lane == 63) wave_sums[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t k = 0; k < 16; k++) { if (k < wave) before += wave_sums[k]; total += wave_sums[k]; }
        __syncthreads();
        if (i < tiles) tile_prefix[i] = carry + before + (incl - v);
        carry += total;
    }
}

struct EmitArgs {
    const uint64_t* bitmap;
    const uint64_t* tile_prefix;
    uint64_t W, words;                  // words in all, words per bitmap row
    uint32_t gates, lookups, copies;    // rows of the first three regions (the rest: shuffles)
    dehalo_check_failure* out;
    uint64_t cap;
    uint64_t* bounds;                   // [4]: set bits in front of the lookups' region, in front of the copies' region, in front of the shuffles' region, in all
};
// the position of every set bit among all set bits = tile prefix + scan inside the tile; the first `cap` are written as failures, in bitmap order
__global__ __launch_bounds__(CK_THREADS) void k_check_emit(EmitArgs A) {
    __shared__ uint32_t wave_sums[CK_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t w = (uint64_t)blockIdx.x * CK_THREADS + threadIdx.x;
    uint64_t bits = w < A.W ? A.bitmap[w] : 0ull;
    const uint32_t cnt = (uint32_t)__popcll(bits);
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t x = __shfl_up(incl, d); if ((int)lane >= d) incl += x; }
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t k = 0; k < wave; k++) before += wave_sums[k];
    if (w >= A.W) return;
    uint64_t off = A.tile_prefix[blockIdx.x] + before + (incl - cnt);
    const uint64_t bound[4] = {(uint64_t)A.gates * A.words, (uint64_t)(A.gates + A.lookups) * A.words, (uint64_t)(A.gates + A.lookups + A.copies) * A.words, A.W};
#pragma unroll
    for (int b = 0; b < 4; b++) {
        if (w == bound[b]) A.bounds[b] = off;
        if (w == A.W - 1 && bound[b] == A.W) A.bounds[b] = off + cnt;
    }
    const uint32_t row_of = (uint32_t)(w / A.words);
    const uint64_t row0 = (w % A.words) * 64;
    uint32_t kind = DEHALO_CHECK_GATE, index = row_of;
    if (row_of >= A.gates + A.lookups + A.copies) { kind = DEHALO_CHECK_SHUFFLE; index = row_of - A.gates - A.lookups - A.copies; }
    else if (row_of >= A.gates + A.lookups) { kind = DEHALO_CHECK_COPY; index = row_of - A.gates - A.lookups; }
    else if (row_of >= A.gates) { kind = DEHALO_CHECK_LOOKUP; index = row_of - A.gates; }
    while (bits && off < A.cap) {
        const uint32_t bit = (uint32_t)__builtin_ctzll(bits);
        bits &= bits - 1;
        dehalo_check_failure f;
        f.kind = kind; f.index = index; f.row = (uint32_t)(row0 + bit); f.reserved = 0;
        A.out[off++] = f;
    }
}

struct CheckHeader { uint64_t bounds[4]; uint32_t bad_mapping, pad; };

int check_body(dehalo_ctx* ctx, const dehalo_pk* pk, const uint64_t* advice, const uint64_t* const* instances, const size_t* instance_lens, uint32_t num_instance_columns,
               const uint64_t* mapping, uint32_t flags, const uint64_t* challenges, uint32_t num_challenges, dehalo_check_failure* failures, size_t cap,
               dehalo_check_report* report, std::vector<const fe*>& colptrs) {
    const HostCS& cs = pk->cs;
    const HostField* f = pk->f;
    const FieldOps* ops = dh_field_ops(f->id);
    if (!ops) return dh_fail(ctx, DEHALO_ERR_INVALID, "unknown field id");
    hipStream_t s = ctx->stream.get();
    const uint32_t k = pk->k, A = cs.num_advice, I = cs.num_instance, NF = cs.num_fixed, G = (uint32_t)cs.gates.size(), L = (uint32_t)cs.lookups.size(), H = (uint32_t)cs.shuffles.size();
    const uint32_t P = mapping ? (uint32_t)cs.perm_cols.size() : 0;
    const size_t n = pk->dom.n, u = n - (cs.blinding_factors() + 1);
    const uint64_t words = (n + 63) / 64;
    if (A && !advice) return dh_fail(ctx, DEHALO_ERR_INVALID, "check_witness: null advice");
    if (num_instance_columns != I) return dh_fail(ctx, DEHALO_ERR_INVALID, "instances.len() != num_instance_columns");      // as dehalo_create_proof
    for (uint32_t i = 0; i < I; i++) {
        const size_t len = instance_lens ? instance_lens[i] : 0;
        if (len > u) return dh_fail(ctx, DEHALO_ERR_INVALID, "instance column too long");
        if (len && (!instances || !instances[i])) return dh_fail(ctx, DEHALO_ERR_INVALID, "null instance column");
    }
    // lookups with the same table expressions share one compressed, sorted table (their representative's)
    std::vector<uint32_t> rep(L), tslot(L, 0);
    uint32_t T = 0;
    for (uint32_t l = 0; l < L; l++) { rep[l] = cs.table_representative(l); if (rep[l] == l) tslot[l] = T++; }

    // ---- workspace: [advice copy | instance | compressed inputs | compressed tables | per shuffle: compressed inputs, compressed shuffle side], [bitmap | tile sums | tile prefixes | mapping | column pointers], [header | failures]
    const bool own_advice = !(flags & DEHALO_PROOF_ADVICE_ON_DEVICE) || (flags & DEHALO_PROOF_ADVICE_CANONICAL);
    const size_t adv_elems = own_advice ? (size_t)A * n : 0;
    TRY(dh_ensure(ctx, ctx->ws_check[0], std::max<size_t>(32, (adv_elems + (size_t)(I + L + T + 2 * H) * n) * sizeof(fe))));
    fe* d_adv = (fe*)ctx->ws_check[0].p;
    fe* d_inst = d_adv + adv_elems;
    fe* d_cin = d_inst + (size_t)I * n;
    fe* d_ctab = d_cin + (size_t)L * n;
    fe* d_shuf = d_ctab + (size_t)T * n;      // shuffle j: inputs at 2 j, shuffle side at 2 j + 1
    const uint64_t R = (uint64_t)G + L + P + H, W = R * words, tiles = (W + CK_THREADS - 1) / CK_THREADS;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_sums = up(W * 8), o_prefix = o_sums + up(tiles * 4), o_map = o_prefix + up(tiles * 8), o_ptrs = o_map + up((size_t)P * n * 8);
    TRY(dh_ensure(ctx, ctx->ws_check[1], o_ptrs + up((size_t)P * sizeof(void*)) + 256));
    char* b1 = (char*)ctx->ws_check[1].p;
    uint64_t* d_bitmap = (uint64_t*)b1;
    uint32_t* d_sums = (uint32_t*)(b1 + o_sums);
    uint64_t* d_prefix = (uint64_t*)(b1 + o_prefix);
    uint64_t* d_map = (uint64_t*)(b1 + o_map);
    const fe** d_ptrs = (const fe**)(b1 + o_ptrs);
    const uint64_t capd = std::min<uint64_t>(cap, R * n);      // no more failures than bits
    const size_t res_bytes = sizeof(CheckHeader) + (size_t)capd * sizeof(dehalo_check_failure);
    TRY(dh_ensure(ctx, ctx->ws_check[2], res_bytes));
    CheckHeader* d_hdr = (CheckHeader*)ctx->ws_check[2].p;
    dehalo_check_failure* d_fail = (dehalo_check_failure*)(d_hdr + 1);
    HIP_TRY(ctx, hipMemsetAsync(d_hdr, 0, sizeof(CheckHeader), s));

    // ---- the columns, in upstream's standard form, as the prover takes them
    const fe* adv = (const fe*)advice;
    if (own_advice && A) {
        if (flags & DEHALO_PROOF_ADVICE_ON_DEVICE) HIP_TRY(ctx, hipMemcpyAsync(d_adv, advice, (size_t)A * n * 32, hipMemcpyDeviceToDevice, s));
        else TRY(dh_h2d(ctx, d_adv, advice, (size_t)A * n * 32, s));
        if (flags & DEHALO_PROOF_ADVICE_CANONICAL) TRY(ops->field_op(ctx, 4, d_adv, nullptr, d_adv, (uint64_t)A * n, s));
        adv = d_adv;
    }
    if (I) HIP_TRY(ctx, hipMemsetAsync(d_inst, 0, (size_t)I * n * 32, s));
    for (uint32_t i = 0; i < I; i++)
        if (instance_lens && instance_lens[i]) TRY(dh_h2d(ctx, d_inst + (size_t)i * n, instances[i], instance_lens[i] * 32, s));
    std::vector<const uint64_t*> fixed_v(NF), adv_v(A), inst_v(I);
    for (uint32_t i = 0; i < NF; i++) fixed_v[i] = (const uint64_t*)pk->fixed_values.at((size_t)i * n);
    for (uint32_t i = 0; i < A; i++) adv_v[i] = (const uint64_t*)(adv + (size_t)i * n);
    for (uint32_t i = 0; i < I; i++) inst_v[i] = (const uint64_t*)(d_inst + (size_t)i * n);
    // theta, fixed per key: the report of a key and a witness is reproducible
    Fe theta;
    {
        Blake2b h;
        h.init(64, "Dehalo-CheckTheta");      // (BLAKE2b's personalisation is 16 bytes: the first 16 of the string)
        uint8_t b[32], d[64];
        f->to_bytes(pk->transcript_repr, b);
        h.update(b, 32);
        h.digest(d);
        theta = f->from_u512(d);
    }
    dehalo_eval_inputs in{};
    in.fixed = fixed_v.data(); in.num_fixed = NF;
    in.advice = adv_v.data(); in.num_advice = A;
    in.instance = inst_v.data(); in.num_instance = I;
    in.theta = theta.v;
    in.challenges = challenges; in.num_challenges = num_challenges;      // (the caller's values; none for a key without challenges)

    // ---- gates
    if (G) TRY(ops->graph_check(ctx, pk->check_gates.get(), &in, k, u, d_bitmap, words, s));
    // ---- lookups: compressed inputs and tables on the original domain, the usable rows' table values sorted, every usable input row searched
    if (L) {
        std::vector<const dehalo_graph*> graphs;
        std::vector<fe*> outs;
        for (uint32_t l = 0; l < L; l++) {
            graphs.push_back(pk->compress_graphs[l].first.get());
            outs.push_back(d_cin + (size_t)l * n);
            if (rep[l] == l) {
                graphs.push_back(pk->compress_graphs[l].second.get());
                outs.push_back(d_ctab + (size_t)tslot[l] * n);
            }
        }
        TRY(ops->graph_evaluate_batch(ctx, graphs.data(), (uint32_t)graphs.size(), &in, k, 1, outs.data(), s));
        for (uint32_t t0 = 0; t0 < T; t0 += 16) {      // (the sort takes 16 columns a call; its output lives until the next one)
            const uint32_t tc = std::min<uint32_t>(16, T - t0);
            std::vector<const fe*> tabs(tc);
            for (uint32_t t = 0; t < tc; t++) tabs[t] = d_ctab + (size_t)(t0 + t) * n;
            const fe* sorted = nullptr;
            uint64_t npad = 0;
            TRY(lookup_sort_tables(ctx, f->id, tabs.data(), tc, u, &sorted, &npad, s));
            for (uint32_t l = 0; l < L; l++) {
                const uint32_t t = tslot[rep[l]];
                if (t < t0 || t >= t0 + tc) continue;
                TRY(ops->check_member(ctx, d_cin + (size_t)l * n, sorted + (size_t)(t - t0) * npad, u, k, u, d_bitmap + (uint64_t)(G + l) * words, s));
            }
        }
    }
    // ---- copy constraints
    uint64_t in_cycles = 0;
    if (P) {
        const uint64_t cells = (uint64_t)P * n;
        TRY(dh_h2d(ctx, d_map, mapping, cells * 8, s));
        k_check_range<<<(unsigned)((cells + 255) / 256), 256, 0, s>>>(d_map, cells, &d_hdr->bad_mapping);
        colptrs.resize(P);
        for (uint32_t j = 0; j < P; j++) {
            const dehalo_column_query& q = cs.perm_cols[j];
            colptrs[j] = q.kind == DEHALO_COLUMN_ADVICE ? adv + (size_t)q.index * n : q.kind == DEHALO_COLUMN_FIXED ? pk->fixed_values.at((size_t)q.index * n) : d_inst + (size_t)q.index * n;
        }
        TRY(dh_h2d(ctx, d_ptrs, colptrs.data(), (size_t)P * sizeof(void*), s));
        CopyArgs C{d_map, d_ptrs, n, words, k, &d_hdr->bad_mapping, d_bitmap + (uint64_t)(G + L) * words, {f->p[0], f->p[1], f->p[2], f->p[3]}};
        k_check_copy<<<dim3((unsigned)((n + CK_THREADS - 1) / CK_THREADS), P), CK_THREADS, 0, s>>>(C);
        HIP_TRY(ctx, hipGetLastError());
    }
    // ---- shuffles: both sides compressed with the key's theta (the programs of the proof, gamma = 0) on the original domain, the usable rows' values of each
    // sorted; every usable input row counts its value in both lists
    if (H) {
        std::vector<const dehalo_graph*> graphs;
        std::vector<fe*> outs;
        for (uint32_t j = 0; j < H; j++) {
            graphs.push_back(pk->shuffle_graphs[j].first.get());
            outs.push_back(d_shuf + (size_t)(2 * j) * n);
            graphs.push_back(pk->shuffle_graphs[j].second.get());
            outs.push_back(d_shuf + (size_t)(2 * j + 1) * n);
        }
        TRY(ops->graph_evaluate_batch(ctx, graphs.data(), (uint32_t)graphs.size(), &in, k, 1, outs.data(), s));
        for (uint32_t j0 = 0; j0 < H; j0 += 8) {      // (the sort takes 16 columns a call: eight shuffles; its output lives until the next one)
            const uint32_t jc = std::min<uint32_t>(8, H - j0);
            std::vector<const fe*> tabs(2 * jc);
            for (uint32_t t = 0; t < 2 * jc; t++) tabs[t] = d_shuf + (size_t)(2 * j0 + t) * n;
            const fe* sorted = nullptr;
            uint64_t npad = 0;
            TRY(lookup_sort_tables(ctx, f->id, tabs.data(), 2 * jc, u, &sorted, &npad, s));
            for (uint32_t j = 0; j < jc; j++)
                TRY(ops->check_shuffle(ctx, d_shuf + (size_t)(2 * (j0 + j)) * n, sorted + (size_t)(2 * j) * npad, sorted + (size_t)(2 * j + 1) * npad, u, k, u,
                                       d_bitmap + (uint64_t)(G + L + P + j0 + j) * words, s));
        }
    }
    // ---- count, scan, emit
    if (W) {
        k_check_count<<<(unsigned)tiles, CK_THREADS, 0, s>>>(d_bitmap, W, d_sums);
        k_check_scan<<<1, 1024, 0, s>>>(d_sums, tiles, d_prefix);
        EmitArgs E{d_bitmap, d_prefix, W, words, G, L, P, d_fail, capd, d_hdr->bounds};
        k_check_emit<<<(unsigned)tiles, CK_THREADS, 0, s>>>(E);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (P)      // (host work beside the device's: the mapping is the caller's array)
        for (uint64_t c = 0; c < (uint64_t)P * n; c++) in_cycles += mapping[c] != c;
    // ---- one download: the header and the stored failures; the call's one host wait
    std::vector<uint8_t> host(res_bytes);
    TRY(dh_d2h(ctx, host.data(), d_hdr, res_bytes, s));
    CheckHeader hdr;
    memcpy(&hdr, host.data(), sizeof hdr);
    if (hdr.bad_mapping) return dh_fail(ctx, DEHALO_ERR_INVALID, "check_witness: permutation mapping points outside the permutation's columns");
    memset(report, 0, sizeof *report);
    report->gate_failures = hdr.bounds[0];
    report->lookup_failures = hdr.bounds[1] - hdr.bounds[0];
    report->copy_failures = hdr.bounds[2] - hdr.bounds[1];
    report->rows = u;
    report->lookup_inputs = (uint64_t)u * L;
    report->cells_in_cycles = in_cycles;
    report->shuffle_failures = hdr.bounds[3] - hdr.bounds[2];
    report->shuffle_inputs = (uint64_t)u * H;
    report->written = std::min<uint64_t>(cap, hdr.bounds[3]);
    if (report->written) memcpy(failures, host.data() + sizeof hdr, (size_t)report->written * sizeof(dehalo_check_failure));
    return 0;
}

}   // namespace

namespace {
int check_entry(dehalo_ctx* ctx, const dehalo_pk* pk, const uint64_t* advice, const uint64_t* const* instances, const size_t* instance_lens, uint32_t num_instance_columns,
                const uint64_t* permutation_mapping, uint32_t flags, const uint64_t* challenges, uint32_t num_challenges, bool with_challenges, dehalo_check_failure* failures,
                size_t cap, dehalo_check_report* report) {
    if (!ctx) return DEHALO_ERR_INVALID;
    return dh_guard(ctx, [&]() -> int {
        if (!pk || !report) return dh_fail(ctx, DEHALO_ERR_INVALID, "check_witness: null argument");
        if (!with_challenges && pk->cs.has_challenge_node())
            return dh_fail(ctx, DEHALO_ERR_INVALID, "check_witness: the key's expressions read challenges; pass their values to dehalo_check_witness_challenges");
        if (with_challenges && (num_challenges != pk->cs.challenge_phase.size() || (num_challenges && !challenges)))
            return dh_fail(ctx, DEHALO_ERR_INVALID, "check_witness_challenges: one value per challenge of the key (dehalo_pk_phases)");
        if (cap && !failures) return dh_fail(ctx, DEHALO_ERR_INVALID, "check_witness: null failure array with a non-zero capacity");
        if (pk->ctx->device != ctx->device) return dh_fail(ctx, DEHALO_ERR_INVALID, "check_witness: the proving key lives on another device");
        const size_t n = pk->dom.n;
        // page-locked for the call: the uploads are DMA from the caller's pages, which this call's one host wait outlives
        HostPin pin_advice((flags & DEHALO_PROOF_ADVICE_ON_DEVICE) ? nullptr : advice, (size_t)pk->cs.num_advice * n * 32);
        HostPin pin_map(permutation_mapping, pk->cs.perm_cols.size() * n * 8);
        std::vector<const fe*> colptrs;
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        const int rc = check_body(ctx, pk, advice, instances, instance_lens, num_instance_columns, permutation_mapping, flags, challenges, num_challenges, failures, cap, report,
                                  colptrs);
        if (rc) (void)hipStreamSynchronize(ctx->stream.get());      // nothing of this call stays in flight over the caller's buffers
        return rc;
    });
}
}   // namespace

extern "C" int dehalo_check_witness(dehalo_ctx* ctx, const dehalo_pk* pk, const uint64_t* advice, const uint64_t* const* instances, const size_t* instance_lens,
                                    uint32_t num_instance_columns, const uint64_t* permutation_mapping, uint32_t flags, dehalo_check_failure* failures, size_t cap,
                                    dehalo_check_report* report) {
    return check_entry(ctx, pk, advice, instances, instance_lens, num_instance_columns, permutation_mapping, flags, nullptr, 0, false, failures, cap, report);
}

extern "C" int dehalo_check_witness_challenges(dehalo_ctx* ctx, const dehalo_pk* pk, const uint64_t* advice, const uint64_t* const* instances, const size_t* instance_lens,
                                               uint32_t num_instance_columns, const uint64_t* permutation_mapping, uint32_t flags, const uint64_t* challenges,
                                               uint32_t num_challenges, dehalo_check_failure* failures, size_t cap, dehalo_check_report* report) {
    return check_entry(ctx, pk, advice, instances, instance_lens, num_instance_columns, permutation_mapping, flags, challenges, num_challenges, true, failures, cap, report);
}
