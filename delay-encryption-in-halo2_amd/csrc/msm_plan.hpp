// msm_plan.hpp -- the shape policy of the Pippenger MSM (msm.cuh): which window a table gets, and for one launch the sort slices, the windows per
// sort block, the histogram's counter width, every grid, block size and LDS size, and the bytes of every workspace buffer.  run_msm_t only asks for a
// plan, ensures the buffers and launches.  Host-only and free of HIP headers (like guard.hpp), so that the arithmetic most likely to break at an
// untested shape is checked without a device: tests/native_host/msm_plan_check.cpp sweeps it under ASan / UBSan.  The constants that kernels and
// planner share are defined here; msm.cuh includes this header, so device code sees the same definitions.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "experiment_env.hpp"

#ifdef __HIPCC__
#define MSM_PLAN_HD __host__ __device__
#else
#define MSM_PLAN_HD
#endif

#define MSM_SORT_THREADS 1024
#define MSM_ACC_THREADS 128        // the accumulation's default block: 2 waves (4 waves x 122 VGPRs fill a SIMD's register file)
#define MSM_ACC_THREADS_MAX 768    // msm_acc_block = 768: ONE block of 12 waves per CU = 3 waves per SIMD and no room for a second block -- a quarter of every
                                   // SIMD's registers (and all of the LDS) stays free for the <= 128-VGPR kernels of the other contexts
#define MSM_MERGE_COUNTERS 8   // merge-class counters in ws_counters, in front of [L0 | M]

// classes of k_msm_merge2 (msm_bred.cuh) by the number S of partial sums of a bucket; S > MERGE2_CHUNK: cut into parts of MERGE2_CHUNK records
#define MERGE2_CHUNK 512

#define MSM_IDX_FIRST 0x40000000u     // sorted entry, bit 30: first point of its bucket
#define MSM_IDX_MASK 0x3fffffffu      // table index (precomputed tables: window * table_n + point < 2^30, checked at registration: msm_table_fits)

#define SCAN_THREADS 256              // k_msm_colscan, k_scan_offsets: one thread per bucket

// LDS of one wave of k_msm_part: the staging of 512 pairs (8 B + a 2-B partition tag each) and four words per list (count, first slot, cursor, reserved position);
// `lists` = 128, or 256 for the 256 partitions of a 17-bit window
#define MSM_PART_WAVE_LDS(lists) (4 * (lists) * 4 + 512 * 8 + 512 * 2)
#define MSM_BUCKET_SLICES 4
#define MSM_BUCKET_THREADS 256
#define MSM_REC_BYTES 144             // sizeof(xyzz29_rec): four coordinates of nine 29-bit limbs (msm.cuh asserts it)

// the bucket reduction and the merge (msm_bred.cuh)
#define BRED_THREADS 256
#define BRED_BLOCK_BUCKETS 256      // buckets of a block at most (the LDS array): 4 per quad
#define BRED_BLOCK_BUCKETS_MIN 128  // ... and at least (sizes the node buffers); msm_plan picks (bred_bb)
#define BRED_FANIN 16               // node vectors one block combines in the second / third stage
#define BRED_VMAX 17                // points per node vector in HBM: A_0 .. A_15, X
#define BRED_CNT_PER_GROUP 32       // u32 counters per bucket group: clusters [0, 16), group [16]
#define MERGE2_BLOCKS_LIGHT 1024     // per light class
#define MERGE2_BLOCKS_Q8 512
#define MERGE2_BLOCKS_BLOCK 512
#define MERGE2_BLOCKS_PARTS 1024
#define MERGE2_BLOCKS_COPY 256        // buckets with one partial sum (copied) or none (identity): one lane per bucket, the last section of the grid
#define MERGE2_GRID_SUMS (MERGE2_BLOCKS_PARTS + MERGE2_BLOCKS_BLOCK + MERGE2_BLOCKS_Q8 + 3 * MERGE2_BLOCKS_LIGHT)
#define MERGE2_GRID (MERGE2_GRID_SUMS + MERGE2_BLOCKS_COPY)

struct MsmGeom {
    uint32_t n;          // scalars per MSM
    uint32_t table_n;    // registered points (row pitch of the window tables)
    uint32_t c;          // window bits
    uint32_t W;          // windows = ceil(256 / c)
    uint32_t nb;         // buckets per group = 2^(c-1)
    uint32_t G;          // bucket groups per MSM: 1 (precomputed tables) or W
    uint32_t batch;      // independent MSMs in this launch
    uint32_t slices;     // sort blocks per (group, batch)
    uint32_t L0;         // points per lane of k_msm_accum0
    uint32_t wb;         // G == W only: windows (= bucket groups) one sort block covers; the sort's grid.y = ceil(G / wb)
};

// second-level split of the bucket index: buckets = partitions x 2^sub sub-buckets
// (17-bit windows: 512 sub-buckets, so that the 2^16 buckets are still 128 partitions -- k_msm_part's lists -- and a k_msm_bucket round is still 2048 pairs)
MSM_PLAN_HD inline uint32_t msm_sub_bits(uint32_t c) { return c - 1 < 8 ? c - 1 : (c >= 17 ? 9u : 8u); }

// ---- the window of a table ----------------------------------------------------------------
// 4 bits (the bucket reduction wants 8 buckets) .. 16; 17 with precomputed rows only: 2^16 buckets are one group's histogram as packed 16-bit counters
#define MSM_WINDOW_MIN 4u
inline uint32_t msm_window_max(bool precomp) { return precomp ? 17u : 16u; }

inline uint32_t log2_ceil(size_t n) {
    uint32_t l = 0;
    while (((size_t)1 << l) < n) l++;
    return l;
}

// Window bits by measurement on MI355X (tools/sweep_c.py, tools/profile_prover.py with WINDOW_BITS): the bucket
// reduction costs ~ 2^(c-1) group operations on a latency chain, the accumulation n * ceil(256 / c) additions.
// 2^20 and up: 16; 2^17 .. 2^19: 15; 2^10 .. 2^16: 13 (prover-shaped schedule at k = 14: 2.9 ms of MSMs with
// c = 13, 3.1 with 15, 3.5 with 14 -- even c leaves a top window of few bits whose buckets are hot).
inline uint32_t choose_window(size_t n) {
    uint32_t l = log2_ceil(n ? n : 1);
    // 2^20 and up: 17 bits -- 15 rows instead of 16 (6 % fewer additions), 2^16 buckets whose histogram fits the LDS as packed 16-bit counters; four alternating pairs
    // at 2^20: 760.7 -> 779.1 Mpoints/s in the step, one MSM alone 1.55 -> 1.48 ms (profiles/r06_window_17.txt)
    if (l >= 20) return 17;
    if (l >= 19) return 16;      // k = 19 proofs 25.7 -> 25.0 ms against 15 bits (17: 26.4); k = 17 / 18 stay at 15 (7.25 / 12.9 ms against 7.5 / 13.0 at 16): profiles/r06_window_sweep_proofs.txt
    if (l >= 17) return 15;
    if (l >= 10) return 13;
    return std::max<uint32_t>(6, l + 1);
}

// Single-row tables (the one-shot, unregistered path: every window keeps its own buckets and the window sums are combined by
// c (W - 1) doublings): fewer buckets per window pay for the extra windows.  Measured on MI355X (tools/sweep_single_row.py, Pallas,
// uniform scalars, device time): 2^14 c = 10 0.81 ms (13: 0.95, 16: 1.12); 2^17 c = 13 1.15 (10: 1.21, 15: 1.39); 2^20 c = 13 3.13 (16: 3.51).
inline uint32_t choose_window_single(size_t n) {
    uint32_t l = log2_ceil(n ? n : 1);
    if (l >= 16) return 13;
    if (l >= 12) return 10;
    return choose_window(n);
}

// Windows of the signed-digit recoding: the smallest W for which no canonical scalar s < r leaves a carry after window W - 1
// (msm.cuh for_each_digit drops it).  With top = (r - 1) >> c(W - 1) that holds when top + 1 <= 2^(c-1), and also when top == 2^(c-1)
// exactly while the c bits of r - 1 just below the top window are all zero (then s with that top digit has a zero digit in window
// W - 2, which absorbs any carry).  E.g. BN254 Fr, c = 15: 17 windows instead of ceil(256 / 15) = 18; Pasta Fq, c = 17: 15.
inline uint32_t signed_windows(const uint32_t r_words[8], uint32_t c) {
    uint64_t r1[4];                                                  // r - 1 (r is odd)
    for (int i = 0; i < 4; i++) r1[i] = (uint64_t)r_words[2 * i] | ((uint64_t)r_words[2 * i + 1] << 32);
    r1[0] -= 1;
    auto bits_at = [&](uint32_t lo, uint32_t count) -> uint64_t {   // bits [lo, lo + count) of r - 1, count <= 32
        uint64_t v = 0;
        for (uint32_t b = 0; b < count; b++) {
            uint32_t pos = lo + b;
            if (pos < 256 && ((r1[pos >> 6] >> (pos & 63)) & 1)) v |= 1ull << b;
        }
        return v;
    };
    for (uint32_t W = (254 + c - 1) / c; W <= (256 + c - 1) / c; W++) {
        if (W < 2) continue;
        const uint32_t shift = c * (W - 1);
        bool above = false;                                          // anything of r - 1 above the top window?
        for (uint32_t pos = shift + c; pos < 256; pos++) above |= ((r1[pos >> 6] >> (pos & 63)) & 1) != 0;
        if (above) continue;
        const uint64_t top = bits_at(shift, c), half = 1ull << (c - 1);
        if (top + 1 <= half) return W;
        if (top == half && bits_at(shift - c, c) == 0) return W;
    }
    return (256 + c - 1) / c;
}

// a precomputed table of n points x W window rows: its indices fit the 30 bits of a sorted entry (MSM_IDX_MASK)
inline bool msm_table_fits(size_t n, uint32_t W) { return n < (1ull << 30) && (uint64_t)n * W < (1ull << 30); }

// ---- one launch ------------------------------------------------------------------------------
struct MsmShape {
    size_t len, batch;      // scalars per MSM, independent MSMs
    size_t table_n;         // registered points
    uint32_t c, W;          // the table's window bits and windows
    bool precomp;           // a row per window (one bucket group) or a single row (a group per window)
};

// what the caller may tune (dehalo_ctx, dehalo_ctx_set_tuning) and what only a measurement build reads from the environment (msm_experiment_tuning)
struct MsmTuning {
    int sort_block = 1024, acc_block = 128, acc_points = 48, acc_waves = 3, acc_min_layers = 4;      // dehalo_ctx::msm_*
    int num_cus = 256;
    // small precomputed-table launches: 2048 scalars a sort block leave a 2^14 column 8 blocks and a 2^11 column ONE for k_msm_hist / k_msm_part (21 + 34 us of
    // latency where the work is 2); down to 256 scalars a block until ~128 blocks are there (DEHALO_MSM_SMALL_SLICES=0: the A/B)
    bool small_slices = true;
    // block sizes of the two scalar-decoding sort kernels (DEHALO_MSM_HIST_THREADS / DEHALO_MSM_PART_THREADS, 64 .. 1024; 0: sort_block): smaller blocks fit beside a
    // resident accumulation of another context (msm_acc_block = 768 leaves one 128-VGPR wave slot per SIMD: 512 threads x 62 VGPRs, 256 x 77)
    uint32_t hist_threads = 0, part_threads = 0;
    // slices per k_msm_bucket block: 4 (measured best on dense columns) unless DEHALO_MSM_BUCKET_SLICES says otherwise (1 / 2 / 4 / 8: A/B measurements
    // on the skewed columns of a proof, where a block's run can be 17 windows x 4 slices of ONE value) ...
    uint32_t bucket_slices = MSM_BUCKET_SLICES;
    // ... and fewer while the grid would not give every CU a block (2^14: 16 partitions x 8 slices -- 32 blocks of 10 k pairs each took 49 us a column, round 4)
    bool bucket_fill = true;
    // DEHALO_MSM_ACC_LDS (bytes of dynamic LDS per block, unused by the kernel): caps the accumulation's resident blocks per CU so that
    // wave slots and registers stay free for the kernels of other contexts (tuning experiments; results never depend on it)
    uint32_t acc_lds = 0;
    uint32_t bred_block = 0;      // DEHALO_MSM_BRED_BLOCK: 128 or 256 buckets per k_msm_bred block whatever the window (0: by the window)
};

// The experiment switches, read once.  In the default build every DH_EXPERIMENT_ENV is a compile-time null: this is MsmTuning{} and the names are not in the binary.
inline const MsmTuning& msm_experiment_tuning() {
    static const MsmTuning tuning = [] {
        MsmTuning t;
        auto off = [](const char* e) { return e && e[0] == '0'; };
        auto threads = [](const char* e) { const int v = e ? atoi(e) : 0; return (uint32_t)std::max(0, std::min(MSM_SORT_THREADS, v & ~63)); };
        t.small_slices = !off(DH_EXPERIMENT_ENV("DEHALO_MSM_SMALL_SLICES"));
        t.hist_threads = threads(DH_EXPERIMENT_ENV("DEHALO_MSM_HIST_THREADS"));
        t.part_threads = threads(DH_EXPERIMENT_ENV("DEHALO_MSM_PART_THREADS"));
        if (const char* e = DH_EXPERIMENT_ENV("DEHALO_MSM_BUCKET_SLICES")) { const int v = atoi(e); if (v >= 1 && v <= 16) t.bucket_slices = (uint32_t)v; }
        t.bucket_fill = !off(DH_EXPERIMENT_ENV("DEHALO_MSM_BUCKET_FILL"));
        if (const char* e = DH_EXPERIMENT_ENV("DEHALO_MSM_ACC_LDS")) t.acc_lds = (uint32_t)atoi(e);
        if (const char* e = DH_EXPERIMENT_ENV("DEHALO_MSM_BRED_BLOCK")) { const int v = atoi(e); if (v == 128 || v == 256) t.bred_block = (uint32_t)v; }
        return t;
    }();
    return tuning;
}

// the workspace buffers of one launch (dehalo_ctx::ws_*; run_msm_t holds the members in this order)
enum MsmWs {
    MSM_WS_COUNT, MSM_WS_COUNTERS, MSM_WS_BHIST, MSM_WS_PCOUNT, MSM_WS_PAIRS, MSM_WS_OFF, MSM_WS_RECORDS, MSM_WS_MERGE_PARTS, MSM_WS_MERGE_LISTS, MSM_WS_IDX,
    MSM_WS_PARTIAL0, MSM_WS_BUCKETS, MSM_WS_CONTRIB, MSM_WS_TREE, MSM_WS_BRED_CNT, MSM_WS_GSUMS, MSM_WS_BSUM, MSM_WS_N
};

// No heap members: it is built on every MSM call.  LDS sizes are the kernels' own needs, before dh_co_lds_pad.
struct MsmPlan {
    MsmGeom g;
    uint64_t total_groups, total_buckets, Mmax;      // batch * G; ... * nb; sorted points at most: batch * len * W
    uint32_t P;                                      // partitions of a group's buckets: nb >> msm_sub_bits(c)
    bool pack16;                                     // k_msm_hist counts in packed 16-bit counters
    // the sort: k_msm_hist and k_msm_part share a grid; the two scans; k_msm_bucket
    uint32_t hist_threads, part_threads, part_lists, sort_grid[3];
    size_t lds_hist, lds_part;
    uint32_t cs_a, cs_b;                             // k_msm_colscan's blocks over the buckets (= k_scan_offsets' grid) and over the partition counts
    uint32_t bslices, bucket_threads, bucket_grid[2];
    size_t lds_bucket;                               // (static)
    // the accumulation: the device fixes the points per lane from the points actually sorted (k_scan_offsets); the host bounds the lanes
    uint32_t lcap, kmin, acc_block, acc_grid, acc_lds;      // lcap, kmin: msm_acc_points, msm_acc_min_layers as k_scan_offsets takes them
    uint64_t resident, lmax, lanes_max, nt0_max;     // nt0_max: partial-sum records, one per lane + one per non-empty bucket (upper bound)
    // merge and bucket reduction
    uint32_t merge_cap, bred_bb, nblk;
    size_t ws_bytes[MSM_WS_N];
};

// The plan of one launch, or the message of the error that refuses it.  len, batch >= 1.
inline const char* msm_plan(const MsmShape& sh, const MsmTuning& t, MsmPlan* plan) {
    if (sh.c < MSM_WINDOW_MIN) return "msm: window below 4 bits";      // (unreachable through dehalo_bases_register: c >= 4)
    MsmPlan& p = *plan;
    p = MsmPlan{};
    MsmGeom& g = p.g;
    const size_t len = sh.len, batch = sh.batch;
    g.n = (uint32_t)len; g.table_n = (uint32_t)sh.table_n; g.c = sh.c; g.W = sh.W; g.nb = 1u << (g.c - 1);
    g.G = sh.precomp ? 1 : g.W;
    g.batch = (uint32_t)batch;
    g.L0 = 0;
    // sort blocks (k_msm_hist, k_msm_part): msm_sort_block threads, two scalars a thread until the grid has 256 K threads, then longer slices.  1024-thread
    // blocks (the default) take 128 and 115 KiB of LDS and so a compute unit to themselves; 512-thread blocks take 64 KiB (packed 16-bit histogram) and 58 KiB
    // (eight waves' staging) and start beside an NTT tile / merge / reduction block of another context -- which removes the sort's waiting and nothing else:
    // the chip is throughput-bound, the time moves to the kernels the sort now shares a CU with, and twice the per-slice histograms cost 26 us of the lone sort
    // (profiles/r06_sort_block_ab.txt; DESIGN.md sections 4 and 8)
    const uint32_t sort_threads = t.sort_block == 512 ? 512u : 1024u;
    g.slices = (uint32_t)std::min<size_t>(256 * (1024 / sort_threads), std::max<size_t>(1, len / (2 * sort_threads)));
    if (t.small_slices && g.G == 1 && (size_t)g.slices * batch < 128)
        g.slices = (uint32_t)std::max<size_t>(g.slices, std::min<size_t>(std::max<size_t>(1, len / 256), (128 + batch - 1) / batch));
    if ((size_t)g.nb * 4 > 128 * 1024) {      // a 17-bit window (2^16 buckets: precomputed tables only): the histogram fits the LDS only as packed 16-bit counters --
        if (g.G != 1) return "a 17-bit window needs a precomputed table";
        g.slices = (uint32_t)std::max<uint64_t>(g.slices, ((uint64_t)len * g.W + 65534) / 65535);      // -- so a slice's scalars times the windows stay below 2^16
    }
    p.P = g.nb >> msm_sub_bits(g.c);
    {   // single-row tables: windows per sort block -- the block's histograms fit 128 KiB of LDS and its (group, partition) runs the 128 staging lists
        const uint32_t fit = std::min<uint32_t>(std::min<uint32_t>(g.W, 128 / p.P), (128u * 1024 / 4) / g.nb);
        const uint32_t fill = (uint32_t)((uint64_t)g.W * g.slices * batch / 256);        // ... while the grid keeps >= 256 blocks (2^14: one window per block as before)
        g.wb = g.G == 1 ? g.W : std::max<uint32_t>(1, std::min<uint32_t>(fit, fill));
    }
    p.total_groups = (uint64_t)batch * g.G;
    p.total_buckets = p.total_groups * g.nb;
    p.Mmax = (uint64_t)batch * len * g.W;
    if (p.Mmax >= (1ull << 32) || p.total_buckets >= (1ull << 31)) return "batch * len * windows too large for one launch";
    const uint64_t tg = p.total_groups, tb = p.total_buckets;

    // packed 16-bit counters when no bucket of a block can be counted 2^16 times: every scalar of the slice in every window of the block (all windows for G == 1)
    const uint32_t per_slice = (uint32_t)((len + g.slices - 1) / g.slices);
    p.pack16 = g.nb >= 2 && (uint64_t)per_slice * (g.G == 1 ? g.W : g.wb) <= 65535;
    p.lds_hist = (size_t)g.nb * (p.pack16 ? 2 : 4) * (g.G == 1 ? 1 : g.wb);
    p.hist_threads = t.hist_threads ? t.hist_threads : sort_threads;
    p.part_threads = t.part_threads ? t.part_threads : sort_threads;
    p.part_lists = (g.G == 1 ? p.P : 128u) > 128u ? 256u : 128u;      // (G == W: wb windows x P partitions <= 128 by the choice of wb above)
    p.lds_part = 4 * (size_t)p.part_lists + (size_t)(p.part_threads / 64) * MSM_PART_WAVE_LDS(p.part_lists);
    p.sort_grid[0] = g.slices; p.sort_grid[1] = g.G == 1 ? 1 : (g.G + g.wb - 1) / g.wb; p.sort_grid[2] = (uint32_t)batch;
    p.cs_a = ((uint32_t)tb + SCAN_THREADS - 1) / SCAN_THREADS;
    p.cs_b = ((uint32_t)tg * p.P + SCAN_THREADS - 1) / SCAN_THREADS;
    p.bslices = t.bucket_slices;
    while (t.bucket_fill && p.bslices > 1 && (uint64_t)p.P * ((g.slices + p.bslices - 1) / p.bslices) * tg < (uint64_t)t.num_cus) p.bslices >>= 1;
    p.bucket_threads = MSM_BUCKET_THREADS;
    p.bucket_grid[0] = p.P * ((g.slices + p.bslices - 1) / p.bslices); p.bucket_grid[1] = (uint32_t)tg;
    p.lds_bucket = 22 * 1024;

    // points per lane: the lanes fill the chip (msm_acc_waves waves per SIMD of k_msm_accum0) a whole number of times
    p.lcap = (uint32_t)t.acc_points;
    p.kmin = (uint32_t)t.acc_min_layers;
    p.resident = (uint64_t)t.num_cus * 4 * (p.lcap ? 1 : (uint64_t)t.acc_waves) * 64;
    p.lmax = 64 * 4 / (uint64_t)t.acc_waves;
    p.acc_block = t.acc_block == MSM_ACC_THREADS_MAX ? MSM_ACC_THREADS_MAX : MSM_ACC_THREADS;
    if (p.lcap) {
        uint64_t k = 4;
        while (p.Mmax > k * p.resident * p.lcap) k += 2;
        p.lanes_max = k * p.resident + p.acc_block;
    } else {
        const uint64_t rounds_max = std::max<uint64_t>(1, (p.Mmax + p.resident * p.lmax - 1) / (p.resident * p.lmax));
        p.lanes_max = rounds_max * p.resident + p.acc_block;
    }
    p.nt0_max = p.lanes_max + tb;
    p.acc_grid = (uint32_t)((p.lanes_max + p.acc_block - 1) / p.acc_block);
    p.acc_lds = t.acc_lds;

    // merge-class lists: `cap` words per class -- a bucket index per listed bucket, or (classes 5 / 6 of k_msm_merge2) 2 words per 512-record part and 4 per heavy bucket
    p.merge_cap = (uint32_t)std::max<uint64_t>(std::min<uint64_t>(tb, p.nt0_max / 2 + 1), 4 * (p.nt0_max / MERGE2_CHUNK + 2));
    // buckets per k_msm_bred block: 128 up to 2^13 buckets (the kernel alone 119 -> 107 us at 4096 buckets, 134 -> 125 at 16384, 153 -> 153 at 32768 where the third level costs
    // what the shorter first one saves); 256 above: measured on k = 17 proofs the 128-bucket blocks -- twice as many, beside the side context's transforms -- cost
    // 0.1 ms (profiles/r04_bred_block_buckets.txt).  The experiment's value holds only while the first level's blocks fit the two levels of cluster counters above it.
    const bool bred_forced = t.bred_block && g.nb / t.bred_block <= BRED_FANIN * BRED_FANIN;
    p.bred_bb = bred_forced ? t.bred_block : (g.nb <= 8192 ? 128u : 256u);
    p.nblk = std::max<uint32_t>(1, g.nb / p.bred_bb);

    const size_t REC = MSM_REC_BYTES;
    size_t* ws = p.ws_bytes;
    ws[MSM_WS_COUNT] = tb * 4;
    ws[MSM_WS_COUNTERS] = 64;                                        // 8 merge-class counters | L0 | M
    ws[MSM_WS_BHIST] = tb * (size_t)g.slices * 6;                    // per-block histograms: the prefixes (u32), and behind them the packed 16-bit counts when k_msm_hist writes those
    ws[MSM_WS_PCOUNT] = tg * (size_t)g.slices * p.P * 4;             // per-(slice, partition) counts
    ws[MSM_WS_PAIRS] = p.Mmax * 8;                                   // partition-sorted (sub-bucket, reference) pairs
    ws[MSM_WS_OFF] = (tb + 1) * 4;
    ws[MSM_WS_RECORDS] = (tb + 1) * 4 * 3;                           // nrank | rbeg | rend
    ws[MSM_WS_MERGE_PARTS] = (2 * (p.nt0_max / MERGE2_CHUNK) + 4) * REC;      // part sums of the heavy buckets
    ws[MSM_WS_MERGE_LISTS] = (size_t)p.merge_cap * MSM_MERGE_COUNTERS * 4;
    ws[MSM_WS_IDX] = p.Mmax * 4;
    ws[MSM_WS_PARTIAL0] = p.nt0_max * REC;
    ws[MSM_WS_BUCKETS] = tb * REC;
    // (the radix-2 bucket reduction keeps its node vectors in the same two buffers: BRED_VMAX records per block of 128 / 256 buckets / per cluster of 16 blocks)
    ws[MSM_WS_CONTRIB] = tg * std::max<size_t>(1, g.nb / BRED_BLOCK_BUCKETS_MIN) * BRED_VMAX * REC;
    ws[MSM_WS_TREE] = tg * 16 * BRED_VMAX * REC;
    ws[MSM_WS_BRED_CNT] = (size_t)tg * BRED_CNT_PER_GROUP * 4;       // cluster / group arrival counters
    ws[MSM_WS_GSUMS] = tg * REC;
    ws[MSM_WS_BSUM] = (size_t)p.cs_a * 2 * sizeof(uint32_t);         // sums of k_msm_colscan's blocks: points | non-empty buckets
    return nullptr;
}
