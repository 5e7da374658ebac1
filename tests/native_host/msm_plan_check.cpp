// msm_plan_check.cpp -- the MSM's launch planner (csrc/msm_plan.hpp) swept over the shapes a device run never sees; built by g++ with ASan + UBSan
// (make msm_plan_check), run by tests/test_host_logic.py.  Every invariant the kernels rely on and the shape rules only state in comments is asserted for
// every plan that is not an error, and every workspace size is compared with its closed form, spelled out here from MsmGeom alone.
//
// Shapes: every len in 1 .. 2^17 and 2^k, 2^k +- {1, 3, 4369} for k = 17 .. 22; batch 1, 2, 3, 4, 7, 12, 16, 64; precomputed and single-row tables;
// c = 4 .. 17 with W = signed_windows(r, c) for the scalar moduli of the three curves; 256 compute units.
// Tunings: msm_sort_block 512 / 1024, msm_acc_block 128 / 768, msm_acc_points 0 / 48, msm_acc_waves 1 .. 4, msm_acc_min_layers 2 .. 4: 96 combinations.  The edge
// lengths meet all 96.  The dense range 1 .. 2^17 meets both sort blocks (the only tuning the sort's shape depends on) and ONE of the 48 accumulation tunings per
// shape, taken in rotation over len, batch and c (the accumulation's bounds depend on the shape only through Mmax and the bucket total, which move smoothly
// with len): 10^8 plans instead of 5 * 10^9.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../delay-encryption-in-halo2_amd/csrc/field_constants.h"
#include "../../delay-encryption-in-halo2_amd/csrc/msm_plan.hpp"

namespace {

typedef uint64_t u64;
typedef uint32_t u32;

const char* g_what = "";
MsmShape g_sh;
MsmTuning g_tu;
#define CHECK(cond)                                                                                                                                     \
    do {                                                                                                                                                \
        if (!(cond)) {                                                                                                                                  \
            fprintf(stderr, "msm_plan_check: %s: FAILED %s (line %d)\n  len %zu batch %zu table_n %zu c %u W %u precomp %d | sort_block %d acc_block %d " \
                    "acc_points %d acc_waves %d acc_min_layers %d num_cus %d bred_block %u\n", g_what, #cond, __LINE__, g_sh.len, g_sh.batch, g_sh.table_n, \
                    g_sh.c, g_sh.W, (int)g_sh.precomp, g_tu.sort_block, g_tu.acc_block, g_tu.acc_points, g_tu.acc_waves, g_tu.acc_min_layers,            \
                    g_tu.num_cus, g_tu.bred_block);                                                                                                      \
            exit(1);                                                                                                                                    \
        }                                                                                                                                               \
    } while (0)

u64 ceil_div(u64 a, u64 b) { return (a + b - 1) / b; }

// k_scan_offsets' points per lane L for M sorted points (msm.cuh), restated
u64 device_L(u64 M, u64 resident, u64 lmax, u64 lcap, u64 kmin) {
    u64 L;
    if (lcap) {
        u64 k = kmin;
        while (M > k * resident * lcap) k += k < 4 ? 1 : 2;
        L = std::max<u64>(4, (M + k * resident - 1) / (k * resident));
    } else {
        const u64 rounds = std::max<u64>(1, (M + resident * lmax - 1) / (resident * lmax));
        L = (M + rounds * resident - 1) / (rounds * resident);
        L = std::min<u64>(lmax, std::max<u64>(4, L));
    }
    return L;
}

u64 g_plans = 0, g_errors = 0;

void check_shape(const MsmShape& sh, const MsmTuning& tu) {
    g_sh = sh; g_tu = tu; g_what = "plan";
    MsmPlan p;
    const char* err = msm_plan(sh, tu, &p);
    g_plans++;
    const u64 len = sh.len, batch = sh.batch, c = sh.c, W = sh.W, G = sh.precomp ? 1 : W, nb = 1ull << (c - 1);
    const u64 tg = batch * G, tb = tg * nb, Mmax = batch * len * W;
    // the two refusals, and nothing else
    const bool want_17 = c == 17 && !sh.precomp, want_large = Mmax >= (1ull << 32) || tb >= (1ull << 31);
    if (err) {
        g_errors++;
        CHECK(want_17 || want_large);
        CHECK(!strcmp(err, want_17 ? "a 17-bit window needs a precomputed table" : "batch * len * windows too large for one launch"));
        return;
    }
    CHECK(!want_17 && !want_large);
    const MsmGeom& g = p.g;
    CHECK(g.n == len && g.table_n == sh.table_n && g.c == c && g.W == W && g.nb == nb && g.G == G && g.batch == batch && g.L0 == 0);
    CHECK(p.total_groups == tg && p.total_buckets == tb && p.Mmax == Mmax);
    CHECK(Mmax < (1ull << 32) && tb < (1ull << 31));
    if (msm_table_fits(sh.table_n, sh.W)) CHECK((u64)sh.table_n * W < (1ull << 30));
    const u64 sub = c - 1 < 8 ? c - 1 : (c >= 17 ? 9 : 8), P = nb >> sub;
    CHECK(p.P == P);

    // the sort
    CHECK(g.slices >= 1);
    CHECK(g.wb >= 1 && g.wb <= W);
    const u64 windows_per_block = G == 1 ? W : g.wb;
    if (p.pack16) CHECK(ceil_div(len, g.slices) * windows_per_block <= 65535);
    if (4 * nb > 128 * 1024) CHECK(p.pack16);
    CHECK(p.lds_hist == nb * (p.pack16 ? 2 : 4) * (G == 1 ? 1 : g.wb));
    CHECK(p.lds_hist <= 128 * 1024);
    CHECK(p.lds_part <= 160 * 1024);
    CHECK(p.part_lists == 128 || p.part_lists == 256);
    CHECK((G == 1 ? P : g.wb * P) <= p.part_lists);
    CHECK(p.lds_part == 4 * (u64)p.part_lists + (u64)(p.part_threads / 64) * (16 * (u64)p.part_lists + 512 * 8 + 512 * 2));
    const u32 sort_threads = tu.sort_block == 512 ? 512 : 1024;
    CHECK(p.hist_threads == sort_threads && p.part_threads == sort_threads);
    CHECK(p.sort_grid[0] == g.slices && p.sort_grid[2] == batch);
    CHECK((u64)p.sort_grid[1] * windows_per_block >= G && (G == 1 ? p.sort_grid[1] == 1 : (u64)(p.sort_grid[1] - 1) * g.wb < G));
    CHECK(p.cs_a == ceil_div(tb, 256) && p.cs_b == ceil_div(tg * P, 256));
    CHECK(p.bslices == 1 || p.bslices == 2 || p.bslices == 4);
    CHECK(P * ceil_div(g.slices, p.bslices) * tg == (u64)p.bucket_grid[0] * p.bucket_grid[1]);
    CHECK(p.bucket_grid[1] == tg && p.bucket_threads == 256);

    // the accumulation: the lanes and records the device can ask for are there
    const u64 lcap = (u64)tu.acc_points, resident = (u64)tu.num_cus * 4 * (lcap ? 1 : (u64)tu.acc_waves) * 64, lmax = 64 * 4 / (u64)tu.acc_waves;
    CHECK(p.lcap == lcap && p.kmin == (u32)tu.acc_min_layers && p.resident == resident && p.lmax == lmax);
    CHECK(p.acc_block == (u32)tu.acc_block);
    CHECK(p.acc_grid == ceil_div(p.lanes_max, p.acc_block));
    CHECK(p.nt0_max == p.lanes_max + tb);
    const u64 Ms[4] = {1, std::max<u64>(1, Mmax / 7), std::max<u64>(1, Mmax / 2), Mmax};
    for (u64 M : Ms) {
        const u64 L = device_L(M, resident, lmax, lcap, (u64)tu.acc_min_layers);
        CHECK(L >= 4);
        CHECK(ceil_div(M, L) <= (u64)p.acc_grid * p.acc_block);
        CHECK(ceil_div(M, L) + tb <= p.nt0_max);
    }
    u64 lanes_max;      // (the host's bound, restated for the closed forms below)
    if (lcap) {
        u64 k = 4;
        while (Mmax > k * resident * lcap) k += 2;
        lanes_max = k * resident + p.acc_block;
    } else lanes_max = std::max<u64>(1, ceil_div(Mmax, resident * lmax)) * resident + p.acc_block;
    CHECK(p.lanes_max == lanes_max);
    const u64 nt0 = lanes_max + tb;

    // merge and bucket reduction
    CHECK(p.merge_cap == std::max<u64>(std::min<u64>(tb, nt0 / 2 + 1), 4 * (nt0 / 512 + 2)));
    CHECK(p.bred_bb == 128 || p.bred_bb == 256);
    CHECK(p.nblk <= 16 * 16);
    CHECK((u64)p.nblk * p.bred_bb == std::max<u64>(p.bred_bb, nb));
    if (!tu.bred_block) CHECK(p.bred_bb == (nb <= 8192 ? 128u : 256u));

    // every buffer: the closed form of its size
    g_what = "workspace";
    const u64 REC = 144;
    const size_t* ws = p.ws_bytes;
    CHECK(ws[MSM_WS_COUNT] == tb * 4);
    CHECK(ws[MSM_WS_COUNTERS] == 64);
    CHECK(ws[MSM_WS_BHIST] == tb * g.slices * 6);
    CHECK(ws[MSM_WS_PCOUNT] == tg * g.slices * P * 4);
    CHECK(ws[MSM_WS_PAIRS] == Mmax * 8);
    CHECK(ws[MSM_WS_OFF] == (tb + 1) * 4);
    CHECK(ws[MSM_WS_RECORDS] == (tb + 1) * 12);
    CHECK(ws[MSM_WS_MERGE_PARTS] == (2 * (nt0 / 512) + 4) * REC);
    CHECK(ws[MSM_WS_MERGE_LISTS] == (u64)p.merge_cap * 8 * 4);
    CHECK(ws[MSM_WS_IDX] == Mmax * 4);
    CHECK(ws[MSM_WS_PARTIAL0] == nt0 * REC);
    CHECK(ws[MSM_WS_BUCKETS] == tb * REC);
    CHECK(ws[MSM_WS_CONTRIB] == tg * std::max<u64>(1, nb / 128) * 17 * REC);
    CHECK(ws[MSM_WS_TREE] == tg * 16 * 17 * REC);
    CHECK(ws[MSM_WS_BRED_CNT] == tg * 32 * 4);
    CHECK(ws[MSM_WS_GSUMS] == tg * REC);
    CHECK(ws[MSM_WS_BSUM] == ceil_div(tb, 256) * 2 * 4);
    // what the kernels index: k_msm_hist's packed counts sit behind the u32 prefixes; a first-level k_msm_bred block per node vector
    CHECK(ws[MSM_WS_BHIST] >= tb * g.slices * 4 + (p.pack16 ? tb * g.slices * 2 : 0));
    CHECK(ws[MSM_WS_CONTRIB] >= tg * p.nblk * 17 * REC);
}

void check_windows() {
    g_what = "window rules";
    static const u32 pre[27] = {6, 6, 6, 6, 6, 6, 7, 8, 9, 10, 13, 13, 13, 13, 13, 13, 13, 15, 15, 16, 17, 17, 17, 17, 17, 17, 17};
    static const u32 single[27] = {6, 6, 6, 6, 6, 6, 7, 8, 9, 10, 13, 13, 10, 10, 10, 10, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13};
    for (u32 l = 0; l <= 26; l++) {
        const size_t top = (size_t)1 << l, low = l ? (top >> 1) + 1 : 1;      // the largest and the smallest n with log2_ceil(n) == l
        CHECK(log2_ceil(top) == l && log2_ceil(low) == l);
        CHECK(choose_window(top) == pre[l] && choose_window(low) == pre[l]);
        CHECK(choose_window_single(top) == single[l] && choose_window_single(low) == single[l]);
    }
    CHECK(choose_window(0) == 6 && choose_window_single(0) == 6);
    CHECK(signed_windows(Bn254Fr::P, 15) == 17);
    CHECK(signed_windows(PastaFq::P, 17) == 15);
    CHECK(msm_table_fits((1u << 30) / 15 - 1, 15) && !msm_table_fits((1u << 30) / 16, 16) && msm_table_fits((1u << 30) / 16 - 1, 16) && !msm_table_fits(1u << 30, 1));
}

}  // namespace

int main() {
    check_windows();

    // the distinct window counts of each c over the three scalar fields
    std::vector<u32> Ws[18];
    for (u32 c = 4; c <= 17; c++)
        for (const uint32_t* r : {Bn254Fr::P, PastaFq::P, PastaFp::P}) {
            const u32 W = signed_windows(r, c);
            if (W < (254 + c - 1) / c || W > (256 + c - 1) / c) { fprintf(stderr, "msm_plan_check: signed_windows(c = %u) = %u\n", c, W); return 1; }
            if (std::find(Ws[c].begin(), Ws[c].end(), W) == Ws[c].end()) Ws[c].push_back(W);
        }

    std::vector<MsmTuning> acc;      // the 48 accumulation tunings
    for (int block : {128, 768})
        for (int points : {0, 48})
            for (int waves = 1; waves <= 4; waves++)
                for (int layers = 2; layers <= 4; layers++) {
                    MsmTuning t;
                    t.num_cus = 256; t.acc_block = block; t.acc_points = points; t.acc_waves = waves; t.acc_min_layers = layers;
                    acc.push_back(t);
                }
    std::vector<size_t> edges;
    for (u32 k = 17; k <= 22; k++)
        for (long d : {0l, 1l, -1l, 3l, -3l, 4369l, -4369l}) edges.push_back((size_t)(((long)1 << k) + d));
    static const size_t batches[8] = {1, 2, 3, 4, 7, 12, 16, 64};

    auto sweep = [&](size_t len, bool every_tuning) {
        for (u32 bi = 0; bi < 8; bi++)
            for (int precomp = 0; precomp < 2; precomp++)
                for (u32 c = 4; c <= 17; c++)
                    for (u32 W : Ws[c])
                        for (int sort_block : {512, 1024}) {
                            const MsmShape sh{len, batches[bi], len, c, W, precomp != 0};
                            const size_t first = every_tuning ? 0 : (len + bi + c) % acc.size(), last = every_tuning ? acc.size() : first + 1;
                            for (size_t a = first; a < last; a++) {
                                MsmTuning t = acc[a];
                                t.sort_block = sort_block;
                                check_shape(sh, t);
                            }
                        }
    };
    for (size_t len = 1; len <= ((size_t)1 << 17); len++) sweep(len, false);
    for (size_t len : edges) sweep(len, true);

    // DEHALO_MSM_BRED_BLOCK (measurement builds): honoured while the first level's blocks fit the cluster counters, ignored at 2^16 buckets x 128
    for (u32 block : {128u, 256u})
        for (u32 c = 4; c <= 17; c++)
            for (size_t len : {(size_t)1 << 11, (size_t)1 << 20}) {
                MsmTuning t;
                t.bred_block = block;
                check_shape(MsmShape{len, 1, len, c, signed_windows(PastaFq::P, c), true}, t);
                MsmPlan p;
                if (msm_plan(g_sh, t, &p)) return 1;
                g_what = "bred_block";
                CHECK(p.bred_bb == (c == 17 && block == 128 ? 256u : block));
            }

    printf("msm_plan_check: %llu plans (%llu refused), all invariants hold\n", (unsigned long long)g_plans, (unsigned long long)g_errors);
    return 0;
}
