// prover.hip -- create_proof behind the C ABI (KZG / GWC or SHPLONK, and IPA) [UPSTREAM halo2_proofs @ v2023_04_20: plonk/prover.rs,
// plonk/{lookup,permutation,vanishing}/prover.rs, poly/kzg/multiopen/{gwc,shplonk}/prover.rs, poly/ipa/multiopen/prover.rs] -- the call the reference makes at
// benches/delay_enc.rs:120-134 (create_proof into a Blake2bWrite transcript).  dehalo_prover: what outlives a proof; ProofRun: one proof, a function per phase.
//
// Every C entry point runs its body under dh_guard (guard.hpp): an exception leaves as DEHALO_ERR_OOM (std::bad_alloc) or DEHALO_ERR_INVALID, never as an exception.
// Host logic only: it orders the phases, hashes the transcript and does O(1) field arithmetic per challenge (hostfield.hpp); every column
// operation is one of this library's device entry points (include/dehalo.h), called directly.  No CPU path for column work exists.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <thread>
#include <unordered_map>

#include "opening_plan.hpp"
#include "whole_call.hpp"

namespace {

using clk = std::chrono::steady_clock;
inline double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

// the blinding rows of a phase's columns: column c gets `rows` elements at dst + c * dst_pitch from src + c * rows (a 2-D device copy through the
// runtime took 10-45 us for these few hundred bytes on the proving thread's stream, right before the phase's commitment)
__global__ void k_place_rows(fe* __restrict__ dst, uint64_t dst_pitch, const fe* __restrict__ src, uint32_t rows, uint32_t ncols) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows * ncols) dst[(uint64_t)(i / rows) * dst_pitch + i % rows] = src[i];
}

// status[i] = "shuffle product i does not come back to 1 at row u" for the `count` products of `circuits` circuits: circuit c's `per` products start
// circuit_pitch elements behind circuit c - 1's, a product's column is n elements long.  `one`: 1 in the columns' (standard Montgomery) form
__global__ void k_shuffle_closed(const fe* __restrict__ z, uint64_t circuit_pitch, uint64_t n, uint64_t u, uint32_t per, uint32_t count, fe one, int32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint64_t* v = (const uint64_t*)&z[(uint64_t)(i / per) * circuit_pitch + (uint64_t)(i % per) * n + u];
    const uint64_t* o = (const uint64_t*)&one;
    status[i] = (v[0] != o[0]) | (v[1] != o[1]) | (v[2] != o[2]) | (v[3] != o[3]);
}

const uint64_t* col_ptr(const DevMem& mem, size_t col, size_t len) { return (const uint64_t*)mem.at(col * len); }

}   // namespace

// ================================================================================================ create_proof
struct dehalo_prover {
    dehalo_ctx *ctx = nullptr, *side = nullptr;
    const dehalo_params* params = nullptr;
    const dehalo_pk* pk = nullptr;
    const HostField* f = nullptr;
    size_t n = 0, m = 0, u = 0;
    uint32_t k = 0, ek = 0, bf = 0, A = 0, L = 0, S = 0, H = 0, I = 0, pieces = 0;      // H: shuffle arguments
    // circuits proven in one proof [UPSTREAM create_proof's `circuits: &[ConcreteCircuit]`]: N witnesses of the one key.  Every per-circuit buffer below holds
    // circuit 0's columns, then circuit 1's ... (the plan's layout for `cols`), so a commitment phase of all circuits is one run of columns and one MSM launch
    uint32_t N = 1;
    // advice phases [UPSTREAM plonk/prover.rs `for current_phase in phases`]: a phase's columns are committed together, so they sit side by side in `cols` --
    // column c in slot adv_slot[c], phase ph's columns (phase_cols[ph], ascending) in slots [phase_first[ph], phase_first[ph] + phase_cols[ph].size()).  With one
    // phase a column is its own slot
    uint32_t nph = 1, NCH = 0, phase_first[3] = {};
    std::vector<uint32_t> adv_slot, phase_cols[3];
    DevMem cols, polys_own, instance, instance_values, compressed, num, den, ext, h, table_value, shuffle_value, hfold, qbuf, wbuf, jac, evals, blind_dev, omega_col;
    fe* polys = nullptr;      // coefficient forms: polys_own with a side context, cols (in place) without
    std::vector<uint32_t> table_rep;      // per lookup: the first lookup with the same table expressions (shares its compressed table)
    // tables of fixed columns as distinct rows (lookup_permute.hip): per representative lookup one row index per distinct tuple of its table expressions' values over
    // the usable rows and the tuple's multiplicity, on the device; count 0: not such a table, or more distinct rows than the permutation's one-tile path takes
    struct TableRows { DevArray<uint32_t> d_rep, d_mult; uint32_t count = 0; };
    // which value goes where in the evaluations and the multiopen (opening_plan.hpp: depends on the circuit only), with the column and blind layouts; plist: the
    // device pointers in the plan's polynomial order, the folded h (plan.p_hfold, the last one) resolved to hfold
    OpeningPlan plan;
    std::vector<const uint64_t*> plist;
    // ---- ProverIPA (params of DEHALO_SCHEME_IPA) ----
    // One blind per commitment, in one device array laid out by the plan (bi_*).  Everything up to the pieces is drawn before the first launch and uploaded with the
    // blinding rows; the folded h's blind exists on the host only.
    bool ipa = false;
    DevMem ipa_blinds, ipa_q, ipa_wa, ipa_wb, ipa_f, ipa_p;
    const fe* blind_at(uint32_t i) const { return ipa ? ipa_blinds.at(i) : nullptr; }
    // ---- ProverSHPLONK (dehalo_prover_set_multiopen; KZG only): per set its folded polynomial F_i and its quotient Q_i, then h and L; allocated at the first switch
    int multiopen = DEHALO_MULTIOPEN_GWC;
    DevMem shp_f, shp_q, shp_h, shp_l;
    // host staging
    std::vector<uint64_t> blind_host, host_aff, host_jac, host_evals;
    double timings[8] = {};
    // single-proof sharding (dehalo_prover_set_shard): this process computes columns [count * rank / world, count * (rank + 1) / world) of every multi-column
    // commitment and exchanges the points through the caller's all-gather
    uint32_t shard_rank = 0, shard_world = 1;
    dehalo_gather_fn shard_gather = nullptr;
    void* shard_user = nullptr;
    bool trace = false;      // DEHALO_PROVER_TRACE=1: host timestamps inside the phases go to stderr after each proof
    std::vector<std::pair<const char*, double>> ticks;
    clk::time_point t0;
    void tk(const char* label) { if (trace) ticks.push_back({label, ms_since(t0)}); }
    std::mutex mu;      // one create_proof at a time per prover

    // Everything that is not plain device memory comes last and is declared in the reverse of the order it is released in: members are destroyed bottom-up, so the
    // events go first, then the page-locked buffers, the helper's stream, the tables' rows and the arrays above.
    std::vector<TableRows> table_rows;
    Stream hs;                     // a hipStreamSynchronize on the side stream holds that stream against the proving thread's launches (0.4 ms of the lookups' phase):
    Event ev_helper;               // the helper thread's upload runs on a stream of its own beside it, and the helper waits for ITS upload through this event
    Pinned<uint64_t> adv_pin;      // dehalo_create_proof_circuit: the advice columns the witness generator writes (page-locked, kept across proofs)
    Pinned<uint64_t> rand_pin;     // host-drawn random polynomial (page-locked: its upload is one DMA that holds no stream)
    Event ev_side, ev_inst, ev_ready[3];      // ev_ready: one per commitment phase

    int init(dehalo_ctx* c, dehalo_ctx* s, const dehalo_params* pa, const dehalo_pk* key, uint32_t num_circuits) {
        ctx = c; side = s; params = pa; pk = key; f = key->f;
        ipa = pa->scheme == DEHALO_SCHEME_IPA;
        N = num_circuits;
        if (N > 1 && ipa) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "prover_create_multi: several circuits in one proof under ParamsKZG only");
        if (N > 1 && key->cs.num_phases > 1) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "prover_create_multi: the key has later-phase advice columns");
        const HostCS& cs = pk->cs;
        const HostDomain& d = pk->dom;
        n = d.n; m = d.m; k = d.k; ek = d.extended_k;
        bf = cs.blinding_factors();
        u = n - (bf + 1);
        A = cs.num_advice; L = (uint32_t)cs.lookups.size(); S = cs.num_sets(); H = (uint32_t)cs.shuffles.size(); I = cs.num_instance;
        pieces = d.quotient_poly_degree;
        nph = cs.num_phases; NCH = (uint32_t)cs.challenge_phase.size();
        adv_slot.assign(A, 0);
        for (uint32_t ph = 0, slot = 0; ph < nph; ph++) {
            phase_cols[ph].clear();
            phase_first[ph] = slot;
            for (uint32_t c = 0; c < A; c++)
                if (cs.advice_phase[c] == ph) { phase_cols[ph].push_back(c); adv_slot[c] = slot++; }
        }
        if ((size_t)pieces * n > m) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "quotient does not fit the extended domain");
        OpeningShape sh;      // (the plan before anything is allocated: it is host work, and a circuit it refuses costs nothing)
        sh.k = k; sh.A = A; sh.num_fixed = cs.num_fixed; sh.I = I; sh.L = L; sh.S = S; sh.npc = (uint32_t)cs.perm_cols.size(); sh.bf = bf; sh.pieces = pieces;
        sh.query_instance = ipa;
        sh.circuits = N;
        sh.shuffles = H;
        for (auto& q : cs.advice_q) sh.advice_q.push_back({q.index, q.rotation});
        for (auto& q : cs.fixed_q) sh.fixed_q.push_back({q.index, q.rotation});
        for (auto& q : cs.instance_q) sh.instance_q.push_back({q.index, q.rotation});
        plan = OpeningPlan(sh);
        if (!plan.error.empty()) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, plan.error);
        const uint32_t NC = plan.NC;
        if (ipa) TRY(ipa_blinds.alloc(ctx, plan.bi_count));
        TRY(cols.alloc(ctx, (size_t)NC * n));
        if (side) TRY(polys_own.alloc(ctx, (size_t)NC * n));
        polys = side ? polys_own.p : cols.p;
        TRY(instance.alloc(ctx, (size_t)std::max<uint32_t>(N * I, 1) * n));
        TRY(instance_values.alloc(ctx, (size_t)std::max<uint32_t>(N * I, 1) * n));
        TRY(compressed.alloc(ctx, (size_t)std::max<uint32_t>(N * 2 * L, 1) * n));
        TRY(num.alloc(ctx, (size_t)std::max<uint32_t>(N * (S + L + H), 1) * n));
        TRY(den.alloc(ctx, (size_t)std::max<uint32_t>(N * (S + L + H), 1) * n));
        TRY(ext.alloc(ctx, (size_t)(NC - 1 + N * I) * m));
        TRY(h.alloc(ctx, m));
        TRY(table_value.alloc(ctx, (size_t)std::max<uint32_t>(N * L, 1) * m));
        if (H) TRY(shuffle_value.alloc(ctx, (size_t)N * 2 * H * m));      // per circuit and shuffle: compressed input + gamma, compressed shuffle side + gamma
        TRY(hfold.alloc(ctx, n));
        // blinding values of a proof but the random polynomial, compacted: [advice rows | permuted rows | product rows]
        const size_t rows = n - u;
        TRY(blind_dev.alloc(ctx, std::max<size_t>(1, (size_t)N * ((size_t)A * rows + (size_t)2 * L * rows + (size_t)(S + L + H) * bf))));
        TRY(omega_col.alloc(ctx, n, false));
        TRY(omega_powers(ctx, d, omega_col.p));
        table_rep.clear();
        for (uint32_t l = 0; l < L; l++) table_rep.push_back(cs.table_representative(l));
        TRY(find_table_rows());
        plist.clear();
        for (uint32_t c = 0; c < NC; c++) {
            const uint32_t at = c >= plan.o_adv && c < plan.o_adv + A ? plan.o_adv + adv_slot[c - plan.o_adv] : c;
            plist.push_back((const uint64_t*)(polys + (size_t)at * n));
        }
        for (uint32_t c = 0; c < cs.num_fixed; c++) plist.push_back(col_ptr(pk->fixed_polys, c, n));
        for (uint32_t c = 0; c < sh.npc; c++) plist.push_back(col_ptr(pk->perm_polys, c, n));
        for (uint32_t i = 0; i < pieces; i++) plist.push_back((const uint64_t*)h.at(i * n));
        if (ipa) for (uint32_t c = 0; c < I; c++) plist.push_back(col_ptr(instance, c, n));      // opened under IPA only
        plist.push_back(hfold.u64());      // plan.p_hfold
        // GWC: one folded polynomial and one witness per opening point (at least the four every circuit has)
        const size_t ngroups = std::max<size_t>(4, plan.groups.size());
        TRY(qbuf.alloc(ctx, ngroups * n));
        TRY(wbuf.alloc(ctx, ngroups * n));
        const uint32_t maxpts = std::max<uint32_t>(std::max<uint32_t>(NC, (uint32_t)std::max<size_t>(8, plan.groups.size())), std::max<uint32_t>(I, pieces));      // the most points one phase commits
        TRY(jac.alloc(ctx, 3 * (size_t)maxpts + 2 + ((size_t)N * std::max(L, H) + 7) / 8));      // + the lookups' / shuffles' status flags behind a phase's points (one int32 each)
        if (ipa) {      // the multiopen's buffers, sized from the constraint system: one polynomial per point set, twice more for the division chain
            const size_t ns = plan.point_sets.size();
            TRY(ipa_q.alloc(ctx, ns * n));
            TRY(ipa_wa.alloc(ctx, ns * n));
            TRY(ipa_wb.alloc(ctx, ns * n));
            TRY(ipa_f.alloc(ctx, n));
            TRY(ipa_p.alloc(ctx, n));
            TRY(evals.alloc(ctx, plan.eval_count + 8 + ns));
        } else
        TRY(evals.alloc(ctx, plan.eval_count + 8));
        for (Event* e : {&ev_ready[0], &ev_ready[1], &ev_ready[2], &ev_inst, &ev_side, &ev_helper}) HIP_TRY(ctx, make_event(*e, hipEventDisableTiming));
        HIP_TRY(ctx, make_pinned(rand_pin, (size_t)n * 32));
        if (side) HIP_TRY(ctx, make_stream(hs, hipStreamNonBlocking));
        host_aff.resize(8 * (size_t)maxpts);
        host_jac.resize(12 * (size_t)maxpts + 8 + (size_t)N * std::max(L, H));
        host_evals.resize(4 * plan.eval_count);
        TRY(dehalo_ctx_synchronize(ctx));
        return 0;
    }

    // Which rows of a lookup table are equal does not depend on theta when its expressions read fixed columns only: evaluate them once, on the host, over the usable
    // rows and keep one representative row per distinct tuple + its multiplicity (the delay-encryption circuit's (tag, value) range table: 339 tuples in 131,066 rows).
    Fe eval_fixed_expr(uint32_t node, size_t row, const std::vector<std::vector<Fe>>& colv) const {
        const HostCS& cs = pk->cs;
        const dehalo_expr_node& e = cs.nodes[node];
        switch (e.kind) {
            case DEHALO_EXPR_CONSTANT: return cs.constants[e.a];
            case DEHALO_EXPR_FIXED: return colv[e.a][(size_t)(((int64_t)row + e.rotation) % (int64_t)n + (int64_t)n) % n];
            case DEHALO_EXPR_ADVICE: case DEHALO_EXPR_INSTANCE: case DEHALO_EXPR_CHALLENGE: return Fe{{0, 0, 0, 0}};      // (not reached: expr_fixed_only is false for them)
            case DEHALO_EXPR_NEGATED: return f->neg(eval_fixed_expr(e.a, row, colv));
            case DEHALO_EXPR_SCALED: return f->mul(eval_fixed_expr(e.a, row, colv), cs.constants[e.b]);
            case DEHALO_EXPR_SUM: return f->add(eval_fixed_expr(e.a, row, colv), eval_fixed_expr(e.b, row, colv));
            default: return f->mul(eval_fixed_expr(e.a, row, colv), eval_fixed_expr(e.b, row, colv));
        }
    }
    int find_table_rows() {
        const HostCS& cs = pk->cs;
        table_rows = std::vector<TableRows>(L);
        static const bool enabled = [] { const char* e = DH_EXPERIMENT_ENV("DEHALO_PROVER_TABLE_ROWS"); return !(e && e[0] == '0'); }();      // (0: every table sorted in full, for the A/B)
        if (!enabled) return 0;
        std::vector<std::vector<Fe>> colv(cs.num_fixed);
        for (uint32_t l = 0; l < L; l++) {
            if (table_rep[l] != l) continue;
            bool fixed_only = true;
            std::vector<uint32_t> need;
            for (uint32_t e : cs.lookups[l].tables) { fixed_only = fixed_only && cs.expr_fixed_only(e); cs.expr_fixed_columns(e, need); }
            if (!fixed_only) continue;
            for (uint32_t c : need)
                if (colv[c].empty()) {
                    colv[c].resize(n);
                    TRY(dehalo_download(ctx, pk->fixed_values.at((size_t)c * n), n * 32, colv[c].data()));
                }
            const size_t T = cs.lookups[l].tables.size();
            struct Key { std::vector<uint64_t> w; bool operator==(const Key& o) const { return w == o.w; } };
            struct Hash { size_t operator()(const Key& k) const { uint64_t h = 0x9e3779b97f4a7c15ull; for (uint64_t x : k.w) { h ^= x + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2); } return (size_t)h; } };
            std::unordered_map<Key, uint32_t, Hash> seen;
            std::vector<uint32_t> rep, mult;
            bool too_many = false;
            Key key;
            key.w.resize(4 * T);
            for (size_t i = 0; i < u && !too_many; i++) {
                for (size_t t = 0; t < T; t++) {
                    const Fe v = eval_fixed_expr(cs.lookups[l].tables[t], i, colv);
                    memcpy(&key.w[4 * t], v.v, 32);
                }
                auto it = seen.find(key);
                if (it != seen.end()) mult[it->second]++;
                else if (rep.size() == 2048) too_many = true;
                else { seen.emplace(key, (uint32_t)rep.size()); rep.push_back((uint32_t)i); mult.push_back(1); }
            }
            if (too_many || rep.empty()) continue;
            TableRows& tr = table_rows[l];
            TRY(tr.d_rep.alloc(ctx, rep.size(), false));
            TRY(tr.d_mult.alloc(ctx, rep.size(), false));
            TRY(dehalo_upload(ctx, rep.data(), rep.size() * 4, tr.d_rep.p));
            TRY(dehalo_upload(ctx, mult.data(), mult.size() * 4, tr.d_mult.p));
            tr.count = (uint32_t)rep.size();
        }
        return 0;
    }

    // Jacobian {x, y, z} (Montgomery, base field) -> affine on the HOST: one inversion per phase (HostField::batch_invert; a dozen field
    // multiplications per point, one exponentiation per call: ~15 us) instead of a 12 k-instruction safegcd chain on ONE lane of the MSM's last
    // kernel in front of every read-back (~50 us of device latency per commitment phase, six phases per proof).  false: a point at infinity.
    bool normalize_host(const uint64_t* jac, size_t count, uint64_t* affine_out) const {
        const HostField* fq = host_field(curve_base_field(pk->curve));
        std::vector<Fe> zinv(count);
        for (size_t i = 0; i < count; i++) memcpy(zinv[i].v, jac + 12 * i + 8, 32);
        if (!fq->batch_invert(zinv.data(), count)) return false;
        for (size_t i = 0; i < count; i++) {
            const Fe zi2 = fq->sqr(zinv[i]), zi3 = fq->mul(zi2, zinv[i]);
            Fe x, y;
            memcpy(x.v, jac + 12 * i, 32);
            memcpy(y.v, jac + 12 * i + 4, 32);
            x = fq->mul(x, zi2);
            y = fq->mul(y, zi3);
            memcpy(affine_out + 8 * i, x.v, 32);
            memcpy(affine_out + 8 * i + 4, y.v, 32);
        }
        return true;
    }

    // commit `count` columns starting at `src`, read back, normalise, absorb (and append to the proof)
    // `flags` > 0: that many int32 status words sit behind the points in `jac` (deferred lookup permutation; `shuffle_flags`: the shuffle products' closing
    // test) and come back with them; any non-zero one fails the call
    // `d_blinds` (ParamsIPA; null under KZG): one blind per column on the device -- [blind] W joins each point on the stream, behind the MSM, in one launch
    // `to_proof` false: absorbed only (common_point: the instance commitments)
    // `order` (null: column order): the i-th point written is column order[i]'s -- several circuits' products sit circuit by circuit and are written kind by kind
    int commit(dehalo_transcript* tr, const fe* src, size_t count, bool lagrange, const std::function<int()>& before_sync = nullptr, size_t flags = 0,
               const fe* d_blinds = nullptr, bool to_proof = true, const uint32_t* order = nullptr, bool shuffle_flags = false) {
        // sharded (dehalo_prover_set_shard): this process's share of the columns only; everything else of the proof is computed by every process
        const bool sharded = shard_world > 1 && shard_gather && count > 1;
        const size_t lo = sharded ? count * shard_rank / shard_world : 0, hi = sharded ? count * (shard_rank + 1) / shard_world : count;
        if (hi > lo)
            TRY(dehalo_msm_device(ctx, (lagrange ? params->bases_gl : params->bases_g).get(), (const uint64_t*)(src + lo * n), n, hi - lo, jac.u64() + 12 * lo, nullptr));
        if (ipa && !d_blinds) return dh_fail(ctx, DEHALO_ERR_INVALID, "commit: a ParamsIPA commitment without its blind");
        if (ipa && hi > lo)
            TRY(dehalo_fixed_base_blind_device(ctx, params->fb_w.get(), jac.u64() + 12 * lo, (const uint64_t*)(d_blinds + lo), hi - lo, nullptr));
        tk("commit queued");
        if (before_sync) TRY(before_sync());
        tk("side work queued");
        TRY(dehalo_download(ctx, jac.p, count * 96 + flags * 4, host_jac.data()));
        tk("points on host");
        for (size_t i = 0; i < flags; i++)
            if (!reinterpret_cast<const int32_t*>(host_jac.data() + 12 * count)[i]) continue;
            else if (shuffle_flags)
                return dh_fail(ctx, DEHALO_ERR_SHUFFLE, "shuffle " + std::to_string(i % H) + (N > 1 ? " of circuit " + std::to_string(i / H) : std::string()) +
                                                            ": its input and shuffle expressions are not a permutation of each other over the usable rows (the product does not end at 1)");
            else
                return dh_fail(ctx, DEHALO_ERR_NOT_IN_TABLE, "permute_expression_pair: an input value of lookup " + std::to_string(i % L) + (N > 1 ? " of circuit " + std::to_string(i / L) : std::string()) +
                                                                 " is not in the table (ConstraintSystemFailure)");
        if (hi > lo && !normalize_host(host_jac.data() + 12 * lo, hi - lo, host_aff.data() + 8 * lo)) return dh_fail(ctx, DEHALO_ERR_INVALID, "cannot write points at infinity to the transcript");
        if (sharded) {      // every process ends with all `count` affine points, in column order
            std::vector<uint32_t> first(shard_world), num(shard_world);
            for (uint32_t r = 0; r < shard_world; r++) {
                first[r] = (uint32_t)(count * r / shard_world);
                num[r] = (uint32_t)(count * (r + 1) / shard_world) - first[r];
            }
            if (shard_gather(shard_user, host_aff.data(), (uint32_t)count, first.data(), num.data(), shard_world) != 0)
                return dh_fail(ctx, DEHALO_ERR_INVALID, "the shard gather callback failed");
            tk("points gathered");
        }
        for (size_t i = 0; i < count; i++)
            if (!tr->write_point(host_aff.data() + 8 * (order ? order[i] : i), to_proof)) return dh_fail(ctx, DEHALO_ERR_INVALID, "cannot write points at infinity to the transcript");
        return 0;
    }

    // the SHPLONK multiopen's buffers, sized from the plan: one folded polynomial and one quotient per point set, h, L
    int alloc_shplonk() {
        if (shp_l.p) return 0;      // (the last one allocated)
        const size_t ns = plan.point_sets.size();
        TRY(shp_f.alloc(ctx, ns * n));
        TRY(shp_q.alloc(ctx, ns * n));
        TRY(shp_h.alloc(ctx, n));
        TRY(shp_l.alloc(ctx, n));
        return dehalo_ctx_synchronize(ctx);
    }

    size_t proof_size() const { return plan.proof_size(ipa ? OpeningPlan::IPA : multiopen == DEHALO_MULTIOPEN_SHPLONK ? OpeningPlan::SHPLONK : OpeningPlan::GWC); }
};

namespace {

struct EvalIn {      // dehalo_eval_inputs with owned scalar storage
    dehalo_eval_inputs in{};
    void cols(const std::vector<const uint64_t*>& fixed, const std::vector<const uint64_t*>& advice, const std::vector<const uint64_t*>& instance) {
        in.fixed = fixed.data(); in.num_fixed = (uint32_t)fixed.size();
        in.advice = advice.data(); in.num_advice = (uint32_t)advice.size();
        in.instance = instance.data(); in.num_instance = (uint32_t)instance.size();
    }
};

constexpr uint32_t FF = DEHALO_EVAL_COLUMNS_INTERNAL | DEHALO_EVAL_VALUES_INTERNAL;
const Fe zero{{0, 0, 0, 0}};

// 1, c, ..., c^(count - 1), or descending: the coefficients of `count` terms folded as acc <- c acc + term (the multiopen's x_1, x_2, x_4)
std::vector<Fe> powers(const HostField* f, const Fe& c, size_t count, bool descending = false) {
    std::vector<Fe> out(count);
    Fe pw = f->one;
    for (size_t j = 0; j < count; j++) { out[descending ? count - 1 - j : j] = pw; pw = f->mul(pw, c); }
    return out;
}
// sum of coefs[i] terms[i]: a value or a blind folded as its polynomials are
Fe fold(const HostField* f, const Fe* coefs, const Fe* terms, size_t count) {
    Fe acc = zero;
    for (size_t i = 0; i < count; i++) acc = f->add(acc, f->mul(coefs[i], terms[i]));
    return acc;
}

// One create_proof: what lives from the first draw to the last opening.  `p` is the prover (what outlives a proof: buffers, plans, events); the names copied from
// it below are the circuit's shape.  Each phase is one member function, called by run() in upstream's order.
struct ProofRun {
    dehalo_prover& p;
    dehalo_transcript* const tr;
    dehalo_rng* const rng_in;
    dehalo_ctx *const ctx, *const side;
    const hipStream_t ms, ss;
    const HostField* const f;
    const HostCS& cs;
    const HostDomain& d;
    const int fid;
    const size_t n, m, u, rows;
    const uint32_t k, ek, bf, A, L, S, H, I, N, pieces, nco, rot_scale;
    const bool ipa;
    // one gate polynomial: Horner(0, [g], y) = g does not depend on y, so the custom-gate pass of evaluate_h needs the advice (and instance)
    // cosets only -- queued on the side context right behind the last phase's, long before y exists (a circuit with challenges waits for them instead).
    // Of several circuits only the first starts the running value at zero: the others' gate passes multiply by y and wait for it
    const bool gates_early;
    const clk::time_point t_start = clk::now();
    clk::time_point t_phase = t_start;

    HostRng rng, rng_poly;      // the proof's generator; its fork at the random polynomial's position (the helper thread's)
    bool device_rng = false;    // the large draw comes from a ChaCha20 kernel keyed with this proof's entropy
    size_t c_adv = 0, c_advb = 0, c_lk = 0, c_pr = 0;      // how many scalars each group of blinding values draws
    std::vector<Fe> bl;         // the proof's blinds by commitment (dehalo_prover: ipa_blinds)
    std::vector<Fe> bl_slots;   // several phases: the same with the advice blinds in slot order, as the device array holds them
    size_t adv_off[3] = {};     // where a phase's draws start: its columns' blinding rows, then one blind per column
    std::vector<Fe> chal;       // the circuit's challenges by index; zero until squeezed
    dehalo_advice_fn advice_fn = nullptr;      // dehalo_create_proof_phased: the witness of a phase, asked for when its turn comes
    void* advice_user = nullptr;
    std::thread helper;         // draws (and, with a side context, uploads) the random polynomial while the earlier phases run
    std::atomic<int> helper_rc{0};
    double helper_ms[3] = {};
    // a host witness is pinned until this proof ends (every stream has been synchronised by then); one that is page-locked already stays as it is
    std::vector<std::unique_ptr<HostPin>> pin_advice;
    std::vector<const uint64_t*> fixed_v, fixed_c;                                    // pointer tables of the phases: values, cosets;
    std::vector<std::vector<const uint64_t*>> adv_v, inst_v, adv_c, inst_c;           // a circuit's own by circuit
    Fe theta{}, beta{}, gamma{}, y{}, x{}, hfold_eval{};
    std::vector<Fe> point, xs;      // x at every rotation of the plan; x^(n i)
    const Fe* E = nullptr;          // the evaluations on the host, indexed by the opening plan

    ProofRun(dehalo_prover& pv, dehalo_transcript* t, dehalo_rng* r)
        : p(pv), tr(t), rng_in(r), ctx(pv.ctx), side(pv.side), ms(pv.ctx->stream.get()), ss(pv.side ? pv.side->stream.get() : nullptr), f(pv.f), cs(pv.pk->cs), d(pv.pk->dom),
          fid(pv.f->id), n(pv.n), m(pv.m), u(pv.u), rows(pv.n - pv.u), k(pv.k), ek(pv.ek), bf(pv.bf), A(pv.A), L(pv.L), S(pv.S), H(pv.H), I(pv.I), N(pv.N), pieces(pv.pieces), nco(pv.plan.NC - 1),
          rot_scale((uint32_t)(pv.m / pv.n)), ipa(pv.ipa), gates_early(pv.side && pv.pk->cs.gates.size() == 1 && pv.NCH == 0), chal(pv.NCH, Fe{{0, 0, 0, 0}}) {}
    ~ProofRun() {      // whatever path the proof took: the witness' copy (asynchronous) has landed before its pin goes, and the helper has finished
        for (auto& pin : pin_advice)
            if (pin && pin->p) { (void)hipStreamSynchronize(ms); break; }
        pin_advice.clear();
        if (helper.joinable()) helper.join();
    }
    void mark(int slot) {
        const auto now = clk::now();
        p.timings[slot] = std::chrono::duration<double, std::milli>(now - t_phase).count();
        t_phase = now;
    }

    // ---- random scalars, in upstream's order, circuit after circuit within each step (advice: rows then blinds of circuit 0, rows then blinds of circuit 1, ...;
    // the products: every circuit's permutation products, then every circuit's lookup products, then every circuit's shuffle products): per advice phase the blinding rows of its columns (column after column), then one blind per column of it; per lookup (bf + 1 rows
    // permuted input, bf + 1 permuted table, the two columns' blinds), per grand product (bf rows + its blind), the random polynomial (n), its blind,
    // the h pieces' blinds and, under IPA, f's blind.  KZG commitments are not hiding: it draws the blinds and drops them.  No draw depends on the
    // device, so all of them are made here, in that order, and the blinds go up with the blinding rows in one copy.
    int draw_blinds() {
        TRY(rng.init(rng_in, f));
        device_rng = rng.chacha();
        c_adv = (size_t)N * A * rows; c_advb = (size_t)N * A; c_lk = (size_t)N * L * (2 * rows + 2); c_pr = (size_t)N * (S + L + H) * (bf + 1);
        const size_t draws_before = c_adv + c_advb + c_lk + c_pr;
        for (uint32_t ph = 0, off = 0; ph < p.nph; ph++) { adv_off[ph] = off; off += (uint32_t)(p.phase_cols[ph].size() * (rows + 1)); }
        p.blind_host.resize(4 * std::max<size_t>(1, draws_before));
        // the one large draw (n scalars, drawn AFTER every blinding value) is produced and -- with a side context -- uploaded by a helper
        // thread while the earlier phases run
        rng_poly = rng.fork(draws_before, 1);
        TRY(rng.scalars(p.blind_host.data(), draws_before));
        rng.skip(n);                                             // the random polynomial: rng_poly's
        std::vector<Fe> late(1 + (size_t)pieces + (ipa ? 1 : 0));      // random_blind, h_blinds, (IPA) f_blind
        TRY(rng.scalars(late[0].v, late.size()));
        bl.assign(p.plan.bi_count, zero);
        if (ipa) {      // (one circuit)
            const Fe* B = (const Fe*)p.blind_host.data();
            for (uint32_t ph = 0; ph < p.nph; ph++)
                for (size_t j = 0; j < p.phase_cols[ph].size(); j++) bl[p.plan.bi_adv + p.phase_cols[ph][j]] = B[adv_off[ph] + p.phase_cols[ph].size() * rows + j];
            for (uint32_t c = 0; c < 2 * L; c++) bl[p.plan.bi_perm + c] = B[c_adv + c_advb + (size_t)(c / 2) * (2 * rows + 2) + 2 * rows + (c & 1)];
            for (uint32_t s2 = 0; s2 < S + L + H; s2++) bl[p.plan.bi_prod + s2] = B[c_adv + c_advb + c_lk + (size_t)s2 * (bf + 1) + bf];
            bl[p.plan.bi_rand] = late[0];
            for (uint32_t i = 0; i < pieces; i++) bl[p.plan.bi_h + i] = late[1 + i];
            bl[p.plan.bi_f] = late[1 + pieces];
            for (uint32_t i = 0; i < std::max<uint32_t>(I, 1); i++) bl[p.plan.bi_def + i] = f->from_u64(IPA_DEFAULT_BLIND);
            const Fe* up = bl.data();
            if (p.nph > 1) {
                bl_slots = bl;
                for (uint32_t c = 0; c < A; c++) bl_slots[p.plan.bi_adv + p.adv_slot[c]] = bl[p.plan.bi_adv + c];
                up = bl_slots.data();
            }
            TRY(dh_h2d(ctx, p.ipa_blinds.p, up, (size_t)p.plan.bi_count * 32, ctx->stream.get()));      // (waited for with the blinding rows, upload_blinds)
        }
        return 0;
    }

    // The random polynomial's commitment.  Committing COEFFICIENTS over g equals committing their forward transform (the values on the domain) over g_lagrange,
    // and upstream writes the point right behind the grand products' commitments with no challenge in between: so the helper only draws and (with a side
    // context) uploads, and the polynomial rides as ONE MORE COLUMN of the products' MSM launch -- a whole sort / accumulate / merge / reduce pipeline per proof
    // less, and none running beside the lookups' phase.
    void start_random_polynomial() { helper = std::thread([this] { helper_body(); }); }
    void helper_body() {
        (void)hipSetDevice(ctx->device);
        const auto th0 = clk::now();
        int rc = 0;
        if (!device_rng) rc = rng_poly.scalars(p.rand_pin.get(), n);
        helper_ms[0] = ms_since(th0);
        if (!rc && side) {      // (without a side context only the draw is taken off the critical path; the upload is queued by the proving thread)
            fe* dst = p.polys + (size_t)p.plan.o_rand * n;
            hipError_t e = hipSuccess;
            if (device_rng) rc = chacha_scalars_device(ctx, rng_poly, 1, dst, n, p.hs.get());
            else e = hipMemcpyAsync(dst, p.rand_pin.get(), n * 32, hipMemcpyHostToDevice, p.hs.get());
            if (e != hipSuccess) rc = dh_fail(side, DEHALO_ERR_HIP, std::string("random polynomial upload: ") + hipGetErrorString(e));
            helper_ms[1] = ms_since(th0);
            if (!rc) {      // wait for this stream through an event of this thread's own: the coefficients are there before the join
                e = hipEventRecord(p.ev_helper.get(), p.hs.get());
                if (e == hipSuccess) e = hipEventSynchronize(p.ev_helper.get());
                if (e != hipSuccess) rc = dh_fail(side, DEHALO_ERR_HIP, std::string("random polynomial: ") + hipGetErrorString(e));
            }
            helper_ms[2] = ms_since(th0);
        }
        helper_rc.store(rc);
    }

    // create_proof of a CIRCUIT (upstream's call synthesizes inside): the random polynomial's draw and upload start now, on the helper's thread and
    // stream, and run on an otherwise idle device while this thread (and the synthesis pool) writes the advice columns
    int synthesize(const dehalo_circuit_inputs* synth_in, dehalo_synthesis_info* synth_info) {
        if (synth_in->k != k || A != 5) return dh_fail(ctx, DEHALO_ERR_INVALID, "create_proof_circuit: the circuit's k / advice columns differ from the key's");
        if (!p.adv_pin) HIP_TRY(ctx, make_pinned(p.adv_pin, (size_t)A * n * 32));
        start_random_polynomial();
        const int src = dehalo_synthesize(synth_in, p.adv_pin.get(), nullptr, nullptr, nullptr, synth_info);
        if (src) return dh_fail(ctx, src, "create_proof_circuit: the circuit's inputs are invalid or it does not fit 2^k rows");
        p.tk("witness synthesized");
        return 0;
    }

    // compacted blinding rows [advice | permuted | products] -> one upload
    int upload_blinds() {
        const size_t total = (size_t)N * ((size_t)A * rows + (size_t)2 * L * rows + (size_t)(S + L + H) * bf);
        std::vector<uint64_t>& b = p.blind_host;
        std::vector<uint64_t> packed(4 * std::max<size_t>(1, total));
        size_t o = c_adv;
        for (uint32_t c = 0; c < N; c++)      // (a circuit's draws: its columns' rows, then its columns' blinds)
            for (uint32_t ph = 0; ph < p.nph; ph++)      // (slot order is draw order less the blinds between the phases)
                memcpy(packed.data() + 4 * ((size_t)c * A + p.phase_first[ph]) * rows, b.data() + 4 * ((size_t)c * A * (rows + 1) + adv_off[ph]), 32 * p.phase_cols[ph].size() * rows);
        const uint64_t* lk = b.data() + 4 * (c_adv + c_advb);
        for (uint32_t l = 0; l < N * L; l++) {      // (input rows, table rows, two unused blinds) per lookup, circuit after circuit
            memcpy(packed.data() + 4 * o, lk + 4 * (size_t)l * (2 * rows + 2), 32 * 2 * rows);
            o += 2 * rows;
        }
        const uint64_t* pr = b.data() + 4 * (c_adv + c_advb + c_lk);
        for (uint32_t s = 0; s < N * (S + L + H); s++)      // (bf rows, one unused blind) per product, drawn in the order they are written: into its column's place
            memcpy(packed.data() + 4 * (o + (size_t)p.plan.product_order[s] * bf), pr + 4 * (size_t)s * (bf + 1), 32 * bf);
        if (total) TRY(dh_h2d(ctx, p.blind_dev.p, packed.data(), total * 32, ms));
        if (total || ipa) HIP_TRY(ctx, hipStreamSynchronize(ms));      // `packed` is a local (and the blinds' copy of draw_blinds lands here)
        p.tk("blinds drawn and uploaded");
        return 0;
    }

    // ---- instance columns: values into the transcript (KZG: QUERY_INSTANCE = false), polynomials on the device
    int instance_columns(const uint64_t* const* instances, const size_t* instance_lens, uint32_t num_instance_columns) {
        if (num_instance_columns != I) return dh_fail(ctx, DEHALO_ERR_INVALID, "instances.len() != num_instance_columns");      // Error::InvalidInstances
        const uint32_t NI = N * I;      // circuit c's column i is column c * I + i of the arrays and of the buffers
        if (I) HIP_TRY(ctx, hipMemsetAsync(p.instance.p, 0, (size_t)NI * n * 32, ms));
        for (uint32_t i = 0; i < NI; i++) {
            const size_t len = instance_lens ? instance_lens[i] : 0;
            if (len > u) return dh_fail(ctx, DEHALO_ERR_INVALID, "instance column too long");      // Error::InstanceTooLarge
            if (len && (!instances || !instances[i])) return dh_fail(ctx, DEHALO_ERR_INVALID, "null instance column");
            for (size_t j = 0; j < len && !ipa; j++) {
                Fe v;
                memcpy(v.v, instances[i] + 4 * j, 32);
                tr->common_scalar(v);
            }
            if (len) {
                TRY(dh_h2d(ctx, p.instance.at((size_t)i * n), instances[i], len * 32, ms));
                HIP_TRY(ctx, hipStreamSynchronize(ms));
            }
        }
        // IPA (QUERY_INSTANCE = true): commit_lagrange(instance, Blind::default()), absorbed as points
        if (I && ipa) TRY(p.commit(tr, p.instance.p, I, true, nullptr, 0, p.blind_at(p.plan.bi_def), false));
        if (I) HIP_TRY(ctx, hipMemcpyAsync(p.instance_values.p, p.instance.p, (size_t)NI * n * 32, hipMemcpyDeviceToDevice, ms));
        if (I && side) HIP_TRY(ctx, hipEventRecord(p.ev_inst.get(), ms));
        if (I && !side) TRY(dehalo_intt_scaled_device(ctx, fid, p.instance.u64(), k, d.omega_inv.v, d.ifft_divisor.v, NI, nullptr));
        return 0;
    }

    // polys[first..] = lagrange_to_coeff(cols[..]), ext[..] = coeff_to_extended(..) on the side context once `e` (recorded BEFORE the phase's
    // commitment was queued) has passed; the launches themselves are made after the commitment's, while this thread would only wait
    EvalIn coset_inputs(uint32_t c) const {      // every column of circuit c over the extended domain, internal form
        EvalIn e;
        e.cols(fixed_c, adv_c[c], inst_c[c]);
        e.in.form_flags = FF;
        e.in.challenges = (const uint64_t*)chal.data(); e.in.num_challenges = (uint32_t)chal.size();
        return e;
    }
    int side_ntt(uint32_t first, uint32_t count, hipEvent_t e) {
        HIP_TRY(side, hipStreamWaitEvent(ss, e, 0));
        // (out of place: no copy of the columns first -- a 42 MB device-to-device hipMemcpyAsync held this thread for 0.4 ms in the lookups' phase)
        TRY(dehalo_lagrange_to_coeff_device(side, fid, (const uint64_t*)p.cols.at((size_t)first * n), (uint64_t*)(p.polys + (size_t)first * n), k, d.omega_inv.v, d.ifft_divisor.v,
                                            count, nullptr));
        TRY(dehalo_coset_ntt_form_device(side, fid, (const uint64_t*)(p.polys + (size_t)first * n), k, p.ext.u64((size_t)first * m), ek, d.ext_omega.v, d.g_coset.v, count,
                                         DEHALO_FORM_OUT_INTERNAL, nullptr));
        return 0;
    }

    // ---- advice, phase by phase: witness (the caller's, given every challenge squeezed so far), blinding rows, commitments, the phase's challenges
    int advice_of_phase(uint32_t ph, const uint64_t* given, const uint64_t** advice) {
        *advice = given;
        if (!advice_fn) return 0;
        *advice = nullptr;
        const int rc = advice_fn(advice_user, ph, (const uint64_t*)chal.data(), p.NCH, advice);
        if (rc) return dh_fail(ctx, DEHALO_ERR_INVALID, "create_proof_phased: the advice callback returned " + std::to_string(rc) + " in phase " + std::to_string(ph));
        return 0;
    }
    int advice_columns(const uint64_t* const* given, uint32_t flags) {
        for (uint32_t i = 0; i < cs.num_fixed; i++) fixed_v.push_back(col_ptr(p.pk->fixed_values, i, n)), fixed_c.push_back(col_ptr(p.pk->fixed_cosets, i, m));
        adv_v.resize(N); adv_c.resize(N); inst_v.resize(N); inst_c.resize(N);
        for (uint32_t c = 0; c < N; c++) {
            for (uint32_t i = 0; i < A; i++) adv_v[c].push_back(col_ptr(p.cols, p.plan.adv(c) + p.adv_slot[i], n)), adv_c[c].push_back(col_ptr(p.ext, p.plan.adv(c) + p.adv_slot[i], m));
            for (uint32_t i = 0; i < I; i++) inst_v[c].push_back(col_ptr(p.instance_values, c * I + i, n)), inst_c[c].push_back(col_ptr(p.ext, nco + c * I + i, m));
        }
        for (uint32_t ph = 0; ph < p.nph; ph++) {
            const uint64_t* advice = nullptr;
            TRY(advice_of_phase(ph, given ? given[0] : nullptr, &advice));
            if (!advice) return dh_fail(ctx, DEHALO_ERR_INVALID, "null advice");
            const std::vector<uint32_t>& pc = p.phase_cols[ph];
            const uint32_t first = p.phase_first[ph], cnt = N * (uint32_t)pc.size();      // (several circuits: one phase, whose columns are all of them)
            fe* adv = p.cols.at((size_t)(p.plan.o_adv + first) * n);
            if (p.nph == 1) {      // every column at once, circuit after circuit
                for (uint32_t c = 0; c < N; c++) {
                    if (c) advice = given[c];
                    if (!advice) return dh_fail(ctx, DEHALO_ERR_INVALID, "null advice");
                    fe* dst = p.cols.at((size_t)p.plan.adv(c) * n);
                    const bool pin = !(flags & DEHALO_PROOF_ADVICE_ON_DEVICE) && advice != p.adv_pin.get();      // (the witness generator's output is page-locked already)
                    pin_advice.emplace_back(new HostPin(pin ? advice : nullptr, (size_t)A * n * 32));
                    if (flags & DEHALO_PROOF_ADVICE_ON_DEVICE) HIP_TRY(ctx, hipMemcpyAsync(dst, advice, (size_t)A * n * 32, hipMemcpyDeviceToDevice, ms));
                    else TRY(dh_h2d(ctx, dst, advice, (size_t)A * n * 32, ms));      // a DMA from the pinned pages, or staged (witness below 4 MiB)
                }
            } else      // the phase's columns only, a copy per run of neighbouring columns (they are neighbouring slots); the buffer is the caller's until the next
                        // callback: nothing is pinned, and a copy that is still in flight (device or page-locked memory) lands before this phase's commitments come back
                for (uint32_t j = 0, run; j < cnt; j += run) {
                    for (run = 1; j + run < cnt && pc[j + run] == pc[j] + run; run++) {}
                    const uint64_t* src = advice + 4 * (size_t)pc[j] * n;
                    if (flags & DEHALO_PROOF_ADVICE_ON_DEVICE) HIP_TRY(ctx, hipMemcpyAsync(adv + (size_t)j * n, src, (size_t)run * n * 32, hipMemcpyDeviceToDevice, ms));
                    else TRY(dh_h2d(ctx, adv + (size_t)j * n, src, (size_t)run * n * 32, ms));
                }
            if (flags & DEHALO_PROOF_ADVICE_CANONICAL) TRY(dehalo_field_op_device(ctx, fid, 4, (uint64_t*)adv, nullptr, (uint64_t*)adv, (size_t)cnt * n, nullptr));
            if (cnt) k_place_rows<<<(unsigned)((rows * cnt + 255) / 256), 256, 0, ms>>>(adv + u, n, p.blind_dev.p + (size_t)first * rows, (uint32_t)rows, cnt);
            if (side) HIP_TRY(ctx, hipEventRecord(p.ev_ready[0].get(), ms));
            TRY(p.commit(tr, adv, cnt, true, [this, ph] { return after_advice_queued(ph); }, 0, p.blind_at(p.plan.bi_adv + first)));
            for (uint32_t j = 0; j < p.NCH; j++)
                if (cs.challenge_phase[j] == ph) chal[j] = tr->squeeze();
        }
        return 0;
    }
    int after_advice_queued(uint32_t ph) {
        if (I && side && ph == 0) {
            HIP_TRY(side, hipStreamWaitEvent(ss, p.ev_inst.get(), 0));
            TRY(dehalo_intt_scaled_device(side, fid, p.instance.u64(), k, d.omega_inv.v, d.ifft_divisor.v, N * I, nullptr));
            TRY(dehalo_coset_ntt_form_device(side, fid, p.instance.u64(), k, p.ext.u64((size_t)nco * m), ek, d.ext_omega.v, d.g_coset.v, N * I, DEHALO_FORM_OUT_INTERNAL, nullptr));
        }
        if (side) TRY(side_ntt(p.plan.o_adv + p.phase_first[ph], N * (uint32_t)p.phase_cols[ph].size(), p.ev_ready[0].get()));
        if (gates_early && ph + 1 == p.nph) {      // (circuit 0's)
            EvalIn e = coset_inputs(0);
            e.in.y = zero.v;
            TRY(dehalo_graph_evaluate_device(side, p.pk->custom_gates.get(), &e.in, ek, rot_scale, nullptr, p.h.u64(), nullptr));
        }
        if (!helper.joinable()) start_random_polynomial();      // (unless it runs since the synthesis) the host is idle from here to the read-back
        return 0;
    }

    // ---- lookups: compress, permute, blind, commit
    int lookups() {
        if (!L) return 0;
        const uint32_t NL = N * L;      // circuit c's lookup l is pair c * L + l of `compressed` and of the permuted columns
        for (uint32_t c = 0; c < N; c++) {      // (the compressions of a circuit read its own columns: a call per circuit)
            std::vector<const dehalo_graph*> graphs;
            std::vector<uint64_t*> outs;
            for (uint32_t l = 0; l < L; l++) {      // lookups with the same table expressions share ONE compressed table column (their representative's)
                graphs.push_back(p.pk->compress_graphs[l].first.get());
                outs.push_back(p.compressed.u64((size_t)2 * (c * L + l) * n));
                if (p.table_rep[l] == l) {
                    graphs.push_back(p.pk->compress_graphs[l].second.get());
                    outs.push_back(p.compressed.u64((size_t)(2 * (c * L + l) + 1) * n));
                }
            }
            EvalIn e;
            e.cols(fixed_v, adv_v[c], inst_v[c]);
            e.in.theta = theta.v;
            e.in.challenges = (const uint64_t*)chal.data(); e.in.num_challenges = (uint32_t)chal.size();
            TRY(dehalo_graph_evaluate_batch_device(ctx, graphs.data(), (uint32_t)graphs.size(), &e.in, k, 1, outs.data(), nullptr));
        }
        p.tk("compress queued");
        // the blinding rows [u, n) first: the permutation writes rows [0, u) only and ends with a read-back
        const fe* bl_perm = p.blind_dev.p + (size_t)N * A * rows;
        k_place_rows<<<(unsigned)((rows * 2 * NL + 255) / 256), 256, 0, ms>>>(p.cols.at((size_t)p.plan.o_perm * n + u), n, bl_perm, (uint32_t)rows, 2 * NL);
        std::vector<const uint64_t*> pin, ptab;
        std::vector<uint64_t*> pout_in, pout_tab;
        // status flags behind the 2 N L points of this phase: the stream runs from the permutation straight into the commitment, the flags come back with the points
        std::vector<const uint32_t*> trep, tmult;
        std::vector<uint32_t> tcount;
        for (uint32_t c = 0; c < N; c++)
            for (uint32_t l = 0; l < L; l++) {
                pin.push_back(p.compressed.u64((size_t)2 * (c * L + l) * n));
                ptab.push_back(p.compressed.u64((size_t)(2 * (c * L + p.table_rep[l]) + 1) * n));
                pout_in.push_back(p.cols.u64((size_t)(p.plan.perm(c) + 2 * l) * n));
                pout_tab.push_back(p.cols.u64((size_t)(p.plan.perm(c) + 2 * l + 1) * n));
                const dehalo_prover::TableRows& t = p.table_rows[p.table_rep[l]];      // (of the key: every circuit's)
                trep.push_back(t.d_rep.p); tmult.push_back(t.d_mult.p); tcount.push_back(t.count);
            }
        TRY(dehalo_permute_expression_pair_distinct_device(ctx, fid, pin.data(), ptab.data(), u, NL, pout_in.data(), pout_tab.data(), trep.data(), tmult.data(), tcount.data(),
                                                           reinterpret_cast<int32_t*>(p.jac.u64() + 12 * 2 * (size_t)NL), nullptr));
        p.tk("permute queued");
        if (side) HIP_TRY(ctx, hipEventRecord(p.ev_ready[1].get(), ms));
        return p.commit(tr, p.cols.at((size_t)p.plan.o_perm * n), 2 * NL, true, side ? std::function<int()>([this] { return after_lookups_queued(); }) : nullptr, NL, p.blind_at(p.plan.bi_perm));
    }
    int after_lookups_queued() { return side_ntt(p.plan.o_perm, 2 * N * L, p.ev_ready[1].get()); }

    // ---- grand products: permutation sets, then lookups, then shuffles; one batched inversion.  The random polynomial's values are the launch's last column
    // (cols[o_rand] sits right behind the products): its commitment is written with theirs
    int products_and_random() {
        const uint32_t npc = (uint32_t)cs.perm_cols.size();
        if (helper.joinable()) helper.join();              // (long finished: the draw takes 0.5 ms at k = 17 and started before the advice commitment)
        p.tk("helper joined");
        if (helper_rc.load()) return helper_rc.load();
        fe* rl = p.cols.at((size_t)p.plan.o_rand * n);
        if (side) HIP_TRY(ctx, hipMemcpyAsync(rl, p.polys + (size_t)p.plan.o_rand * n, n * sizeof(fe), hipMemcpyDeviceToDevice, ms));      // (the helper put the coefficients there)
        else {      // without a side context the coefficient forms live in `cols` itself: keep a copy for after the commitment
            if (device_rng) TRY(chacha_scalars_device(ctx, rng_poly, 1, rl, n, ms));
            else HIP_TRY(ctx, hipMemcpyAsync(rl, p.rand_pin.get(), n * 32, hipMemcpyHostToDevice, ms));      // (rand_pin: page-locked, the library's own)
            HIP_TRY(ctx, hipMemcpyAsync(p.wbuf.p, rl, n * sizeof(fe), hipMemcpyDeviceToDevice, ms));
        }
        TRY(dehalo_ntt_device(ctx, fid, (uint64_t*)rl, k, d.omega.v, 1, nullptr));
        if (S + L + H == 0) return p.commit(tr, rl, 1, true, [this] { return restore_random(); }, 0, p.blind_at(p.plan.bi_rand));
        std::vector<Fe> pchal(std::max<uint32_t>(npc, 1));
        Fe dj = beta;
        for (uint32_t j = 0; j < npc; j++) {
            pchal[j] = dj;
            dj = f->mul(dj, f->delta);
        }
        // every product's numerator and denominator columns in ONE launch per circuit (k_product_terms) instead of a GraphEvaluator program per column: circuit c's
        // S + L columns at its place in num / den, which is its products' place in `cols`
        std::vector<const uint64_t*> psig;
        for (uint32_t j = 0; j < npc; j++) psig.push_back(col_ptr(p.pk->perm_values, j, n));
        std::vector<Fe> set_factors(std::max<uint32_t>(S, 1));
        for (uint32_t s2 = 0; s2 < S; s2++) set_factors[s2] = pchal[std::min<uint32_t>(s2 * cs.chunk_len(), npc ? npc - 1 : 0)];      // beta delta^(first column of the set)
        const uint32_t PC = S + L + H, NP = N * PC;      // products per circuit, of the proof
        for (uint32_t c = 0; c < N; c++) {
            std::vector<const uint64_t*> pcolv, pA, pS, pa, ps;
            for (auto& pc : cs.perm_cols) pcolv.push_back(pc.kind == DEHALO_COLUMN_ADVICE ? adv_v[c][pc.index] : pc.kind == DEHALO_COLUMN_FIXED ? fixed_v[pc.index] : inst_v[c][pc.index]);
            for (uint32_t l = 0; l < L; l++) {
                pA.push_back(col_ptr(p.compressed, 2 * (c * L + l), n));
                pS.push_back(col_ptr(p.compressed, 2 * (c * L + p.table_rep[l]) + 1, n));
                pa.push_back(col_ptr(p.cols, p.plan.perm(c) + 2 * l, n));
                ps.push_back(col_ptr(p.cols, p.plan.perm(c) + 2 * l + 1, n));
            }
            dehalo_product_inputs pin{};
            pin.columns = pcolv.data(); pin.sigma = psig.data(); pin.num_columns = npc; pin.chunk_len = cs.chunk_len();
            pin.omega_powers = p.omega_col.u64();
            pin.beta = beta.v; pin.gamma = gamma.v; pin.delta = f->delta.v;
            pin.set_factors = (const uint64_t*)set_factors.data();
            pin.compressed_input = pA.data(); pin.compressed_table = pS.data(); pin.permuted_input = pa.data(); pin.permuted_table = ps.data();
            pin.num_lookups = L;
            if (S + L) TRY(dehalo_product_terms_device(ctx, fid, &pin, n, p.num.u64((size_t)c * PC * n), p.den.u64((size_t)c * PC * n), n, nullptr));
            if (H) {      // a shuffle's numerator and denominator columns are its two programs' values on the original domain: compress(inputs) + gamma, compress(shuffle side) + gamma
                std::vector<const dehalo_graph*> graphs;
                std::vector<uint64_t*> outs;
                for (uint32_t j = 0; j < H; j++) {
                    graphs.push_back(p.pk->shuffle_graphs[j].first.get());
                    outs.push_back(p.num.u64((size_t)(c * PC + S + L + j) * n));
                    graphs.push_back(p.pk->shuffle_graphs[j].second.get());
                    outs.push_back(p.den.u64((size_t)(c * PC + S + L + j) * n));
                }
                EvalIn e;
                e.cols(fixed_v, adv_v[c], inst_v[c]);
                e.in.theta = theta.v; e.in.gamma = gamma.v;
                e.in.challenges = (const uint64_t*)chal.data(); e.in.num_challenges = (uint32_t)chal.size();
                TRY(dehalo_graph_evaluate_batch_device(ctx, graphs.data(), (uint32_t)graphs.size(), &e.in, k, 1, outs.data(), nullptr));
            }
        }
        p.tk("product graphs queued");
        TRY(dehalo_grand_product_batch_device(ctx, fid, p.num.u64(), p.den.u64(), n, NP, n, p.cols.u64((size_t)p.plan.o_pz * n), nullptr));
        for (uint32_t c = 0; c < N; c++)
            for (uint32_t s = 1; s < S; s++)      // z_s starts where z_{s-1} ended: z = vec![last_z] (a circuit's first set starts at 1)
                TRY(dehalo_scale_device(ctx, fid, p.cols.u64((size_t)(p.plan.pz(c) + s) * n), n, nullptr, 0, p.cols.u64((size_t)(p.plan.pz(c) + s - 1) * n + u), nullptr));
        // a shuffle's product ends at 1 exactly when its two sides are a permutation of each other (but for a negligible probability over gamma): one flag per
        // shuffle behind the phase's points, read with them
        if (H) {
            fe one_std;
            memcpy(&one_std, f->one.v, 32);
            k_shuffle_closed<<<(N * H + 63) / 64, 64, 0, ms>>>(p.cols.at((size_t)p.plan.o_sz * n), (uint64_t)PC * n, n, u, H, N * H, one_std,
                                                               reinterpret_cast<int32_t*>(p.jac.u64() + 12 * (size_t)(NP + 1)));
        }
        // per column: bf blinding rows (n - bf .. n)
        const fe* bl_prod = p.blind_dev.p + (size_t)N * (A + 2 * L) * rows;
        k_place_rows<<<(unsigned)(((size_t)bf * NP + 255) / 256), 256, 0, ms>>>(p.cols.at((size_t)p.plan.o_pz * n + (n - bf)), n, bl_prod, bf, NP);
        if (side) HIP_TRY(ctx, hipEventRecord(p.ev_ready[2].get(), ms));
        return p.commit(tr, p.cols.at((size_t)p.plan.o_pz * n), NP + 1, true, [this] { return after_products_queued(); }, (size_t)N * H, p.blind_at(p.plan.bi_prod), true,
                        N > 1 ? p.plan.product_order.data() : nullptr, true);
    }
    int restore_random() {      // (queued behind the MSM's kernels on the same stream)
        if (!side) HIP_TRY(ctx, hipMemcpyAsync(p.cols.at((size_t)p.plan.o_rand * n), p.wbuf.p, n * sizeof(fe), hipMemcpyDeviceToDevice, ms));
        return 0;
    }
    int after_products_queued() {
        TRY(restore_random());
        if (!side) return 0;
        TRY(side_ntt(p.plan.o_pz, N * (S + L + H), p.ev_ready[2].get()));
        // the lookups' (compressed input + beta)(compressed table + gamma) over the extended domain need theta, beta, gamma and the advice /
        // fixed cosets: all there -- on the side context, beside the products' commitment, instead of after y
        for (uint32_t c = 0; c < N && L; c++) {
            std::vector<const dehalo_graph*> graphs;
            for (auto& g : p.pk->lookup_graphs) graphs.push_back(g.get());
            std::vector<uint64_t*> outs;
            for (uint32_t l = 0; l < L; l++) outs.push_back(p.table_value.u64((size_t)(c * L + l) * m));
            EvalIn e = coset_inputs(c);
            e.in.beta = beta.v; e.in.gamma = gamma.v; e.in.theta = theta.v;
            TRY(dehalo_graph_evaluate_batch_device(side, graphs.data(), L, &e.in, ek, rot_scale, outs.data(), nullptr));
        }
        for (uint32_t c = 0; c < N && H; c++) TRY(shuffle_values(side, c));      // likewise the shuffles' two sides
        return 0;
    }
    // circuit c's shuffles over the extended domain: compress(inputs) + gamma and compress(shuffle side) + gamma, one call for all of them
    int shuffle_values(dehalo_ctx* on, uint32_t c) {
        std::vector<const dehalo_graph*> graphs;
        std::vector<uint64_t*> outs;
        for (uint32_t j = 0; j < H; j++) {
            graphs.push_back(p.pk->shuffle_graphs[j].first.get());
            outs.push_back(p.shuffle_value.u64((size_t)(2 * (c * H + j)) * m));
            graphs.push_back(p.pk->shuffle_graphs[j].second.get());
            outs.push_back(p.shuffle_value.u64((size_t)(2 * (c * H + j) + 1) * m));
        }
        EvalIn e = coset_inputs(c);
        e.in.gamma = gamma.v; e.in.theta = theta.v;
        return dehalo_graph_evaluate_batch_device(on, graphs.data(), (uint32_t)graphs.size(), &e.in, ek, rot_scale, outs.data(), nullptr);
    }

    // ---- coefficient forms and cosets of everything committed so far; evaluate_h, / t(X), extended_to_coeff; the pieces' commitments
    int quotient() {
        const uint32_t npc = (uint32_t)cs.perm_cols.size();
        if (!side) {
            TRY(dehalo_intt_scaled_device(ctx, fid, p.cols.u64(), k, d.omega_inv.v, d.ifft_divisor.v, nco, nullptr));
            TRY(dehalo_coset_ntt_form_device(ctx, fid, p.cols.u64(), k, p.ext.u64(), ek, d.ext_omega.v, d.g_coset.v, nco, DEHALO_FORM_OUT_INTERNAL, nullptr));
            if (I) TRY(dehalo_coset_ntt_form_device(ctx, fid, p.instance.u64(), k, p.ext.u64((size_t)nco * m), ek, d.ext_omega.v, d.g_coset.v, N * I, DEHALO_FORM_OUT_INTERNAL, nullptr));
        } else {      // queued phase by phase on the side context: wait for it
            HIP_TRY(side, hipEventRecord(p.ev_side.get(), ss));
            HIP_TRY(ctx, hipStreamWaitEvent(ms, p.ev_side.get(), 0));
        }
        const uint64_t *l0 = p.pk->l_ext.u64(0), *l_last = p.pk->l_ext.u64(m), *l_active = p.pk->l_ext.u64(2 * m);
        // evaluate_h: ONE running value over the circuits -- circuit c's gates, permutation terms and lookup terms continue from circuit c - 1's value
        std::vector<const uint64_t*> sigma;
        for (uint32_t j = 0; j < npc; j++) sigma.push_back(col_ptr(p.pk->perm_cosets, j, m));
        const Fe beta_zeta = f->mul(beta, d.g_coset);
        for (uint32_t c = 0; c < N; c++) {
            if (c || !gates_early) {
                EvalIn e = coset_inputs(c);
                e.in.y = y.v;
                TRY(dehalo_graph_evaluate_device(ctx, p.pk->custom_gates.get(), &e.in, ek, rot_scale, c ? p.h.u64() : nullptr, p.h.u64(), nullptr));
            }
            if (S) {
                std::vector<const uint64_t*> z, pcols;
                for (uint32_t s = 0; s < S; s++) z.push_back(col_ptr(p.ext, p.plan.pz(c) + s, m));
                for (auto& pc : cs.perm_cols) pcols.push_back(pc.kind == DEHALO_COLUMN_ADVICE ? adv_c[c][pc.index] : pc.kind == DEHALO_COLUMN_FIXED ? fixed_c[pc.index] : inst_c[c][pc.index]);
                dehalo_perm_inputs pi{};
                pi.z = z.data(); pi.num_sets = S;
                pi.columns = pcols.data(); pi.sigma = sigma.data(); pi.num_columns = npc;
                pi.chunk_len = cs.chunk_len();
                pi.last_rotation = -(int32_t)(bf + 1);
                pi.l0 = l0; pi.l_last = l_last; pi.l_active_row = l_active;
                pi.beta = beta.v; pi.gamma = gamma.v; pi.y = y.v; pi.delta = f->delta.v; pi.beta_zeta = beta_zeta.v; pi.extended_omega = d.ext_omega.v;
                pi.form_flags = FF;
                TRY(dehalo_permutation_h_device(ctx, fid, &pi, ek, rot_scale, p.h.u64(), nullptr));
            }
            for (uint32_t l = 0; l < L && !side; l++) {
                EvalIn e = coset_inputs(c);
                e.in.beta = beta.v; e.in.gamma = gamma.v; e.in.theta = theta.v;
                TRY(dehalo_graph_evaluate_device(ctx, p.pk->lookup_graphs[l].get(), &e.in, ek, rot_scale, nullptr, p.table_value.u64((size_t)(c * L + l) * m), nullptr));
            }
            for (uint32_t first = 0; first < L; first += 8) {
                std::vector<dehalo_lookup_inputs> li;
                for (uint32_t l = first; l < std::min(L, first + 8); l++) {
                    dehalo_lookup_inputs q{};
                    q.product_coset = col_ptr(p.ext, p.plan.lz(c) + l, m);
                    q.permuted_input_coset = col_ptr(p.ext, p.plan.perm(c) + 2 * l, m);
                    q.permuted_table_coset = col_ptr(p.ext, p.plan.perm(c) + 2 * l + 1, m);
                    q.table_value = p.table_value.u64((size_t)(c * L + l) * m);
                    q.l0 = l0; q.l_last = l_last; q.l_active_row = l_active;
                    q.beta = beta.v; q.gamma = gamma.v; q.y = y.v;
                    q.form_flags = FF;
                    li.push_back(q);
                }
                TRY(dehalo_lookup_h_batch_device(ctx, fid, li.data(), (uint32_t)li.size(), ek, rot_scale, p.h.u64(), nullptr));
            }
            if (H && !side) TRY(shuffle_values(ctx, c));
            for (uint32_t first = 0; first < H; first += 8) {      // (the batched pass takes eight at a time)
                std::vector<dehalo_shuffle_inputs> si;
                for (uint32_t j = first; j < std::min(H, first + 8); j++) {
                    dehalo_shuffle_inputs q{};
                    q.product_coset = col_ptr(p.ext, p.plan.sz(c) + j, m);
                    q.input_value = p.shuffle_value.u64((size_t)(2 * (c * H + j)) * m);
                    q.shuffle_value = p.shuffle_value.u64((size_t)(2 * (c * H + j) + 1) * m);
                    q.l0 = l0; q.l_last = l_last; q.l_active_row = l_active;
                    q.y = y.v;
                    q.form_flags = FF;
                    si.push_back(q);
                }
                TRY(dehalo_shuffle_h_batch_device(ctx, fid, si.data(), (uint32_t)si.size(), ek, rot_scale, p.h.u64(), nullptr));
            }
        }
        TRY(dehalo_scale_device(ctx, fid, p.h.u64(), m, (const uint64_t*)d.t_inv.data(), (uint32_t)d.t_inv.size(), nullptr, nullptr));      // divide_by_vanishing_poly
        TRY(dehalo_coset_intt_form_device(ctx, fid, p.h.u64(), ek, d.ext_omega_inv.v, d.ext_ifft_divisor.v, d.g_coset.v, 1, DEHALO_FORM_IN_INTERNAL, nullptr));
        p.tk("quotient queued");
        return p.commit(tr, p.h.p, pieces, false, nullptr, 0, p.blind_at(p.plan.bi_h));
    }

    // ---- evaluations, in upstream's order: every opened polynomial at every rotation in ONE call
    int evaluations() {
        const OpeningPlan& pl = p.plan;
        point.resize(pl.rots.size());
        for (size_t i = 0; i < pl.rots.size(); i++) point[i] = d.rotate_omega(x, pl.rots[i]);
        if (pl.rots.size() <= 4)
            TRY(dehalo_eval_polynomial_multi_masked_device(ctx, fid, p.plist.data(), pl.num_polys, n, (const uint64_t*)point.data(), (uint32_t)pl.rots.size(), pl.eval_wanted8.data(),
                                                           p.evals.u64(), nullptr));
        else      // gates that query rotations beyond {-1, 0, 1}: up to 32 points, every polynomial still read once
            TRY(dehalo_eval_polynomial_points_device(ctx, fid, p.plist.data(), pl.num_polys, n, (const uint64_t*)point.data(), (uint32_t)pl.rots.size(), pl.eval_wanted.data(),
                                                     p.evals.u64(), nullptr));
        // the folded quotient h(X) = sum_i x^(n i) h_i(X) (opened below; its value at x comes from the pieces' values)
        xs = powers(f, f->pow_u64(x, (uint64_t)n), pieces);
        TRY(dehalo_lincomb_device(ctx, fid, p.plist.data() + pl.p_hpiece, (const uint64_t*)xs.data(), pieces, n, p.hfold.u64(), nullptr, nullptr));
        p.tk("evaluations queued");
        TRY(dehalo_download(ctx, p.evals.p, pl.eval_count * 32, p.host_evals.data()));
        p.tk("evaluations on host");
        E = (const Fe*)p.host_evals.data();
        hfold_eval = fold(f, xs.data(), E + pl.hpiece0, pieces);
        for (int64_t i : pl.instance_write) tr->write_scalar(E[i]);      // (IPA: the instance evaluations come first)
        for (int64_t i : pl.write) tr->write_scalar(E[i]);
        return 0;
    }

    // ---- ProverIPA::create_proof [UPSTREAM poly/ipa/multiopen/prover.rs]
    int open_ipa() {
        const Fe x1 = tr->squeeze();
        const Fe x2 = tr->squeeze();
        bl[p.plan.bi_hfold] = fold(f, xs.data(), &bl[p.plan.bi_h], pieces);      // h's blinds fold with x^n as its pieces do
        const OpeningPlan& pl = p.plan;
        const size_t ns = pl.point_sets.size();
        // q_i = the set's polynomials folded with x_1 in commitment order (q <- x_1 q + poly), the blinds likewise
        std::vector<Fe> pblinds(1 + ns);      // of f and of every q_i
        size_t depth = 0;
        for (size_t si = 0; si < ns; si++) {
            std::vector<const uint64_t*> ptrs;
            std::vector<Fe> blinds;
            for (uint32_t ci : pl.set_members[si]) { ptrs.push_back(p.plist[pl.commitments[ci].poly]); blinds.push_back(bl[pl.commitments[ci].blind]); }
            const std::vector<Fe> coefs = powers(f, x1, ptrs.size(), true);
            pblinds[1 + si] = fold(f, coefs.data(), blinds.data(), ptrs.size());
            TRY(dehalo_lincomb_device(ctx, fid, ptrs.data(), (const uint64_t*)coefs.data(), ptrs.size(), n, p.ipa_q.u64(si * n), nullptr, nullptr));
            depth = std::max(depth, pl.point_sets[si].size());
        }
        // each q_i divided by (X - point) for every point of its set in turn, remainders dropped: one batched launch per division depth over the sets
        // that still have a point left (a division writes n - 1 coefficients: the top one of both buffers stays zero)
        HIP_TRY(ctx, hipMemsetAsync(p.ipa_wa.p, 0, ns * n * 32, ms));
        HIP_TRY(ctx, hipMemsetAsync(p.ipa_wb.p, 0, ns * n * 32, ms));
        std::vector<const uint64_t*> cur(ns);
        for (size_t si = 0; si < ns; si++) cur[si] = p.ipa_q.u64(si * n);
        for (size_t dd = 0; dd < depth; dd++) {
            std::vector<const uint64_t*> ins;
            std::vector<uint64_t*> outs;
            std::vector<Fe> pts;
            std::vector<size_t> which;
            for (size_t si = 0; si < ns; si++)
                if (pl.point_sets[si].size() > dd) {
                    ins.push_back(cur[si]);
                    outs.push_back((dd & 1 ? p.ipa_wb : p.ipa_wa).u64(si * n));
                    pts.push_back(d.rotate_omega(x, pl.point_rot[pl.point_sets[si][dd]]));
                    which.push_back(si);
                }
            for (size_t first = 0; first < ins.size(); first += 8)      // (the batched division takes eight at a time)
                TRY(dehalo_kate_division_batch_device(ctx, fid, ins.data() + first, n, (const uint64_t*)(pts.data() + first), outs.data() + first,
                                                      std::min<size_t>(8, ins.size() - first), nullptr));
            for (size_t j = 0; j < which.size(); j++) cur[which[j]] = outs[j];
        }
        // f = the quotients folded with x_2; commit(f, f_blind)
        TRY(dehalo_lincomb_device(ctx, fid, cur.data(), (const uint64_t*)powers(f, x2, ns, true).data(), ns, n, p.ipa_f.u64(), nullptr, nullptr));
        TRY(p.commit(tr, p.ipa_f.p, 1, false, nullptr, 0, p.blind_at(p.plan.bi_f)));
        const Fe x3 = tr->squeeze();
        // q_i(x_3) for every set: one evaluation call, one download
        fe* qe = p.evals.at(pl.eval_count + 8);
        TRY(dehalo_eval_polynomial_device(ctx, fid, p.ipa_q.u64(), n, n, ns, x3.v, (uint64_t*)qe, nullptr));
        std::vector<Fe> qev(ns);
        TRY(dehalo_download(ctx, qe, ns * 32, qev.data()));
        for (size_t si = 0; si < ns; si++) tr->write_scalar(qev[si]);
        const Fe x4 = tr->squeeze();
        // p = f, then p <- x_4 p + q_i over the sets; the blind likewise
        std::vector<const uint64_t*> ptrs = {p.ipa_f.u64()};
        for (size_t si = 0; si < ns; si++) ptrs.push_back(p.ipa_q.u64(si * n));
        pblinds[0] = bl[p.plan.bi_f];
        const std::vector<Fe> coefs = powers(f, x4, ns + 1, true);
        TRY(dehalo_lincomb_device(ctx, fid, ptrs.data(), (const uint64_t*)coefs.data(), ns + 1, n, p.ipa_p.u64(), nullptr, nullptr));
        const Fe pblind = fold(f, coefs.data(), pblinds.data(), ns + 1);
        p.tk("multiopen done");
        // commitment::create_proof on p at x_3: same transcript, same generator (right behind f's blind)
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        return ipa_open_body(ctx, p.params, p.ipa_p.u64(), pblind, x3, rng, 2, tr);
    }

    // ---- ProverGWC::create_proof: one witness polynomial per distinct point, in order of first appearance
    int open_gwc() {
        const Fe v = tr->squeeze();
        p.tk("v");
        const OpeningPlan& pl = p.plan;
        const size_t ng = pl.groups.size();
        HIP_TRY(ctx, hipMemsetAsync(p.wbuf.p, 0, std::max<size_t>(4, ng) * n * 32, ms));
        std::vector<const uint64_t*> qptrs;
        std::vector<uint64_t*> wptrs;
        std::vector<Fe> qpoints;
        for (size_t gi = 0; gi < ng; gi++) {
            const OpeningPlan::Group& g = pl.groups[gi];
            const std::vector<Fe> coefs = powers(f, v, g.evals.size());
            std::vector<Fe> values;
            for (int64_t i : g.evals) values.push_back(i >= 0 ? E[i] : hfold_eval);
            const Fe eval_batch = fold(f, coefs.data(), values.data(), values.size());
            std::vector<const uint64_t*> ptrs;
            for (uint32_t id : g.polys) ptrs.push_back(p.plist[id]);
            TRY(dehalo_lincomb_device(ctx, fid, ptrs.data(), (const uint64_t*)coefs.data(), ptrs.size(), n, p.qbuf.u64(gi * n), eval_batch.v, nullptr));
            qptrs.push_back(p.qbuf.u64(gi * n));
            wptrs.push_back(p.wbuf.u64(gi * n));
            qpoints.push_back(point[pl.rot_index(g.rot)]);
        }
        for (size_t first = 0; first < ng; first += 8)      // (the batched division takes eight at a time); the witnesses are committed in one MSM
            TRY(dehalo_kate_division_batch_device(ctx, fid, qptrs.data() + first, n, (const uint64_t*)(qpoints.data() + first), wptrs.data() + first, std::min<size_t>(8, ng - first), nullptr));
        return p.commit(tr, p.wbuf.p, ng, false);
    }

    // ---- ProverSHPLONK::create_proof [UPSTREAM poly/kzg/multiopen/shplonk/prover.rs]: two commitments whatever the rotations are.  Per rotation set i (the
    // plan's sets: points T_i, polynomials P_ij in order of first appearance) F_i = sum_j y^j P_ij and Q_i = F_i div Z_i, Z_i = prod_{z in T_i} (X - z) -- upstream
    // divides sum_j y^j (P_ij - R_ij), R_ij the polynomial of degree < |T_i| through P_ij's values on T_i: subtracting it only removes the remainder, which the
    // division here drops.  h = sum_i v^i Q_i; then at u, with zdiff_i = prod_{z in super \ T_i} (u - z) and r_ij = R_ij(u),
    //   L = sum_i v^i zdiff_i (F_i - sum_j y^j r_ij) - Z_T(u) h,  L(u) = 0,  h' = L / ((X - u) zdiff_0).
    // Each committed polynomial is read once (into its F_i); the quotients come from one pass per eight sets (dehalo_vanishing_quotient_batch_device).
    int open_shplonk() {
        const Fe y_ = tr->squeeze();
        const Fe v = tr->squeeze();
        const OpeningPlan& pl = p.plan;
        const size_t ns = pl.point_sets.size();
        std::vector<std::vector<Fe>> pts(ns), ycoef(ns);
        std::vector<const uint64_t*> fptrs(ns), pt_ptrs(ns);
        std::vector<uint64_t*> qptrs(ns);
        std::vector<uint32_t> npts(ns);
        for (size_t si = 0; si < ns; si++) {
            std::vector<const uint64_t*> ptrs;
            for (uint32_t ci : pl.set_members[si]) ptrs.push_back(p.plist[pl.commitments[ci].poly]);
            ycoef[si] = powers(f, y_, ptrs.size());
            TRY(dehalo_lincomb_device(ctx, fid, ptrs.data(), (const uint64_t*)ycoef[si].data(), ptrs.size(), n, p.shp_f.u64(si * n), nullptr, nullptr));
            for (uint32_t pi : pl.point_sets[si]) pts[si].push_back(d.rotate_omega(x, pl.point_rot[pi]));
            fptrs[si] = p.shp_f.u64(si * n); qptrs[si] = p.shp_q.u64(si * n); pt_ptrs[si] = pts[si][0].v; npts[si] = (uint32_t)pts[si].size();
        }
        for (size_t first = 0; first < ns; first += 8)      // (eight sets a launch; every Q_i comes out n coefficients long, its top |T_i| zero)
            TRY(dehalo_vanishing_quotient_batch_device(ctx, fid, fptrs.data() + first, n, pt_ptrs.data() + first, npts.data() + first, qptrs.data() + first,
                                                       std::min<size_t>(8, ns - first), nullptr));
        const std::vector<Fe> vpow = powers(f, v, ns);
        TRY(dehalo_lincomb_device(ctx, fid, (const uint64_t* const*)qptrs.data(), (const uint64_t*)vpow.data(), ns, n, p.shp_h.u64(), nullptr, nullptr));
        TRY(p.commit(tr, p.shp_h.p, 1, false));      // (Blind::default() is dropped under KZG, as in GWC)
        const Fe u_ = tr->squeeze();
        // host: per set zdiff_i and the Lagrange basis of T_i at u, every denominator (and zdiff_0) inverted together
        std::vector<Fe> super;
        for (int32_t r : pl.point_rot) super.push_back(d.rotate_omega(x, r));
        Fe zt = f->one;
        for (const Fe& z : super) zt = f->mul(zt, f->sub(u_, z));
        std::vector<Fe> zdiff(ns, f->one), inv;      // inv: [zdiff_0 | per set, per point: prod_{s != t} (z_t - z_s)]
        std::vector<std::vector<Fe>> basis(ns);      // prod_{s != t} (u - z_s), then times the inverted denominator
        for (size_t si = 0; si < ns; si++) {
            const std::vector<uint32_t>& T = pl.point_sets[si];
            for (uint32_t pi = 0; pi < super.size(); pi++)
                if (std::find(T.begin(), T.end(), pi) == T.end()) zdiff[si] = f->mul(zdiff[si], f->sub(u_, super[pi]));
            if (si == 0) inv.push_back(zdiff[0]);
            for (size_t t = 0; t < T.size(); t++) {
                Fe num = f->one, den = f->one;
                for (size_t s2 = 0; s2 < T.size(); s2++)
                    if (s2 != t) { num = f->mul(num, f->sub(u_, pts[si][s2])); den = f->mul(den, f->sub(pts[si][t], pts[si][s2])); }
                basis[si].push_back(num);
                inv.push_back(den);
            }
        }
        // (u is none of the points and the points differ, but for a negligible probability: a zero here is refused, not divided by)
        if (!f->batch_invert(inv.data(), inv.size())) return dh_fail(ctx, DEHALO_ERR_INVALID, "shplonk: the challenge u is an opening point");
        const Fe zdiff0_inv = inv[0];
        // L's ns + 1 coefficients, already over zdiff_0, and its constant: sum_i v^i zdiff_i sum_j y^j r_ij, r_ij = sum_t basis_t eval_ij(z_t)
        std::vector<const uint64_t*> lptrs(fptrs);
        lptrs.push_back(p.shp_h.u64());
        std::vector<Fe> lcoef(ns + 1);
        Fe lconst = zero;
        size_t io = 1;
        for (size_t si = 0; si < ns; si++) {
            for (Fe& b : basis[si]) b = f->mul(b, inv[io++]);
            Fe rsum = zero;
            size_t j = 0;
            for (uint32_t ci : pl.set_members[si]) {
                const OpeningPlan::Commitment& cm = pl.commitments[ci];
                Fe r = zero;
                for (size_t t = 0; t < basis[si].size(); t++) r = f->add(r, f->mul(basis[si][t], cm.evals[t] >= 0 ? E[cm.evals[t]] : hfold_eval));
                rsum = f->add(rsum, f->mul(ycoef[si][j++], r));
            }
            lcoef[si] = f->mul(f->mul(vpow[si], zdiff[si]), zdiff0_inv);
            lconst = f->add(lconst, f->mul(lcoef[si], rsum));
        }
        lcoef[ns] = f->neg(f->mul(zt, zdiff0_inv));
        TRY(dehalo_lincomb_device(ctx, fid, lptrs.data(), (const uint64_t*)lcoef.data(), ns + 1, n, p.shp_l.u64(), lconst.v, nullptr));
        // h' = L / (X - u) into Q_0's buffer (read for the last time by h's fold): n - 1 coefficients under a top one that Q_0 left zero
        const uint64_t* lp = p.shp_l.u64();
        uint64_t* wp = p.shp_q.u64();
        TRY(dehalo_kate_division_batch_device(ctx, fid, &lp, n, u_.v, &wp, 1, nullptr));
        return p.commit(tr, p.shp_q.p, 1, false);
    }

    void finish() {
        mark(6);
        p.timings[7] = ms_since(t_start);
        if (p.trace) {
            double prev = 0;
            for (auto& t : p.ticks) {
                fprintf(stderr, "  %8.3f (+%6.3f) %s\n", t.second, t.second - prev, t.first);
                prev = t.second;
            }
            fprintf(stderr, "  %8.3f total\n", p.timings[7]);
        }
        rng.write_back(rng_in);
    }

    // create_proof [UPSTREAM plonk/prover.rs]; `synth_in`: of a circuit, synthesized inside (its advice replaces `advice`)
    int run(const uint64_t* const* advice, const uint64_t* const* instances, const size_t* instance_lens, uint32_t num_instance_columns, uint32_t flags,
            const dehalo_circuit_inputs* synth_in, dehalo_synthesis_info* synth_info, dehalo_advice_fn fn = nullptr, void* user = nullptr) {
        advice_fn = fn; advice_user = user;
        p.ticks.clear();
        p.t0 = t_start;
        p.trace = getenv("DEHALO_PROVER_TRACE") != nullptr;
        (void)hipSetDevice(ctx->device);
        TRY(draw_blinds());
        const uint64_t* synthesized = nullptr;
        if (synth_in) {
            TRY(synthesize(synth_in, synth_info));
            synthesized = p.adv_pin.get();
            advice = &synthesized;
            flags = (flags & ~(uint32_t)DEHALO_PROOF_ADVICE_ON_DEVICE) | DEHALO_PROOF_ADVICE_CANONICAL;
        }
        TRY(upload_blinds());
        tr->common_scalar(p.pk->transcript_repr);      // vk.hash_into
        TRY(instance_columns(instances, instance_lens, num_instance_columns));
        TRY(advice_columns(advice, flags));
        mark(0);
        theta = tr->squeeze();
        p.tk("theta");
        TRY(lookups());
        mark(1);
        beta = tr->squeeze();
        gamma = tr->squeeze();
        p.tk("beta gamma");
        TRY(products_and_random());
        mark(2);
        p.tk("products done");
        p.tk("helper joined");      // (joined in front of the products since the random polynomial rides with them; the label stays where traces have it)
        if (p.trace) fprintf(stderr, "  helper: draw %.3f, upload queued %.3f, upload done %.3f ms after its start\n", helper_ms[0], helper_ms[1], helper_ms[2]);
        mark(3);
        y = tr->squeeze();
        p.tk("y");
        TRY(quotient());
        mark(4);
        x = tr->squeeze();
        TRY(evaluations());
        mark(5);
        TRY(ipa ? open_ipa() : p.multiopen == DEHALO_MULTIOPEN_SHPLONK ? open_shplonk() : open_gwc());
        finish();
        return 0;
    }
};

// `advice`: one witness per circuit of the prover (null: synthesized inside, or asked for phase by phase)
int prove(dehalo_prover* p, const uint64_t* const* advice, const uint64_t* const* instances, const size_t* instance_lens, uint32_t num_instance_columns, dehalo_rng* rng,
          dehalo_transcript* transcript, uint32_t flags, const dehalo_circuit_inputs* synth_in, dehalo_synthesis_info* synth_info, dehalo_advice_fn fn = nullptr,
          void* user = nullptr) {
    if (p->N > 1 && (synth_in || fn)) return dh_fail(p->ctx, DEHALO_ERR_UNSUPPORTED, "a prover of several circuits takes their witnesses through dehalo_create_proof_multi only");
    if (transcript->curve != p->pk->curve) return dh_fail(p->ctx, DEHALO_ERR_INVALID, "create_proof: the transcript's curve differs from the key's");
    if (p->nph > 1 && synth_in) return dh_fail(p->ctx, DEHALO_ERR_UNSUPPORTED, "create_proof_circuit: the key has later-phase advice columns");
    if (p->nph > 1 && !fn)      // (its advice would have to exist before the first commitment)
        return dh_fail(p->ctx, DEHALO_ERR_INVALID, "create_proof: the key has later-phase advice columns, whose witness depends on the proof's challenges: use dehalo_create_proof_phased");
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->nph > 1 && p->shard_world > 1) return dh_fail(p->ctx, DEHALO_ERR_UNSUPPORTED, "create_proof_phased: a sharded prover proves single-phase circuits only");
    if (p->N > 1 && p->shard_world > 1) return dh_fail(p->ctx, DEHALO_ERR_UNSUPPORTED, "create_proof_multi: a sharded prover proves one circuit per proof");
    const int rc = ProofRun(*p, transcript, rng).run(advice, instances, instance_lens, num_instance_columns, flags, synth_in, synth_info, fn, user);
    if (rc) {      // leave nothing of this proof in flight on either context
        (void)hipStreamSynchronize(p->ctx->stream.get());
        if (p->side) (void)hipStreamSynchronize(p->side->stream.get());
    }
    return rc;
}

}   // namespace

extern "C" int dehalo_prover_create(dehalo_ctx* ctx, dehalo_ctx* side_ctx, const dehalo_params* params, const dehalo_pk* pk, dehalo_prover** out) {
    return dehalo_prover_create_multi(ctx, side_ctx, params, pk, 1, out);
}

extern "C" int dehalo_prover_create_multi(dehalo_ctx* ctx, dehalo_ctx* side_ctx, const dehalo_params* params, const dehalo_pk* pk, uint32_t num_circuits, dehalo_prover** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !params || !pk || !out) return dh_fail(ctx, DEHALO_ERR_INVALID, "prover_create: null argument");
        if (!num_circuits) return dh_fail(ctx, DEHALO_ERR_INVALID, "prover_create_multi: no circuit");
        if (params->k != pk->k || params->curve != pk->curve) return dh_fail(ctx, DEHALO_ERR_INVALID, "prover_create: params and proving key disagree on k / curve");
        if (side_ctx && (side_ctx == ctx || side_ctx->device != ctx->device)) return dh_fail(ctx, DEHALO_ERR_INVALID, "prover_create: the side context must be another context of the same device");
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        std::unique_ptr<dehalo_prover> p(new dehalo_prover);
        TRY(p->init(ctx, side_ctx, params, pk, num_circuits));
        *out = p.release();
        return 0;
    });
}

extern "C" int dehalo_prover_release(dehalo_prover* p) {
    return dh_guard(p ? p->ctx : nullptr, [&]() -> int {
        if (!p) return 0;
        (void)hipSetDevice(p->ctx->device);
        (void)hipStreamSynchronize(p->ctx->stream.get());
        if (p->side) (void)hipStreamSynchronize(p->side->stream.get());
        delete p;
        return 0;
    });
}

extern "C" int dehalo_create_proof(dehalo_prover* p, const uint64_t* advice, const uint64_t* const* instances, const size_t* instance_lens, uint32_t num_instance_columns,
                                   dehalo_rng* rng, dehalo_transcript* transcript, uint32_t flags) {
    return dh_guard(p ? p->ctx : nullptr, [&]() -> int {
        if (!p || !transcript) return DEHALO_ERR_INVALID;
        if (p->N > 1) return dh_fail(p->ctx, DEHALO_ERR_INVALID, "create_proof: the prover was made for several circuits: use dehalo_create_proof_multi");
        return prove(p, &advice, instances, instance_lens, num_instance_columns, rng, transcript, flags, nullptr, nullptr);
    });
}

extern "C" int dehalo_create_proof_multi(dehalo_prover* p, const uint64_t* const* advice, const uint64_t* const* instances, const size_t* instance_lens,
                                         uint32_t num_instance_columns, uint32_t num_circuits, dehalo_rng* rng, dehalo_transcript* transcript, uint32_t flags) {
    return dh_guard(p ? p->ctx : nullptr, [&]() -> int {
        if (!p || !transcript) return DEHALO_ERR_INVALID;
        if (!num_circuits || num_circuits != p->N) return dh_fail(p->ctx, DEHALO_ERR_INVALID, "create_proof_multi: num_circuits differs from the prover's");
        if (!advice) return dh_fail(p->ctx, DEHALO_ERR_INVALID, "null advice");
        return prove(p, advice, instances, instance_lens, num_instance_columns, rng, transcript, flags, nullptr, nullptr);
    });
}

extern "C" int dehalo_create_proof_phased(dehalo_prover* p, dehalo_advice_fn fn, void* user, const uint64_t* const* instances, const size_t* instance_lens,
                                          uint32_t num_instance_columns, dehalo_rng* rng, dehalo_transcript* transcript, uint32_t flags) {
    return dh_guard(p ? p->ctx : nullptr, [&]() -> int {
        if (!p || !transcript) return DEHALO_ERR_INVALID;
        if (!fn) return dh_fail(p->ctx, DEHALO_ERR_INVALID, "create_proof_phased: null advice callback");
        return prove(p, nullptr, instances, instance_lens, num_instance_columns, rng, transcript, flags, nullptr, nullptr, fn, user);
    });
}

extern "C" int dehalo_prover_set_shard(dehalo_prover* p, uint32_t rank, uint32_t world, dehalo_gather_fn gather, void* user) {
    return dh_guard(p ? p->ctx : nullptr, [&]() -> int {
        if (!p || world == 0 || rank >= world || (world > 1 && !gather)) return DEHALO_ERR_INVALID;
        if (world > 1 && p->nph > 1) return dh_fail(p->ctx, DEHALO_ERR_UNSUPPORTED, "prover_set_shard: the key has later-phase advice columns");
        if (world > 1 && p->N > 1) return dh_fail(p->ctx, DEHALO_ERR_UNSUPPORTED, "prover_set_shard: the prover was made for several circuits");
        p->shard_rank = rank; p->shard_world = world; p->shard_gather = world > 1 ? gather : nullptr; p->shard_user = user;
        return 0;
    });
}

extern "C" int dehalo_prover_set_multiopen(dehalo_prover* p, int multiopen) {
    return dh_guard(p ? p->ctx : nullptr, [&]() -> int {
        if (!p) return DEHALO_ERR_INVALID;
        if (p->ipa) return dh_fail(p->ctx, DEHALO_ERR_UNSUPPORTED, "prover_set_multiopen: a prover over ParamsIPA has one multiopen");
        if (multiopen != DEHALO_MULTIOPEN_GWC && multiopen != DEHALO_MULTIOPEN_SHPLONK) return dh_fail(p->ctx, DEHALO_ERR_INVALID, "prover_set_multiopen: unknown multiopen");
        std::lock_guard<std::mutex> lk(p->mu);
        if (multiopen == DEHALO_MULTIOPEN_SHPLONK) {
            std::lock_guard<std::recursive_mutex> lc(p->ctx->mu);
            (void)hipSetDevice(p->ctx->device);
            TRY(p->alloc_shplonk());
        }
        p->multiopen = multiopen;
        return 0;
    });
}

extern "C" size_t dehalo_prover_proof_size(const dehalo_prover* p) { return p ? p->proof_size() : 0; }

extern "C" int dehalo_prover_last_timings(const dehalo_prover* p, double out[8]) {
    return dh_guard(p ? p->ctx : nullptr, [&]() -> int {
        if (!p || !out) return DEHALO_ERR_INVALID;
        memcpy(out, p->timings, sizeof p->timings);
        return 0;
    });
}

extern "C" int dehalo_create_proof_circuit(dehalo_prover* p, const dehalo_circuit_inputs* in, dehalo_synthesis_info* info, const uint64_t* const* instances,
                                           const size_t* instance_lens, uint32_t num_instance_columns, dehalo_rng* rng, dehalo_transcript* transcript) {
    return dh_guard(p ? p->ctx : nullptr, [&]() -> int {
        if (!p || !transcript || !in) return DEHALO_ERR_INVALID;
        return prove(p, nullptr, instances, instance_lens, num_instance_columns, rng, transcript, 0, in, info);
    });
}

namespace {
// proof i on prover i mod num_provers, one library thread per prover; `one` makes proof i on prover p into `tr`
template <class One>
int proofs_on_threads(dehalo_prover* const* provers, uint32_t num_provers, uint32_t count, uint8_t* const* proofs_out, size_t proof_cap, size_t* proof_lens, One one) {
    for (uint32_t i = 0; i < num_provers; i++)
        if (!provers[i]) return DEHALO_ERR_INVALID;
    std::vector<int> rcs(num_provers, 0);
    auto work = [&](uint32_t t) {
        dehalo_prover* p = provers[t];
        for (uint32_t i = t; i < count && !rcs[t]; i += num_provers) {
            dehalo_transcript tr;
            tr.init(p->pk->curve);
            int rc = one(p, i, &tr);
            if (!rc && tr.proof.size() > proof_cap) rc = dh_fail(p->ctx, DEHALO_ERR_INVALID, "create_proofs: proof buffer too small");
            if (!rc) {
                memcpy(proofs_out[i], tr.proof.data(), tr.proof.size());
                proof_lens[i] = tr.proof.size();
            }
            rcs[t] = rc;
        }
    };
    std::vector<std::thread> th;
    for (uint32_t t = 1; t < num_provers; t++) th.emplace_back(work, t);
    work(0);
    for (auto& t : th) t.join();
    for (int rc : rcs)
        if (rc) return rc;
    return 0;
}
}   // namespace

extern "C" int dehalo_create_proofs(dehalo_prover* const* provers, uint32_t num_provers, const uint64_t* const* advice, uint32_t count, dehalo_rng* rngs, uint32_t flags,
                                    uint8_t* const* proofs_out, size_t proof_cap, size_t* proof_lens) {
    return dh_guard(nullptr, [&]() -> int {
        if (!provers || !num_provers || (count && (!advice || !proofs_out || !proof_lens))) return DEHALO_ERR_INVALID;
        for (uint32_t i = 0; i < num_provers; i++)
            if (provers[i] && (provers[i]->nph > 1 || provers[i]->N > 1))
                return dh_fail(provers[i]->ctx, DEHALO_ERR_UNSUPPORTED, provers[i]->N > 1 ? "create_proofs: the prover was made for several circuits" : "create_proofs: the key has later-phase advice columns");
        return proofs_on_threads(provers, num_provers, count, proofs_out, proof_cap, proof_lens, [&](dehalo_prover* p, uint32_t i, dehalo_transcript* tr) {
            return dehalo_create_proof(p, advice[i], nullptr, nullptr, p->I ? p->I : 0, rngs ? &rngs[i] : nullptr, tr, flags);
        });
    });
}

// the same with every proof's circuit synthesized inside its call (dehalo_create_proof_circuit): inputs[i] -> proof i
extern "C" int dehalo_create_proofs_circuit(dehalo_prover* const* provers, uint32_t num_provers, const dehalo_circuit_inputs* inputs, uint32_t count, dehalo_rng* rngs,
                                            uint8_t* const* proofs_out, size_t proof_cap, size_t* proof_lens) {
    return dh_guard(nullptr, [&]() -> int {
        if (!provers || !num_provers || (count && (!inputs || !proofs_out || !proof_lens))) return DEHALO_ERR_INVALID;
        for (uint32_t i = 0; i < num_provers; i++)
            if (provers[i] && (provers[i]->nph > 1 || provers[i]->N > 1))
                return dh_fail(provers[i]->ctx, DEHALO_ERR_UNSUPPORTED, provers[i]->N > 1 ? "create_proofs_circuit: the prover was made for several circuits" : "create_proofs_circuit: the key has later-phase advice columns");
        return proofs_on_threads(provers, num_provers, count, proofs_out, proof_cap, proof_lens, [&](dehalo_prover* p, uint32_t i, dehalo_transcript* tr) {
            return dehalo_create_proof_circuit(p, &inputs[i], nullptr, nullptr, nullptr, p->I ? p->I : 0, rngs ? &rngs[i] : nullptr, tr);
        });
    });
}
