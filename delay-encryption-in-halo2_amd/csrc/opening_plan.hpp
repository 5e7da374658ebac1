// opening_plan.hpp -- which value goes where in create_proof's last two phases, from the circuit's shape alone (host only: no HIP header, no device pointer;
// tests/native_host/opening_plan_check.cpp prints it under ASan + UBSan and tests/test_opening_plan.py compares it with the CPU restatement's, symbol by symbol).
// The transcript's order of the evaluations [UPSTREAM halo2_proofs @ v2023_04_20 plonk/prover.rs: instance (IPA), advice, fixed, vanishing random_eval,
// permutation (sigma; products), lookups, shuffles (halo2_proofs v0.3.0)], the opening queries in upstream's order [UPSTREAM permutation::Constructed::open, lookup::Evaluated::open,
// pk.permutation.open, vanishing::Evaluated::open] and the three multiopens' views of that one list: grouped by point (gwc/prover.rs), and as intermediate
// sets (poly/ipa/multiopen.rs and poly/kzg/multiopen/shplonk.rs construct_intermediate_sets).  A polynomial is named by its id in the numbering below.
// One proof over `circuits` witnesses of one key (upstream's slice of circuits): every per-circuit block below comes circuit after circuit, and what the key
// owns (fixed, sigma) or the proof has once (the pieces of h, the random polynomial, the folded h) appears once.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

// what the plan reads of a circuit (the prover fills it from HostCS and the domain)
struct OpeningShape {
    uint32_t k = 0, A = 0, num_fixed = 0, I = 0, L = 0, S = 0, npc = 0, bf = 0, pieces = 0;      // npc: permutation columns; pieces: of the quotient h
    bool query_instance = false;      // the scheme's QUERY_INSTANCE: true under IPA
    uint32_t circuits = 1;            // witnesses proven in the one proof (KZG only)
    uint32_t shuffles = 0;            // shuffle arguments: one grand product each
    struct Query { uint32_t column; int32_t rotation; };
    std::vector<Query> advice_q, fixed_q, instance_q;
};

struct OpeningPlan {
    static constexpr size_t MAX_ROTATIONS = 32;      // the evaluation's masks are 32 bits wide
    enum Multiopen { GWC, SHPLONK, IPA };
    std::string error;      // not empty: the shape is refused and nothing below is filled
    uint32_t k = 0;         // (an IPA proof has 2 k rounds)

    // ---- layouts
    // the prover's own columns (values, then coefficient forms): [advice A | permuted (input, table) x L | permutation products S | lookup products L | shuffle products H | random 1]
    // With N circuits every block but the last holds circuit 0's columns, then circuit 1's ...: [advice A x N | permuted 2 L x N | (products S, products L,
    // products H) x N | random 1].  o_adv .. o_sz are circuit 0's; adv(c) .. sz(c) circuit c's.  A commitment phase is one run of columns: advice, permuted, products + random.
    uint32_t circuits = 1, A = 0, L = 0, S = 0, H = 0;
    uint32_t o_adv = 0, o_perm = 0, o_pz = 0, o_lz = 0, o_sz = 0, o_rand = 0, NC = 0;
    uint32_t adv(uint32_t c) const { return o_adv + c * A; }
    uint32_t perm(uint32_t c) const { return o_perm + c * 2 * L; }
    uint32_t pz(uint32_t c) const { return o_pz + c * (S + L + H); }
    uint32_t lz(uint32_t c) const { return o_lz + c * (S + L + H); }
    uint32_t sz(uint32_t c) const { return o_sz + c * (S + L + H); }
    // the order the products' commitments are written in: every circuit's permutation products, then every circuit's lookup products, then every circuit's
    // shuffle products, then the random polynomial
    // (as offsets from o_pz).  The identity with one circuit
    std::vector<uint32_t> product_order;
    // one blind per commitment: [the columns above, in their order | h pieces | folded h | f | default x max(I, 1)].  Fixed, sigma and instance
    // columns are committed under the default blind (bi_def); f is the IPA multiopen's own polynomial.  KZG commitments are not hiding: the slots exist, nobody reads them.
    uint32_t bi_adv = 0, bi_perm = 0, bi_prod = 0, bi_rand = 0, bi_h = 0, bi_hfold = 0, bi_f = 0, bi_def = 0, bi_count = 0;
    // polynomial ids: [NC columns | fixed | sigma | h pieces | instance (only when queried)]; the evaluation reads these num_polys.  One more id, p_hfold = num_polys,
    // names the folded quotient h = sum_i x^(n i) h_i: it is opened but never evaluated (its value comes from the pieces')
    uint32_t p_fixed = 0, p_sigma = 0, p_hpiece = 0, p_instance = 0, num_polys = 0, p_hfold = 0;

    // ---- evaluations: slot = (index of the rotation in rots) * num_polys + polynomial id
    std::vector<int32_t> rots;      // sorted, distinct; always holds the prover's own 0, 1, -1, -(bf + 1)
    size_t eval_count = 0, hpiece0 = 0;      // rots.size() * num_polys; the slot of h piece 0 at rotation 0
    std::vector<int64_t> instance_write, write;      // the slots the transcript takes, in its order: instance_write first
    std::vector<uint32_t> eval_wanted;      // per polynomial id: the rotations (bits, in rots' order) anyone reads its value at
    std::vector<uint8_t> eval_wanted8;      // the same as bytes where rots.size() <= 4 (the four-point evaluation), else empty

    // ---- the opening queries in upstream's order; eval: the slot of the value, -1 for the folded h
    struct Query { int32_t rot; uint32_t poly; int64_t eval; uint32_t blind; };
    std::vector<Query> queries;
    // GWC: the queries by rotation, groups in order of first appearance, members in query order
    struct Group { int32_t rot; std::vector<uint32_t> polys; std::vector<int64_t> evals; };
    std::vector<Group> groups;
    // construct_intermediate_sets: the distinct commitments in order of first appearance; points numbered by first appearance (point_rot: point -> rotation); a
    // commitment's point set is the ascending list of its points, sets numbered in order of first appearance over the commitments.  evals: per point of the
    // commitment's set, in the set's order, the slot of its first query there.  Commitments are told apart by polynomial id -- what (pointer, blind) told apart
    // before: no polynomial has two blinds, and distinct polynomials have distinct pointers.  (Upstream's SHPLONK verifier compares points instead, so two
    // identical fixed columns would make one commitment there.)
    struct Commitment { uint32_t poly, blind, set; std::vector<int64_t> evals; };
    std::vector<Commitment> commitments;
    std::vector<std::vector<uint32_t>> point_sets;
    std::vector<int32_t> point_rot;
    std::vector<std::vector<uint32_t>> set_members;      // per set: its commitments (indices into `commitments`), in order

    size_t rot_index(int32_t r) const { return (size_t)(std::find(rots.begin(), rots.end(), r) - rots.begin()); }
    int64_t slot(uint32_t poly, int32_t r) const { return (int64_t)(rot_index(r) * num_polys + poly); }

    size_t proof_size(Multiopen mo) const {
        const size_t points = (size_t)NC + p_instance - p_hpiece;      // every column and the pieces of h
        if (mo != IPA) return 32 * (points + (mo == SHPLONK ? 2 : groups.size()) + write.size());      // SHPLONK: h and h'
        return 32 * (points + 2 + 2 * (size_t)k + instance_write.size() + write.size() + point_sets.size() + 2);
    }

    OpeningPlan() = default;
    explicit OpeningPlan(const OpeningShape& sh) : k(sh.k), circuits(sh.circuits), A(sh.A), L(sh.L), S(sh.S), H(sh.shuffles) {
        const uint32_t N = sh.circuits;
        const int32_t last = -(int32_t)(sh.bf + 1);
        if (N == 0) { error = "no circuit"; return; }
        if (N > 1 && sh.query_instance) { error = "several circuits in one proof: KZG only"; return; }
        rots = {0, 1, -1, last};
        for (auto& q : sh.advice_q) rots.push_back(q.rotation);
        for (auto& q : sh.fixed_q) rots.push_back(q.rotation);
        if (sh.query_instance) for (auto& q : sh.instance_q) rots.push_back(q.rotation);
        std::sort(rots.begin(), rots.end());
        rots.erase(std::unique(rots.begin(), rots.end()), rots.end());
        if (rots.size() > MAX_ROTATIONS) {      // (rots holds the prover's own four rotations too)
            error = std::to_string(rots.size()) + " distinct opening rotations: more than " + std::to_string(MAX_ROTATIONS);
            rots.clear();
            return;
        }
        o_adv = 0; o_perm = N * A; o_pz = o_perm + N * 2 * L; o_lz = o_pz + S; o_sz = o_lz + L; o_rand = o_pz + N * (S + L + H); NC = o_rand + 1;
        for (uint32_t c = 0; c < N; c++) for (uint32_t s = 0; s < S; s++) product_order.push_back(pz(c) + s - o_pz);
        for (uint32_t c = 0; c < N; c++) for (uint32_t l = 0; l < L; l++) product_order.push_back(lz(c) + l - o_pz);
        for (uint32_t c = 0; c < N; c++) for (uint32_t j = 0; j < H; j++) product_order.push_back(sz(c) + j - o_pz);
        product_order.push_back(o_rand - o_pz);
        bi_adv = o_adv; bi_perm = o_perm; bi_prod = o_pz; bi_rand = o_rand; bi_h = bi_rand + 1; bi_hfold = bi_h + sh.pieces; bi_f = bi_hfold + 1; bi_def = bi_f + 1;
        bi_count = bi_def + std::max<uint32_t>(sh.I, 1);
        p_fixed = NC; p_sigma = p_fixed + sh.num_fixed; p_hpiece = p_sigma + sh.npc; p_instance = p_hpiece + sh.pieces;
        num_polys = p_instance + (sh.query_instance ? sh.I : 0);
        p_hfold = num_polys;
        eval_count = rots.size() * num_polys;
        hpiece0 = (size_t)slot(p_hpiece, 0);

        auto wr = [&](uint32_t poly, int32_t r) { write.push_back(slot(poly, r)); };
        for (uint32_t c = 0; c < N; c++)
            for (auto& q : sh.advice_q) wr(adv(c) + q.column, q.rotation);
        for (auto& q : sh.fixed_q) wr(p_fixed + q.column, q.rotation);
        wr(o_rand, 0);                                                  // vanishing: random_eval
        for (uint32_t j = 0; j < sh.npc; j++) wr(p_sigma + j, 0);      // pk.permutation.evaluate
        for (uint32_t c = 0; c < N; c++)
            for (uint32_t s = 0; s < S; s++) {                          // permutation products
                wr(pz(c) + s, 0);
                wr(pz(c) + s, 1);
                if (s != S - 1) wr(pz(c) + s, last);
            }
        for (uint32_t c = 0; c < N; c++)
            for (uint32_t l = 0; l < L; l++) {                          // lookups
                const uint32_t zc = lz(c) + l, ai = perm(c) + 2 * l, ti = ai + 1;
                wr(zc, 0); wr(zc, 1); wr(ai, 0); wr(ai, -1); wr(ti, 0);
            }
        for (uint32_t c = 0; c < N; c++)
            for (uint32_t j = 0; j < H; j++) { wr(sz(c) + j, 0); wr(sz(c) + j, 1); }      // shuffles

        auto qu = [&](int32_t r, uint32_t poly, uint32_t blind) { queries.push_back({r, poly, slot(poly, r), blind}); };
        if (sh.query_instance)      // under IPA the instance columns' queries come first, and so do their values in the transcript
            for (auto& q : sh.instance_q) {
                qu(q.rotation, p_instance + q.column, bi_def);
                instance_write.push_back(queries.back().eval);
            }
        for (uint32_t c = 0; c < N; c++) {      // (a column of the prover's own has the blind of its number)
            for (auto& q : sh.advice_q) qu(q.rotation, adv(c) + q.column, adv(c) + q.column);
            for (uint32_t s = 0; s < S; s++) {                              // permutation::Constructed::open
                qu(0, pz(c) + s, pz(c) + s);
                qu(1, pz(c) + s, pz(c) + s);
            }
            for (uint32_t s = S > 1 ? S - 1 : 0; s-- > 0;) qu(last, pz(c) + s, pz(c) + s);      // sets.iter().rev().skip(1)
            for (uint32_t l = 0; l < L; l++) {                              // lookup::Evaluated::open
                const uint32_t zc = lz(c) + l, ai = perm(c) + 2 * l, ti = ai + 1;
                qu(0, zc, zc); qu(0, ai, ai); qu(0, ti, ti); qu(-1, ai, ai); qu(1, zc, zc);
            }
            for (uint32_t j = 0; j < H; j++) { qu(0, sz(c) + j, sz(c) + j); qu(1, sz(c) + j, sz(c) + j); }      // shuffle::Evaluated::open
        }
        for (auto& q : sh.fixed_q) qu(q.rotation, p_fixed + q.column, bi_def);
        for (uint32_t j = 0; j < sh.npc; j++) qu(0, p_sigma + j, bi_def);      // pk.permutation.open
        queries.push_back({0, p_hfold, -1, bi_hfold});                          // vanishing::Evaluated::open: h, then the random polynomial
        qu(0, o_rand, bi_rand);

        // (all three views are of the whole list.  Only a KZG prover opens by groups, and its list has no instance query: QUERY_INSTANCE is false there)
        std::vector<std::vector<uint32_t>> cpoints;      // per commitment: the point of each of its queries, in query order
        std::vector<std::vector<int64_t>> cevals;
        for (auto& q : queries) {
            auto g = std::find_if(groups.begin(), groups.end(), [&](const Group& gg) { return gg.rot == q.rot; });
            if (g == groups.end()) g = groups.insert(g, Group{q.rot, {}, {}});
            g->polys.push_back(q.poly);
            g->evals.push_back(q.eval);
            const uint32_t pi = (uint32_t)(std::find(point_rot.begin(), point_rot.end(), q.rot) - point_rot.begin());
            if (pi == point_rot.size()) point_rot.push_back(q.rot);
            size_t ci = 0;
            while (ci < commitments.size() && commitments[ci].poly != q.poly) ci++;
            if (ci == commitments.size()) {
                commitments.push_back({q.poly, q.blind, 0, {}});
                cpoints.push_back({});
                cevals.push_back({});
            }
            cpoints[ci].push_back(pi);
            cevals[ci].push_back(q.eval);
        }
        for (size_t ci = 0; ci < commitments.size(); ci++) {
            std::vector<uint32_t> ps = cpoints[ci];
            std::sort(ps.begin(), ps.end());
            ps.erase(std::unique(ps.begin(), ps.end()), ps.end());
            const size_t si = (size_t)(std::find(point_sets.begin(), point_sets.end(), ps) - point_sets.begin());
            if (si == point_sets.size()) { point_sets.push_back(ps); set_members.push_back({}); }
            commitments[ci].set = (uint32_t)si;
            set_members[si].push_back((uint32_t)ci);
            for (uint32_t pt : ps) commitments[ci].evals.push_back(cevals[ci][(size_t)(std::find(cpoints[ci].begin(), cpoints[ci].end(), pt) - cpoints[ci].begin())]);
        }

        eval_wanted.assign(num_polys, 0);
        auto want = [&](int64_t i) { if (i >= 0) eval_wanted[(size_t)i % num_polys] |= 1u << ((size_t)i / num_polys); };
        for (int64_t i : instance_write) want(i);
        for (int64_t i : write) want(i);
        for (auto& q : queries) want(q.eval);
        for (uint32_t i = 0; i < sh.pieces; i++) want((int64_t)hpiece0 + i);      // the pieces of h at x: the folded quotient's value
        if (rots.size() <= 4) eval_wanted8.assign(eval_wanted.begin(), eval_wanted.end());
    }
};
