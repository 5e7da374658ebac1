// shuffle_cs_check.cpp -- the shuffle argument on the host (csrc/plonk_host.hpp, csrc/opening_plan.hpp: no HIP headers).  A program of its own, built by g++ with
// ASan + UBSan (make shuffle_cs_check), run by tests/test_shuffle.py in two modes:
//   cs      what HostCS::load accepts and refuses of the shuffle fields, the degree rule, the encoding hashed into the substitute transcript_repr, the two programs
//           of a shuffle.  Prints one line per check; exits 1 at the first that fails.
//   plan    the prover's opening plan for shapes with shuffles, one JSON object per input line
//             circuits shuffles  k A num_fixed I L S npc bf pieces query_instance  n_advice_q (column rotation)*  n_fixed_q (column rotation)*  n_instance_q (..)*
//           with every polynomial spelled by name -- [name, circuit, index] for a circuit's own, [name, index] / [name] for what the proof has once -- and every
//           evaluation as [polynomial, rotation].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../delay-encryption-in-halo2_amd/csrc/opening_plan.hpp"
#include "../../delay-encryption-in-halo2_amd/csrc/plonk_host.hpp"

namespace {

int checks = 0;
void expect(bool ok, const char* what) {
    checks++;
    if (!ok) { std::printf("FAILED: %s\n", what); std::exit(1); }
    std::printf("ok: %s\n", what);
}

// advice a0, a1, a2 (a2 in phase 1), fixed q, challenge c0; a gate q (a0 - a1); shuffle 0: [a0, a1] ~ [a1, a0]; shuffle 1: [a0 + c0 a1] ~ [a2]
struct Circuit {
    std::vector<dehalo_expr_node> nodes;
    std::vector<uint64_t> constants = {3, 0, 0, 0};
    std::vector<uint32_t> gates, slens = {2, 1}, sin, stab;
    std::vector<dehalo_column_query> aq = {{DEHALO_COLUMN_ADVICE, 0, 0}, {DEHALO_COLUMN_ADVICE, 1, 0}, {DEHALO_COLUMN_ADVICE, 2, 0}}, fq = {{DEHALO_COLUMN_FIXED, 0, 0}};
    std::vector<uint8_t> aph = {0, 0, 1}, cph = {0};
    uint32_t n(uint32_t kind, uint32_t a = 0, uint32_t b = 0, int32_t rot = 0) { nodes.push_back(dehalo_expr_node{kind, a, b, rot}); return (uint32_t)nodes.size() - 1; }
    uint32_t q = 0, a0 = 0, a1 = 0, a2 = 0, deg2 = 0, deg3 = 0, konst = 0;
    Circuit() {
        q = n(DEHALO_EXPR_FIXED, 0); a0 = n(DEHALO_EXPR_ADVICE, 0); a1 = n(DEHALO_EXPR_ADVICE, 1); a2 = n(DEHALO_EXPR_ADVICE, 2);
        gates.push_back(n(DEHALO_EXPR_PRODUCT, q, n(DEHALO_EXPR_SUM, a0, n(DEHALO_EXPR_NEGATED, a1))));
        const uint32_t c0 = n(DEHALO_EXPR_CHALLENGE, 0);
        const uint32_t rlc = n(DEHALO_EXPR_SUM, a0, n(DEHALO_EXPR_PRODUCT, c0, a1));
        deg2 = n(DEHALO_EXPR_PRODUCT, q, a0);
        deg3 = n(DEHALO_EXPR_PRODUCT, deg2, a1);
        konst = n(DEHALO_EXPR_CONSTANT, 0);
        sin = {a0, a1, rlc};
        stab = {a1, a0, a2};
    }
    dehalo_constraint_system view() const {
        dehalo_constraint_system d{};
        d.num_advice = 3; d.num_fixed = 1;
        d.nodes = nodes.data(); d.num_nodes = (uint32_t)nodes.size();
        d.constants = constants.data(); d.num_constants = 1;
        d.gates = gates.data(); d.num_gates = (uint32_t)gates.size();
        d.advice_queries = aq.data(); d.num_advice_queries = (uint32_t)aq.size();
        d.fixed_queries = fq.data(); d.num_fixed_queries = (uint32_t)fq.size();
        d.advice_phases = aph.data(); d.challenge_phases = cph.data(); d.num_challenges = (uint32_t)cph.size();
        d.shuffle_lens = slens.data(); d.shuffle_inputs = sin.data(); d.shuffle_tables = stab.data(); d.num_shuffles = (uint32_t)slens.size();
        return d;
    }
};

uint32_t degree_of(const Circuit& c) {
    const dehalo_constraint_system d = c.view();
    HostCS cs;
    if (!cs.load(&d).empty()) return 0;
    return cs.degree();
}
bool refused(const dehalo_constraint_system& d) {
    HostCS cs;
    return !cs.load(&d).empty() && !cs.unsupported;
}

int check_cs() {
    Circuit c;
    dehalo_constraint_system d = c.view();
    HostCS cs;
    expect(cs.load(&d).empty(), "a circuit with two shuffles loads");
    expect(cs.shuffles.size() == 2 && cs.shuffles[0].inputs == std::vector<uint32_t>({c.a0, c.a1}) && cs.shuffles[0].tables == std::vector<uint32_t>({c.a1, c.a0}) &&
               cs.shuffles[1].inputs.size() == 1 && cs.shuffles[1].tables == std::vector<uint32_t>({c.a2}) && cs.lookups.empty(),
           "the pairs are kept shuffle by shuffle, inputs and shuffle side apart");
    expect(cs.degree() == 3 && cs.blinding_factors() == 5, "degree-1 sides need 2 + 1; blinding_factors() does not read the shuffles");
    { Circuit x; x.sin[0] = x.deg2; expect(degree_of(x) == 4, "a degree-2 input expression needs 4"); }
    { Circuit x; x.stab[2] = x.deg3; expect(degree_of(x) == 5, "a degree-3 expression on the shuffle side lifts the key's degree to 5"); }
    { Circuit x; x.sin[2] = x.deg3; x.stab[2] = x.deg2; expect(degree_of(x) == 5, "the maximum over both sides, not their sum"); }
    { Circuit x; x.slens = {1}; x.sin = {x.konst}; x.stab = {x.konst}; expect(degree_of(x) == 3, "either side counts as degree 1 at least"); }

    // encoding
    std::vector<uint8_t> with, none_null, none_zero, other;
    cs.encode(with);
    dehalo_constraint_system d0 = c.view();
    d0.num_shuffles = 0;
    HostCS a, b;
    expect(a.load(&d0).empty() && a.shuffles.empty(), "a zero count with arrays given is no shuffle");
    d0.shuffle_lens = nullptr; d0.shuffle_inputs = nullptr; d0.shuffle_tables = nullptr;
    expect(b.load(&d0).empty() && b.shuffles.empty(), "null arrays with a zero count are no shuffle");
    a.encode(none_zero); b.encode(none_null);
    expect(none_zero == none_null && with.size() == none_null.size() + 4 + 4 + (4 + 16) + (4 + 8) && std::equal(none_null.begin(), none_null.end(), with.begin()),
           "without shuffles the encoding is what it was; shuffles add a marker, their count and their pairs at the end");
    { Circuit x; std::swap(x.stab[0], x.stab[1]); const dehalo_constraint_system dx = x.view(); HostCS h; h.load(&dx); h.encode(other); }
    expect(other.size() == with.size() && other != with, "other pairs, another encoding");

    // refusals
    { dehalo_constraint_system x = c.view(); x.shuffle_lens = nullptr; expect(refused(x), "null lengths with a non-zero count are refused"); }
    { dehalo_constraint_system x = c.view(); x.shuffle_inputs = nullptr; expect(refused(x), "null inputs with a non-zero count are refused"); }
    { dehalo_constraint_system x = c.view(); x.shuffle_tables = nullptr; expect(refused(x), "a null shuffle side with a non-zero count is refused"); }
    { Circuit x; x.sin[1] = (uint32_t)x.nodes.size(); expect(refused(x.view()), "an input root out of range is refused"); }
    { Circuit x; x.stab[2] = 0xffffffffu; expect(refused(x.view()), "a shuffle-side root out of range is refused"); }
    { Circuit x; x.slens = {3, 0}; expect(refused(x.view()), "a shuffle without a pair is refused"); }

    // the programs: Horner(0, expressions, theta) + gamma
    const HostField* f = host_field(DEHALO_FIELD_BN254_FR);
    const GraphBuilder gi = shuffle_side_graph(cs, cs.shuffles[0].inputs, f), gs = shuffle_side_graph(cs, cs.shuffles[0].tables, f);
    auto shape_ok = [](const GraphBuilder& g, size_t parts) {
        if (g.calcs.size() < 2) return false;
        const GCalc &h = g.calcs[g.calcs.size() - 2], &last = g.calcs.back();
        return h.op == DEHALO_CALC_HORNER && h.b.kind == DEHALO_SRC_THETA && h.parts.size() == parts && last.op == DEHALO_CALC_ADD && last.b.kind == DEHALO_SRC_GAMMA &&
               last.a.kind == DEHALO_SRC_INTERMEDIATE && last.a.index == h.target;
    };
    expect(shape_ok(gi, 2) && shape_ok(gs, 2) && !(gi.calcs[0].a == gs.calcs[0].a), "a side's program is the theta compression of its expressions, in order, plus gamma");
    const GraphBuilder gc = shuffle_side_graph(cs, cs.shuffles[1].inputs, f);
    bool reads = false;
    for (auto& k : gc.calcs) reads = reads || k.a.kind == DEHALO_SRC_CHALLENGE || k.b.kind == DEHALO_SRC_CHALLENGE;
    expect(reads && shape_ok(gc, 1), "a shuffle expression may read a challenge");
    std::printf("%d checks passed\n", checks);
    return 0;
}

// ---- plan
std::string key(const OpeningPlan& p, uint32_t id) {
    auto one = [](const char* name, uint32_t i) { return std::string("[\"") + name + "\"," + std::to_string(i) + "]"; };
    auto own = [](const char* name, uint32_t c, uint32_t i) { return std::string("[\"") + name + "\"," + std::to_string(c) + "," + std::to_string(i) + "]"; };
    if (id == p.p_hfold) return "[\"h\"]";
    if (id >= p.p_instance) return one("instance", id - p.p_instance);
    if (id >= p.p_hpiece) return one("hpiece", id - p.p_hpiece);
    if (id >= p.p_sigma) return one("sigma", id - p.p_sigma);
    if (id >= p.p_fixed) return one("fixed", id - p.p_fixed);
    if (id == p.o_rand) return "[\"random\"]";
    if (id >= p.o_pz) {
        const uint32_t per = p.S + p.L + p.H, c = (id - p.o_pz) / per, i = (id - p.o_pz) % per;
        return i < p.S ? own("perm_z", c, i) : i < p.S + p.L ? own("lookup_z", c, i - p.S) : own("shuffle_z", c, i - p.S - p.L);
    }
    if (id >= p.o_perm) {
        const uint32_t c = (id - p.o_perm) / (2 * p.L), i = (id - p.o_perm) % (2 * p.L);
        return own(i & 1 ? "lookup_s" : "lookup_a", c, i / 2);
    }
    return own("advice", (id - p.o_adv) / p.A, (id - p.o_adv) % p.A);
}

template <class V, class F>
std::string list(const V& v, F item) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + item(v[i]);
    return s + "]";
}

bool read_queries(std::istream& in, std::vector<OpeningShape::Query>& out) {
    size_t count;
    if (!(in >> count)) return false;
    out.resize(count);
    for (auto& q : out)
        if (!(in >> q.column >> q.rotation)) return false;
    return true;
}

int print_plans() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        OpeningShape sh;
        int qi = 0;
        if (!(in >> sh.circuits >> sh.shuffles >> sh.k >> sh.A >> sh.num_fixed >> sh.I >> sh.L >> sh.S >> sh.npc >> sh.bf >> sh.pieces >> qi) || !read_queries(in, sh.advice_q) ||
            !read_queries(in, sh.fixed_q) || !read_queries(in, sh.instance_q)) {
            fprintf(stderr, "shuffle_cs_check: cannot read the shape \"%s\"\n", line.c_str());
            return 2;
        }
        sh.query_instance = qi != 0;
        const OpeningPlan p(sh);
        if (!p.error.empty()) {
            printf("{\"refused\":\"%s\"}\n", p.error.c_str());
            continue;
        }
        auto K = [&](uint32_t id) { return key(p, id); };
        auto slot = [&](int64_t e) {
            if (e < 0) return std::string("null");
            return "[" + K((uint32_t)((size_t)e % p.num_polys)) + "," + std::to_string(p.rots[(size_t)e / p.num_polys]) + "]";
        };
        std::string s = "{\"NC\":" + std::to_string(p.NC);
        s += ",\"product_order\":" + list(p.product_order, [&](uint32_t o) { return K(p.o_pz + o); });
        s += ",\"write\":" + list(p.write, slot);
        s += ",\"queries\":" + list(p.queries, [&](const OpeningPlan::Query& q) {
                 return "{\"rot\":" + std::to_string(q.rot) + ",\"poly\":" + K(q.poly) + ",\"eval\":" + slot(q.eval) + ",\"blind\":" + std::to_string(q.blind) + "}";
             });
        s += ",\"proof_size\":{\"gwc\":" + std::to_string(p.proof_size(OpeningPlan::GWC)) + ",\"shplonk\":" + std::to_string(p.proof_size(OpeningPlan::SHPLONK)) +
             ",\"ipa\":" + std::to_string(p.proof_size(OpeningPlan::IPA)) + "}}";
        puts(s.c_str());
    }
    return 0;
}

}   // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "cs")) return check_cs();
    if (argc == 2 && !strcmp(argv[1], "plan")) return print_plans();
    fprintf(stderr, "usage: shuffle_cs_check cs | plan\n");
    return 2;
}
