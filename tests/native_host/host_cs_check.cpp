// host_cs_check.cpp -- the constraint system on the host (csrc/plonk_host.hpp: no HIP headers) with the Challenge API: what HostCS::load accepts and refuses,
// what every function that switches over node kinds makes of a challenge, the encoding hashed into the substitute transcript_repr, and the programs the graph
// builders emit.  A program of its own, built by g++ with ASan + UBSan (make host_cs_check), run by tests/test_phases_host.py.  Prints one line per check; exits 1
// at the first that fails.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../delay-encryption-in-halo2_amd/csrc/plonk_host.hpp"

namespace {

int checks = 0;
void expect(bool ok, const char* what) {
    checks++;
    if (!ok) { std::printf("FAILED: %s\n", what); std::exit(1); }
    std::printf("ok: %s\n", what);
}

// q (r - (a0 + c0 a1)) with r in phase 1; a lookup (a0 + c0 a1) in (t0 + c0 t1); one gate of c1 alone
struct Circuit {
    std::vector<dehalo_expr_node> nodes;
    std::vector<uint64_t> constants = {2, 0, 0, 0};
    std::vector<uint32_t> gates, lens = {1}, lin, ltab;
    std::vector<dehalo_column_query> aq = {{DEHALO_COLUMN_ADVICE, 0, 0}, {DEHALO_COLUMN_ADVICE, 1, 0}, {DEHALO_COLUMN_ADVICE, 2, 0}}, fq = {{DEHALO_COLUMN_FIXED, 0, 0}};
    std::vector<uint8_t> aph = {0, 0, 1}, cph = {0, 1};
    uint32_t n(uint32_t kind, uint32_t a = 0, uint32_t b = 0, int32_t rot = 0) { nodes.push_back(dehalo_expr_node{kind, a, b, rot}); return (uint32_t)nodes.size() - 1; }
    uint32_t c0a1 = 0, table = 0, c0_again = 0, c1 = 0, fixed_sum = 0;
    Circuit() {
        const uint32_t q = n(DEHALO_EXPR_FIXED, 0), a0 = n(DEHALO_EXPR_ADVICE, 0), a1 = n(DEHALO_EXPR_ADVICE, 1), r = n(DEHALO_EXPR_ADVICE, 2);
        const uint32_t c0 = n(DEHALO_EXPR_CHALLENGE, 0);
        c0a1 = n(DEHALO_EXPR_PRODUCT, c0, a1);
        const uint32_t rlc = n(DEHALO_EXPR_SUM, a0, c0a1);
        gates.push_back(n(DEHALO_EXPR_PRODUCT, q, n(DEHALO_EXPR_SUM, r, n(DEHALO_EXPR_NEGATED, rlc))));
        c1 = n(DEHALO_EXPR_CHALLENGE, 1);
        gates.push_back(c1);
        const uint32_t t0 = n(DEHALO_EXPR_FIXED, 1), t1 = n(DEHALO_EXPR_FIXED, 2);
        c0_again = n(DEHALO_EXPR_CHALLENGE, 0);
        table = n(DEHALO_EXPR_SUM, t0, n(DEHALO_EXPR_PRODUCT, c0_again, t1));
        fixed_sum = n(DEHALO_EXPR_SUM, t0, n(DEHALO_EXPR_SCALED, t1, 0));
        lin.push_back(rlc);
        ltab.push_back(table);
    }
    dehalo_constraint_system view() const {
        dehalo_constraint_system d{};
        d.num_advice = 3; d.num_fixed = 3;
        d.nodes = nodes.data(); d.num_nodes = (uint32_t)nodes.size();
        d.constants = constants.data(); d.num_constants = 1;
        d.gates = gates.data(); d.num_gates = (uint32_t)gates.size();
        d.lookup_lens = lens.data(); d.num_lookups = 1; d.lookup_inputs = lin.data(); d.lookup_tables = ltab.data();
        d.advice_queries = aq.data(); d.num_advice_queries = (uint32_t)aq.size();
        d.fixed_queries = fq.data(); d.num_fixed_queries = (uint32_t)fq.size();
        d.advice_phases = aph.data(); d.challenge_phases = cph.data(); d.num_challenges = (uint32_t)cph.size();
        return d;
    }
};

std::string load_error(const Circuit& c, bool* unsupported = nullptr) {
    const dehalo_constraint_system d = c.view();
    HostCS cs;
    const std::string e = cs.load(&d);
    if (unsupported) *unsupported = cs.unsupported;
    return e;
}

}   // namespace

int main() {
    Circuit c;
    dehalo_constraint_system d = c.view();
    HostCS cs;
    expect(cs.load(&d).empty(), "a two-phase circuit with two challenges loads");
    expect(cs.num_phases == 2 && cs.challenge_phase.size() == 2 && cs.phased() && cs.has_challenge_node(), "phases and challenges are kept");
    expect(cs.expr_degree(c.c1) == 0 && cs.expr_degree(c.c0a1) == 1 && cs.expr_degree(cs.gates[0]) == 2, "a challenge has degree 0");
    expect(cs.degree() == 4 && cs.blinding_factors() == 5, "degree and blinding factors are those of the circuit with constants for challenges");
    expect(cs.expr_equal(c.c0_again, c.c0a1 - 1) && !cs.expr_equal(c.c1, c.c0_again), "challenges are equal by index");
    expect(!cs.expr_fixed_only(c.table) && cs.expr_fixed_only(c.fixed_sum), "a table that reads a challenge does not belong to the key");
    std::vector<uint32_t> cols;
    cs.expr_fixed_columns(c.table, cols);
    expect(cols == std::vector<uint32_t>({1, 2}), "the fixed columns under a challenge product are found");

    // the programs: a challenge is a source of its own, never a calculation
    const HostField* f = host_field(DEHALO_FIELD_BN254_FR);
    const GateCheckProgram chk = gate_check_graph(cs, f);
    bool reads = false, root1 = false;
    for (auto& k : chk.g.calcs) {
        reads = reads || (k.a.kind == DEHALO_SRC_CHALLENGE && k.a.index == 0) || (k.b.kind == DEHALO_SRC_CHALLENGE && k.b.index == 0);
        root1 = root1 || (k.op == DEHALO_CALC_STORE && k.a.kind == DEHALO_SRC_CHALLENGE && k.a.index == 1);
    }
    expect(reads && root1 && chk.root_of.size() == chk.g.calcs.size(), "the checking program reads DEHALO_SRC_CHALLENGE sources");
    const GraphBuilder lk = lookup_table_value_graph(cs, cs.lookups[0], f), cg = custom_gates_graph(cs, f), cp = compress_graph(cs, cs.lookups[0].tables, f);
    auto uses = [](const GraphBuilder& g) {
        for (auto& k : g.calcs) {
            if (k.a.kind == DEHALO_SRC_CHALLENGE || k.b.kind == DEHALO_SRC_CHALLENGE) return true;
            for (auto& p : k.parts) if (p.kind == DEHALO_SRC_CHALLENGE) return true;
        }
        return false;
    };
    expect(uses(lk) && uses(cg) && uses(cp), "the lookup, gate and compression programs read them too");

    // encoding: phases and challenges appended only when there are any
    std::vector<uint8_t> with, plain_null, plain_zero;
    cs.encode(with);
    Circuit one;      // the same circuit in one phase without challenges: challenge nodes replaced by the constant
    for (auto& nd : one.nodes) if (nd.kind == DEHALO_EXPR_CHALLENGE) nd = dehalo_expr_node{DEHALO_EXPR_CONSTANT, 0, 0, 0};
    one.aph = {0, 0, 0}; one.cph.clear();
    dehalo_constraint_system d1 = one.view();
    HostCS a, b;
    expect(a.load(&d1).empty() && !a.phased() && !a.has_challenge_node(), "an all-zero phase array is one phase");
    d1.advice_phases = nullptr; d1.challenge_phases = nullptr;
    expect(b.load(&d1).empty(), "null phase arrays are one phase");
    a.encode(plain_zero); b.encode(plain_null);
    expect(plain_zero == plain_null && with.size() == plain_null.size() + 3 + 4 + 2, "one phase encodes as before; phases add their bytes at the end");

    // refusals
    bool unsup = false;
    { Circuit x; x.aph = {0, 0, 2}; expect(!load_error(x, &unsup).empty() && !unsup, "a phase gap is refused"); }
    { Circuit x; x.aph = {0, 3, 1}; expect(!load_error(x, &unsup).empty() && unsup, "a fourth phase is unsupported"); }
    { Circuit x; x.cph = {0, 2}; expect(!load_error(x, &unsup).empty() && !unsup, "a challenge after a phase without columns is refused"); }
    { Circuit x; x.nodes[x.c1].a = 2; expect(!load_error(x, &unsup).empty() && !unsup, "a challenge index out of range is refused"); }
    { Circuit x; dehalo_constraint_system dx = x.view(); dx.challenge_phases = nullptr; HostCS h; expect(!h.load(&dx).empty(), "a challenge count without phases is refused"); }
    std::printf("%d checks passed\n", checks);
    return 0;
}
