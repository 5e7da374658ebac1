// opening_plan_multi_check.cpp -- the prover's opening plan (csrc/opening_plan.hpp) for a proof over several circuits of one key, printed as JSON; built by g++
// with ASan + UBSan (make opening_plan_multi_check), run by tests/test_multi_circuit.py, which compares every plan with oracle/plonk_oracle.py's lists.
//
// One shape per line, plain integers (opening_plan_check.cpp's line behind the number of circuits):
//   circuits  k A num_fixed I L S npc bf pieces query_instance  n_advice_q (column rotation)*  n_fixed_q (column rotation)*  n_instance_q (column rotation)*
// One JSON object per shape, or {"refused": message}.  A polynomial of a circuit's own is spelled [name, circuit, index]; what the proof has once as the
// single-circuit program spells it.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../delay-encryption-in-halo2_amd/csrc/opening_plan.hpp"

namespace {

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
        const uint32_t c = (id - p.o_pz) / (p.S + p.L), i = (id - p.o_pz) % (p.S + p.L);
        return i < p.S ? own("perm_z", c, i) : own("lookup_z", c, i - p.S);
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
template <class V>
std::string nums(const V& v) { return list(v, [](auto x) { return std::to_string(x); }); }

bool read_queries(std::istream& in, std::vector<OpeningShape::Query>& out) {
    size_t count;
    if (!(in >> count)) return false;
    out.resize(count);
    for (auto& q : out)
        if (!(in >> q.column >> q.rotation)) return false;
    return true;
}

}   // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        OpeningShape sh;
        int qi = 0;
        if (!(in >> sh.circuits >> sh.k >> sh.A >> sh.num_fixed >> sh.I >> sh.L >> sh.S >> sh.npc >> sh.bf >> sh.pieces >> qi) || !read_queries(in, sh.advice_q) ||
            !read_queries(in, sh.fixed_q) || !read_queries(in, sh.instance_q)) {
            fprintf(stderr, "opening_plan_multi_check: cannot read the shape \"%s\"\n", line.c_str());
            return 2;
        }
        sh.query_instance = qi != 0;
        const OpeningPlan p(sh);
        if (!p.error.empty()) {
            printf("{\"refused\":\"%s\"}\n", p.error.c_str());
            continue;
        }
        auto K = [&](uint32_t id) { return key(p, id); };
        std::vector<uint32_t> ids(p.num_polys + 1);
        for (uint32_t i = 0; i < ids.size(); i++) ids[i] = i;
        std::string s = "{\"circuits\":" + std::to_string(p.circuits);
        s += ",\"NC\":" + std::to_string(p.NC) + ",\"o_pz\":" + std::to_string(p.o_pz) + ",\"product_order\":" + nums(p.product_order);
        s += ",\"polys\":" + list(ids, K) + ",\"num_polys\":" + std::to_string(p.num_polys);      // in id order; the folded h last, behind the num_polys evaluated ones
        s += ",\"rots\":" + nums(p.rots) + ",\"eval_count\":" + std::to_string(p.eval_count) + ",\"hpiece0\":" + std::to_string(p.hpiece0);
        s += ",\"write\":" + nums(p.write) + ",\"eval_wanted\":" + nums(p.eval_wanted);
        s += ",\"queries\":" + list(p.queries, [&](const OpeningPlan::Query& q) {
                 return "{\"rot\":" + std::to_string(q.rot) + ",\"poly\":" + K(q.poly) + ",\"eval\":" + std::to_string(q.eval) + ",\"blind\":" + std::to_string(q.blind) + "}";
             });
        s += ",\"groups\":" + list(p.groups, [&](const OpeningPlan::Group& g) {
                 return "{\"rot\":" + std::to_string(g.rot) + ",\"polys\":" + list(g.polys, K) + ",\"evals\":" + nums(g.evals) + "}";
             });
        s += ",\"commitments\":" + list(p.commitments, [&](const OpeningPlan::Commitment& c) {
                 return "{\"poly\":" + K(c.poly) + ",\"blind\":" + std::to_string(c.blind) + ",\"set\":" + std::to_string(c.set) + ",\"evals\":" + nums(c.evals) + "}";
             });
        s += ",\"point_sets\":" + list(p.point_sets, [](const std::vector<uint32_t>& ps) { return nums(ps); }) + ",\"point_rot\":" + nums(p.point_rot);
        s += ",\"set_members\":" + list(p.set_members, [](const std::vector<uint32_t>& m) { return nums(m); });
        s += ",\"proof_size\":{\"gwc\":" + std::to_string(p.proof_size(OpeningPlan::GWC)) + ",\"shplonk\":" + std::to_string(p.proof_size(OpeningPlan::SHPLONK)) + "}}";
        puts(s.c_str());
    }
    return 0;
}
