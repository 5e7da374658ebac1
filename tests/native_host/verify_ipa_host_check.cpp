// verify_ipa_host_check -- the IPA half of csrc/verify_host.hpp on the CPU (g++, ASan + UBSan; tests/test_verify_ipa_host.py writes the case file and compares the
// verdicts with the library's and the oracle's).  argv[1]: a file of little-endian words --
//   curve, k, num_selectors, vk_len, instance values : u32 | g: 2^k x 64 B | g_lagrange: 2^k x 64 B | w: 64 B | u: 64 B | transcript_repr: 32 B | vk (RawBytes): vk_len B
//   the constraint system, as verify_host_check.cpp reads it
//   the values of instance column 0 (4 x u64 Montgomery each; every other instance column is empty)
//   then proofs until the end of the file: len: u32 | bytes
// One "accept:reason" per proof on stdout.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../delay-encryption-in-halo2_amd/csrc/verify_host.hpp"

struct Reader {
    std::vector<uint8_t> data;
    size_t pos = 0;
    bool ok = true;
    const uint8_t* take(size_t n) {
        static const uint8_t none = 0;
        if (n > data.size() - pos) { ok = false; return &none; }
        const uint8_t* p = data.data() + pos;
        pos += n;
        return n ? p : &none;
    }
    void copy(void* dst, size_t n) {
        const uint8_t* p = take(n);
        if (ok && n) memcpy(dst, p, n);
    }
    uint32_t u32() {
        const uint8_t* p = take(4);
        return ok ? (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24) : 0;
    }
    std::vector<uint32_t> u32s(size_t n) {
        std::vector<uint32_t> v;
        for (size_t i = 0; i < n && ok; i++) v.push_back(u32());
        return v;
    }
    std::vector<dehalo_column_query> queries(size_t n) {
        std::vector<dehalo_column_query> v;
        for (size_t i = 0; i < n && ok; i++) {
            dehalo_column_query q;
            q.kind = u32(); q.index = u32(); q.rotation = (int32_t)u32();
            v.push_back(q);
        }
        return v;
    }
};

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    Reader r;
    r.data.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    const uint32_t curve = r.u32(), k = r.u32(), nsel = r.u32(), vk_len = r.u32(), nvalues = r.u32();
    if (k > 12 || (curve != DEHALO_CURVE_PALLAS && curve != DEHALO_CURVE_VESTA)) return 3;
    VerifierKey key;
    key.scheme = DEHALO_SCHEME_IPA;
    std::vector<uint64_t> g((size_t)8 << k), g_lagrange((size_t)8 << k);
    r.copy(g.data(), 8 * g.size());
    r.copy(g_lagrange.data(), 8 * g_lagrange.size());
    r.copy(key.w, 64);
    r.copy(key.u, 64);
    memcpy(key.g0, g.data(), 64);
    Fe repr{};
    r.copy(repr.v, 32);
    std::vector<uint8_t> vk(vk_len <= r.data.size() ? vk_len : 0);
    r.copy(vk.data(), vk.size());
    uint32_t c[14];
    for (uint32_t& w : c) w = r.u32();
    if (!r.ok) return 3;
    dehalo_constraint_system d{};
    d.num_advice = c[0]; d.num_fixed = c[1]; d.num_instance = c[2]; d.minimum_degree = c[3];
    d.num_nodes = c[4]; d.num_constants = c[5]; d.num_gates = c[6]; d.num_lookups = c[7]; d.num_permutation_columns = c[8];
    d.num_advice_queries = c[9]; d.num_fixed_queries = c[10]; d.num_instance_queries = c[11]; d.num_challenges = c[12]; d.num_shuffles = c[13];
    std::vector<dehalo_expr_node> nodes;
    for (uint32_t i = 0; i < d.num_nodes && r.ok; i++) {
        dehalo_expr_node e;
        e.kind = r.u32(); e.a = r.u32(); e.b = r.u32(); e.rotation = (int32_t)r.u32();
        nodes.push_back(e);
    }
    std::vector<uint64_t> constants(4 * (size_t)d.num_constants + 1);
    r.copy(constants.data(), 32 * (size_t)d.num_constants);
    const std::vector<uint32_t> gates = r.u32s(d.num_gates), lookup_lens = r.u32s(d.num_lookups);
    size_t tl = 0, ts = 0;
    for (uint32_t l : lookup_lens) tl += l;
    const std::vector<uint32_t> lookup_inputs = r.u32s(tl), lookup_tables = r.u32s(tl);
    const std::vector<dehalo_column_query> perm = r.queries(d.num_permutation_columns), aq = r.queries(d.num_advice_queries), fq = r.queries(d.num_fixed_queries),
                                           iq = r.queries(d.num_instance_queries);
    std::vector<uint8_t> advice_phases(d.num_advice <= r.data.size() ? d.num_advice : 0), challenge_phases(d.num_challenges <= r.data.size() ? d.num_challenges : 0);
    r.copy(advice_phases.data(), advice_phases.size());
    r.copy(challenge_phases.data(), challenge_phases.size());
    const std::vector<uint32_t> shuffle_lens = r.u32s(d.num_shuffles);
    for (uint32_t l : shuffle_lens) ts += l;
    const std::vector<uint32_t> shuffle_inputs = r.u32s(ts), shuffle_tables = r.u32s(ts);
    std::vector<uint64_t> values(4 * (size_t)(nvalues <= r.data.size() ? nvalues : 0) + 1);
    r.copy(values.data(), 32 * (values.size() / 4));
    if (!r.ok) return 3;
    d.nodes = nodes.data(); d.constants = constants.data(); d.gates = gates.data();
    d.lookup_lens = lookup_lens.data(); d.lookup_inputs = lookup_inputs.data(); d.lookup_tables = lookup_tables.data();
    d.permutation_columns = perm.data(); d.advice_queries = aq.data(); d.fixed_queries = fq.data(); d.instance_queries = iq.data();
    d.advice_phases = advice_phases.data(); d.challenge_phases = challenge_phases.data();
    d.shuffle_lens = shuffle_lens.data(); d.shuffle_inputs = shuffle_inputs.data(); d.shuffle_tables = shuffle_tables.data();

    std::string err = key.init_cs((int)curve, &d, k);
    if (err.empty()) err = key.load_vk(vk.data(), vk.size(), DEHALO_SERDE_RAW_BYTES, nsel);
    if (!err.empty()) { fprintf(stderr, "%s\n", err.c_str()); return 4; }
    key.transcript_repr = repr;
    HostVerifyBackend be(key.fq, key.f, curve_b_host((int)curve));
    be.set_ipa(g.data(), g_lagrange.data(), key.w, k);
    const Fe weight = key.f->one;
    const uint32_t circuits = 1;
    std::vector<const uint64_t*> inst(d.num_instance + 1, nullptr);
    std::vector<size_t> inst_lens(d.num_instance + 1, 0);
    if (d.num_instance && nvalues) { inst[0] = values.data(); inst_lens[0] = nvalues; }
    while (r.pos < r.data.size()) {
        const uint32_t len = r.u32();
        const uint8_t* at = r.take(len);
        if (!r.ok) return 3;
        const std::vector<uint8_t> proof(at, at + len);      // exactly the proof's bytes: ASan sees a read past them
        const uint8_t* pp = proof.data();
        const size_t plen = proof.size();
        int accept = -1, reason = -1;
        int64_t first = -2;
        VerifyStats st;
        const int rc = verify_proofs_host(key, be, &pp, &plen, 1, inst.data(), inst_lens.data(), d.num_instance, circuits, &weight, &accept, &first, &reason, &st, &err);
        if (rc) { fprintf(stderr, "rc %d: %s\n", rc, err.c_str()); return 5; }
        printf("%d:%d\n", accept, reason);
    }
    return 0;
}
