// verify_ipa_host_check -- the IPA half of csrc/verify_host.hpp on the CPU (g++, ASan + UBSan; tests/test_verify_ipa_host.py writes the case file and compares the
// verdicts with the library's and the oracle's).  argv[1]: a file of little-endian words --
//   curve, k, num_selectors, vk_len, instance values : u32 | g: 2^k x 64 B | g_lagrange: 2^k x 64 B | w: 64 B | u: 64 B | transcript_repr: 32 B | vk (RawBytes): vk_len B
//   the constraint system (verify_case_reader.hpp)
//   the values of instance column 0 (4 x u64 Montgomery each; every other instance column is empty)
//   then proofs until the end of the file: len: u32 | bytes
// One "accept:reason" per proof on stdout.
#include <cstdio>

#include "../../delay-encryption-in-halo2_amd/csrc/verify_host.hpp"
#include "verify_case_reader.hpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    Reader r(argv[1]);
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
    const std::vector<uint8_t> vk = r.bytes(vk_len);
    CaseCS cs;
    if (!cs.read(r)) return 3;
    std::vector<uint64_t> values(4 * (size_t)(nvalues <= r.data.size() ? nvalues : 0) + 1);
    r.copy(values.data(), 32 * (values.size() / 4));
    if (!r.ok) return 3;

    std::string err = key.init_cs((int)curve, &cs.d, k);
    if (err.empty()) err = key.load_vk(vk.data(), vk.size(), DEHALO_SERDE_RAW_BYTES, nsel);
    if (!err.empty()) { fprintf(stderr, "%s\n", err.c_str()); return 4; }
    key.transcript_repr = repr;
    HostVerifyBackend be(key.fq, key.f, curve_b_host((int)curve));
    be.set_ipa(g.data(), g_lagrange.data(), key.w, k);
    const Fe weight = key.f->one;
    std::vector<const uint64_t*> inst(cs.d.num_instance + 1, nullptr);
    std::vector<size_t> inst_lens(cs.d.num_instance + 1, 0);
    if (cs.d.num_instance && nvalues) { inst[0] = values.data(); inst_lens[0] = nvalues; }
    while (r.pos < r.data.size()) {
        const uint32_t len = r.u32();
        const uint8_t* at = r.take(len);
        if (!r.ok) return 3;
        const std::vector<uint8_t> proof(at, at + len);      // exactly the proof's bytes: ASan sees a read past them
        const uint8_t* pp = proof.data();
        const size_t plen = proof.size();
        VerifyInput in{&pp, &plen, 1, inst.data(), inst_lens.data(), cs.d.num_instance, 1, &weight, OpeningPlan()};
        VerifyVerdict out;
        int rc = verify_check_arguments(key, in, &err);
        if (!rc) rc = verify_proofs_host(key, be, in, out, &err);
        if (rc) { fprintf(stderr, "rc %d: %s\n", rc, err.c_str()); return 5; }
        printf("%d:%d\n", out.accept, out.reason);
    }
    return 0;
}
