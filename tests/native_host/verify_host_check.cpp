// verify_host_check -- csrc/verify_host.hpp on the CPU (g++, ASan + UBSan; tests/test_verify_host.py writes the case file and compares the verdicts with the
// library's and the oracle's).  argv[1]: a file of little-endian words --
//   k, num_selectors, circuits, multiopen, vk_len : u32 | g0: 64 B | g2: 128 B | s_g2: 128 B | transcript_repr: 32 B | vk (RawBytes): vk_len B
//   the constraint system (verify_case_reader.hpp)
//   then proofs until the end of the file: len: u32 | bytes
// (circuits without instance values).  One "accept:reason" per proof on stdout.
#include <cstdio>

#include "../../delay-encryption-in-halo2_amd/csrc/verify_host.hpp"
#include "verify_case_reader.hpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    Reader r(argv[1]);
    const uint32_t k = r.u32(), nsel = r.u32(), circuits = r.u32(), multiopen = r.u32(), vk_len = r.u32();
    VerifierKey key;
    r.copy(key.g0, 64);
    r.copy(key.g2, 128);
    r.copy(key.s_g2, 128);
    Fe repr{};
    r.copy(repr.v, 32);
    const std::vector<uint8_t> vk = r.bytes(vk_len);
    CaseCS cs;
    if (!cs.read(r)) return 3;

    std::string err = key.init_cs(DEHALO_CURVE_BN254_G1, &cs.d, k);
    if (err.empty()) err = key.load_vk(vk.data(), vk.size(), DEHALO_SERDE_RAW_BYTES, nsel);
    if (err.empty()) err = key.check_g2();
    if (!err.empty()) { fprintf(stderr, "%s\n", err.c_str()); return 4; }
    key.transcript_repr = repr;
    key.multiopen = (int)multiopen;
    HostVerifyBackend be(key.fq, key.f, 3);
    const Fe weight = key.f->one;
    const size_t ninst = (size_t)circuits * cs.d.num_instance;
    const std::vector<const uint64_t*> inst(ninst + 1, nullptr);
    const std::vector<size_t> inst_lens(ninst + 1, 0);
    while (r.pos < r.data.size()) {
        const uint32_t len = r.u32();
        const uint8_t* at = r.take(len);
        if (!r.ok) return 3;
        const std::vector<uint8_t> proof(at, at + len);      // exactly the proof's bytes: ASan sees a read past them
        const uint8_t* pp = proof.data();
        const size_t plen = proof.size();
        VerifyInput in{&pp, &plen, 1, inst.data(), inst_lens.data(), cs.d.num_instance, circuits, &weight, OpeningPlan()};
        VerifyVerdict out;
        int rc = verify_check_arguments(key, in, &err);
        if (!rc) rc = verify_proofs_host(key, be, in, out, &err);
        if (rc) { fprintf(stderr, "rc %d: %s\n", rc, err.c_str()); return 5; }
        printf("%d:%d\n", out.accept, out.reason);
    }
    return 0;
}
