// example.cpp -- the reference's bench flow (benches/pose_enc.rs:41-135: ParamsKZG::setup when no params file is cached, else read it; keygen_vk /
// keygen_pk, write and re-read the proving key, create_proof into a Blake2bWrite transcript) from C++ over the C ABI, with no interpreter anywhere.  The
// key the proof runs under comes from keygen_pk under the verifying key in its Processed form (benches/delay_enc.rs:88-103).
//
//   example                 build / link check: one tiny best_fft (needs a GPU to run)
//   example <dir>           <dir>/params.bin   ParamsKZG RawBytes; when it does not exist it is MADE (ParamsKZG::setup on the device) from
//                                              <dir>/secret.bin (32 B: the scalar the reference would draw from OsRng, Montgomery form) and written;
//                                              the proof then runs under the same SRS cut out of a Processed file written at k + 1 (read_custom)
//                           <dir>/circuit.bin  u32 k | fixed columns (9 x 2^k x 32 B, Montgomery) | permutation mapping (6 x 2^k u64) |
//                                              advice (5 x 2^k x 32 B, Montgomery) | transcript_repr (32 B) | PCG64 state, inc (2 x 16 B)
//                           -> <dir>/pk.bin (ProvingKey RawBytes), <dir>/vk.bin, <dir>/proof.bin
// The circuit shape is the MainGate of PoseidonEncCircuit (5 advice, 9 fixed, 1 instance; halo2wrong maingate [UPSTREAM]) built here
// with the ConstraintSystem builder; tests/test_native.py writes the inputs, runs this program and checks the proof it wrote.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>

#include "halo2_backend.hpp"

using namespace halo2_amd;

static std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static void dump(const std::string& path, const std::vector<uint8_t>& b) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char*)b.data(), (std::streamsize)b.size());
    if (!f) throw std::runtime_error("cannot write " + path);
}

// MainGate::configure: a sa + b sb + c sc + d sd + e se + a b s_mul_ab + c d s_mul_cd + e(next) s_next + s_constant = 0
static void maingate(ConstraintSystem& cs) {
    for (uint32_t i = 0; i < 5; i++) cs.enable_equality(DEHALO_COLUMN_ADVICE, i);
    cs.enable_equality(DEHALO_COLUMN_INSTANCE, 0);
    ConstraintSystem::Expr adv[5], fx[9];
    for (uint32_t i = 0; i < 5; i++) adv[i] = cs.query_advice(i);
    const ConstraintSystem::Expr e_next = cs.query_advice(4, 1);
    for (uint32_t i = 0; i < 9; i++) fx[i] = cs.query_fixed(i);
    ConstraintSystem::Expr g = cs.product(adv[0], fx[0]);
    for (uint32_t i = 1; i < 5; i++) g = cs.sum(g, cs.product(adv[i], fx[i]));
    g = cs.sum(g, cs.product(cs.product(adv[0], adv[1]), fx[5]));
    g = cs.sum(g, cs.product(cs.product(adv[2], adv[3]), fx[6]));
    g = cs.sum(g, cs.product(e_next, fx[7]));
    g = cs.sum(g, fx[8]);
    cs.create_gate({g});
}

int main(int argc, char** argv) {
    try {
        Backend be(0);
        if (argc < 2) {
            std::vector<Fe> a(4, Fe{0, 0, 0, 0});
            Fe one_m{0x34786d38fffffffdULL, 0x992c350be41914adULL, 0xffffffffffffffffULL, 0x3fffffffffffffffULL};  // pasta::Fp R
            be.best_fft(DEHALO_FIELD_PASTA_FP, a, one_m, 2);
            {   // ParamsIPA over Vesta from g alone (g[i] = [i + 2] G, G = (-1, 2)), written, read back and written again
                const uint32_t k = 3;
                uint64_t info[24];
                be.check(dehalo_field_info(DEHALO_FIELD_PASTA_FQ, info));      // Vesta's base field: info[4 .. 8) = R = 1 in Montgomery form
                Fe zero{0, 0, 0, 0}, one, two, minus_one;
                memcpy(one.data(), info + 4, 32);
                be.check(dehalo_field_op(be.raw(), DEHALO_FIELD_PASTA_FQ, 0 /* add */, one.data(), one.data(), two.data(), 1));
                be.check(dehalo_field_op(be.raw(), DEHALO_FIELD_PASTA_FQ, 1 /* sub */, zero.data(), one.data(), minus_one.data(), 1));
                Affine gen;
                memcpy(gen.data(), minus_one.data(), 32);
                memcpy(gen.data() + 4, two.data(), 32);
                std::vector<Affine> pts((size_t(1) << k) + 2);
                for (size_t i = 0; i < pts.size(); i++) {
                    Fe s{i + 2, 0, 0, 0};
                    be.check(dehalo_field_op(be.raw(), DEHALO_FIELD_PASTA_FP, 4 /* canonical -> Montgomery */, s.data(), nullptr, s.data(), 1));
                    const Projective pr = be.best_multiexp(DEHALO_CURVE_VESTA, {s}, {gen});
                    be.check(dehalo_to_affine(be.raw(), DEHALO_CURVE_VESTA, pr.data(), 1, pts[i].data()));
                }
                const Affine w = pts[pts.size() - 2], u = pts[pts.size() - 1];
                pts.resize(size_t(1) << k);
                const std::vector<uint8_t> written = ParamsIPAHandle::from_g(be, DEHALO_CURVE_VESTA, k, pts, w, u).write();
                const std::vector<uint8_t> again = ParamsIPAHandle::read(be, DEHALO_CURVE_VESTA, written).write();
                if (written.size() != 4 + 64 * (size_t(1) << k) + 64 || written != again) throw std::runtime_error("ParamsIPA: from_g -> write -> read -> write changed the bytes");
                std::printf("ParamsIPA from_g / write / read: %zu bytes\n", written.size());
            }
            std::printf("%s ok\n", dehalo_version());
            return 0;
        }
        const std::string dir = argv[1];
        const std::vector<uint8_t> c = slurp(dir + "/circuit.bin");
        uint32_t k;
        memcpy(&k, c.data(), 4);
        std::unique_ptr<ParamsKZG> params_owner;
        if (std::ifstream(dir + "/params.bin", std::ios::binary)) params_owner.reset(new ParamsKZG(be, DEHALO_CURVE_BN254_G1, slurp(dir + "/params.bin")));
        else {      // benches/pose_enc.rs:44-54: no cached file -> setup, write
            const std::vector<uint8_t> sb = slurp(dir + "/secret.bin");
            if (sb.size() != 32) throw std::runtime_error("secret.bin: 32 bytes expected");
            Fe s;
            memcpy(s.data(), sb.data(), 32);
            params_owner.reset(new ParamsKZG(be, DEHALO_CURVE_BN254_G1, k, s));
            dump(dir + "/params.bin", params_owner->write());
            // what a deployment does with a universal SRS: the file was written at a larger k, with compressed points; the circuit's prefix of it is read,
            // g_lagrange comes from the group FFT -- and the proof below runs under THOSE params, which must be the ones just written
            const std::vector<uint8_t> universal = ParamsKZG(be, DEHALO_CURVE_BN254_G1, k + 1, s).write_custom(DEHALO_SERDE_PROCESSED);
            std::unique_ptr<ParamsKZG> cut(new ParamsKZG(ParamsKZG::read_custom(be, DEHALO_CURVE_BN254_G1, universal, DEHALO_SERDE_PROCESSED, k)));
            if (cut->write() != params_owner->write()) throw std::runtime_error("ParamsKZG: setup(k + 1) -> write_custom(Processed) -> read_custom(downsize = k) is not setup(k)");
            params_owner = std::move(cut);
        }
        ParamsKZG& params = *params_owner;
        const size_t n = (size_t)1 << k;
        if (c.size() != 4 + 9 * n * 32 + 6 * n * 8 + 5 * n * 32 + 32 + 32) throw std::runtime_error("circuit.bin: unexpected size");
        std::vector<Fe> fixed(9 * n), advice(5 * n);
        std::vector<uint64_t> mapping(6 * n);
        const uint8_t* p = c.data() + 4;
        memcpy(fixed.data(), p, 9 * n * 32); p += 9 * n * 32;
        memcpy(mapping.data(), p, 6 * n * 8); p += 6 * n * 8;
        memcpy(advice.data(), p, 5 * n * 32); p += 5 * n * 32;
        Fe repr;
        memcpy(repr.data(), p, 32); p += 32;
        dehalo_rng rng{};
        rng.kind = DEHALO_RNG_PCG64;
        memcpy(rng.pcg_state, p, 16);
        memcpy(rng.pcg_inc, p + 16, 16);

        ConstraintSystem cs(5, 9, 1);
        maingate(cs);
        {
            ProvingKey fresh(be, params, cs, fixed, mapping);      // keygen_vk + keygen_pk
            dump(dir + "/pk.bin", fresh.write());
            dump(dir + "/vk.bin", fresh.vk_write());
        }
        {   // benches/delay_enc.rs:88-103: the vk leaves in the portable format, and keygen_pk under it (no commitment is recomputed) gives the key just written;
            // so does reading that key back from its Processed form
            const std::vector<uint8_t> raw = slurp(dir + "/pk.bin");
            ProvingKey cached(be, DEHALO_CURVE_BN254_G1, cs, raw, 0);
            const std::vector<uint8_t> vk_processed = cached.vk_write(DEHALO_SERDE_PROCESSED);
            if (ProvingKey::keygen_pk(be, params, cs, vk_processed, DEHALO_SERDE_PROCESSED, 0, fixed, mapping).write() != raw)
                throw std::runtime_error("keygen_pk under the Processed vk is not the key keygen made");
            const std::vector<uint8_t> processed = cached.write(DEHALO_SERDE_PROCESSED);
            if (processed.size() + 32 * (9 + 6) != raw.size() || ProvingKey::read(be, DEHALO_CURVE_BN254_G1, cs, processed, 0, DEHALO_SERDE_PROCESSED).write() != raw)
                throw std::runtime_error("ProvingKey: write(Processed) -> read(Processed) changed the key");
        }
        // the proof runs under the key that keygen_pk builds from the Processed vk on disk
        ProvingKey pk = ProvingKey::keygen_pk(be, params, cs, ProvingKey(be, DEHALO_CURVE_BN254_G1, cs, slurp(dir + "/pk.bin"), 0).vk_write(DEHALO_SERDE_PROCESSED),
                                                    DEHALO_SERDE_PROCESSED, 0, fixed, mapping);
        pk.set_transcript_repr(repr);
        Backend side(0);
        Prover prover(be, params, pk, &side);
        Blake2bWrite transcript(DEHALO_CURVE_BN254_G1);
        prover.create_proof(advice, {{}}, &rng, transcript);
        const std::vector<uint8_t> proof = transcript.finalize();
        dump(dir + "/proof.bin", proof);
        std::printf("k = %u: proof of %zu bytes written\n", k, proof.size());
        // benches/delay_enc.rs:147-165: verify_proof(..) and assert!(accept) -- on the device verifier made from the objects at hand, and on a host verifier made
        // from what a verifier elsewhere would hold: g[0], g2, s_g2 of the params file and the Processed vk
        Verifier verifier(be, params, pk);
        int reason = 0;
        if (!verifier.verify(proof, {{}}, &reason)) throw std::runtime_error("verify_proof rejected the proof just made (reason " + std::to_string(reason) + ")");
        std::vector<uint8_t> tampered = proof;
        tampered[tampered.size() / 2] ^= 1;
        if (verifier.verify(tampered, {{}}, &reason) || reason == DEHALO_REJECT_NONE) throw std::runtime_error("verify_proof accepted a tampered proof");
        const std::vector<uint8_t> pbytes = params.write();
        Affine g0;
        memcpy(g0.data(), pbytes.data() + 4, 64);
        Verifier elsewhere(nullptr, DEHALO_CURVE_BN254_G1, k, g0, pbytes.data() + pbytes.size() - 256, pbytes.data() + pbytes.size() - 128, cs,
                           ProvingKey(be, DEHALO_CURVE_BN254_G1, cs, slurp(dir + "/pk.bin"), 0).vk_write(DEHALO_SERDE_PROCESSED), DEHALO_SERDE_PROCESSED, 0);
        elsewhere.set_transcript_repr(repr);
        if (!elsewhere.verify(proof, {{}}) || elsewhere.verify(tampered, {{}})) throw std::runtime_error("the host verifier disagrees with the device verifier");
        std::printf("k = %u: proof accepted by the device verifier and by a host verifier made from the vk bytes\n", k);
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
