// host_sanitize.cpp -- the HOST-only parts of the library (witness generation: big-integer division, the layouter, Grain / Poseidon; field arithmetic;
// Blake2b; ChaCha20 / PCG64) built with AddressSanitizer + UndefinedBehaviorSanitizer by g++ and exercised on the reference's circuit sizes.  GPU
// sanitizers are not available on the pool; this covers the code that needs no device.  Prints a digest of everything it computed: the test compares it
// with the digest of the regular build's dehalo_synthesize output.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dehalo.h"
#include "../../delay-encryption-in-halo2_amd/csrc/blake2b.hpp"
#include "../../delay-encryption-in-halo2_amd/csrc/guard.hpp"
#include "../../delay-encryption-in-halo2_amd/csrc/hostrng.hpp"

int main(int argc, char** argv) {
    const uint32_t k = argc > 1 ? (uint32_t)atoi(argv[1]) : 15;
    const uint32_t exp_bits = argc > 2 ? (uint32_t)atoi(argv[2]) : 3;
    std::vector<uint64_t> n(32), x(32);
    uint64_t s = 0x9E3779B97F4A7C15ULL;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (auto& v : n) v = next();
    for (auto& v : x) v = next();
    n[31] |= 1ULL << 63; n[0] |= 1; x[31] >>= 8;
    const uint64_t message[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // the reference's circuit is satisfiable for the zero message only (witness.hip)
    dehalo_circuit_inputs in{};
    in.circuit = DEHALO_CIRCUIT_DELAY_ENC; in.k = k; in.bits_len = 2048; in.exp_bits = exp_bits; in.n = n.data(); in.x = x.data();
    in.e = (1ULL << (exp_bits - 1)) | 1; in.message = message; in.message_len = 2;
    const size_t rows = (size_t)1 << k;
    std::vector<uint64_t> advice(5 * rows * 4), fixed(15 * rows * 4), mapping(6 * rows);
    std::vector<uint8_t> s0(rows), s1(rows);
    uint8_t* sels[2] = {s0.data(), s1.data()};
    dehalo_synthesis_info info{};
    int rc = dehalo_synthesize(&in, advice.data(), fixed.data(), mapping.data(), sels, &info);
    if (rc != 0) { printf("synthesize failed: %d\n", rc); return 1; }
    Blake2b h;
    h.init(32, "host-sanitize-ru");      // (16-byte personalisation)
    h.update(advice.data(), advice.size() * 8);
    h.update(fixed.data(), fixed.size() * 8);
    h.update(mapping.data(), mapping.size() * 8);
    h.update(s0.data(), rows); h.update(s1.data(), rows);
    // a proving call (advice only) writes its regions from the synthesis pool's threads: the same columns
    {
        std::vector<uint64_t> advice2(5 * rows * 4, ~0ull);
        dehalo_synthesis_info info2{};
        rc = dehalo_synthesize(&in, advice2.data(), nullptr, nullptr, nullptr, &info2);
        if (rc != 0 || advice2 != advice || info2.total_rows != info.total_rows) { printf("proving-mode advice differs from keygen-mode advice (%d)\n", rc); return 1; }
    }
    // the too-small circuit and bad arguments are refused, not overrun
    in.k = 10;
    if (dehalo_synthesize(&in, advice.data(), nullptr, nullptr, nullptr, nullptr) == 0) { printf("k = 10 accepted\n"); return 1; }
    in.k = k; in.exp_bits = 65;
    if (dehalo_synthesize(&in, advice.data(), nullptr, nullptr, nullptr, nullptr) == 0) { printf("exp_bits = 65 accepted\n"); return 1; }
    // a constraint that cannot hold (the circuit is satisfiable for the zero message only) throws inside the call and leaves it as DEHALO_ERR_INVALID
    in.exp_bits = exp_bits;
    const uint64_t message1[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    in.message = message1;
    if (dehalo_synthesize(&in, advice.data(), nullptr, nullptr, nullptr, nullptr) != DEHALO_ERR_INVALID) { printf("non-zero message not refused\n"); return 1; }
    in.message = message;
    // the entry points' guard: return codes pass through, exceptions become codes (std::bad_alloc: OOM; anything else: INVALID, its message noted)
    {
        struct Unsatisfied : std::runtime_error { using std::runtime_error::runtime_error; };      // as witness.hip's NotSatisfied
        std::string noted;
        auto note = [&](const char* m) { noted = m; };
        auto expect = [&](const char* what, int got, int want, const char* msg) {
            const bool ok = got == want && noted == msg;
            if (!ok) printf("guard: %s returned %d (noted \"%s\"), not %d (\"%s\")\n", what, got, noted.c_str(), want, msg);
            noted.clear();
            return ok;
        };
        if (!expect("0", dh_guard_noting(note, [] { return 0; }), 0, "")) return 1;
        if (!expect("a code", dh_guard_noting(note, [] { return (int)DEHALO_ERR_UNSUPPORTED; }), DEHALO_ERR_UNSUPPORTED, "")) return 1;
        if (!expect("bad_alloc", dh_guard_noting(note, []() -> int { throw std::bad_alloc(); }), DEHALO_ERR_OOM, "")) return 1;
        if (!expect("runtime_error", dh_guard_noting(note, []() -> int { throw std::runtime_error("runtime"); }), DEHALO_ERR_INVALID, "runtime")) return 1;
        if (!expect("derived", dh_guard_noting(note, []() -> int { throw Unsatisfied("derived"); }), DEHALO_ERR_INVALID, "derived")) return 1;
        if (!expect("int", dh_guard_noting(note, []() -> int { throw 7; }), DEHALO_ERR_INVALID, "unexpected exception")) return 1;
        if (!expect("no context", dh_guard(nullptr, []() -> int { throw std::runtime_error("x"); }), DEHALO_ERR_INVALID, "")) return 1;
        if (!expect("no context, bad_alloc", dh_guard(nullptr, []() -> int { throw std::bad_alloc(); }), DEHALO_ERR_OOM, "")) return 1;
    }
    // random scalars: OS entropy below p, PCG64 with a seek
    const HostField* f = host_field(0);
    HostRng r;
    if (r.init(nullptr, f) != 0) return 1;
    std::vector<uint64_t> sc(4 * 1000);
    if (r.scalars(sc.data(), 1000) != 0) return 1;
    for (int i = 0; i < 1000; i++) if (HostField::geq(sc.data() + 4 * i, f->p)) { printf("scalar >= p\n"); return 1; }
    // HostField::batch_invert: every inverse from one inversion; a zero anywhere is refused and nothing is written
    {
        std::vector<Fe> v(1000);
        memcpy(v.data(), sc.data(), 32 * v.size());
        std::vector<Fe> w = v;
        if (!f->batch_invert(w.data(), w.size())) { printf("batch_invert refused non-zero scalars\n"); return 1; }
        for (size_t i = 0; i < v.size(); i++) if (f->mul(v[i], w[i]) != f->one || w[i] != f->invert(v[i])) { printf("batch_invert: element %zu is not the inverse\n", i); return 1; }
        w = v;
        w[500] = Fe{{0, 0, 0, 0}};
        const std::vector<Fe> before = w;
        if (f->batch_invert(w.data(), w.size()) || memcmp(w.data(), before.data(), 32 * w.size())) { printf("batch_invert: a zero was not refused, or the values were touched\n"); return 1; }
        if (!f->batch_invert(nullptr, 0)) { printf("batch_invert refused the empty list\n"); return 1; }
    }
    dehalo_rng pr{};
    pr.kind = DEHALO_RNG_PCG64; pr.pcg_state[0] = 123; pr.pcg_inc[0] = 457;
    if (r.init(&pr, f) != 0) return 1;
    HostRng fk = r.fork(5000, 1);
    r.skip(5000);
    uint64_t a4[4], b4[4];
    r.scalars(a4, 1); fk.scalars(b4, 1);
    if (memcmp(a4, b4, 32)) { printf("fork != skip\n"); return 1; }
    h.update(a4, 32);
    uint8_t d[32];
    h.digest(d);
    for (int i = 0; i < 32; i++) printf("%02x", d[i]);
    printf(" rows %llu\n", (unsigned long long)info.total_rows);
    return 0;
}
