// hostrng_check.cpp -- the acceptance step of the ChaCha20 generator kinds (csrc/hostrng.hpp: chacha_accept, the one function HostRng::scalars and the kernel
// k_chacha_scalars share) on crafted candidates.  No real keystream reaches the lower words of its comparison -- a tie in the top word has probability 2^-30 per
// draw -- so for each of the four moduli it is fed p, p - 1, p + 1; for every 32-bit word j a value equal to p above word j and one less / one more in word j,
// with the words below set against the verdict (all ones / all zero); all ones before the mask; and candidates whose only excess is in the masked-off bits.
// Expected, by subtraction on 64-bit limbs: accepted iff the masked value is < p, and the value left behind is the masked one.  Then HostRng itself: the keyed
// kind draws from the caller's key (RFC 8439's first vector), leaves the caller's struct alone, and kinds >= 4 are refused.
// A program of its own, built by g++ with ASan + UBSan (make hostrng_check), run by tests/test_rng_chacha.py.  Prints one line per check; exits 1 at the first that fails.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../delay-encryption-in-halo2_amd/csrc/hostrng.hpp"

namespace {

int checks = 0;
void expect(bool ok, const std::string& what) {
    checks++;
    if (!ok) { std::printf("FAILED: %s\n", what.c_str()); std::exit(1); }
    std::printf("ok: %s\n", what.c_str());
}

struct Words { uint32_t w[8]; };

Words words_of(const uint64_t p[4]) {
    Words r;
    for (int i = 0; i < 4; i++) { r.w[2 * i] = (uint32_t)p[i]; r.w[2 * i + 1] = (uint32_t)(p[i] >> 32); }
    return r;
}

// the expectation, independent of the word-by-word chain: mask on 64-bit limbs, then v - p borrows iff v < p
bool expected(const Words& in, const HostField* f, Words& masked) {
    uint64_t v[4], d[4];
    for (int i = 0; i < 4; i++) v[i] = (uint64_t)in.w[2 * i] | ((uint64_t)in.w[2 * i + 1] << 32);
    if (f->bits < 256) v[3] &= ((uint64_t)1 << (f->bits - 192)) - 1;
    masked = words_of(v);
    return HostField::sub_limbs(d, v, f->p) == 1;
}

int accepted = 0, rejected = 0;
void candidate(const HostField* f, Words c, int want /* 1 accept, 0 reject, -1 whatever the expectation says */, const std::string& what) {
    const Words p = words_of(f->p);
    Words masked;
    const bool exp_ok = expected(c, f, masked);
    if (want >= 0) expect(exp_ok == (want == 1), what + ": the expectation itself");
    const bool got = chacha_accept(c.w, p.w, f->bits);
    expect(got == exp_ok, what + (exp_ok ? ": accepted" : ": rejected"));
    expect(memcmp(c.w, masked.w, 32) == 0, what + ": the value left is the masked one");
    (got ? accepted : rejected)++;
}

void field(int id, const char* name) {
    const HostField* f = host_field(id);
    const std::string n = std::string(name) + " ";
    expect(f && f->bits >= 225 && f->bits < 256, n + "a modulus of 225 .. 255 bits");
    const Words p = words_of(f->p);
    const uint32_t top_mask = ((uint32_t)1 << (f->bits - 224)) - 1, off_bits = ~top_mask;
    Words c = p;
    candidate(f, c, 0, n + "p");
    c = p; c.w[0] -= 1;                       // (every modulus here is odd: no borrow)
    candidate(f, c, 1, n + "p - 1");
    c = p; c.w[0] += 1;                       // (p's low word is not all ones)
    candidate(f, c, 0, n + "p + 1");
    for (int j = 0; j < 8; j++) {
        if (p.w[j] != 0) {
            c = p; c.w[j] -= 1;
            for (int i = 0; i < j; i++) c.w[i] = 0xffffffffu;
            candidate(f, c, 1, n + "one less in word " + std::to_string(j) + ", all ones below");
        }
        if (p.w[j] != 0xffffffffu && (j < 7 || p.w[7] < top_mask)) {
            c = p; c.w[j] += 1;
            for (int i = 0; i < j; i++) c.w[i] = 0;
            candidate(f, c, 0, n + "one more in word " + std::to_string(j) + ", zero below");
        }
    }
    for (int i = 0; i < 8; i++) c.w[i] = 0xffffffffu;
    candidate(f, c, 0, n + "all ones before the mask");
    c = p; c.w[0] -= 1; c.w[7] |= off_bits;
    candidate(f, c, 1, n + "p - 1 with every masked-off bit set");
    c = p; c.w[7] |= off_bits;
    candidate(f, c, 0, n + "p with every masked-off bit set");
    memset(c.w, 0, 32); c.w[7] = off_bits;
    candidate(f, c, 1, n + "only masked-off bits: zero");
    memset(c.w, 0, 32); c.w[7] = 0x80000000u;
    candidate(f, c, 1, n + "only the top bit: zero");
}

}   // namespace

int main() {
    field(DEHALO_FIELD_BN254_FR, "bn254_fr");
    field(DEHALO_FIELD_BN254_FQ, "bn254_fq");
    field(DEHALO_FIELD_PASTA_FP, "pasta_fp");
    field(DEHALO_FIELD_PASTA_FQ, "pasta_fq");
    expect(accepted >= 4 * 9 && rejected >= 4 * 9, "both verdicts were exercised for every word");

    // HostRng under the keyed kind: the all-zero key's first serial candidate is the first half of RFC 8439's first test vector (2.3.2's function on a zero
    // key, counter and nonce: 76 b8 e0 ad ...), which is below BN254 Fr's modulus after the mask -- so the first scalar is those 32 bytes, masked
    dehalo_rng r;
    memset(&r, 0, sizeof r);
    r.kind = DEHALO_RNG_CHACHA20;
    HostRng g;
    expect(g.init(&r, host_field(DEHALO_FIELD_BN254_FR)) == 0 && g.chacha(), "kind 3 is taken and is a ChaCha20 kind");
    uint64_t out[8];
    expect(g.scalars(out, 2) == 0, "two scalars");
    static const uint8_t rfc[32] = {0x76, 0xb8, 0xe0, 0xad, 0xa0, 0xf1, 0x3d, 0x90, 0x40, 0x5d, 0x6a, 0xe5, 0x53, 0x86, 0xbd, 0x28,
                                    0xbd, 0xd2, 0x19, 0xb8, 0xa0, 0x8d, 0xed, 0x1a, 0xa8, 0x36, 0xef, 0xcc, 0x8b, 0x77, 0x0d, 0xc7};
    uint8_t want[32];
    memcpy(want, rfc, 32);
    want[31] &= 0x3f;      // 254 bits: the top word becomes 0x070d778b, below p's 0x30644e72
    expect(memcmp(out, want, 32) == 0, "the first scalar of the zero key is RFC 8439's first block, masked");
    dehalo_rng before = r;
    g.write_back(&r);
    expect(memcmp(&before, &r, sizeof r) == 0, "write_back leaves a keyed generator's struct alone");
    HostRng fk = g.fork(5, 1);
    uint64_t a[4], b[4];
    HostRng g2;
    g2.init(&r, host_field(DEHALO_FIELD_BN254_FR));
    g2.skip(30);
    expect(g2.scalars(a, 1) == 0 && memcmp(a, out, 32) == 0, "skip moves no ChaCha20 stream");
    expect(fk.scalars(b, 1) == 0 && memcmp(b, out, 32) != 0, "a fork on stream 1 is another stream");
    for (int kind = 4; kind < 8; kind++) {
        r.kind = kind;
        HostRng h;
        expect(h.init(&r, host_field(DEHALO_FIELD_BN254_FR)) == DEHALO_ERR_INVALID, "kind " + std::to_string(kind) + " is refused");
    }
    r.kind = -1;
    HostRng h;
    expect(h.init(&r, host_field(DEHALO_FIELD_BN254_FR)) == DEHALO_ERR_INVALID, "kind -1 is refused");
    std::printf("%d checks passed\n", checks);
    return 0;
}
