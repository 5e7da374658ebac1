// g1_host_check -- csrc/g1_host.hpp on the CPU (g++, ASan + UBSan; tests/test_g1_host.py builds and runs it): the one host codec of a G1 point against the group
// law and against the bytes the transcript appends to a proof, on all three curves; the refusals of the decoder; the texts of the status bits.
// No input.  Every case that fails prints a line saying which; the exit status is non-zero when any did.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../delay-encryption-in-halo2_amd/csrc/g1_host.hpp"
#include "../../delay-encryption-in-halo2_amd/csrc/transcript_host.hpp"

static int failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            failures++;                  \
            printf("FAILED %s: ", name); \
            printf(__VA_ARGS__);         \
            printf("\n");                \
        }                                \
    } while (0)

static bool all_zero(const uint64_t xy[8]) {
    for (int i = 0; i < 8; i++)
        if (xy[i]) return false;
    return true;
}

static void check_curve(int curve, const char* name) {
    const HostField* fq = host_field(curve_base_field(curve));
    const G1Host g1(fq, curve_b_host(curve));
    // the generator: (1, 2) on BN254, (p - 1, 2) on Pallas and Vesta
    const Fe gx = curve == DEHALO_CURVE_BN254_G1 ? fq->one : fq->neg(fq->one), gy = fq->from_u64(2);
    CHECK(g1.on_curve(gx, gy), "the generator is not on the curve");
    dehalo_transcript t;
    t.init(curve);
    G1Host::Jac acc = g1.identity();
    for (int i = 1; i <= 16; i++) {
        acc = g1.add_affine(acc, gx, gy);
        uint64_t P[8], back[8];
        g1.to_affine(acc, P);
        Fe x, y;
        memcpy(x.v, P, 32);
        memcpy(y.v, P + 4, 32);
        CHECK(!all_zero(P) && g1.on_curve(x, y), "[%d]G is not a point of the curve", i);
        uint8_t enc[32];
        g1_compress_host(fq, P, enc);
        const uint32_t st = g1_decompress_host(fq, g1.b, enc, back);
        CHECK(st == 0 && !memcmp(back, P, 64), "decompress(compress([%d]G)) != [%d]G (status %u)", i, i, st);
        const size_t before = t.proof.size();
        CHECK(t.write_point(P) && t.proof.size() == before + 32 && !memcmp(t.proof.data() + before, enc, 32), "write_point([%d]G) appends other bytes than compress", i);
    }
    uint8_t enc[32];
    uint64_t xy[8];
    {   // the identity: 32 zero bytes, and back with status 0
        const uint64_t zero[8] = {};
        memset(enc, 0xff, 32);
        g1_compress_host(fq, zero, enc);
        bool z = true;
        for (int i = 0; i < 32; i++) z = z && enc[i] == 0;
        CHECK(z, "the identity does not compress to 32 zero bytes");
        memset(xy, 0xff, 64);
        CHECK(g1_decompress_host(fq, g1.b, enc, xy) == 0 && all_zero(xy), "32 zero bytes do not decompress to the identity with status 0");
    }
    // x = p: bit 1
    memcpy(enc, fq->p, 32);
    CHECK(g1_decompress_host(fq, g1.b, enc, xy) == POINT_NOT_BELOW_P && all_zero(xy), "x = p is not refused with bit 1");
    {   // the first x from 2 upward with x^3 + b a non-residue: bit 2, with either sign
        uint64_t bad = 0;
        for (uint64_t v = 2; v < 64 && !bad; v++) {
            const Fe x = fq->from_u64(v);
            Fe y;
            if (!fq->sqrt(fq->add(fq->mul(fq->sqr(x), x), g1.b), y)) bad = v;
        }
        CHECK(bad != 0, "no x in [2, 64) with x^3 + b a non-residue");
        memset(enc, 0, 32);
        enc[0] = (uint8_t)bad;
        CHECK(g1_decompress_host(fq, g1.b, enc, xy) == POINT_NOT_ON_CURVE && all_zero(xy), "x = %llu off the curve is not refused with bit 2", (unsigned long long)bad);
        enc[31] = 0x80;
        CHECK(g1_decompress_host(fq, g1.b, enc, xy) == POINT_NOT_ON_CURVE && all_zero(xy), "x = %llu off the curve, sign set, is not refused with bit 2", (unsigned long long)bad);
    }
    // x = 0 with the sign bit set: bit 4
    memset(enc, 0, 32);
    enc[31] = 0x80;
    CHECK(g1_decompress_host(fq, g1.b, enc, xy) == POINT_ZERO_X_SIGNED && all_zero(xy), "x = 0 with the sign bit set is not refused with bit 4");
}

static void check_texts() {
    const char* name = "texts";
    const struct { uint32_t status; bool encodings; const char* want; } cases[] = {
        {0, true, ""},
        {0, false, ""},
        {1, true, "an x coordinate is not below the modulus"},
        {1, false, "a coordinate's stored word is not below the modulus"},
        {2, true, "an x coordinate is not on the curve"},
        {2, false, "a point is neither on the curve nor the identity"},
        {4, true, "x = 0 with the sign bit set is not an encoding"},
        {4, false, "x = 0 with the sign bit set is not an encoding"},
        // several bits (a vector of points): below the modulus first, then the signed zero, then the curve -- the order of the three copies this replaced
        {7, true, "an x coordinate is not below the modulus"},
        {6, true, "x = 0 with the sign bit set is not an encoding"},
        {3, false, "a coordinate's stored word is not below the modulus"},
    };
    for (const auto& c : cases)
        CHECK(std::string(point_status_text(c.status, c.encodings)) == c.want, "point_status_text(%u, %d) = \"%s\"", c.status, (int)c.encodings, point_status_text(c.status, c.encodings));
    CHECK(POINT_NOT_BELOW_P == 1 && POINT_NOT_ON_CURVE == 2 && POINT_ZERO_X_SIGNED == 4, "the status bits moved");
    CHECK(serde_format_known(DEHALO_SERDE_PROCESSED) && serde_format_known(DEHALO_SERDE_RAW_BYTES) && serde_format_known(DEHALO_SERDE_RAW_BYTES_UNCHECKED) && !serde_format_known(-1) &&
              !serde_format_known(3),
          "serde_format_known");
}

int main() {
    check_curve(DEHALO_CURVE_BN254_G1, "bn254");
    check_curve(DEHALO_CURVE_PALLAS, "pallas");
    check_curve(DEHALO_CURVE_VESTA, "vesta");
    check_texts();
    if (failures) printf("%d case(s) failed\n", failures);
    else printf("ok\n");
    return failures ? 1 : 0;
}
