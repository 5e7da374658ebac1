// The search behind dehalo_verify_proofs_each (csrc/blame_search.hpp: host only) over EVERY bad set of n = 0 .. 12 members, as a program of its own under
// ASan + UBSan (tests/test_blame_search_host.py builds and runs it).  The predicate is the additive one the search assumes -- a run of members passes iff none
// of them is bad -- and counts its own calls.  Checked per bad set: the set the search names is the bad set; the checks it reports are the calls the predicate
// saw; 1 check when nothing is bad, at most 1 + 2 b ceil(log2 n) for b >= 1 bad members, none for n = 0; no run the search asks about is empty or leaves the set.
// Prints the worst case per n and "<cases> cases passed".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../delay-encryption-in-halo2_amd/csrc/blame_search.hpp"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint32_t ceil_log2(size_t n) {
    uint32_t l = 0;
    while (((size_t)1 << l) < n) l++;
    return l;
}

int main() {
    size_t cases = 0;
    for (size_t n = 0; n <= 12; n++) {
        uint32_t worst_one = 0, worst = 0;
        for (uint32_t mask = 0; mask < (1u << n); mask++) {
            uint32_t calls = 0;
            bool in_range = true;
            auto check = [&](size_t first, size_t count) {
                calls++;
                if (count == 0 || first + count > n) in_range = false;
                for (size_t i = first; i < first + count && i < n; i++)
                    if ((mask >> i) & 1u) return false;
                return true;
            };
            std::vector<uint8_t> bad(3, 7);      // (whatever it held: the search sizes and clears it)
            const uint32_t checks = blame_search(n, check, bad);
            cases++;
            EXPECT(in_range, "n = %zu, mask = %#x: a run outside the set", n, mask);
            EXPECT(bad.size() == n, "n = %zu: %zu verdicts", n, bad.size());
            uint32_t named = 0, b = 0;
            for (size_t i = 0; i < n && i < bad.size(); i++) {
                named |= (uint32_t)(bad[i] ? 1 : 0) << i;
                EXPECT(bad[i] <= 1, "n = %zu: a verdict is %u", n, bad[i]);
            }
            for (size_t i = 0; i < n; i++) b += (mask >> i) & 1u;
            EXPECT(named == mask, "n = %zu, bad set %#x: named %#x", n, mask, named);
            EXPECT(checks == calls, "n = %zu, bad set %#x: reports %u checks, made %u", n, mask, checks, calls);
            const uint32_t bound = n == 0 ? 0 : b == 0 ? 1 : 1 + 2 * b * ceil_log2(n);
            EXPECT(checks <= bound, "n = %zu, bad set %#x: %u checks, bound %u", n, mask, checks, bound);
            if (b == 0) EXPECT(checks == (n ? 1u : 0u), "n = %zu, nothing bad: %u checks", n, checks);
            if (b == 1 && checks > worst_one) worst_one = checks;
            if (checks > worst) worst = checks;
        }
        printf("n = %zu: at most %u checks for one bad member, %u for any bad set\n", n, worst_one, worst);
    }
    // the figures the header quotes for n = 64: 13 checks for one bad member wherever it stands, 127 when all are bad
    for (size_t at = 0; at <= 64; at++) {
        uint32_t calls = 0;
        auto check = [&](size_t first, size_t count) {
            calls++;
            return at == 64 ? false : !(first <= at && at < first + count);
        };
        std::vector<uint8_t> bad;
        const uint32_t checks = blame_search(64, check, bad);
        cases++;
        for (size_t i = 0; i < 64; i++) EXPECT(bad[i] == (at == 64 || i == at ? 1 : 0), "n = 64, bad %zu: verdict %zu is %u", at, i, bad[i]);
        EXPECT(checks == calls && checks <= (at == 64 ? 127u : 13u), "n = 64, bad %zu: %u checks", at, checks);
    }
    if (failures) { printf("%d FAILED\n", failures); return 1; }
    printf("%zu cases passed\n", cases);
    return 0;
}
