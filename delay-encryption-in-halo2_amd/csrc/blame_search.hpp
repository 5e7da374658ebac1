// blame_search.hpp -- which members of a set fail, given only a predicate over subsets: the search behind dehalo_verify_proofs_each (verify_host.hpp), where a
// member is a proof, a subset's check is one pairing check (IPA: one sum over g) on the subset's summed terms, and checks are what costs.
// The predicate must be ADDITIVE: a subset passes iff none of its members is bad.  (A weighted batch check is, up to the negligible chance that the random weights
// let bad members cancel.)  Then a set that fails and whose first half passes has its bad members in the second half, and that half needs no check of its own:
//     find(S), S known to hold a bad member:
//         |S| = 1: its member is bad
//         else A = the first ceil(|S| / 2) members, B = the rest
//              if check(A): find(B)                              -- S is bad and A is clean, so B is bad: no check of B
//              else:        find(A); if !check(B): find(B)
//     root: if !check(all): find(all)
// Enumerated over every bad set for n <= 12 (tests/native_host/blame_search_check.cpp): it names exactly the bad members, with 1 check when none is bad and at
// most 1 + 2 b ceil(log2 n) checks for b >= 1 bad members -- n = 64: 13 checks for one bad member, 127 when all are bad.  No check at all for n = 0.
// Members are the positions 0 .. n - 1 and every subset the search asks about is a run of consecutive positions: check(first, count).
// Host only, no HIP header.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

template <class Check>
struct BlameSearch {
    Check& check;
    std::vector<uint8_t>& bad;
    uint32_t checks = 0;
    bool passes(size_t first, size_t count) {
        checks++;
        return check(first, count);
    }
    void find(size_t first, size_t count) {      // the run is known to hold a bad member
        if (count == 1) { bad[first] = 1; return; }
        const size_t a = (count + 1) / 2;
        if (passes(first, a)) { find(first + a, count - a); return; }
        find(first, a);
        if (!passes(first + a, count - a)) find(first + a, count - a);
    }
};

// bad[i] = 1 iff member i fails, for i < n; returns the number of checks made.  check(first, count) -> "the members first .. first + count - 1 pass together"
template <class Check>
inline uint32_t blame_search(size_t n, Check&& check, std::vector<uint8_t>& bad) {
    bad.assign(n, 0);
    if (n == 0) return 0;
    BlameSearch<Check> s{check, bad};
    if (!s.passes(0, n)) s.find(0, n);
    return s.checks;
}
