// bigint_host.hpp -- big integers as little-endian 64-bit limbs: what witness generation (witness.hip) needs of them -- product, Knuth's division,
// difference, fixed-length limb views.  Host only, no HIP include; tests/native_host/witness_units_check.cpp runs it under ASan / UBSan.
// (This header and poseidon_host.hpp, maingate_host.hpp, synth_chips.hpp, synth_pool.hpp keep the internal linkage their code had as one file: with external
// linkage the compiler stops inlining the chips' single-caller functions and a k = 17 synthesis takes 8 % longer.  One library unit includes them: witness.hip.)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace synth { namespace {

typedef unsigned __int128 u128;
typedef std::vector<uint64_t> Big;

inline void big_trim(Big& a) { while (!a.empty() && a.back() == 0) a.pop_back(); }
inline int big_cmp(const Big& a, const Big& b) {
    size_t na = a.size(), nb = b.size();
    while (na && a[na - 1] == 0) na--;
    while (nb && b[nb - 1] == 0) nb--;
    if (na != nb) return na < nb ? -1 : 1;
    for (size_t i = na; i-- > 0;)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
inline Big big_mul(const Big& a, const Big& b) {
    Big r(a.size() + b.size(), 0);
    for (size_t i = 0; i < a.size(); i++) {
        u128 c = 0;
        for (size_t j = 0; j < b.size(); j++) {
            c += (u128)a[i] * b[j] + r[i + j];
            r[i + j] = (uint64_t)c;
            c >>= 64;
        }
        r[i + b.size()] = (uint64_t)c;
    }
    return r;
}
// Knuth algorithm D: (q, r) = divmod(u, v), v != 0
inline void big_divmod(const Big& u_in, const Big& v_in, Big& q, Big& r) {
    Big u = u_in, v = v_in;
    big_trim(u);
    big_trim(v);
    if (big_cmp(u, v) < 0) {
        q.clear();
        r = u;
        return;
    }
    const size_t n = v.size(), m = u.size() - n;
    if (n == 1) {
        q.assign(u.size(), 0);
        u128 rem = 0;
        for (size_t i = u.size(); i-- > 0;) {
            const u128 cur = (rem << 64) | u[i];
            q[i] = (uint64_t)(cur / v[0]);
            rem = cur % v[0];
        }
        r.assign(1, (uint64_t)rem);
        big_trim(q);
        big_trim(r);
        return;
    }
    const int s = __builtin_clzll(v[n - 1]);
    Big vn(n), un(u.size() + 1);
    for (size_t i = n - 1; i > 0; i--) vn[i] = s ? (v[i] << s) | (v[i - 1] >> (64 - s)) : v[i];
    vn[0] = v[0] << s;
    un[u.size()] = s ? u[u.size() - 1] >> (64 - s) : 0;
    for (size_t i = u.size() - 1; i > 0; i--) un[i] = s ? (u[i] << s) | (u[i - 1] >> (64 - s)) : u[i];
    un[0] = u[0] << s;
    q.assign(m + 1, 0);
    for (size_t j = m + 1; j-- > 0;) {
        const u128 num = ((u128)un[j + n] << 64) | un[j + n - 1];
        u128 qhat = num / vn[n - 1], rhat = num % vn[n - 1];
        while ((qhat >> 64) || (uint64_t)qhat * (u128)vn[n - 2] > ((rhat << 64) | un[j + n - 2])) {
            qhat--;
            rhat += vn[n - 1];
            if (rhat >> 64) break;
        }
        // multiply and subtract
        u128 borrow = 0, carry = 0;
        for (size_t i = 0; i < n; i++) {
            const u128 p = (u128)(uint64_t)qhat * vn[i] + carry;
            carry = p >> 64;
            const u128 t = (u128)un[i + j] - (uint64_t)p - borrow;
            un[i + j] = (uint64_t)t;
            borrow = (t >> 64) & 1;
        }
        const u128 t = (u128)un[j + n] - carry - borrow;
        un[j + n] = (uint64_t)t;
        if ((t >> 64) & 1) {      // qhat was one too large: add back
            qhat--;
            u128 c = 0;
            for (size_t i = 0; i < n; i++) {
                c += (u128)un[i + j] + vn[i];
                un[i + j] = (uint64_t)c;
                c >>= 64;
            }
            un[j + n] += (uint64_t)c;
        }
        q[j] = (uint64_t)qhat;
    }
    r.assign(n, 0);
    for (size_t i = 0; i < n; i++) r[i] = s ? (un[i] >> s) | (un[i + 1] << (64 - s)) : un[i];
    big_trim(q);
    big_trim(r);
}
inline Big big_sub(const Big& a, const Big& b, bool& negative) {      // a - b over max(len) limbs
    const size_t n = std::max(a.size(), b.size());
    Big r(n, 0);
    u128 borrow = 0;
    for (size_t i = 0; i < n; i++) {
        const u128 d = (u128)(i < a.size() ? a[i] : 0) - (i < b.size() ? b[i] : 0) - borrow;
        r[i] = (uint64_t)d;
        borrow = (d >> 64) & 1;
    }
    negative = borrow != 0;
    return r;
}
inline Big big_limbs(const Big& a, size_t n) {
    Big r(n, 0);
    for (size_t i = 0; i < std::min(n, a.size()); i++) r[i] = a[i];
    return r;
}

} }   // namespace synth
