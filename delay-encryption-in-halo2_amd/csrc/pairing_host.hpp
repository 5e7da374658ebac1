// pairing_host.hpp -- the BN254 pairing check on the host: prod_i e(P_i, Q_i) == 1, what a KZG verifier ends with [UPSTREAM halo2_proofs/src/poly/kzg/strategy.rs:
// the guard's final `multi_miller_loop(..).final_exponentiation().is_identity()`, halo2curves bn256 engine].  Written from the textbook construction, not from a
// source: the tower Fq2 = Fq[i] / (i^2 + 1), Fq6 = Fq2[v] / (v^3 - xi), Fq12 = Fq6[w] / (w^2 - v) with xi = 9 + i, the optimal ate Miller loop over 6x + 2 with its
// two Frobenius line steps, and the final exponentiation (q^12 - 1) / r = (q^6 - 1)(q^2 + 1) . (q^4 - q^2 + 1) / r, the last factor by plain square-and-multiply.
// The only typed constant is the curve parameter x: the Frobenius coefficient xi^((q - 1) / 6) and the hard exponent (q^4 - q^2 + 1) / r are computed at first use
// from q, r and xi.  O(1) per proof: affine line steps with one Fq2 inversion each, no sparse multiplication -- a check costs milliseconds beside a proof's.
// Host only, no HIP header: transcript.hip includes it, and tests/native_host/pairing_check.cpp drives it on the CPU against an independent pairing's verdicts.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/dehalo.h"
#include "hostfield.hpp"
#include "params_format.hpp"

constexpr uint64_t BN254_X = 4965661367192848881ull;      // the BN parameter: q and r are polynomials in it, the ate loop runs over 6x + 2

struct Fq6 { Fq2 a, b, c; };       // a + b v + c v^2
struct Fq12 { Fq6 a, b; };         // a + b w

struct PairingHost {
    const HostField *q, *r;
    G2Host e2;
    Fq2 xi{}, frob1{};                       // 9 + i; xi^((q - 1) / 6): w^q = frob1 . w
    Fq2 frob[6] = {};                        // frob1^j: the factor of w^j under the q-power Frobenius
    std::vector<uint64_t> hard;              // (q^4 - q^2 + 1) / r, little-endian limbs
    bool ok = false;                         // the derived constants passed their own checks (6 | q - 1, r | q^4 - q^2 + 1, w^(q^2) of order 6)

    // ---- little-endian multi-limb integers, for the two exponents only
    typedef std::vector<uint64_t> Big;
    static Big big_mul(const Big& x, const Big& y) {
        Big z(x.size() + y.size(), 0);
        for (size_t i = 0; i < x.size(); i++) {
            unsigned __int128 c = 0;
            for (size_t j = 0; j < y.size(); j++) {
                c += (unsigned __int128)x[i] * y[j] + z[i + j];
                z[i + j] = (uint64_t)c;
                c >>= 64;
            }
            z[i + y.size()] = (uint64_t)c;
        }
        return z;
    }
    static bool big_geq(const Big& x, const Big& y) {      // equal lengths
        for (size_t i = x.size(); i-- > 0;) {
            if (x[i] != y[i]) return x[i] > y[i];
        }
        return true;
    }
    static void big_sub(Big& x, const Big& y) {             // x -= y, x >= y, y no longer than x
        uint64_t br = 0;
        for (size_t i = 0; i < x.size(); i++) {
            const uint64_t yi = i < y.size() ? y[i] : 0;
            const unsigned __int128 d = (unsigned __int128)x[i] - yi - br;
            x[i] = (uint64_t)d;
            br = (uint64_t)(d >> 64) & 1;
        }
    }
    // x / d by shift and subtract; *exact = the remainder is zero
    static Big big_div(const Big& x, const Big& d, bool* exact) {
        Big quo(x.size(), 0), rem(d.size() + 1, 0), dd(d);
        dd.push_back(0);
        for (size_t bit = 64 * x.size(); bit-- > 0;) {
            for (size_t i = rem.size(); i-- > 1;) rem[i] = (rem[i] << 1) | (rem[i - 1] >> 63);
            rem[0] = (rem[0] << 1) | ((x[bit >> 6] >> (bit & 63)) & 1);
            if (big_geq(rem, dd)) {
                big_sub(rem, dd);
                quo[bit >> 6] |= (uint64_t)1 << (bit & 63);
            }
        }
        bool zero = true;
        for (uint64_t w : rem) zero = zero && w == 0;
        *exact = zero;
        return quo;
    }

    explicit PairingHost(const HostField* fq, const HostField* fr) : q(fq), r(fr), e2(fq) {
        xi = {q->from_u64(9), q->one};
        // (q - 1) / 6
        Big qm1(q->p, q->p + 4), six{6};
        qm1[0] -= 1;
        bool exact6 = false, exact_r = false;
        const Big e6 = big_div(qm1, six, &exact6);
        frob1 = pow2(xi, e6);
        frob[0] = {q->one, Fe{}};
        for (int j = 1; j < 6; j++) frob[j] = e2.mul(frob[j - 1], frob1);
        // (q^4 - q^2 + 1) / r
        const Big qq(q->p, q->p + 4), q2 = big_mul(qq, qq);
        Big n = big_mul(q2, q2);
        big_sub(n, q2);
        {   // n += 1
            uint64_t c = 1;
            for (size_t i = 0; i < n.size() && c; i++) { n[i] += c; c = n[i] == 0; }
        }
        hard = big_div(n, Big(r->p, r->p + 4), &exact_r);
        // a check that the constants came out as meant: frob1^6 . xi = xi^q, and the q-power Frobenius of Fq2 is the conjugation
        const Fq2 six_th = e2.mul(e2.mul(frob[3], frob[3]), xi);
        ok = exact6 && exact_r && e2.eq(six_th, conj2(xi));
    }

    // ---- Fq2 beyond G2Host
    Fq2 conj2(const Fq2& x) const { return {x.a, q->neg(x.b)}; }
    Fq2 mul_xi(const Fq2& x) const { return e2.mul(x, xi); }
    Fq2 pow2(const Fq2& x, const Big& e) const {
        Fq2 acc{q->one, Fe{}};
        for (size_t bit = 64 * e.size(); bit-- > 0;) {
            acc = e2.mul(acc, acc);
            if ((e[bit >> 6] >> (bit & 63)) & 1) acc = e2.mul(acc, x);
        }
        return acc;
    }
    Fq2 zero2() const { return {Fe{}, Fe{}}; }
    Fq2 one2() const { return {q->one, Fe{}}; }

    // ---- Fq6
    Fq6 add6(const Fq6& x, const Fq6& y) const { return {e2.add(x.a, y.a), e2.add(x.b, y.b), e2.add(x.c, y.c)}; }
    Fq6 sub6(const Fq6& x, const Fq6& y) const { return {e2.sub(x.a, y.a), e2.sub(x.b, y.b), e2.sub(x.c, y.c)}; }
    Fq6 neg6(const Fq6& x) const { return {e2.neg(x.a), e2.neg(x.b), e2.neg(x.c)}; }
    Fq6 mul6(const Fq6& x, const Fq6& y) const {      // schoolbook with v^3 = xi
        const Fq2 aa = e2.mul(x.a, y.a), ab = e2.mul(x.a, y.b), ac = e2.mul(x.a, y.c), ba = e2.mul(x.b, y.a), bb = e2.mul(x.b, y.b), bc = e2.mul(x.b, y.c),
                  ca = e2.mul(x.c, y.a), cb = e2.mul(x.c, y.b), cc = e2.mul(x.c, y.c);
        return {e2.add(aa, mul_xi(e2.add(bc, cb))), e2.add(e2.add(ab, ba), mul_xi(cc)), e2.add(e2.add(ac, bb), ca)};
    }
    Fq6 mul6_v(const Fq6& x) const { return {mul_xi(x.c), x.a, x.b}; }
    Fq6 inv6(const Fq6& x) const {
        const Fq2 t0 = e2.sub(e2.mul(x.a, x.a), mul_xi(e2.mul(x.b, x.c))), t1 = e2.sub(mul_xi(e2.mul(x.c, x.c)), e2.mul(x.a, x.b)),
                  t2 = e2.sub(e2.mul(x.b, x.b), e2.mul(x.a, x.c));
        const Fq2 n = e2.inv(e2.add(e2.mul(x.a, t0), mul_xi(e2.add(e2.mul(x.c, t1), e2.mul(x.b, t2)))));
        return {e2.mul(t0, n), e2.mul(t1, n), e2.mul(t2, n)};
    }
    bool eq6(const Fq6& x, const Fq6& y) const { return e2.eq(x.a, y.a) && e2.eq(x.b, y.b) && e2.eq(x.c, y.c); }

    // ---- Fq12
    Fq12 one12() const { return {{one2(), zero2(), zero2()}, {zero2(), zero2(), zero2()}}; }
    Fq12 mul12(const Fq12& x, const Fq12& y) const {
        const Fq6 aa = mul6(x.a, y.a), bb = mul6(x.b, y.b);
        return {add6(aa, mul6_v(bb)), add6(mul6(x.a, y.b), mul6(x.b, y.a))};
    }
    Fq12 conj12(const Fq12& x) const { return {x.a, neg6(x.b)}; }      // the q^6-power Frobenius
    Fq12 inv12(const Fq12& x) const {
        const Fq6 n = inv6(sub6(mul6(x.a, x.a), mul6_v(mul6(x.b, x.b))));
        return {mul6(x.a, n), neg6(mul6(x.b, n))};
    }
    bool is_one12(const Fq12& x) const { const Fq12 o = one12(); return eq6(x.a, o.a) && eq6(x.b, o.b); }
    // the q-power Frobenius: with x = sum_j c_j w^j (c_j in Fq2; w^0, w^2, w^4 = a.a, a.b, a.c and w^1, w^3, w^5 = b.a, b.b, b.c), x^q = sum_j conj(c_j) frob[j] w^j
    Fq12 frobenius(const Fq12& x) const {
        return {{conj2(x.a.a), e2.mul(conj2(x.a.b), frob[2]), e2.mul(conj2(x.a.c), frob[4])},
                {e2.mul(conj2(x.b.a), frob[1]), e2.mul(conj2(x.b.b), frob[3]), e2.mul(conj2(x.b.c), frob[5])}};
    }
    Fq12 pow12(const Fq12& x, const Big& e) const {
        Fq12 acc = one12();
        for (size_t bit = 64 * e.size(); bit-- > 0;) {
            acc = mul12(acc, acc);
            if ((e[bit >> 6] >> (bit & 63)) & 1) acc = mul12(acc, x);
        }
        return acc;
    }

    // ---- Miller loop.  A point (x', y') of the twist stands for (x' w^2, y' w^3) on E(Fq12); a line of twist slope lam through T = (xt, yt), evaluated at
    // P = (xp, yp) in G1, is  yp - lam xp w + (lam xt - yt) w^3  (up to a factor in Fq, which the final exponentiation removes).
    Fq12 line(const Fq2& lam, const G2Host::Pt& T, const Fe& xp, const Fe& yp) const {
        Fq12 l = {{{yp, Fe{}}, zero2(), zero2()}, {zero2(), zero2(), zero2()}};
        l.b.a = e2.neg({q->mul(lam.a, xp), q->mul(lam.b, xp)});
        l.b.b = e2.sub(e2.mul(lam, T.x), T.y);
        return l;
    }
    // f <- f . l_{T, S}(P), T <- T + S (S = T: the tangent).  A vertical line (T = -S) lies in a proper subfield and contributes 1.
    void step(Fq12& f, G2Host::Pt& T, const G2Host::Pt& S, const Fe& xp, const Fe& yp) const {
        if (T.inf || S.inf) { T = e2.padd(T, S); return; }
        Fq2 lam;
        if (e2.eq(T.x, S.x)) {
            if (!e2.eq(T.y, S.y) || e2.is_zero(T.y)) { T = G2Host::Pt{{}, {}, true}; return; }
            const Fq2 xx = e2.mul(T.x, T.x);
            lam = e2.mul(e2.add(e2.add(xx, xx), xx), e2.inv(e2.add(T.y, T.y)));
        } else lam = e2.mul(e2.sub(S.y, T.y), e2.inv(e2.sub(S.x, T.x)));
        f = mul12(f, line(lam, T, xp, yp));
        T = e2.padd(T, S);
    }
    // pi(Q) on the twist: (conj(x) xi^((q-1)/3), conj(y) xi^((q-1)/2))
    G2Host::Pt frob_pt(const G2Host::Pt& Q) const { return G2Host::Pt{e2.mul(conj2(Q.x), frob[2]), e2.mul(conj2(Q.y), frob[3]), false}; }
    // f_{6x+2, Q}(P) . l_{[6x+2]Q, pi(Q)}(P) . l_{[6x+2]Q + pi(Q), -pi^2(Q)}(P); 1 when either point is the identity
    Fq12 miller(const Fe& xp, const Fe& yp, bool p_inf, const G2Host::Pt& Q) const {
        Fq12 f = one12();
        if (p_inf || Q.inf) return f;
        const unsigned __int128 loop = (unsigned __int128)6 * BN254_X + 2;      // 65 bits, the top one implicit in T = Q
        G2Host::Pt T = Q;
        for (int i = 63; i >= 0; i--) {
            f = mul12(f, f);
            step(f, T, T, xp, yp);
            if ((uint64_t)(loop >> i) & 1) step(f, T, Q, xp, yp);
        }
        const G2Host::Pt Q1 = frob_pt(Q);
        G2Host::Pt Q2 = frob_pt(Q1);
        Q2.y = e2.neg(Q2.y);
        step(f, T, Q1, xp, yp);
        step(f, T, Q2, xp, yp);
        return f;
    }
    Fq12 final_exponentiation(const Fq12& f) const {
        const Fq12 a = mul12(conj12(f), inv12(f));             // f^(q^6 - 1)
        const Fq12 b = mul12(frobenius(frobenius(a)), a);      // ^(q^2 + 1)
        return pow12(b, hard);
    }

    // ---- The line table of a FIXED Q (a KZG verifier's g2 and s_g2): everything miller() does on the twist depends on Q alone, so it is done once.  Step by
    // step in miller()'s own order -- for i = 63 .. 0 the tangent, then the addition where bit i of 6x + 2 is set, then pi(Q) and -pi^2(Q): 64 + 36 + 2 = 102
    // steps -- the table keeps lam and lam xt - yt, the two values line() needs besides xp and yp.  one: Q is the identity, the factor 1, no steps.
    static constexpr size_t LINE_STEPS = 102;
    struct LineTable { std::vector<Fq2> lines; bool one = false; };      // lines: lam | lam xt - yt per step
    // step()'s slope and T <- T + S; false: a degenerate step (T or S at infinity, a vertical line), which a Q of order r never meets
    bool table_step(G2Host::Pt& T, const G2Host::Pt& S, LineTable& t) const {
        if (T.inf || S.inf) return false;
        Fq2 lam;
        if (e2.eq(T.x, S.x)) {
            if (!e2.eq(T.y, S.y) || e2.is_zero(T.y)) return false;
            const Fq2 xx = e2.mul(T.x, T.x);
            lam = e2.mul(e2.add(e2.add(xx, xx), xx), e2.inv(e2.add(T.y, T.y)));
        } else lam = e2.mul(e2.sub(S.y, T.y), e2.inv(e2.sub(S.x, T.x)));
        t.lines.push_back(lam);
        t.lines.push_back(e2.sub(e2.mul(lam, T.x), T.y));
        T = e2.padd(T, S);
        return true;
    }
    // Q as load_g2 left it; false: a degenerate step
    bool line_table(const G2Host::Pt& Q, LineTable& t) const {
        t.lines.clear();
        t.one = Q.inf;
        if (Q.inf) return true;
        const unsigned __int128 loop = (unsigned __int128)6 * BN254_X + 2;
        G2Host::Pt T = Q;
        for (int i = 63; i >= 0; i--) {
            if (!table_step(T, T, t)) return false;
            if (((uint64_t)(loop >> i) & 1) && !table_step(T, Q, t)) return false;
        }
        const G2Host::Pt Q1 = frob_pt(Q);
        G2Host::Pt Q2 = frob_pt(Q1);
        Q2.y = e2.neg(Q2.y);
        return table_step(T, Q1, t) && table_step(T, Q2, t) && t.lines.size() == 2 * LINE_STEPS;
    }
    // line() from a table's step
    Fq12 table_line(const Fq2& lam, const Fq2& mu, const Fe& xp, const Fe& yp) const {
        Fq12 l = {{{yp, Fe{}}, zero2(), zero2()}, {zero2(), zero2(), zero2()}};
        l.b.a = e2.neg({q->mul(lam.a, xp), q->mul(lam.b, xp)});
        l.b.b = mu;
        return l;
    }
    // miller() of the table's Q, word for word
    Fq12 miller_table(const Fe& xp, const Fe& yp, bool p_inf, const LineTable& t) const {
        Fq12 f = one12();
        if (p_inf || t.one) return f;
        const unsigned __int128 loop = (unsigned __int128)6 * BN254_X + 2;
        const Fq2* ln = t.lines.data();
        for (int i = 63; i >= 0; i--) {
            f = mul12(f, f);
            f = mul12(f, table_line(ln[0], ln[1], xp, yp));
            ln += 2;
            if ((uint64_t)(loop >> i) & 1) { f = mul12(f, table_line(ln[0], ln[1], xp, yp)); ln += 2; }
        }
        f = mul12(f, table_line(ln[0], ln[1], xp, yp));
        return mul12(f, table_line(ln[2], ln[3], xp, yp));
    }
    // an Fq12 value as the C ABI hands it out: the Fq2 coefficients of w^0 .. w^5, a | b each, 48 words
    void store12(const Fq12& x, uint64_t out[48]) const {
        const Fq2* c[6] = {&x.a.a, &x.b.a, &x.a.b, &x.b.b, &x.a.c, &x.b.c};
        for (int j = 0; j < 6; j++) {
            memcpy(out + 8 * j, c[j]->a.v, 32);
            memcpy(out + 8 * j + 4, c[j]->b.v, 32);
        }
    }
    // checks independent checks over the same tables: status[c] = DEHALO_PAIRING_ONE iff prod_j e(P[c][j], Q_j) = 1, _OFF_CURVE (and gt zero words) for a P off
    // y^2 = x^3 + 3; gt (may be null): 48 words a check
    void table_checks(const std::vector<LineTable>& tables, const uint64_t* g1_affine_xy, uint32_t checks, uint8_t* status, uint64_t* gt) const {
        const size_t pairs = tables.size();
        for (uint32_t c = 0; c < checks; c++) {
            Fq12 f = one12();
            bool on_curve = true;
            for (size_t j = 0; j < pairs && on_curve; j++) {
                Fe x, y;
                bool inf;
                on_curve = load_g1(g1_affine_xy + 8 * ((size_t)c * pairs + j), x, y, inf);
                if (on_curve) f = mul12(f, miller_table(x, y, inf, tables[j]));
            }
            if (!on_curve) {
                status[c] = DEHALO_PAIRING_OFF_CURVE;
                if (gt) memset(gt + 48 * (size_t)c, 0, 48 * 8);
                continue;
            }
            const Fq12 g = final_exponentiation(f);
            status[c] = is_one12(g) ? DEHALO_PAIRING_ONE : DEHALO_PAIRING_NOT_ONE;
            if (gt) store12(g, gt + 48 * (size_t)c);
        }
    }

    // ---- points as the C ABI hands them over
    // G1: affine x | y, Montgomery words standing for their residues; (0, 0) words = the identity.  false: not on y^2 = x^3 + 3
    bool load_g1(const uint64_t xy[8], Fe& x, Fe& y, bool& inf) const {
        memcpy(x.v, xy, 32);
        memcpy(y.v, xy + 4, 32);
        inf = x.is_zero() && y.is_zero();
        if (inf) return true;
        x = q->mul(x, q->one);      // a word not below q stands for its residue
        y = q->mul(y, q->one);
        return q->sqr(y) == q->add(q->mul(q->sqr(x), x), q->from_u64(3));
    }
    // G2: the 128-byte raw form; 0, or the reason it is refused
    enum { G2_OK = 0, G2_NOT_BELOW_Q = 1, G2_OFF_CURVE = 2, G2_NOT_IN_SUBGROUP = 3 };
    int load_g2(const uint8_t raw[128], G2Host::Pt& Q, bool subgroup_known = false) const {
        const int st = e2.from_raw_checked(raw, Q);
        if (st) return st == POINT_NOT_BELOW_P ? G2_NOT_BELOW_Q : G2_OFF_CURVE;
        if (Q.inf || subgroup_known) return G2_OK;
        return e2.scalar_mul(r->p, Q).inf ? G2_OK : G2_NOT_IN_SUBGROUP;      // the twist's group has a cofactor: [r] Q = O is the membership test
    }

    // prod_i e(P_i, Q_i) == 1: one final exponentiation over the product of the Miller loops.  DEHALO_ERR_INVALID for a point off its curve or subgroup.
    // g2_subgroup_known: the caller has put every Q_i through load_g2 before (a verifier's g2 and s_g2, checked once when it is made): the [r] Q test is skipped.
    int check(const uint64_t* g1_affine_xy, const uint8_t* g2_raw, size_t count, int* is_one, bool g2_subgroup_known = false) const {
        if (!ok) return DEHALO_ERR_UNSUPPORTED;
        Fq12 f = one12();
        for (size_t i = 0; i < count; i++) {
            Fe x, y;
            bool inf;
            G2Host::Pt Q;
            if (!load_g1(g1_affine_xy + 8 * i, x, y, inf) || load_g2(g2_raw + 128 * i, Q, g2_subgroup_known) != G2_OK) return DEHALO_ERR_INVALID;
            f = mul12(f, miller(x, y, inf, Q));
        }
        *is_one = is_one12(final_exponentiation(f)) ? 1 : 0;
        return 0;
    }
};

// the one pairing-friendly curve of the library; nullptr for the others
inline const PairingHost* pairing_host(int curve) {
    if (curve != DEHALO_CURVE_BN254_G1) return nullptr;
    static const PairingHost bn254(host_field(DEHALO_FIELD_BN254_FQ), host_field(DEHALO_FIELD_BN254_FR));
    return &bn254;
}
