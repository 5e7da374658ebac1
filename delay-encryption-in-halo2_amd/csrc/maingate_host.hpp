// maingate_host.hpp -- the MainGate / RangeChip layouter (dehalo2_amd/witness.py Layouter, row for row): every MainGateInstructions / RangeInstructions call the
// reference makes, laid out the way [UPSTREAM] halo2wrong maingate's `apply` lays it out (term i in column i).  Host only, no HIP include.
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "poseidon_host.hpp"

namespace synth { namespace {

constexpr int LIMB_WIDTH = 64;

enum { MG_SA = 0, MG_SB, MG_SC, MG_SD, MG_SE, MG_MUL_AB, MG_MUL_CD, MG_NEXT, MG_CONST, RC_T_TAG, RC_T_VALUE, RC_TAG_COMPOSITION, RC_TAG_OVERFLOW, RC_S_COMPOSITION, RC_S_OVERFLOW, NUM_FIX };
// RangeChip::configure(composition_bit_lens = [8, 1, 8, 4], overflow_bit_lens = [0, 0, 6]) (src/lib.rs:144-149): the distinct non-zero lengths in
// ascending order carry the tags 1..4
// -- {1, 4, 6, 8} for the reference's 2048-bit modulus.  Only the carries' overflow length depends on the modulus length (compute_range_lens(num_limbs):
// 2 x (num_limbs (2^64 - 1)^2 + 2^64 - 1) has 134 bits at 32 limbs -- 70-bit carries, a 6-bit overflow limb --, 133 at 16 limbs -- 5 bits).
struct RangeLens {
    unsigned bits[5] = {0, 0, 0, 0, 0};
    unsigned count = 0;
    explicit RangeLens(size_t num_limbs) {
        // bit length of 2 * word_max = 1 + bit length of num_limbs * (2^64 - 1)^2 + (2^64 - 1), which is 128 + bit length of num_limbs, less one when num_limbs is
        // a power of two (num_limbs * (2^64 - 1)^2 + 2^64 - 1 < num_limbs * 2^128 for every num_limbs >= 1)
        unsigned bl = 0;
        for (size_t v = num_limbs; v; v >>= 1) bl++;
        const bool pow2 = num_limbs && !(num_limbs & (num_limbs - 1));
        const unsigned wm_bits = 1 + 128 + bl - (pow2 ? 1 : 0);
        const unsigned carry_bits = wm_bits - 64, comp = std::max(1u, carry_bits / 8), over = carry_bits % comp;
        unsigned cand[5] = {1, 4, 8, comp, over};
        std::sort(cand, cand + 5);
        for (unsigned c : cand)
            if (c && (count == 0 || bits[count - 1] != c)) bits[count++] = c;
    }
    uint64_t tag(unsigned b) const {
        for (unsigned i = 0; i < count; i++)
            if (bits[i] == b) return i + 1;
        return 0;
    }
};
constexpr unsigned NUM_LOOKUP_LIMBS = 8;      // src/big_integer/chip.rs:1167
inline unsigned sublimb_bit_len(unsigned bits) { return std::max(1u, bits / NUM_LOOKUP_LIMBS); }

struct NotSatisfied : std::runtime_error { using std::runtime_error::runtime_error; };      // a constraint of the reference's circuit fails for these inputs

struct Cell { int col = -1; uint32_t row = 0; Fe val{}; bool is_cell() const { return col >= 0; } };
struct Arg {      // a cell (copied), a value, or nothing (0)
    Cell c;
    Arg() { c.val = Fe{{0, 0, 0, 0}}; }
    Arg(const Cell& cell) : c(cell) {}
    Arg(const Fe& v) { c.val = v; }
};
struct Sel { int col; Fe val; };
struct Copy { uint32_t c0, r0, c1, r1; };

struct Layouter {
    Fld F;
    bool want_fixed;                 // fixed columns and copies are only needed at keygen
    std::vector<Fe> fix[NUM_FIX];
    std::vector<Copy> copies;
    RangeLens range{32};             // the RangeChip table this circuit configures (dehalo_synthesize sets it from the modulus length)
    uint64_t range_tag(unsigned bits) const { return range.tag(bits); }
    Layouter(const HostField* f, bool fixed_too, uint64_t* advice, size_t n) : F{f}, want_fixed(fixed_too), cap(n) {
        if (!advice) own.resize(5 * n);
        Fe* base = advice ? reinterpret_cast<Fe*>(advice) : own.data();
        for (int i = 0; i < 5; i++) adv[i] = base + (size_t)i * n;
        one_ = F.u(1); m1_ = F.neg(one_);
    }
    // a second cursor over the same columns, starting at row `start` (proving only: no fixed columns, no copies): the rows of independent regions whose
    // positions are known in advance are written by several host threads at once (BigIntChip::pow_mod); rows() tells where it ended
    Layouter(const Layouter& parent, uint32_t start) : F(parent.F), want_fixed(false), range(parent.range), cap(parent.cap), nrows(start), one_(parent.one_), m1_(parent.m1_) {
        for (int i = 0; i < 5; i++) adv[i] = parent.adv[i];
    }
    uint32_t rows() const { return nrows; }
    void advance_to(uint32_t r) { nrows = r; }      // behind regions that second cursors wrote

    void row(const Arg* cells, int ncells, const Sel* sel, int nsel, Cell out[5]) {
        const uint32_t r = nrows++;
        const bool store = r < cap;
        for (int i = 0; i < 5; i++) {
            Fe v{{0, 0, 0, 0}};
            if (i < ncells) {
                v = cells[i].c.val;
                if (cells[i].c.is_cell() && want_fixed) copies.push_back(Copy{(uint32_t)cells[i].c.col, cells[i].c.row, (uint32_t)i, r});
            }
            if (store) adv[i][r] = v;
            out[i].col = i; out[i].row = r; out[i].val = v;
        }
        if (want_fixed) {
            for (auto& col : fix) col.push_back(Fe{{0, 0, 0, 0}});
            for (int i = 0; i < nsel; i++) fix[sel[i].col][r] = sel[i].val;
        }
    }
    // proving only: a row of five values, nothing copied, no fixed columns; the row's index
    uint32_t value_row(const Fe& a, const Fe& b, const Fe& c, const Fe& d, const Fe& e) {
        const uint32_t r = nrows++;
        if (r < cap) { adv[0][r] = a; adv[1][r] = b; adv[2][r] = c; adv[3][r] = d; adv[4][r] = e; }
        return r;
    }
    template <int NC, int NS> Cell apply(const Arg (&x)[NC], const Sel (&s)[NS], int ret) {      // one row; its cell in column `ret`
        Cell o[5];
        row(x, NC, s, NS, o);
        return o[ret];
    }
    const Fe& one() const { return one_; }
    const Fe& m1() const { return m1_; }
    [[noreturn]] void fail(const char* what) const { throw NotSatisfied(std::string(what) + " at row " + std::to_string(nrows)); }

    // --- MainGateInstructions, one row each unless said otherwise
    Cell assign_value(const Fe& v) { Cell o[5]; Arg a[1] = {Arg(v)}; row(a, 1, nullptr, 0, o); return o[0]; }
    Cell assign_constant(const Fe& c) { return apply({Arg(c)}, {{MG_SA, m1()}, {MG_CONST, c}}, 0); }      // -a + c = 0
    Cell assign_bit(uint64_t b) {      // a b - c = 0 with a = b = c
        const Fe v = F.u(b);
        const Cell o = apply({Arg(v), Arg(v), Arg(v)}, {{MG_MUL_AB, one()}, {MG_SC, m1()}}, 2);
        if (want_fixed) { copies.push_back(Copy{0, o.row, 1, o.row}); copies.push_back(Copy{1, o.row, 2, o.row}); }
        return o;
    }
    void assert_equal(const Cell& a, const Cell& b) {      // a - b = 0
        if (!(a.val == b.val)) fail("assert_equal on different values");
        apply({Arg(a), Arg(b)}, {{MG_SA, one()}, {MG_SB, m1()}}, 0);
    }
    void assert_one(const Cell& a) {
        if (!(a.val == one())) fail("assert_one fails");
        apply({Arg(a)}, {{MG_SA, one()}, {MG_CONST, m1()}}, 0);
    }
    Cell add_with_constant(const Cell& a, const Cell& b, const Fe& constant) {
        return apply({Arg(a), Arg(b), Arg(F.add(F.add(a.val, b.val), constant))}, {{MG_SA, one()}, {MG_SB, one()}, {MG_SC, m1()}, {MG_CONST, constant}}, 2);
    }
    Cell add(const Cell& a, const Cell& b) { return add_with_constant(a, b, F.zero()); }
    Cell sub(const Cell& a, const Cell& b) { return apply({Arg(a), Arg(b), Arg(F.sub(a.val, b.val))}, {{MG_SA, one()}, {MG_SB, m1()}, {MG_SC, m1()}}, 2); }
    Cell add_constant(const Cell& a, const Fe& constant) {
        return apply({Arg(a), Arg(F.add(a.val, constant))}, {{MG_SA, one()}, {MG_SB, m1()}, {MG_CONST, constant}}, 1);
    }
    Cell mul(const Arg& a, const Arg& b) { return apply({a, b, Arg(F.mul(a.c.val, b.c.val))}, {{MG_MUL_AB, one()}, {MG_SC, m1()}}, 2); }
    Cell mul_add(const Arg& a, const Arg& b, const Arg& c) {
        return apply({a, b, c, Arg(F.add(F.mul(a.c.val, b.c.val), c.c.val))}, {{MG_MUL_AB, one()}, {MG_SC, one()}, {MG_SD, m1()}}, 3);
    }
    Cell mul_add_constant(const Cell& a, const Cell& b, const Fe& constant) {
        return apply({Arg(a), Arg(b), Arg(F.add(F.mul(a.val, b.val), constant))}, {{MG_MUL_AB, one()}, {MG_SC, m1()}, {MG_CONST, constant}}, 2);
    }
    Cell and_(const Cell& a, const Cell& b) { return mul(Arg(a), Arg(b)); }
    Cell not_(const Cell& c) {      // c + not_c - 1 = 0
        return apply({Arg(c), Arg(F.sub(one(), c.val))}, {{MG_SA, one()}, {MG_SB, one()}, {MG_CONST, m1()}}, 1);
    }
    Cell select(const Cell& a, const Cell& b, const Cell& cond) {      // cond a - cond b + b - res = 0, columns | cond | a | cond | b | res |
        return apply({Arg(cond), Arg(a), Arg(cond), Arg(b), Arg(cond.val.is_zero() ? b.val : a.val)}, {{MG_MUL_AB, one()}, {MG_MUL_CD, m1()}, {MG_SD, one()}, {MG_SE, m1()}}, 4);
    }
    Cell is_equal(const Cell& a, const Cell& b) {      // four rows: r (a bit), dif = a - b, u = r - r x + x, dif u + r - 1 = 0  (x = 1 / dif, or 1 when dif = 0)
        const Fe dv = F.sub(a.val, b.val);
        const bool eq = dv.is_zero();
        const Fe x = eq ? one() : F.inv(dv);
        const Cell r = assign_bit(eq ? 1 : 0);
        const Cell dif = sub(a, b);
        // u = r - r x + x = x in both cases (r = 0: x; r = 1: x = 1)
        const Cell u = apply({Arg(r), Arg(x), Arg(r), Arg(x), Arg(x)}, {{MG_MUL_AB, one()}, {MG_SC, m1()}, {MG_SD, m1()}, {MG_SE, one()}}, 4);
        apply({Arg(dif), Arg(u), Arg(r)}, {{MG_MUL_AB, one()}, {MG_SC, one()}, {MG_CONST, m1()}}, 0);
        return r;
    }
    Cell is_zero(const Cell& a) {      // MainGate::invert's flag, three rows: r (a bit), a a' + r - 1 = 0, r a' - r = 0
        const bool z = a.val.is_zero();
        const Fe a_inv = z ? one() : F.inv(a.val);
        const Cell r = assign_bit(z ? 1 : 0);
        const Cell inv = apply({Arg(a), Arg(a_inv), Arg(r)}, {{MG_MUL_AB, one()}, {MG_SC, one()}, {MG_CONST, m1()}}, 1);
        apply({Arg(r), Arg(inv), Arg(r)}, {{MG_MUL_AB, one()}, {MG_SC, m1()}}, 0);
        return r;
    }
    // compose: four terms a row, column e holds what is still to be added (the total in the first row).  prod[i] = coeff[i] * cells[i].val (the caller's
    // cheapest way to it); coeff is only read at keygen
    Cell compose(const Cell* cells, const Fe* coeff, const Fe* prod, int n, const Fe& constant) {
        Fe remaining = constant;
        for (int i = 0; i < n; i++) remaining = F.add(remaining, prod[i]);
        Cell result, o[5];
        for (int g = 0; g < n; g += 4) {
            const int cnt = std::min(4, n - g);
            const bool last = g + 4 >= n;
            Arg a[5];
            Sel s[8];
            int ns = 0;
            for (int i = 0; i < cnt; i++) {
                a[i] = Arg(cells[g + i]);
                if (want_fixed) s[ns++] = {MG_SA + i, coeff[g + i]};
            }
            a[4] = Arg(remaining);
            s[ns++] = {MG_SE, m1()};
            if (!last) s[ns++] = {MG_NEXT, one()};
            if (g == 0) s[ns++] = {MG_CONST, constant};
            row(a, 5, s, ns, o);
            if (g == 0) { result = o[4]; remaining = F.sub(remaining, constant); }
            for (int i = 0; i < cnt; i++) remaining = F.sub(remaining, prod[g + i]);
        }
        return result;
    }
    std::vector<Cell> to_bits(const Cell& v, unsigned nbits) {
        if (nbits < 64 ? (v.val.v[0] >> nbits) != 0 || v.val.v[1] || v.val.v[2] || v.val.v[3] : (v.val.v[1] || v.val.v[2] || v.val.v[3])) fail("to_bits: the value does not fit");
        std::vector<Cell> bits;
        std::vector<Fe> coeff, prod;
        for (unsigned i = 0; i < nbits; i++) {
            bits.push_back(assign_bit((v.val.v[0] >> i) & 1));
            coeff.push_back(F.pow2(i));
            prod.push_back(bits.back().val.is_zero() ? F.zero() : coeff.back());
        }
        assert_equal(compose(bits.data(), coeff.data(), prod.data(), (int)nbits, F.zero()), v);
        return bits;
    }
    // RangeInstructions::assign: `limb_bits`-bit limbs four to a row with the composition lookup on a..d, the (bit_len mod limb_bits)-bit overflow limb
    // last, alone in column a of its row, with the overflow lookup.  value < 2^bit_len <= 2^128; the first row's e is the value, the later rows' what is left.
    Cell range_assign(u128 value, unsigned limb_bits, unsigned bit_len) {
        if (bit_len < 128 && (value >> bit_len)) fail("range_assign: the value does not fit");
        const unsigned full = bit_len / limb_bits, over = bit_len % limb_bits, nl = full + (over ? 1 : 0);
        if (over && full % 4) throw std::runtime_error("the overflow limb must open a row");
        if (!range_tag(limb_bits) || (over && !range_tag(over))) fail("range_assign: the range table has no rows for this bit length");
        const u128 mask = ((u128)1 << limb_bits) - 1;
        Cell result, o[5];
        for (unsigned g = 0; g < nl; g += 4) {
            const unsigned cnt = std::min(4u, nl - g);
            const bool last = g + 4 >= nl;
            Arg a[5];
            Sel s[10];
            int ns = 0;
            for (unsigned i = 0; i < cnt; i++) {
                a[i] = Arg(F.u((uint64_t)((value >> (limb_bits * (g + i))) & mask)));
                if (want_fixed) s[ns++] = {MG_SA + (int)i, F.pow2(limb_bits * (g + i))};
            }
            const unsigned sh = limb_bits * g;
            a[4] = Arg(F.from_u128(sh ? (value >> sh) << sh : value));
            if (want_fixed) {
                s[ns++] = {MG_SE, m1()};
                if (!last) s[ns++] = {MG_NEXT, one()};
                s[ns++] = {RC_S_COMPOSITION, one()};
                s[ns++] = {RC_TAG_COMPOSITION, F.u(range_tag(limb_bits))};
                if (last && over) { s[ns++] = {RC_S_OVERFLOW, one()}; s[ns++] = {RC_TAG_OVERFLOW, F.u(range_tag(over))}; }
            }
            row(a, 5, s, ns, o);
            if (g == 0) result = o[4];
        }
        return result;
    }

private:
    // the advice columns are written where they are wanted: straight into the caller's 2^k-row columns (or into `own` when the caller only asks for
    // the summary); rows past the capacity are counted, not stored -- the caller's "not enough rows" check then refuses the circuit
    Fe* adv[5];
    size_t cap;
    uint32_t nrows = 0;
    std::vector<Fe> own;
    Fe one_, m1_;
};

} }   // namespace synth
