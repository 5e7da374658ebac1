// synth_chips.hpp -- the reference's chips over the layouter (maingate_host.hpp), and the regions its three circuits are made of:
//   BigIntChip      src/big_integer/chip.rs: assign_integer :64-85, assign_constant :1255-1285, max_value :141-157, add :250-300, sub :313-376, mul :389-422,
//                   mul_mod :545-632, pow_mod :667-699, is_equal_fresh :778-803, is_equal_muled :825-898, is_less_than :911-923, assert_in_field :1153-1161,
//                   sub_unchecked :1290-1322, div_mod_main_gate :1327-1353
//   PoseidonChip    src/poseidon/chip.rs:199-419
//   rsa_region      RSAChip::{assign_public_key, modpow_public_key} src/rsa/chip.rs:61-73, 102-117; src/lib.rs:179-215
//   hash_region, cipher_region      src/hash/chip.rs:63-85, src/encryption/chip.rs:72-110, src/lib.rs:216-316
// Host only, no HIP include.
#pragma once
#include <chrono>
#include <cstdio>

#include "bigint_host.hpp"
#include "maingate_host.hpp"
#include "synth_pool.hpp"

namespace synth { namespace {

// rows behind an exponentiation that read nothing of it but its VALUE, which the integer chain gives before any row is written: given a cursor at the
// row where the exponentiation will end, and the result's values
typedef std::function<void(Layouter&, const std::vector<Cell>&)> PowTail;
struct PowResult { std::vector<Cell> powed; bool tail_ran; };
struct PowStep { Big acc, sq, q_mul, r_mul, q_sq, r_sq; };      // one exponent bit: the operands, and (quotient, remainder) of acc * sq and of sq^2
struct PowRegions { bool ok, unsat; size_t tasks; uint32_t end; };

// ---- BigIntChip (src/big_integer/chip.rs) ----
struct BigIntChip {
    Layouter& lay;
    size_t num_limbs;
    Big to_big(const std::vector<Cell>& limbs) const {
        Big r;
        for (auto& c : limbs) r.push_back(c.val.v[0]);
        return r;
    }
    std::vector<Cell> value_cells(const Big& x) const {      // values only: nothing of the proving path reads where a cell sits
        std::vector<Cell> out(num_limbs);
        const Big l = big_limbs(x, num_limbs);
        for (size_t i = 0; i < num_limbs; i++) out[i].val = Fe{{l[i], 0, 0, 0}};
        return out;
    }
    Cell range_limb(uint64_t v) { return lay.range_assign(v, sublimb_bit_len(LIMB_WIDTH), LIMB_WIDTH); }
    std::vector<Cell> assign_integer(const Big& x, size_t n) {      // :64-85
        std::vector<Cell> out;
        for (uint64_t v : big_limbs(x, n)) out.push_back(range_limb(v));
        return out;
    }
    // :1255-1285: one row per limb the integer HAS, then one zero row whose cell pads the rest
    std::vector<Cell> assign_constant(Big x, size_t max_num_limbs) {
        big_trim(x);
        if (x.size() > max_num_limbs) throw std::runtime_error("assign_constant: too many limbs");
        std::vector<Cell> out;
        for (uint64_t v : x) out.push_back(lay.assign_constant(lay.F.u(v)));
        const Cell zero = lay.assign_constant(lay.F.zero());
        while (out.size() < max_num_limbs) out.push_back(zero);
        return out;
    }
    std::vector<Cell> max_value(size_t n) {
        std::vector<Cell> out;
        for (size_t i = 0; i < n; i++) out.push_back(lay.assign_constant(lay.F.u(~(uint64_t)0)));
        return out;
    }
    // :250-300: limb sums with range-checked (c, carry) pairs; max(n1, n2) + 1 limbs
    std::vector<Cell> add(std::vector<Cell> a, std::vector<Cell> b) {
        const size_t max_n = std::max(a.size(), b.size());
        const Cell zero = lay.assign_constant(lay.F.zero());
        a.resize(max_n, zero);
        b.resize(max_n, zero);
        Cell carry = zero;
        const Cell limb_max = lay.assign_constant(lay.F.pow2(LIMB_WIDTH));
        std::vector<Cell> out;
        for (size_t i = 0; i < max_n; i++) {
            const Cell s = lay.add(lay.add(a[i], b[i]), carry);
            const Cell c = range_limb(s.val.v[0]);
            if (s.val.v[2] | s.val.v[3]) lay.fail("add: a limb sum left 128 bits");
            carry = range_limb(s.val.v[1]);
            lay.assert_equal(s, lay.mul_add(Arg(carry), Arg(limb_max), Arg(c)));
            out.push_back(c);
        }
        out.push_back(carry);
        return out;
    }
    // :1290-1322: c = a - b as fresh limbs, then a = b + c
    std::vector<Cell> sub_unchecked(const std::vector<Cell>& a, const std::vector<Cell>& b) {
        bool neg = false;
        const Big c_big = big_sub(to_big(a), to_big(b), neg);
        if (neg) lay.fail("sub_unchecked: a < b");
        std::vector<Cell> c;
        for (uint64_t v : big_limbs(c_big, a.size())) c.push_back(range_limb(v));
        assert_equal_fresh(a, add(b, c));
        return c;
    }
    // :313-376: (|a - b|, is_overflowed) through a + max - b
    std::vector<Cell> sub(const std::vector<Cell>& a, const std::vector<Cell>& b, Cell& is_overflowed) {
        const size_t n2 = b.size();
        const std::vector<Cell> max_int = max_value(n2);
        const std::vector<Cell> inflated_subed = sub_unchecked(add(a, max_int), b);
        const Cell one = lay.assign_bit(1);
        const Cell is_not_overflowed = lay.is_equal(inflated_subed[n2], one);
        is_overflowed = lay.not_(is_not_overflowed);
        const size_t num_l = inflated_subed.size(), num_r = std::max(a.size(), n2);
        const Cell zero = lay.assign_constant(lay.F.zero());
        std::vector<Cell> sel_l, sel_r;
        for (size_t i = 0; i < num_l; i++) sel_l.push_back(lay.select(inflated_subed[i], i >= n2 ? zero : b[i], is_not_overflowed));
        for (size_t i = 0; i < num_r; i++) {
            if (i >= a.size()) sel_r.push_back(lay.select(max_int[i], zero, is_not_overflowed));
            else if (i >= n2) sel_r.push_back(lay.select(zero, a[i], is_not_overflowed));
            else sel_r.push_back(lay.select(max_int[i], a[i], is_not_overflowed));
        }
        return sub_unchecked(sel_l, sel_r);
    }
    // :389-422: limb i of the product = sum_{j + k = i} a_j b_k by a chain of mul_add rows
    std::vector<Cell> mul(const std::vector<Cell>& a, const std::vector<Cell>& b) {
        const size_t d0 = a.size(), d1 = b.size();
        // Proving (no fixed columns, no copies wanted) with one-word limbs -- every call of these circuits: the same rows written directly.  A product
        // limb is a sum of <= min(d0, d1) products of two 64-bit words: three words hold it, no field arithmetic is needed (half of all rows of the
        // delay-encryption circuit are these: 1087 per multiplication, 60 multiplications at a 15-bit exponent).
        bool words = !lay.want_fixed && std::min(d0, d1) <= ((size_t)1 << 60);
        for (size_t i = 0; words && i < d0; i++) words = !(a[i].val.v[1] | a[i].val.v[2] | a[i].val.v[3]);
        for (size_t i = 0; words && i < d1; i++) words = !(b[i].val.v[1] | b[i].val.v[2] | b[i].val.v[3]);
        if (words) return mul_words(a, b);
        std::vector<Cell> out;
        for (size_t i = 0; i + 1 < d0 + d1; i++) {
            Cell acc = lay.assign_constant(lay.F.zero());
            for (size_t j = d1 >= i + 1 ? 0 : i + 1 - d1; j < d0 && j <= i; j++) acc = lay.mul_add(Arg(a[j]), Arg(b[i - j]), Arg(acc));
            out.push_back(acc);
        }
        return out;
    }
    std::vector<Cell> mul_words(const std::vector<Cell>& a, const std::vector<Cell>& b) {
        const size_t d0 = a.size(), d1 = b.size();
        std::vector<Cell> out;
        out.reserve(d0 + d1 - 1);
        const Fe zero{{0, 0, 0, 0}};
        for (size_t i = 0; i + 1 < d0 + d1; i++) {
            Cell acc = lay.assign_constant(zero);
            uint64_t w0 = 0, w1 = 0, w2 = 0;
            for (size_t j = d1 >= i + 1 ? 0 : i + 1 - d1; j < d0 && j <= i; j++) {
                const uint64_t x = a[j].val.v[0], y = b[i - j].val.v[0];
                const u128 p = (u128)x * y;
                const u128 s0 = (u128)w0 + (uint64_t)p;
                const u128 s1 = (u128)w1 + (uint64_t)(p >> 64) + (uint64_t)(s0 >> 64);
                const Fe prev{{w0, w1, w2, 0}};
                w0 = (uint64_t)s0; w1 = (uint64_t)s1; w2 += (uint64_t)(s1 >> 64);
                acc.col = 3; acc.val = Fe{{w0, w1, w2, 0}};
                acc.row = lay.value_row(Fe{{x, 0, 0, 0}}, Fe{{y, 0, 0, 0}}, prev, acc.val, zero);
            }
            out.push_back(acc);
        }
        return out;
    }
    // :1327-1353 with n = 2^64 (its only use), five rows: q, a mod n assigned; n q; a - n q; equal to a mod n.  a is far below p.
    void div_mod_limb(const Cell& a, const Cell& limb_max, Cell& q, Cell& r) {
        const Fe qv{{a.val.v[1], a.val.v[2], a.val.v[3], 0}}, rv{{a.val.v[0], 0, 0, 0}};
        q = lay.assign_value(qv);
        r = lay.assign_value(rv);
        lay.assert_equal(r, lay.sub(a, lay.mul(Arg(limb_max), Arg(q))));
    }
    Cell is_equal_fresh(const std::vector<Cell>& a, const std::vector<Cell>& b) {      // :778-803
        const size_t n1 = a.size(), n2 = b.size();
        Cell eq = lay.assign_bit(1);
        for (size_t i = 0; i < std::max(n1, n2); i++) {
            Cell flag;
            if (n1 > n2 && i >= n2) flag = lay.is_zero(a[i]);
            else if (n1 <= n2 && i >= n1) flag = lay.is_zero(b[i]);
            else flag = lay.is_equal(a[i], b[i]);
            eq = lay.and_(eq, flag);
        }
        return eq;
    }
    void assert_equal_fresh(const std::vector<Cell>& a, const std::vector<Cell>& b) { lay.assert_one(is_equal_fresh(a, b)); }
    // :825-898 + assert_one (:1056-1066): a - b + word_max carried limb by limb, carries range-checked
    void assert_equal_muled(const std::vector<Cell>& a, const std::vector<Cell>& b, size_t n1, size_t n2) {
        Fld& F = lay.F;
        const size_t min_n = std::min(n1, n2);
        // word_max = min_n * limb_max^2 + limb_max (compute_mul_word_max): below 2^134 for 32 limbs
        const u128 limb_max_v = ~(uint64_t)0;
        Fe word_max;
        {
            const Fe lm2 = F.mul(F.from_u128(limb_max_v), F.from_u128(limb_max_v));
            word_max = F.add(F.mul(F.u(min_n), lm2), F.from_u128(limb_max_v));
        }
        unsigned wm_bits = 256;      // bit length of 2 * word_max
        {
            Fe two_wm = F.add(word_max, word_max);
            while (wm_bits && !((two_wm.v[(wm_bits - 1) >> 6] >> ((wm_bits - 1) & 63)) & 1)) wm_bits--;
        }
        const unsigned carry_bits = wm_bits - LIMB_WIDTH;
        const Cell limb_max = lay.assign_constant(F.pow2(LIMB_WIDTH));
        Cell accumulated_extra = lay.assign_constant(F.zero());
        Cell carry = lay.assign_constant(F.zero());
        Cell eq_bit = lay.assign_bit(1);
        const size_t num = n1 + n2 - 1;
        for (size_t i = 0; i < num; i++) {
            const Cell s = lay.add_with_constant(lay.sub(a[i], b[i]), carry, word_max);
            if (s.val.v[3]) lay.fail("is_equal_muled: the carried sum left the integers");
            Cell new_carry, c, q_acc, mod_acc;
            div_mod_limb(s, limb_max, new_carry, c);
            accumulated_extra = lay.add_constant(accumulated_extra, word_max);
            div_mod_limb(accumulated_extra, limb_max, q_acc, mod_acc);
            eq_bit = lay.and_(eq_bit, lay.is_equal(c, mod_acc));
            accumulated_extra = q_acc;
            if (i + 1 < num) {
                if (new_carry.val.v[2] | new_carry.val.v[3]) lay.fail("is_equal_muled: a carry left 128 bits");
                const u128 nc = ((u128)new_carry.val.v[1] << 64) | new_carry.val.v[0];
                const Cell ranged = lay.range_assign(nc, sublimb_bit_len(carry_bits), carry_bits);
                eq_bit = lay.and_(eq_bit, lay.is_equal(new_carry, ranged));
            } else {
                eq_bit = lay.and_(eq_bit, lay.is_equal(new_carry, accumulated_extra));
            }
            carry = new_carry;
        }
        lay.assert_one(eq_bit);
    }
    // :911-923, :1153-1161: (a <= b through sub's overflow flag) and not (a == b), asserted
    void assert_in_field(const std::vector<Cell>& a, const std::vector<Cell>& n) {
        Cell is_overflowed;
        sub(a, n, is_overflowed);
        lay.assert_one(lay.and_(is_overflowed, lay.not_(is_equal_fresh(a, n))));
    }
    // :545-632
    std::vector<Cell> mul_mod(const std::vector<Cell>& a, const std::vector<Cell>& b, const std::vector<Cell>& n, const Big& n_big) {
        Big q_big, r_big;
        big_divmod(big_mul(to_big(a), to_big(b)), n_big, q_big, r_big);
        return mul_mod_rows(a, b, n, q_big, r_big);
    }
    // the rows of a * b = q * n + r for a quotient and remainder already known
    std::vector<Cell> mul_mod_rows(const std::vector<Cell>& a, const std::vector<Cell>& b, const std::vector<Cell>& n, const Big& q_big, const Big& r_big) {
        const size_t n1 = a.size(), n2 = b.size();
        std::vector<Cell> q, r;
        for (uint64_t v : big_limbs(q_big, n2)) q.push_back(range_limb(v));
        for (uint64_t v : big_limbs(r_big, n1)) r.push_back(range_limb(v));
        const std::vector<Cell> ab = mul(a, b), qn = mul(q, n);
        std::vector<Cell> eq_b;
        for (size_t i = 0; i + 1 < n1 + n2; i++) eq_b.push_back(i < n1 ? lay.add(qn[i], r[i]) : qn[i]);
        assert_equal_muled(ab, eq_b, n1, n2);
        return r;
    }
    // :667-699: the exponent's limbs into bits, then per bit (LSB first) acc * squared, select, squared^2.  `tail`: see pow_mod_threads
    PowResult pow_mod(const std::vector<Cell>& a, const std::vector<Cell>& e, const std::vector<Cell>& n, const Big& n_big, unsigned exp_limb_bits, const PowTail* tail) {
        std::vector<Cell> e_bits;
        for (auto& limb : e)
            for (auto& b : lay.to_bits(limb, exp_limb_bits)) e_bits.push_back(b);
        std::vector<Cell> acc = assign_constant(Big{1}, num_limbs);      // assign_constant_fresh(1)
        std::vector<Cell> squared = a;
        if (!lay.want_fixed && e_bits.size() >= 3 && synth_threads() > 1) return pow_mod_threads(acc, squared, e_bits, n, n_big, tail);
        for (auto& bit : e_bits) {
            const std::vector<Cell> muled = mul_mod(acc, squared, n, n_big);
            for (size_t j = 0; j < acc.size(); j++) acc[j] = lay.select(muled[j], acc[j], bit);
            squared = mul_mod(squared, squared, n, n_big);
        }
        return {acc, false};
    }

    // Proving (values only): the two multiplications of every exponent bit are regions of a fixed number of rows whose operands follow from the
    // integers alone, so the chain x^(2^i), acc_i is computed first (two 2048-bit products and divisions per bit) and the regions are then written
    // by several host threads, each through a cursor of its own at the row where the sequential order puts it -- the same rows, bit for bit
    // (tests/test_witness.py compares with the one-thread keygen path).  The first bit runs on the caller's cursor and gives the regions' lengths.
    // What follows the exponentiation in the circuit may be given as `tail`: it is then written as one more task beside the multiplication regions.
    typedef std::chrono::steady_clock Clock;
    PowResult pow_mod_threads(const std::vector<Cell>& acc, const std::vector<Cell>& squared, const std::vector<Cell>& e_bits, const std::vector<Cell>& n, const Big& n_big, const PowTail* tail) {
        const auto T0 = Clock::now();
        Big result;
        const std::vector<PowStep> st = pow_chain(to_big(acc), to_big(squared), e_bits, n_big, result);
        const auto T1 = Clock::now();
        // bit 0 on the caller's cursor: the lengths of the two regions
        const uint32_t r0 = lay.rows();
        mul_region(acc, squared, e_bits[0], n, st[0]);
        const uint32_t len_a = lay.rows() - r0;
        mul_mod_rows(squared, squared, n, st[0].q_sq, st[0].r_sq);
        const uint32_t len_b = lay.rows() - r0 - len_a;
        const auto T2 = Clock::now();
        const std::vector<Cell> powed = value_cells(result);
        const PowRegions done = pow_regions(st, e_bits, n, len_a, len_b, powed, tail);
        const auto T3 = Clock::now();
        if (getenv("DEHALO_SYNTH_TRACE")) fprintf(stderr, "pow_mod: chain %.3f ms, bit 0 %.3f ms, %zu regions on %u threads %.3f ms\n", std::chrono::duration<double, std::milli>(T1 - T0).count(), std::chrono::duration<double, std::milli>(T2 - T1).count(), done.tasks, synth_threads(), std::chrono::duration<double, std::milli>(T3 - T2).count());
        if (done.unsat) throw NotSatisfied("a constraint behind the first exponent bit fails");
        if (!done.ok) throw std::runtime_error("pow_mod: a region's length depends on its values");
        lay.advance_to(done.end);
        return {powed, tail != nullptr};
    }
    // the integer chain: per bit (LSB first) acc, x^(2^i) and both multiplications' quotient and remainder; `result` = x^e mod n
    static std::vector<PowStep> pow_chain(Big a_cur, Big s_cur, const std::vector<Cell>& e_bits, const Big& n_big, Big& result) {
        std::vector<PowStep> st(e_bits.size());
        for (size_t i = 0; i < st.size(); i++) {
            st[i].acc = a_cur; st[i].sq = s_cur;
            big_divmod(big_mul(a_cur, s_cur), n_big, st[i].q_mul, st[i].r_mul);
            big_divmod(big_mul(s_cur, s_cur), n_big, st[i].q_sq, st[i].r_sq);
            if (!e_bits[i].val.is_zero()) a_cur = st[i].r_mul;
            s_cur = st[i].r_sq;
        }
        result = a_cur;
        return st;
    }
    void mul_region(const std::vector<Cell>& ac, const std::vector<Cell>& sq, const Cell& bit, const std::vector<Cell>& n, const PowStep& s) {
        const std::vector<Cell> muled = mul_mod_rows(ac, sq, n, s.q_mul, s.r_mul);
        for (size_t j = 0; j < ac.size(); j++) lay.select(muled[j], ac[j], bit);
    }
    // regions 2 (i - 1) and 2 (i - 1) + 1 of bit i >= 1, from the caller's row on, and the tail behind them: tasks for the pool
    PowRegions pow_regions(const std::vector<PowStep>& st, const std::vector<Cell>& e_bits, const std::vector<Cell>& n, uint32_t len_a, uint32_t len_b, const std::vector<Cell>& powed, const PowTail* tail) {
        const size_t nb = st.size(), tasks = 2 * (nb - 1) + (tail ? 1 : 0);
        const uint32_t base = lay.rows(), end_row = base + (uint32_t)(nb - 1) * (len_a + len_b);
        uint32_t tail_end = end_row;
        std::atomic<size_t> next{0};
        std::atomic<bool> ok{true}, unsat{false};
        const std::function<void()> work = [&]() {
            for (;;) try {
                size_t t = next.fetch_add(1);
                if (t >= tasks) return;
                if (tail) {      // the longest task first
                    if (t == 0) {
                        Layouter sub(lay, end_row);
                        (*tail)(sub, powed);
                        tail_end = sub.rows();
                        continue;
                    }
                    t--;
                }
                const size_t i = 1 + t / 2;
                const uint32_t start = base + (uint32_t)(i - 1) * (len_a + len_b) + (t & 1 ? len_a : 0);
                Layouter sub(lay, start);
                BigIntChip chip{sub, num_limbs};
                const std::vector<Cell> sq = value_cells(st[i].sq);
                if (t & 1) chip.mul_mod_rows(sq, sq, n, st[i].q_sq, st[i].r_sq);
                else chip.mul_region(value_cells(st[i].acc), sq, e_bits[i], n, st[i]);
                if (sub.rows() != start + (t & 1 ? len_b : len_a)) ok = false;
            } catch (const NotSatisfied&) { unsat = true; ok = false; return;
            } catch (...) { ok = false; return; }
        };
        synth_pool()->run_or_alone(work);
        return {ok, unsat, tasks, tail_end};
    }
};

// ---- PoseidonChip (src/poseidon/chip.rs): the optimised permutation as MainGate rows -- 5 (absorb) + 8 x (15 + 10) + 57 x (3 + 6) = 718 rows for T = 5 ----
struct PoseidonChip {
    Layouter& lay;
    const PoseidonSpec& sp;
    std::vector<Cell> state;
    void sbox(Cell& w, const Fe& constant) {      // :199-222: w^2, w^4, w^4 w + constant
        Cell t = lay.mul(Arg(w), Arg(w));
        t = lay.mul(Arg(t), Arg(t));
        w = lay.mul_add_constant(t, w, constant);
    }
    void sbox_full(const std::vector<Fe>& constants) { for (uint32_t i = 0; i < sp.t; i++) sbox(state[i], constants[i]); }
    // :225-262: word 0 + c0; the inputs added to the words behind it with their constants; the rest + constant (+ 1 on the first of them when hashing)
    void absorb_with_pre_constants(const std::vector<Cell>& inputs, const std::vector<Fe>& pre, bool h_flag) {
        const size_t offset = inputs.size() + 1;
        state[0] = lay.add_constant(state[0], pre[0]);
        for (size_t i = 0; i < inputs.size(); i++) state[1 + i] = lay.add_with_constant(state[1 + i], inputs[i], pre[1 + i]);
        for (size_t i = offset; i < sp.t; i++) state[i] = lay.add_constant(state[i], h_flag && i == offset ? lay.F.add(pre[i], lay.one()) : pre[i]);
    }
    Cell linear(const Cell* cells, const Fe* coeff, const Fe* coeff_m, int n) {
        Fe prod[8];
        for (int i = 0; i < n; i++) prod[i] = lay.F.f->mul(coeff_m[i], cells[i].val);
        return lay.compose(cells, coeff, prod, n, lay.F.zero());
    }
    void apply_mds(const Mat& m, const Mat& m_mont) {      // :264-288: every output word a compose over the five state words (two rows)
        std::vector<Cell> nx;
        for (uint32_t i = 0; i < sp.t; i++) nx.push_back(linear(state.data(), m[i].data(), m_mont[i].data(), (int)sp.t));
        state = nx;
    }
    void apply_sparse_mds(uint32_t r) {      // :291-330: word 0 a compose over the state, word i a compose of (word 0, col_hat) and (word i, 1)
        std::vector<Cell> nx = {linear(state.data(), sp.sparse_row[r].data(), sp.sparse_row_m[r].data(), (int)sp.t)};
        const Fe one_m = lay.F.f->one;
        for (uint32_t i = 1; i < sp.t; i++) {
            const Cell c[2] = {state[0], state[i]};
            const Fe k[2] = {sp.sparse_col[r][i - 1], lay.one()}, km[2] = {sp.sparse_col_m[r][i - 1], one_m};
            nx.push_back(linear(c, k, km, 2));
        }
        state = nx;
    }
    void permutation(const std::vector<Cell>& inputs, bool h_flag) {      // :333-419
        const uint32_t half = sp.r_f / 2;
        absorb_with_pre_constants(inputs, sp.start[0], h_flag);
        for (uint32_t r = 1; r < half; r++) {
            sbox_full(sp.start[r]);
            apply_mds(sp.mds, sp.mds_m);
        }
        sbox_full(sp.start[half]);
        apply_mds(sp.pre_sparse, sp.pre_sparse_m);
        for (uint32_t r = 0; r < sp.r_p; r++) {
            sbox(state[0], sp.partial[r]);
            apply_sparse_mds(r);
        }
        for (auto& c : sp.end) {
            sbox_full(c);
            apply_mds(sp.mds, sp.mds_m);
        }
        sbox_full(std::vector<Fe>(sp.t, lay.F.zero()));
        apply_mds(sp.mds, sp.mds_m);
    }
};

// the expected value x^e mod n as constants, asserted equal to the exponentiation's result (src/lib.rs:205-215)
inline std::vector<Cell> rsa_expected_rows(Layouter& lay, const std::vector<Cell>& powed) {
    BigIntChip chip{lay, powed.size()};
    const std::vector<Cell> valid = chip.assign_constant(chip.to_big(powed), powed.size());
    chip.assert_equal_fresh(powed, valid);
    return valid;
}

// src/lib.rs:179-215 / benches/mod_pow.rs:91-116: assign (n, e), x; x < n; x^e mod n in-circuit; equal to the native big_pow_mod.  `tail` (optional): what the
// caller lays out behind the exponentiation, expected value included; tail_ran tells whether it was written beside it -- `cells` are then the result's values only
struct RsaOut { std::vector<Cell> cells; Big want; bool tail_ran; };
inline RsaOut rsa_region(Layouter& lay, const Big& n_big, uint64_t e, const Big& x, unsigned exp_bits, size_t num_limbs, const PowTail* tail) {
    BigIntChip chip{lay, num_limbs};
    const std::vector<Cell> n_limbs = chip.assign_integer(n_big, num_limbs);      // assign_public_key: n, then the one-limb exponent
    const std::vector<Cell> e_limbs = chip.assign_integer(Big{e}, 1);
    const std::vector<Cell> x_limbs = chip.assign_integer(x, num_limbs);
    chip.assert_in_field(x_limbs, n_limbs);                                        // modpow_public_key, src/rsa/chip.rs:109
    const PowResult pow = chip.pow_mod(x_limbs, e_limbs, n_limbs, n_big, exp_bits, tail);
    // the native big_pow_mod(x, e, n) the reference assigns as the expected value: the rows above hold exactly its square-and-multiply chain (every
    // mul_mod's remainder came from the same big-integer division), so its value is read off them instead of being computed a second time
    Big want = chip.to_big(pow.powed);
    big_trim(want);
    if (pow.tail_ran) return {pow.powed, want, true};      // (the rows behind the exponentiation were written beside it)
    return {rsa_expected_rows(lay, pow.powed), want, false};
}

// src/lib.rs:261-316 / src/encryption/chip.rs:150-200: the Poseidon cipher in-circuit, constrained equal to the native one.  pose_enc (no key cells): the
// initial state is five constants (new_enc); delay_enc: five witnesses (new_enc_de), words 2 and 3 equal to the digest.
inline std::vector<Cell> cipher_region(Layouter& lay, const PoseidonSpec& spec, const Fe key_vals[2], const std::vector<Fe>& message, const Cell* key_cells, uint32_t rate) {
    std::vector<Cell> expected;
    for (auto& v : native_encrypt(spec, key_vals, message, 1, rate)) expected.push_back(lay.assign_value(v));
    const Fe init[5] = {lay.F.zero(), lay.F.zero(), key_vals[0], key_vals[1], lay.F.u(1)};
    PoseidonChip chip{lay, spec, {}};
    for (auto& v : init) chip.state.push_back(key_cells ? lay.assign_value(v) : lay.assign_constant(v));
    if (key_cells) {
        lay.assert_equal(chip.state[2], key_cells[0]);
        lay.assert_equal(chip.state[3], key_cells[1]);
    }
    chip.permutation({}, false);
    std::vector<Cell> msg, cipher;
    for (auto& m : message) msg.push_back(lay.assign_value(m));
    for (size_t c0 = 0; c0 < msg.size(); c0 += rate) {      // absorb_and_relese, src/encryption/chip.rs:72-110
        const std::vector<Cell> chunk(msg.begin() + (long)c0, msg.begin() + (long)std::min<size_t>(msg.size(), c0 + rate));
        for (size_t j = 0; j < chunk.size(); j++) {
            chip.state[1 + j] = lay.add(chip.state[1 + j], chunk[j]);
            cipher.push_back(chip.state[1 + j]);
        }
        chip.permutation(chunk, false);
    }
    cipher.push_back(chip.state[1]);
    for (size_t i = 0; i < cipher.size(); i++) lay.assert_equal(cipher[i], expected[i]);
    return cipher;
}

// src/lib.rs:222-259: limbs packed three to a field element, HasherChip::hash (src/hash/chip.rs:63-85) with perm_hash's padding; returns the two key words
inline void hash_region(Layouter& L, const PoseidonSpec& spec, const std::vector<Cell>& rsa_out, uint32_t rate, Cell key_cells[2]) {
    Fld& F = L.F;
    PoseidonChip chip{L, spec, {}};
    chip.state.push_back(L.assign_constant(F.pow2(64)));      // State::default: capacity word 2^64
    for (uint32_t i = 1; i < spec.t; i++) chip.state.push_back(L.assign_constant(F.zero()));
    const Cell base1 = L.assign_constant(F.pow2(LIMB_WIDTH));
    const Cell base2 = L.mul(Arg(base1), Arg(base1));
    std::vector<Cell> inputs;
    for (size_t i = 0; i < rsa_out.size() / 3; i++) {
        const Cell a = L.mul_add(Arg(rsa_out[3 * i + 1]), Arg(base1), Arg(rsa_out[3 * i]));
        inputs.push_back(L.mul_add(Arg(rsa_out[3 * i + 2]), Arg(base2), Arg(a)));
    }
    if (rsa_out.size() % 3 == 2) inputs.push_back(L.mul_add(Arg(rsa_out[rsa_out.size() - 1]), Arg(base1), Arg(rsa_out[rsa_out.size() - 2])));      // limbs 30, 31 of the reference's 32
    else if (rsa_out.size() % 3 == 1) inputs.push_back(rsa_out.back());
    size_t padding_offset = 0;
    for (size_t c0 = 0; c0 < inputs.size(); c0 += rate) {
        const std::vector<Cell> chunk(inputs.begin() + (long)c0, inputs.begin() + (long)std::min<size_t>(inputs.size(), c0 + rate));
        padding_offset = rate - chunk.size();
        chip.permutation(chunk, true);
    }
    if (padding_offset == 0) chip.permutation({}, true);
    key_cells[0] = chip.state[1];
    key_cells[1] = chip.state[2];
}

} }   // namespace synth
