// poseidon_host.hpp -- the native side of the reference's Poseidon: canonical field values over hostfield.hpp, the Grain LFSR, Spec::new's optimised
// parameters and permutation, the process-wide parameter cache and the native cipher.  Restated from src/poseidon/grain.rs:12-157, spec.rs:170-180,
// 310-397, permutation.rs:7-46, src/encryption/poseidon_enc.rs:66-133.  Host only, no HIP include.
#pragma once
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <tuple>
#include <vector>

#include "hostfield.hpp"

namespace synth { namespace {

typedef unsigned __int128 u128;

// ---- field values: canonical 4 x u64 ----
struct Fld {
    const HostField* f;
    Fe zero() const { return Fe{{0, 0, 0, 0}}; }
    Fe u(uint64_t x) const { return Fe{{x, 0, 0, 0}}; }
    Fe add(const Fe& a, const Fe& b) const { return f->add(a, b); }
    Fe sub(const Fe& a, const Fe& b) const { return f->sub(a, b); }
    Fe neg(const Fe& a) const { return f->neg(a); }
    Fe mul(const Fe& a, const Fe& b) const {
        // most products of these circuits are limb x limb or limb x word (64 x 64, 128 x 64 bits): below 2^192 < p, the integer product IS the field product
        const int la = a.v[3] ? 4 : a.v[2] ? 3 : a.v[1] ? 2 : 1, lb = b.v[3] ? 4 : b.v[2] ? 3 : b.v[1] ? 2 : 1;
        if (la + lb <= 3) {
            const Fe& x = la >= lb ? a : b;      // x: up to two limbs, y: one
            const uint64_t y = la >= lb ? b.v[0] : a.v[0];
            const u128 p0 = (u128)x.v[0] * y, p1 = (u128)x.v[1] * y + (uint64_t)(p0 >> 64);
            return Fe{{(uint64_t)p0, (uint64_t)p1, (uint64_t)(p1 >> 64), 0}};
        }
        return f->mul(f->mul(a, b), f->r2);      // (a b / R) R^2 / R = a b
    }
    Fe inv(const Fe& a) const {      // canonical inverse: to Montgomery, invert, back
        if (a.is_zero()) return a;
        return f->to_canonical(f->invert(f->from_canonical(a)));
    }
    Fe pow2(unsigned k) const {      // 2^k mod p, k < 256
        Fe r{{0, 0, 0, 0}};
        r.v[k >> 6] = (uint64_t)1 << (k & 63);
        while (HostField::geq(r.v, f->p)) HostField::sub_limbs(r.v, r.v, f->p);
        return r;
    }
    Fe from_u128(u128 x) const { return Fe{{(uint64_t)x, (uint64_t)(x >> 64), 0, 0}}; }
};

// ---- Poseidon (native) ----
struct Grain {
    const HostField* f;
    std::vector<uint8_t> bits;      // 80-bit state as a sliding window over a growing vector
    size_t head = 0;
    Grain(const HostField* field, uint32_t t, uint32_t r_f, uint32_t r_p) : f(field) {
        auto put = [&](unsigned width, uint32_t v) { for (int i = (int)width - 1; i >= 0; i--) bits.push_back((v >> i) & 1); };
        put(2, 1); put(4, 0); put(12, f->bits); put(12, t); put(10, r_f); put(10, r_p); put(30, (1u << 30) - 1);
        for (int i = 0; i < 160; i++) new_bit();
    }
    int new_bit() {
        const uint8_t* b = bits.data() + head;
        const uint8_t nb = b[0] ^ b[62] ^ b[51] ^ b[38] ^ b[23] ^ b[13];
        head++;
        bits.push_back(nb);
        if (head > (1u << 16)) {      // compact
            bits.erase(bits.begin(), bits.begin() + (long)head);
            head = 0;
        }
        return nb;
    }
    int bit() {
        while (!new_bit()) new_bit();
        return new_bit();
    }
    Fe draw() {      // nbits bits, MSB first
        Fe v{{0, 0, 0, 0}};
        for (uint32_t i = 0; i < f->bits; i++) {
            for (int j = 3; j > 0; j--) v.v[j] = (v.v[j] << 1) | (v.v[j - 1] >> 63);
            v.v[0] = (v.v[0] << 1) | (uint64_t)bit();
        }
        return v;
    }
    Fe field_element() {      // with rejection: round constants
        for (;;) {
            const Fe v = draw();
            if (!HostField::geq(v.v, f->p)) return v;
        }
    }
    Fe field_element_mod() {      // without rejection: the MDS x, y (value < 2^bits < 2 p: one subtraction)
        Fe v = draw();
        while (HostField::geq(v.v, f->p)) HostField::sub_limbs(v.v, v.v, f->p);
        return v;
    }
};

// Spec::new(r_f, r_p) (src/poseidon/spec.rs:310-397): Grain's round constants and the Cauchy MDS, then the optimised form the chip's rows follow --
// start / partial / end constants, the pre-sparse matrix, one sparse matrix (first row, first column) per partial round.
typedef std::vector<std::vector<Fe>> Mat;
struct PoseidonSpec {
    Fld F;
    uint32_t t, r_f, r_p;
    Mat constants, mds;                       // Grain's (canonical)
    Mat start, end, pre_sparse;               // optimised constants; the transition matrix
    std::vector<Fe> partial;
    std::vector<std::vector<Fe>> sparse_row, sparse_col;      // per partial round: the sparse matrix's first row (t) and first column below it (t - 1)
    Mat mds_m, pre_sparse_m;                  // the same matrices times R (Montgomery form): ONE Montgomery product gives m * x for a canonical x
    std::vector<std::vector<Fe>> sparse_row_m, sparse_col_m;
    static Mat mat_mul(const Fld& F, const Mat& a, const Mat& b) {
        const size_t n = a.size();
        Mat r(n, std::vector<Fe>(n, F.zero()));
        for (size_t i = 0; i < n; i++) for (size_t j = 0; j < n; j++) for (size_t k = 0; k < n; k++) r[i][j] = F.add(r[i][j], F.mul(a[i][k], b[k][j]));
        return r;
    }
    static std::vector<Fe> mat_vec(const Fld& F, const Mat& a, const std::vector<Fe>& v) {
        std::vector<Fe> r(a.size(), F.zero());
        for (size_t i = 0; i < a.size(); i++) for (size_t j = 0; j < v.size(); j++) r[i] = F.add(r[i], F.mul(a[i][j], v[j]));
        return r;
    }
    static Mat transpose(const Mat& a) {
        Mat r(a.size(), std::vector<Fe>(a.size()));
        for (size_t i = 0; i < a.size(); i++) for (size_t j = 0; j < a.size(); j++) r[j][i] = a[i][j];
        return r;
    }
    static Mat mat_inv(const Fld& F, const Mat& a) {      // Gauss-Jordan (src/poseidon/matrix.rs:84-121 computes the same inverse)
        const size_t n = a.size();
        Mat m(n, std::vector<Fe>(2 * n, F.zero()));
        for (size_t i = 0; i < n; i++) {
            for (size_t j = 0; j < n; j++) m[i][j] = a[i][j];
            m[i][n + i] = F.u(1);
        }
        for (size_t i = 0; i < n; i++) {
            size_t piv = i;
            while (piv < n && m[piv][i].is_zero()) piv++;
            if (piv == n) throw std::runtime_error("singular matrix");
            std::swap(m[i], m[piv]);
            const Fe inv = F.inv(m[i][i]);
            for (auto& x : m[i]) x = F.mul(x, inv);
            for (size_t r = 0; r < n; r++) {
                if (r == i || m[r][i].is_zero()) continue;
                const Fe f = m[r][i];
                for (size_t c = 0; c < 2 * n; c++) m[r][c] = F.sub(m[r][c], F.mul(f, m[i][c]));
            }
        }
        Mat r(n, std::vector<Fe>(n));
        for (size_t i = 0; i < n; i++) for (size_t j = 0; j < n; j++) r[i][j] = m[i][n + j];
        return r;
    }
    Mat to_mont(const Mat& a) const {
        Mat r = a;
        for (auto& row : r) for (auto& m : row) m = F.f->from_canonical(m);
        return r;
    }
    PoseidonSpec(const HostField* f, uint32_t t_, uint32_t rf, uint32_t rp) : F{f}, t(t_), r_f(rf), r_p(rp) {
        Grain g(f, t, r_f, r_p);
        constants.assign(r_f + r_p, std::vector<Fe>(t));
        for (auto& row : constants) for (auto& c : row) c = g.field_element();
        std::vector<Fe> xs(t), ys(t);
        for (auto& x : xs) x = g.field_element_mod();
        for (auto& y : ys) y = g.field_element_mod();
        mds.assign(t, std::vector<Fe>(t));
        for (uint32_t i = 0; i < t; i++) for (uint32_t j = 0; j < t; j++) mds[i][j] = F.inv(F.add(xs[i], ys[j]));
        optimized_constants();
        sparse_matrices();
        mds_m = to_mont(mds);
        pre_sparse_m = to_mont(pre_sparse);
        sparse_row_m = to_mont(sparse_row);
        sparse_col_m = to_mont(sparse_col);
    }
    void optimized_constants() {      // calculate_optimized_constants, spec.rs:325-378
        const uint32_t half = r_f / 2;
        const Mat inv = mat_inv(F, mds);
        start.push_back(constants[0]);
        for (uint32_t i = 1; i < half; i++) start.push_back(mat_vec(F, inv, constants[i]));
        std::vector<Fe> acc = constants[half + r_p];
        partial.assign(r_p, F.zero());
        for (uint32_t i = r_p; i-- > 0;) {      // constants[half .. half + r_p) walked backwards
            std::vector<Fe> tmp = mat_vec(F, inv, acc);
            partial[i] = tmp[0];
            tmp[0] = F.zero();
            for (uint32_t j = 0; j < t; j++) acc[j] = F.add(tmp[j], constants[half + i][j]);
        }
        start.push_back(mat_vec(F, inv, acc));
        for (uint32_t i = half + r_p + 1; i < r_f + r_p; i++) end.push_back(mat_vec(F, inv, constants[i]));
    }
    void sparse_matrices() {      // calculate_sparse_matrices, spec.rs:380-397 with factorise :203-241
        const Mat mds_t = transpose(mds);
        Mat acc_m = mds_t;
        for (uint32_t r = 0; r < r_p; r++) {
            std::vector<Fe> w(t - 1);
            Mat hat(t - 1, std::vector<Fe>(t - 1));
            for (uint32_t i = 1; i < t; i++) {
                w[i - 1] = acc_m[i][0];
                for (uint32_t j = 1; j < t; j++) hat[i - 1][j - 1] = acc_m[i][j];
            }
            const std::vector<Fe> w_hat = mat_vec(F, mat_inv(F, hat), w);
            Mat prime(t, std::vector<Fe>(t, F.zero()));
            prime[0][0] = F.u(1);
            for (uint32_t i = 1; i < t; i++) for (uint32_t j = 1; j < t; j++) prime[i][j] = hat[i - 1][j - 1];
            std::vector<Fe> row = {acc_m[0][0]};
            row.insert(row.end(), w_hat.begin(), w_hat.end());
            sparse_row.push_back(row);
            sparse_col.push_back(std::vector<Fe>(acc_m[0].begin() + 1, acc_m[0].end()));
            acc_m = mat_mul(F, mds_t, prime);
        }
        std::reverse(sparse_row.begin(), sparse_row.end());
        std::reverse(sparse_col.begin(), sparse_col.end());
        pre_sparse = transpose(acc_m);
    }
    Fe pow5(const Fe& x) const {
        const Fe x2 = F.mul(x, x);
        return F.mul(F.mul(x2, x2), x);
    }
    std::vector<Fe> apply_m(const Mat& m_mont, const std::vector<Fe>& st) const {
        std::vector<Fe> nx(t, F.zero());
        for (uint32_t i = 0; i < t; i++) for (uint32_t j = 0; j < t; j++) nx[i] = F.add(nx[i], F.f->mul(m_mont[i][j], st[j]));
        return nx;
    }
    std::vector<Fe> permute(std::vector<Fe> st) const {      // src/poseidon/permutation.rs:7-46 (the optimised permutation)
        const uint32_t half = r_f / 2;
        for (uint32_t i = 0; i < t; i++) st[i] = F.add(st[i], start[0][i]);
        for (uint32_t r = 1; r < half; r++) {
            for (uint32_t i = 0; i < t; i++) st[i] = F.add(pow5(st[i]), start[r][i]);
            st = apply_m(mds_m, st);
        }
        for (uint32_t i = 0; i < t; i++) st[i] = F.add(pow5(st[i]), start[half][i]);
        st = apply_m(pre_sparse_m, st);
        for (uint32_t r = 0; r < r_p; r++) {
            st[0] = F.add(pow5(st[0]), partial[r]);
            std::vector<Fe> nx(t, F.zero());
            for (uint32_t j = 0; j < t; j++) nx[0] = F.add(nx[0], F.f->mul(sparse_row_m[r][j], st[j]));
            for (uint32_t i = 1; i < t; i++) nx[i] = F.add(F.f->mul(sparse_col_m[r][i - 1], st[0]), st[i]);
            st = nx;
        }
        for (uint32_t r = 0; r < end.size(); r++) {
            for (uint32_t i = 0; i < t; i++) st[i] = F.add(pow5(st[i]), end[r][i]);
            st = apply_m(mds_m, st);
        }
        for (uint32_t i = 0; i < t; i++) st[i] = pow5(st[i]);
        return apply_m(mds_m, st);
    }
};

// The parameters depend on (T, R_F, R_P) only -- 325 Grain draws, 58 matrix inversions at the reference's parameters, a few milliseconds, many times a
// PoseidonEnc witness -- so a process keeps each parameter set it has used (the reference rebuilds the Spec in every synthesize: src/poseidon/spec.rs).
inline std::shared_ptr<const PoseidonSpec> poseidon_spec(const HostField* f, uint32_t t, uint32_t r_f, uint32_t r_p) {
    static std::mutex mu;
    static std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::shared_ptr<const PoseidonSpec>> cache;
    std::lock_guard<std::mutex> lk(mu);
    if (cache.size() >= 16) cache.clear();      // (callers hold their own reference)
    auto& slot = cache[std::make_tuple(t, r_f, r_p)];
    if (!slot) slot = std::make_shared<const PoseidonSpec>(f, t, r_f, r_p);
    return slot;
}

// PoseidonCipher::{initial_state, encrypt} (src/encryption/poseidon_enc.rs:66-133), T = 5, RATE = 4, MESSAGE_CAPACITY = message.size(): the message is added
// to a COPY of the state (`state.words()`, :108-119); a full chunk is then absorbed and permuted (update), a short one permutes the state as it is (squeeze(0)
// with an empty absorbing line)
inline std::vector<Fe> native_encrypt(const PoseidonSpec& sp, const Fe key[2], const std::vector<Fe>& message, uint64_t nonce, uint32_t rate) {
    const Fld& F = sp.F;
    std::vector<Fe> st = sp.permute({F.zero(), F.zero(), key[0], key[1], F.u(nonce)});
    std::vector<Fe> cipher;
    for (size_t c0 = 0; c0 < message.size(); c0 += rate) {
        const size_t cnt = std::min<size_t>(rate, message.size() - c0);
        for (size_t j = 0; j < cnt; j++) cipher.push_back(F.add(st[1 + j], message[c0 + j]));
        if (cnt == rate) for (size_t j = 0; j < cnt; j++) st[1 + j] = F.add(st[1 + j], message[c0 + j]);
        st = sp.permute(st);
    }
    cipher.push_back(st[1]);
    return cipher;
}

} }   // namespace synth
