// halo2_backend.hpp -- C++ host-side mirror of the upstream interface the reference reaches
// through create_proof (benches/delay_enc.rs:123-131): halo2_proofs::arithmetic::{best_multiexp,
// best_fft}, poly::EvaluationDomain::{lagrange_to_coeff, coeff_to_extended, extended_to_coeff}
// and ParamsKZG::{commit, commit_lagrange} [UPSTREAM halo2_proofs @ v2023_04_20], as thin
// wrappers over the C ABI (include/dehalo.h).  Same names and argument meaning; upstream's
// assert_eq! panics become std::invalid_argument, library errors std::runtime_error.
// Header-only; link with -ldehalo.  No CPU path: constructing Backend without a gfx950 throws.
#pragma once
#include <array>
#include <cstdint>
#include <exception>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dehalo.h"

namespace halo2_amd {

using Fe = std::array<uint64_t, 4>;        // halo2curves field element (Montgomery, 4 x u64 LE)
using Affine = std::array<uint64_t, 8>;    // {x, y}; identity = all zero
using Projective = std::array<uint64_t, 12>;  // Jacobian {x, y, z}; identity z = 0

class Backend {
  public:
    explicit Backend(int device = 0) {
        int rc = dehalo_ctx_create(device, &ctx_);
        if (rc != 0) throw std::runtime_error("dehalo_ctx_create failed (" + std::to_string(rc) + "): no gfx950 device; there is no CPU fallback");
    }
    ~Backend() { dehalo_ctx_destroy(ctx_); }
    Backend(const Backend&) = delete;
    Backend& operator=(const Backend&) = delete;
    dehalo_ctx* raw() const { return ctx_; }

    // arithmetic::best_multiexp(coeffs, bases) -> C::Curve
    Projective best_multiexp(dehalo_curve curve, const std::vector<Fe>& coeffs, const std::vector<Affine>& bases) const {
        if (coeffs.size() != bases.size()) throw std::invalid_argument("best_multiexp: coeffs.len() != bases.len()");
        Projective out{};
        check(dehalo_best_multiexp(ctx_, curve, coeffs.empty() ? nullptr : coeffs[0].data(), bases.empty() ? nullptr : bases[0].data(), coeffs.size(), out.data()));
        return out;
    }
    // arithmetic::best_fft(a, omega, log_n): in place
    void best_fft(dehalo_field field, std::vector<Fe>& a, const Fe& omega, uint32_t log_n) const {
        if (a.size() != (size_t(1) << log_n)) throw std::invalid_argument("best_fft: a.len() != 1 << log_n");
        check(dehalo_ntt(ctx_, field, a[0].data(), log_n, omega.data()));
    }
    // arithmetic::eval_polynomial(poly, point) -> F
    Fe eval_polynomial(dehalo_field field, const std::vector<Fe>& poly, const Fe& point) const {
        Fe out{};
        check(dehalo_eval_polynomial(ctx_, field, poly.empty() ? nullptr : poly[0].data(), poly.size(), point.data(), out.data()));
        return out;
    }
    // ff::BatchInvert: in place, zeros stay zero
    void batch_invert(dehalo_field field, std::vector<Fe>& values) const {
        check(dehalo_batch_invert(ctx_, field, values.empty() ? nullptr : values[0].data(), values.size()));
    }
    // z[0] = 1, z[i] = prod_{j<i} num[j] / den[j]  (permutation::commit / lookup::commit_product without the blinding rows)
    std::vector<Fe> grand_product(dehalo_field field, const std::vector<Fe>& num, const std::vector<Fe>& den) const {
        if (num.size() != den.size()) throw std::invalid_argument("grand_product: num.len() != den.len()");
        std::vector<Fe> z(num.size());
        if (!num.empty()) check(dehalo_grand_product(ctx_, field, num[0].data(), den[0].data(), num.size(), z[0].data()));
        return z;
    }
    // arithmetic::kate_division(a, point) -> (a(X) - a(point)) / (X - point), a.len() - 1 coefficients
    std::vector<Fe> kate_division(dehalo_field field, const std::vector<Fe>& a, const Fe& point) const {
        if (a.empty()) throw std::invalid_argument("kate_division: empty polynomial");
        std::vector<Fe> q(a.size() - 1);
        check(dehalo_kate_division(ctx_, field, a[0].data(), a.size(), point.data(), q.empty() ? nullptr : q[0].data()));
        return q;
    }
    // plonk::lookup::prover::permute_expression_pair over the first `usable_rows` values (the caller appends the blinding rows);
    // Err(ConstraintSystemFailure) -> std::runtime_error carrying DEHALO_ERR_NOT_IN_TABLE
    std::pair<std::vector<Fe>, std::vector<Fe>> permute_expression_pair(dehalo_field field, const std::vector<Fe>& input, const std::vector<Fe>& table,
                                                                        size_t usable_rows) const {
        if (input.size() < usable_rows || table.size() < usable_rows) throw std::invalid_argument("permute_expression_pair: fewer than usable_rows values");
        std::vector<Fe> pi(usable_rows), pt(usable_rows);
        if (usable_rows) check(dehalo_permute_expression_pair(ctx_, field, input[0].data(), table[0].data(), usable_rows, pi[0].data(), pt[0].data()));
        return {pi, pt};
    }
    void check(int rc) const {
        if (rc != 0) throw std::runtime_error(std::string("dehalo error ") + std::to_string(rc) + ": " + dehalo_last_error(ctx_));
    }

  private:
    dehalo_ctx* ctx_ = nullptr;
};

// poly::EvaluationDomain -- the caller supplies the domain constants it already holds
// (omega_inv, ifft_divisor, extended_omega, ..., g_coset = F::ZETA), exactly upstream's fields.
struct EvaluationDomain {
    const Backend& be;
    dehalo_field field;
    uint32_t k, extended_k, quotient_poly_degree;
    Fe omega_inv, ifft_divisor, extended_omega, extended_omega_inv, extended_ifft_divisor, g_coset;

    void lagrange_to_coeff(std::vector<Fe>& a) const {
        if (a.size() != (size_t(1) << k)) throw std::invalid_argument("lagrange_to_coeff: wrong length");
        be.check(dehalo_intt_scaled(be.raw(), field, a[0].data(), k, omega_inv.data(), ifft_divisor.data()));
    }
    std::vector<Fe> coeff_to_extended(const std::vector<Fe>& a) const {
        if (a.size() != (size_t(1) << k)) throw std::invalid_argument("coeff_to_extended: wrong length");
        std::vector<Fe> ext(size_t(1) << extended_k);
        be.check(dehalo_coset_ntt(be.raw(), field, a[0].data(), k, ext[0].data(), extended_k, extended_omega.data(), g_coset.data()));
        return ext;
    }
    void extended_to_coeff(std::vector<Fe>& a) const {
        if (a.size() != (size_t(1) << extended_k)) throw std::invalid_argument("extended_to_coeff: wrong length");
        be.check(dehalo_coset_intt(be.raw(), field, a[0].data(), extended_k, extended_omega_inv.data(), extended_ifft_divisor.data(), g_coset.data()));
        a.resize((size_t(1) << k) * quotient_poly_degree);   // upstream truncates
    }
};

// ParamsKZG / ParamsIPA: g and g_lagrange resident in HBM
class Params {
  public:
    Params(const Backend& be, dehalo_curve curve, const std::vector<Affine>& g, const std::vector<Affine>* g_lagrange = nullptr) : be_(be) {
        be_.check(dehalo_bases_register(be_.raw(), curve, g[0].data(), g.size(), 64, 0, 1, &g_));
        if (g_lagrange) be_.check(dehalo_bases_register(be_.raw(), curve, (*g_lagrange)[0].data(), g_lagrange->size(), 64, 0, 1, &gl_));
    }
    ~Params() {
        if (g_) dehalo_bases_release(be_.raw(), g_);
        if (gl_) dehalo_bases_release(be_.raw(), gl_);
    }
    Projective commit(const std::vector<Fe>& poly) const { return msm(g_, poly); }
    Projective commit_lagrange(const std::vector<Fe>& poly) const {
        if (!gl_) throw std::invalid_argument("commit_lagrange: no g_lagrange registered");
        return msm(gl_, poly);
    }

  private:
    Projective msm(dehalo_bases* b, const std::vector<Fe>& poly) const {
        Projective out{};
        be_.check(dehalo_msm(be_.raw(), b, poly.empty() ? nullptr : poly[0].data(), poly.size(), out.data()));
        return out;
    }
    const Backend& be_;
    dehalo_bases* g_ = nullptr;
    dehalo_bases* gl_ = nullptr;
};

// ParamsIPA::{commit, commit_lagrange}(poly, r) = <poly, g> + r * w: tables registered over g || w (n + 1 points)
class ParamsIPA {
  public:
    ParamsIPA(const Backend& be, dehalo_curve curve, std::vector<Affine> g, std::vector<Affine> g_lagrange, const Affine& w) : be_(be), n_(g.size()) {
        if (g_lagrange.size() != n_) throw std::invalid_argument("ParamsIPA: g and g_lagrange differ in length");
        g.push_back(w);
        g_lagrange.push_back(w);
        be_.check(dehalo_bases_register(be_.raw(), curve, g[0].data(), g.size(), 64, 0, 1, &g_));
        be_.check(dehalo_bases_register(be_.raw(), curve, g_lagrange[0].data(), g_lagrange.size(), 64, 0, 1, &gl_));
    }
    ~ParamsIPA() {
        if (g_) dehalo_bases_release(be_.raw(), g_);
        if (gl_) dehalo_bases_release(be_.raw(), gl_);
    }
    Projective commit(const std::vector<Fe>& poly, const Fe& blind) const { return msm(g_, poly, blind); }
    Projective commit_lagrange(const std::vector<Fe>& poly, const Fe& blind) const { return msm(gl_, poly, blind); }

  private:
    Projective msm(dehalo_bases* b, std::vector<Fe> poly, const Fe& blind) const {
        if (poly.size() != n_) throw std::invalid_argument("commit: poly.len() != params.n");   // upstream: assert_eq!
        poly.push_back(blind);
        Projective out{};
        be_.check(dehalo_msm(be_.raw(), b, poly[0].data(), poly.size(), out.data()));
        return out;
    }
    const Backend& be_;
    size_t n_;
    dehalo_bases* g_ = nullptr;
    dehalo_bases* gl_ = nullptr;
};

// [s] P for one fixed point P over its resident window table (dehalo_fixed_base_*): device pointers in and out, one launch per call, asynchronous on
// the stream.  A table made here is released here; ParamsIPAHandle::fixed_base() lends the table of W, which the params own.
class FixedBase {
  public:
    FixedBase(const Backend& be, dehalo_curve curve, const Affine& p) : be_(be), owned_(true) {
        dehalo_fixed_base* fb = nullptr;
        be_.check(dehalo_fixed_base_create(be_.raw(), curve, p.data(), &fb));
        fb_ = fb;
    }
    FixedBase(const Backend& be, const dehalo_fixed_base* borrowed) : be_(be), fb_(borrowed), owned_(false) {}
    ~FixedBase() { if (owned_ && fb_) dehalo_fixed_base_release(be_.raw(), const_cast<dehalo_fixed_base*>(fb_)); }
    FixedBase(const FixedBase&) = delete;
    FixedBase& operator=(const FixedBase&) = delete;
    FixedBase(FixedBase&& o) : be_(o.be_), fb_(o.fb_), owned_(o.owned_) { o.fb_ = nullptr; }
    // d_out_affine_xy[i] = [d_scalars[i]] P, (0, 0) for the identity
    void mul_device(const uint64_t* d_scalars, size_t count, uint64_t* d_out_affine_xy, void* stream = nullptr) const {
        be_.check(dehalo_fixed_base_mul_device(be_.raw(), fb_, d_scalars, count, d_out_affine_xy, stream));
    }
    // d_jacobian[i] += [d_blinds[i]] P in place: ParamsIPA's blinding term for the results of one batched MSM
    void blind_device(uint64_t* d_jacobian, const uint64_t* d_blinds, size_t count, void* stream = nullptr) const {
        be_.check(dehalo_fixed_base_blind_device(be_.raw(), fb_, d_jacobian, d_blinds, count, stream));
    }
    const dehalo_fixed_base* raw() const { return fb_; }

  private:
    const Backend& be_;
    const dehalo_fixed_base* fb_ = nullptr;
    bool owned_;
};

// ---- the whole call: plonk::{ConstraintSystem, keygen_vk, keygen_pk, create_proof}, ParamsKZG, Blake2bWrite ---------------------------
// (include/dehalo.h "the whole call"; reference call sites benches/delay_enc.rs:41-54, 84-115, 120-134)

// plonk::ConstraintSystem as the prover reads it, built the way a circuit's configure() builds it; expressions are handles.
class ConstraintSystem {
  public:
    using Expr = uint32_t;
    ConstraintSystem(uint32_t num_advice, uint32_t num_fixed, uint32_t num_instance) { d_.num_advice = num_advice; d_.num_fixed = num_fixed; d_.num_instance = num_instance; }
    Expr constant(const Fe& c) { return node(DEHALO_EXPR_CONSTANT, add_constant(c), 0, 0); }
    Expr query_advice(uint32_t col, int32_t rot = 0) { query(aq_, DEHALO_COLUMN_ADVICE, col, rot); return node(DEHALO_EXPR_ADVICE, col, 0, rot); }
    Expr query_fixed(uint32_t col, int32_t rot = 0) { query(fq_, DEHALO_COLUMN_FIXED, col, rot); return node(DEHALO_EXPR_FIXED, col, 0, rot); }
    Expr query_instance(uint32_t col, int32_t rot = 0) { query(iq_, DEHALO_COLUMN_INSTANCE, col, rot); return node(DEHALO_EXPR_INSTANCE, col, 0, rot); }
    Expr neg(Expr a) { return node(DEHALO_EXPR_NEGATED, a, 0, 0); }
    Expr sum(Expr a, Expr b) { return node(DEHALO_EXPR_SUM, a, b, 0); }
    Expr product(Expr a, Expr b) { return node(DEHALO_EXPR_PRODUCT, a, b, 0); }
    Expr scaled(Expr a, const Fe& c) { return node(DEHALO_EXPR_SCALED, a, add_constant(c), 0); }
    // the Challenge API: advice_column_in(phase) for column `col` (columns not named stay in the first phase); challenge_usable_after(phase).expr()
    void set_advice_phase(uint32_t col, uint8_t phase) { if (aph_.size() < d_.num_advice) aph_.resize(d_.num_advice, 0); aph_.at(col) = phase; }
    Expr challenge_usable_after(uint8_t phase) { cph_.push_back(phase); return node(DEHALO_EXPR_CHALLENGE, (uint32_t)cph_.size() - 1, 0, 0); }
    void enable_equality(dehalo_column_kind kind, uint32_t col) {
        std::vector<dehalo_column_query>& q = kind == DEHALO_COLUMN_ADVICE ? aq_ : kind == DEHALO_COLUMN_FIXED ? fq_ : iq_;
        query(q, kind, col, 0);
        for (auto& c : perm_) if (c.kind == (uint32_t)kind && c.index == col) return;
        perm_.push_back(dehalo_column_query{(uint32_t)kind, col, 0});
    }
    void create_gate(const std::vector<Expr>& polys) { gates_.insert(gates_.end(), polys.begin(), polys.end()); }
    void lookup(const std::vector<std::pair<Expr, Expr>>& pairs) {
        lens_.push_back((uint32_t)pairs.size());
        for (auto& pr : pairs) { lin_.push_back(pr.first); ltab_.push_back(pr.second); }
    }
    // ConstraintSystem::shuffle: the rows' input tuples are a permutation of the rows' shuffle tuples; at least one (input, shuffle) pair
    void shuffle(const std::vector<std::pair<Expr, Expr>>& pairs) {
        slens_.push_back((uint32_t)pairs.size());
        for (auto& pr : pairs) { sin_.push_back(pr.first); stab_.push_back(pr.second); }
    }
    void set_minimum_degree(uint32_t d) { d_.minimum_degree = d; }
    const dehalo_constraint_system* descriptor() {
        d_.nodes = nodes_.data(); d_.num_nodes = (uint32_t)nodes_.size();
        d_.constants = consts_.empty() ? nullptr : consts_[0].data(); d_.num_constants = (uint32_t)consts_.size();
        d_.gates = gates_.data(); d_.num_gates = (uint32_t)gates_.size();
        d_.lookup_lens = lens_.data(); d_.num_lookups = (uint32_t)lens_.size(); d_.lookup_inputs = lin_.data(); d_.lookup_tables = ltab_.data();
        d_.permutation_columns = perm_.data(); d_.num_permutation_columns = (uint32_t)perm_.size();
        d_.advice_queries = aq_.data(); d_.num_advice_queries = (uint32_t)aq_.size();
        d_.fixed_queries = fq_.data(); d_.num_fixed_queries = (uint32_t)fq_.size();
        d_.instance_queries = iq_.data(); d_.num_instance_queries = (uint32_t)iq_.size();
        d_.advice_phases = aph_.empty() ? nullptr : aph_.data();
        d_.challenge_phases = cph_.empty() ? nullptr : cph_.data(); d_.num_challenges = (uint32_t)cph_.size();
        d_.shuffle_lens = slens_.empty() ? nullptr : slens_.data(); d_.shuffle_inputs = slens_.empty() ? nullptr : sin_.data();
        d_.shuffle_tables = slens_.empty() ? nullptr : stab_.data(); d_.num_shuffles = (uint32_t)slens_.size();
        return &d_;
    }

  private:
    Expr node(uint32_t kind, uint32_t a, uint32_t b, int32_t rot) { nodes_.push_back(dehalo_expr_node{kind, a, b, rot}); return (Expr)nodes_.size() - 1; }
    uint32_t add_constant(const Fe& c) {
        for (size_t i = 0; i < consts_.size(); i++) if (consts_[i] == c) return (uint32_t)i;
        consts_.push_back(c);
        return (uint32_t)consts_.size() - 1;
    }
    static void query(std::vector<dehalo_column_query>& q, uint32_t kind, uint32_t col, int32_t rot) {
        for (auto& e : q) if (e.index == col && e.rotation == rot) return;
        q.push_back(dehalo_column_query{kind, col, rot});
    }
    dehalo_constraint_system d_{};
    std::vector<dehalo_expr_node> nodes_;
    std::vector<Fe> consts_;
    std::vector<uint32_t> gates_, lens_, lin_, ltab_, slens_, sin_, stab_;
    std::vector<dehalo_column_query> perm_, aq_, fq_, iq_;
    std::vector<uint8_t> aph_, cph_;
};

// ParamsKZG<Bn256>
class ParamsKZG {
  public:
    ParamsKZG(const Backend& be, dehalo_curve curve, const std::vector<uint8_t>& raw_bytes) : be_(be) {      // ParamsKZG::read (RawBytes)
        be_.check(dehalo_params_read(be_.raw(), curve, raw_bytes.data(), raw_bytes.size(), &p_));
    }
    // ParamsKZG::setup(k, rng) with the rng's draw handed over: `s` = the secret scalar in Montgomery form (benches/delay_enc.rs:43); made on the device
    ParamsKZG(const Backend& be, dehalo_curve curve, uint32_t k, const Fe& s) : be_(be) { be_.check(dehalo_params_setup(be_.raw(), curve, k, s.data(), &p_)); }
    // ParamsKZG::read_custom(reader, format), and with downsize_k = k' the same followed by Params::downsize(k') in one step: only g[0 .. 2^k') is taken
    // from the file, g_lagrange is the group FFT of it on the device -- a large SRS and a small circuit
    static ParamsKZG read_custom(const Backend& be, dehalo_curve curve, const std::vector<uint8_t>& bytes, dehalo_serde_format format, uint32_t downsize_k = DEHALO_KEEP_K) {
        ParamsKZG p(be);
        be.check(dehalo_params_read_custom(be.raw(), curve, bytes.data(), bytes.size(), format, downsize_k, &p.p_));
        return p;
    }
    // from g, g2 and s_g2 alone: g_lagrange = g_to_lagrange(g) on the device
    static ParamsKZG from_g(const Backend& be, dehalo_curve curve, uint32_t k, const std::vector<Affine>& g, const std::array<uint8_t, 128>& g2, const std::array<uint8_t, 128>& s_g2) {
        if (g.size() != (size_t(1) << k)) throw std::invalid_argument("ParamsKZG::from_g: g.len() != 1 << k");
        ParamsKZG p(be);
        be.check(dehalo_params_from_g(be.raw(), curve, k, g[0].data(), g2.data(), s_g2.data(), &p.p_));
        return p;
    }
    ~ParamsKZG() { if (p_) dehalo_params_release(be_.raw(), p_); }
    ParamsKZG(const ParamsKZG&) = delete;
    ParamsKZG(ParamsKZG&& o) : be_(o.be_), p_(o.p_) { o.p_ = nullptr; }
    std::vector<uint8_t> write() const {
        std::vector<uint8_t> out(dehalo_params_size(p_));
        be_.check(dehalo_params_write(p_, out.data(), out.size()));
        return out;
    }
    // ParamsKZG::write_custom(writer, format); Processed compresses the points on the device
    std::vector<uint8_t> write_custom(dehalo_serde_format format) const {
        std::vector<uint8_t> out(dehalo_params_size_custom(p_, format));
        be_.check(dehalo_params_write_custom(p_, format, out.data(), out.size()));
        return out;
    }
    // Params::downsize(k) as a new object; this one stays as it is
    ParamsKZG downsize(uint32_t k) const {
        ParamsKZG p(be_);
        be_.check(dehalo_params_downsize(be_.raw(), p_, k, &p.p_));
        return p;
    }
    dehalo_params* raw() const { return p_; }

  private:
    explicit ParamsKZG(const Backend& be) : be_(be) {}
    const Backend& be_;
    dehalo_params* p_ = nullptr;
};

// ParamsIPA<C> of the whole call (Pallas / Vesta): the object dehalo_prover_create takes for ProverIPA proofs.  (The class ParamsIPA above is the
// fine-grained commit / commit_lagrange mirror over two registered tables; this one owns a dehalo_params.)
class ParamsIPAHandle {
  public:
    // from g alone, as upstream's ParamsIPA::new ends: g_lagrange = g_to_lagrange(g), a group FFT on the device
    static ParamsIPAHandle from_g(const Backend& be, dehalo_curve curve, uint32_t k, const std::vector<Affine>& g, const Affine& w, const Affine& u) {
        if (g.size() != (size_t(1) << k)) throw std::invalid_argument("ParamsIPA::from_g: g.len() != 1 << k");
        ParamsIPAHandle p(be);
        be.check(dehalo_params_ipa_from_g(be.raw(), curve, k, g[0].data(), w.data(), u.data(), &p.p_));
        return p;
    }
    // ParamsIPA at any k without a file: g, W, U derived on the device by the library's public rule (include/dehalo.h, "Generated points"; key32 = 32 bytes,
    // null = the default key), g_lagrange by the group FFT.  Not upstream's ParamsIPA::new generators: an upstream verifier reads write()'s bytes
    static ParamsIPAHandle generate(const Backend& be, dehalo_curve curve, uint32_t k, const uint8_t* key32 = nullptr) {
        ParamsIPAHandle p(be);
        be.check(dehalo_params_ipa_generate(be.raw(), curve, k, key32, &p.p_));
        return p;
    }
    // ParamsIPA::read: k: u32 LE | g | g_lagrange | w | u, 32-byte compressed points
    static ParamsIPAHandle read(const Backend& be, dehalo_curve curve, const std::vector<uint8_t>& bytes) {
        ParamsIPAHandle p(be);
        be.check(dehalo_params_ipa_read(be.raw(), curve, bytes.data(), bytes.size(), &p.p_));
        return p;
    }
    ~ParamsIPAHandle() { if (p_) dehalo_params_release(be_.raw(), p_); }
    ParamsIPAHandle(const ParamsIPAHandle&) = delete;
    ParamsIPAHandle(ParamsIPAHandle&& o) : be_(o.be_), p_(o.p_) { o.p_ = nullptr; }
    // ParamsIPA::write
    std::vector<uint8_t> write() const {
        std::vector<uint8_t> out(dehalo_params_ipa_size(p_));
        be_.check(dehalo_params_ipa_write(p_, out.data(), out.size()));
        return out;
    }
    // Params::downsize(k) as a new object with its own table of W; this one stays as it is
    ParamsIPAHandle downsize(uint32_t k) const {
        ParamsIPAHandle p(be_);
        be_.check(dehalo_params_downsize(be_.raw(), p_, k, &p.p_));
        return p;
    }
    // W's window table: what every commit / commit_lagrange of these params adds [blind] W from
    FixedBase fixed_base() const { return FixedBase(be_, dehalo_params_fixed_base(p_)); }
    dehalo_params* raw() const { return p_; }

  private:
    explicit ParamsIPAHandle(const Backend& be) : be_(be) {}
    const Backend& be_;
    dehalo_params* p_ = nullptr;
};

// ProvingKey<G1Affine> (with its VerifyingKey)
class ProvingKey {
  public:
    // keygen_vk + keygen_pk: fixed = num_fixed x 2^k elements (Montgomery), mapping = permutation assembly (cell -> cell)
    ProvingKey(const Backend& be, const ParamsKZG& params, ConstraintSystem& cs, const std::vector<Fe>& fixed, const std::vector<uint64_t>& mapping,
               const std::vector<std::vector<uint8_t>>& selectors = {}, uint32_t flags = 0) : be_(be) {
        std::vector<const uint8_t*> sp;
        for (auto& s : selectors) sp.push_back(s.data());
        be_.check(dehalo_keygen(be_.raw(), params.raw(), cs.descriptor(), fixed.empty() ? nullptr : fixed[0].data(), mapping.data(), sp.data(), (uint32_t)sp.size(), flags, &pk_));
    }
    // ProvingKey::read::<_, Circuit>(.., SerdeFormat::RawBytes)
    ProvingKey(const Backend& be, dehalo_curve curve, ConstraintSystem& cs, const std::vector<uint8_t>& raw_bytes, uint32_t num_selectors) : be_(be) {
        be_.check(dehalo_pk_read(be_.raw(), curve, cs.descriptor(), raw_bytes.data(), raw_bytes.size(), num_selectors, &pk_));
    }
    // ProvingKey::read::<_, Circuit>(.., format): Processed decompresses the commitments and converts the elements on the device, RawBytes checks every point and
    // every element, RawBytesUnchecked is the constructor above (dehalo_pk_read_custom)
    static ProvingKey read(const Backend& be, dehalo_curve curve, ConstraintSystem& cs, const std::vector<uint8_t>& bytes, uint32_t num_selectors, dehalo_serde_format format) {
        dehalo_pk* h = nullptr;
        be.check(dehalo_pk_read_custom(be.raw(), curve, cs.descriptor(), bytes.data(), bytes.size(), format, num_selectors, &h));
        return ProvingKey(be, h);
    }
    // VerifyingKey::read(.., vk_format) + keygen_pk(&params, vk, &circuit): the key of these columns UNDER the verifying key `vk_bytes`, whose commitments are
    // taken as they are -- not recomputed (no MSM runs) and not compared with the columns (dehalo_keygen_pk)
    static ProvingKey keygen_pk(const Backend& be, const ParamsKZG& params, ConstraintSystem& cs, const std::vector<uint8_t>& vk_bytes, dehalo_serde_format vk_format,
                                uint32_t num_selectors, const std::vector<Fe>& fixed, const std::vector<uint64_t>& mapping, uint32_t flags = 0) {
        dehalo_pk* h = nullptr;
        be.check(dehalo_keygen_pk(be.raw(), params.raw(), cs.descriptor(), vk_bytes.data(), vk_bytes.size(), vk_format, num_selectors,
                                  fixed.empty() ? nullptr : fixed[0].data(), mapping.data(), flags, &h));
        return ProvingKey(be, h);
    }
    ~ProvingKey() { dehalo_pk_release(be_.raw(), pk_); }
    ProvingKey(const ProvingKey&) = delete;
    ProvingKey(ProvingKey&& o) noexcept : be_(o.be_), pk_(o.pk_) { o.pk_ = nullptr; }
    std::vector<uint8_t> write() const {
        std::vector<uint8_t> out(dehalo_pk_size(pk_));
        be_.check(dehalo_pk_write(be_.raw(), pk_, out.data(), out.size()));
        return out;
    }
    // ProvingKey::write(.., format); both raw formats write write()'s bytes
    std::vector<uint8_t> write(dehalo_serde_format format) const {
        std::vector<uint8_t> out(dehalo_pk_size_custom(pk_, format));
        be_.check(dehalo_pk_write_custom(be_.raw(), pk_, format, out.data(), out.size()));
        return out;
    }
    std::vector<uint8_t> vk_write() const {
        std::vector<uint8_t> out(dehalo_vk_size(pk_));
        be_.check(dehalo_vk_write(pk_, out.data(), out.size()));
        return out;
    }
    // VerifyingKey::write(.., format); both raw formats write vk_write()'s bytes
    std::vector<uint8_t> vk_write(dehalo_serde_format format) const {
        std::vector<uint8_t> out(dehalo_vk_size_custom(pk_, format));
        be_.check(dehalo_vk_write_custom(be_.raw(), pk_, format, out.data(), out.size()));
        return out;
    }
    void set_transcript_repr(const Fe& r) { be_.check(dehalo_pk_set_transcript_repr(pk_, r.data())); }
    // MockProver::verify over this key (dehalo_check_witness): advice / instances as Prover::create_proof takes them, mapping = keygen's (null: copies unchecked).
    // The totals are exact; `failures` receives the first `cap` of them in (kind, index, row) order.  The witness satisfies the circuit when the totals are zero.
    dehalo_check_report check_witness(const std::vector<Fe>& advice, const std::vector<std::vector<Fe>>& instances, const std::vector<uint64_t>* mapping,
                                      std::vector<dehalo_check_failure>& failures, size_t cap = 64, uint32_t flags = 0) const {
        std::vector<const uint64_t*> ip;
        std::vector<size_t> il;
        for (auto& col : instances) { ip.push_back(col.empty() ? nullptr : col[0].data()); il.push_back(col.size()); }
        failures.assign(cap, dehalo_check_failure{});
        dehalo_check_report rep{};
        be_.check(dehalo_check_witness(be_.raw(), pk_, advice.empty() ? nullptr : advice[0].data(), ip.data(), il.data(), (uint32_t)ip.size(), mapping ? mapping->data() : nullptr, flags,
                                       cap ? failures.data() : nullptr, cap, &rep));
        failures.resize((size_t)rep.written);
        return rep;
    }
    dehalo_pk* raw() const { return pk_; }

  private:
    ProvingKey(const Backend& be, dehalo_pk* adopted) : be_(be), pk_(adopted) {}
    const Backend& be_;
    dehalo_pk* pk_ = nullptr;
};

// Blake2bWrite<Vec<u8>, G1Affine, Challenge255<_>>
class Blake2bWrite {
  public:
    explicit Blake2bWrite(dehalo_curve curve) {
        if (dehalo_transcript_create(curve, &t_) != 0) throw std::runtime_error("dehalo_transcript_create failed");
    }
    ~Blake2bWrite() { dehalo_transcript_release(t_); }
    Blake2bWrite(const Blake2bWrite&) = delete;
    std::vector<uint8_t> finalize() const {
        std::vector<uint8_t> out(dehalo_transcript_len(t_));
        if (dehalo_transcript_finalize(t_, out.data(), out.size()) != 0) throw std::runtime_error("dehalo_transcript_finalize failed");
        return out;
    }
    dehalo_transcript* raw() const { return t_; }

  private:
    dehalo_transcript* t_ = nullptr;
};

// create_proof(&params, &pk, &[circuit], &[instances], rng, &mut transcript): `advice` is what circuit.synthesize assigned
class Prover {
  public:
    // num_circuits: how many circuits of the key one proof is over (create_proof's `&[circuit]`); more than one proves through create_proof_multi
    Prover(const Backend& be, const ParamsKZG& params, const ProvingKey& pk, const Backend* side = nullptr, uint32_t num_circuits = 1) : be_(be) {
        be_.check(dehalo_prover_create_multi(be_.raw(), side ? side->raw() : nullptr, params.raw(), pk.raw(), num_circuits, &p_));
    }
    ~Prover() { dehalo_prover_release(p_); }
    Prover(const Prover&) = delete;
    // create_proof::<_, ProverGWC<_>, ..> (DEHALO_MULTIOPEN_GWC, the default) or create_proof::<_, ProverSHPLONK<_>, ..> (DEHALO_MULTIOPEN_SHPLONK); KZG params only
    void set_multiopen(dehalo_multiopen m) { be_.check(dehalo_prover_set_multiopen(p_, m)); }
    size_t proof_size() const { return dehalo_prover_proof_size(p_); }
    // rng == nullptr: operating-system entropy (the reference's OsRng)
    void create_proof(const std::vector<Fe>& advice, const std::vector<std::vector<Fe>>& instances, dehalo_rng* rng, Blake2bWrite& transcript) const {
        std::vector<const uint64_t*> ip;
        std::vector<size_t> il;
        for (auto& col : instances) { ip.push_back(col.empty() ? nullptr : col[0].data()); il.push_back(col.size()); }
        be_.check(dehalo_create_proof(p_, advice[0].data(), ip.data(), il.data(), (uint32_t)ip.size(), rng, transcript.raw(), 0));
    }
    // create_proof(&params, &pk, &[circuit_0, .., circuit_{N-1}], &[instances_0, ..], rng, &mut transcript): ONE proof over advice.size() circuits of the key, on
    // a prover made for that many (dehalo_create_proof_multi).  advice[c] / instances[c]: circuit c's, as create_proof takes them
    void create_proof_multi(const std::vector<std::vector<Fe>>& advice, const std::vector<std::vector<std::vector<Fe>>>& instances, dehalo_rng* rng,
                            Blake2bWrite& transcript) const {
        std::vector<const uint64_t*> ap, ip;
        std::vector<size_t> il;
        for (auto& a : advice) ap.push_back(a.empty() ? nullptr : a[0].data());
        for (auto& circuit : instances)
            for (auto& col : circuit) { ip.push_back(col.empty() ? nullptr : col[0].data()); il.push_back(col.size()); }
        const uint32_t columns = instances.empty() ? 0 : (uint32_t)instances[0].size();
        for (auto& circuit : instances)
            if (circuit.size() != columns) be_.check(DEHALO_ERR_INVALID);      // (every circuit has the key's instance columns)
        if (instances.size() != advice.size()) be_.check(DEHALO_ERR_INVALID);
        be_.check(dehalo_create_proof_multi(p_, ap.data(), ip.data(), il.data(), columns, (uint32_t)ap.size(), rng, transcript.raw(), 0));
    }
    // The same for a circuit with later-phase advice (dehalo_create_proof_phased): witness(phase, challenges) is called once per phase on this thread -- for
    // phase p > 0 after the commitments of phase p - 1 are in the transcript, with every challenge squeezed so far (the others zero) -- and returns all
    // num_advice x 2^k elements, of which the columns of `phase` are read.  The returned vector must stay alive and unchanged until the next call of `witness`
    // or the return of this function; `witness` may call nothing on this prover.  An exception thrown by `witness` ends the proof and is rethrown here.
    using PhaseWitness = std::function<const std::vector<Fe>&(uint32_t phase, const std::vector<Fe>& challenges)>;
    void create_proof_phased(const PhaseWitness& witness, const std::vector<std::vector<Fe>>& instances, dehalo_rng* rng, Blake2bWrite& transcript) const {
        struct Call { const PhaseWitness* fn; std::exception_ptr error; } call{&witness, nullptr};
        auto thunk = [](void* user, uint32_t phase, const uint64_t* challenges, uint32_t count, const uint64_t** advice) -> int {
            Call* c = static_cast<Call*>(user);
            try {
                std::vector<Fe> ch(count);
                for (uint32_t j = 0; j < count; j++) for (int w = 0; w < 4; w++) ch[j][w] = challenges[4 * j + w];
                const std::vector<Fe>& adv = (*c->fn)(phase, ch);
                if (adv.empty()) return 2;
                *advice = adv[0].data();
                return 0;
            } catch (...) { c->error = std::current_exception(); return 1; }      // (an exception must not unwind through the C frames)
        };
        std::vector<const uint64_t*> ip;
        std::vector<size_t> il;
        for (auto& col : instances) { ip.push_back(col.empty() ? nullptr : col[0].data()); il.push_back(col.size()); }
        const int rc = dehalo_create_proof_phased(p_, thunk, &call, ip.data(), il.data(), (uint32_t)ip.size(), rng, transcript.raw(), 0);
        if (call.error) std::rethrow_exception(call.error);
        be_.check(rc);
    }

  private:
    const Backend& be_;
    dehalo_prover* p_ = nullptr;
};

// verify_proof::<KZGCommitmentScheme<Bn256>, VerifierGWC | VerifierSHPLONK, Challenge255<_>, Blake2bRead<_, _, _>, SingleStrategy | AccumulatorStrategy>
// (benches/delay_enc.rs:147-165): the verifying half of the params and of the key.  Made from a Backend, the points and the two sums of the reduction run on
// the device; made without one (the second constructor with be == nullptr) it is a host verifier -- a mode the caller chooses, not a fallback.
class Verifier {
  public:
    Verifier(const Backend& be, const ParamsKZG& params, const ProvingKey& pk, dehalo_multiopen m = DEHALO_MULTIOPEN_GWC) {
        be.check(dehalo_verifier_create(be.raw(), params.raw(), pk.raw(), &v_));
        check(dehalo_verifier_set_multiopen(v_, m));
    }
    // ParamsVerifierKZG + VerifyingKey::read: g0 = g[0], g2 / s_g2 the params' 128 raw bytes, the vk in any format
    Verifier(const Backend* be, dehalo_curve curve, uint32_t k, const Affine& g0, const uint8_t g2[128], const uint8_t s_g2[128], ConstraintSystem& cs,
             const std::vector<uint8_t>& vk_bytes, dehalo_serde_format vk_format, uint32_t num_selectors, dehalo_multiopen m = DEHALO_MULTIOPEN_GWC) {
        const int rc = dehalo_verifier_create_vk(be ? be->raw() : nullptr, curve, k, g0.data(), g2, s_g2, cs.descriptor(), vk_bytes.data(), vk_bytes.size(), vk_format,
                                                 num_selectors, &v_);
        if (be) be->check(rc);
        else if (rc != 0) {      // no context to ask: the constructor's own text
            char why[512];
            dehalo_verifier_create_error(why, sizeof why);
            throw std::runtime_error(std::string(why) + " (" + std::to_string(rc) + ")");
        }
        check(dehalo_verifier_set_multiopen(v_, m));
    }
    // IPA (Pallas / Vesta): from a ParamsIPA and a key made under it.  The params are borrowed: they must outlive the verifier.  One multiopen: none to choose
    Verifier(const Backend& be, const ParamsIPAHandle& params, const ProvingKey& pk) { be.check(dehalo_verifier_create_ipa(be.raw(), params.raw(), pk.raw(), &v_)); }
    // IPA, the verifier's side: ParamsIPA::read + VerifyingKey::read, the vk in any format
    Verifier(const Backend& be, const ParamsIPAHandle& params, ConstraintSystem& cs, const std::vector<uint8_t>& vk_bytes, dehalo_serde_format vk_format,
             uint32_t num_selectors) {
        be.check(dehalo_verifier_create_ipa_vk(be.raw(), params.raw(), cs.descriptor(), vk_bytes.data(), vk_bytes.size(), vk_format, num_selectors, &v_));
    }
    ~Verifier() { dehalo_verifier_release(v_); }
    Verifier(const Verifier&) = delete;
    void set_transcript_repr(const Fe& r) { check(dehalo_verifier_set_transcript_repr(v_, r.data())); }
    // DEHALO_PAIRING_ON_HOST (the default) | DEHALO_PAIRING_ON_DEVICE: the pairing checks through the kernel -- verify_each then gives every live proof its own
    // check in ONE launch, without a search.  Throws on a host verifier and on an IPA verifier
    void set_pairing(int mode) { check(dehalo_verifier_set_pairing(v_, mode)); }
    // true: accepted.  false: *reason (if given) says why -- DEHALO_REJECT_MALFORMED, DEHALO_REJECT_PAIRING or (IPA) DEHALO_REJECT_OPENING.  instances: one vector per instance column
    bool verify(const std::vector<uint8_t>& proof, const std::vector<std::vector<Fe>>& instances, int* reason = nullptr) const {
        std::vector<const uint64_t*> ip;
        std::vector<size_t> il;
        for (auto& col : instances) { ip.push_back(col.empty() ? nullptr : col[0].data()); il.push_back(col.size()); }
        int accept = 0;
        check(dehalo_verify_proof(v_, ip.data(), il.data(), (uint32_t)ip.size(), 1, proof.data(), proof.size(), &accept, reason));
        return accept != 0;
    }
    // proofs over one circuit each with the same instance columns' count; ONE pairing check for all (rng == nullptr: operating-system entropy for the weights,
    // which must be unpredictable to whoever made the proofs).  *first_malformed: the first unreadable proof, or -1
    bool verify_batch(const std::vector<std::vector<uint8_t>>& proofs, const std::vector<std::vector<std::vector<Fe>>>& instances, dehalo_rng* rng = nullptr,
                      int64_t* first_malformed = nullptr) const {
        std::vector<const uint8_t*> pp;
        std::vector<size_t> pl, il;
        std::vector<const uint64_t*> ip;
        for (auto& p : proofs) { pp.push_back(p.data()); pl.push_back(p.size()); }
        if (instances.size() != proofs.size()) check(DEHALO_ERR_INVALID);
        const uint32_t columns = instances.empty() ? 0 : (uint32_t)instances[0].size();
        for (auto& one : instances) {
            if (one.size() != columns) check(DEHALO_ERR_INVALID);
            for (auto& col : one) { ip.push_back(col.empty() ? nullptr : col[0].data()); il.push_back(col.size()); }
        }
        int accept = 0;
        check(dehalo_verify_proofs(v_, pp.data(), pl.data(), (uint32_t)pp.size(), ip.data(), il.data(), columns, 1, rng, &accept, first_malformed));
        return accept != 0;
    }
    // a verdict per proof from one batch verification (dehalo_verify_proofs_each): DEHALO_REJECT_NONE for a valid proof, otherwise what verify says of that proof
    // alone.  Arguments and the weights' warning as for verify_batch.  *checks: the subset checks made (1 when every readable proof is valid)
    std::vector<int> verify_each(const std::vector<std::vector<uint8_t>>& proofs, const std::vector<std::vector<std::vector<Fe>>>& instances, dehalo_rng* rng = nullptr,
                                 uint32_t* checks = nullptr) const {
        std::vector<const uint8_t*> pp;
        std::vector<size_t> pl, il;
        std::vector<const uint64_t*> ip;
        for (auto& p : proofs) { pp.push_back(p.data()); pl.push_back(p.size()); }
        if (instances.size() != proofs.size()) check(DEHALO_ERR_INVALID);
        const uint32_t columns = instances.empty() ? 0 : (uint32_t)instances[0].size();
        for (auto& one : instances) {
            if (one.size() != columns) check(DEHALO_ERR_INVALID);
            for (auto& col : one) { ip.push_back(col.empty() ? nullptr : col[0].data()); il.push_back(col.size()); }
        }
        std::vector<int> reasons(proofs.size(), DEHALO_REJECT_NONE);
        check(dehalo_verify_proofs_each(v_, pp.data(), pl.data(), (uint32_t)pp.size(), ip.data(), il.data(), columns, 1, rng, reasons.data(), checks));
        return reasons;
    }
    dehalo_verifier* raw() const { return v_; }

  private:
    void check(int rc) const {
        if (rc != 0) throw std::runtime_error(std::string("dehalo verifier: ") + dehalo_verifier_last_error(v_) + " (" + std::to_string(rc) + ")");
    }
    dehalo_verifier* v_ = nullptr;
};

}  // namespace halo2_amd
