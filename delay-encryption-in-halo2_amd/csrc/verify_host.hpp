// verify_host.hpp -- verify_proof for KZG on the host [UPSTREAM halo2_proofs @ v2023_04_20: plonk/verifier.rs, plonk/{permutation,lookup,vanishing}/verifier.rs,
// poly/kzg/multiopen/{gwc,shplonk}/verifier.rs, poly/kzg/strategy.rs (SingleStrategy, AccumulatorStrategy); shuffles: halo2_proofs v0.3.0], written from the
// published protocol.  A proof is read through the Blake2bRead transcript, the challenges squeezed in the prover's order, the gate, permutation, lookup and shuffle
// expressions evaluated at the read evaluations into expected_h, and either multiopen reduced to TWO term lists  L = sum a_j P_j,  R = sum b_j P_j  over the
// proof's points, the key's commitments and g[0], with  accept  iff  e(L, s_g2) e(-R, g2) = 1:
//   GWC      L = sum_i u^i W_i;  R = sum_i u^i z_i W_i + sum_i u^i sum_j v^j C_ij - (sum_i u^i sum_j v^j e_ij) g[0]
//   SHPLONK  L = h';  R = sum_i c_i sum_j y^j P_ij - (sum_i c_i sum_j y^j r_ij) g[0] - Z_0(u) h + u h',  c_i = v^i zdiff_i / zdiff_0
// (the folded quotient commitment is never computed as a point: its scalar goes to the pieces, times x^(n i)).  A batch multiplies proof i's lists by a weight
// w_i and checks the concatenation with one pairing check.  The order of the evaluations, the queries, their groups and intermediate sets are the EXISTING
// OpeningPlan's (opening_plan.hpp): prover and verifier cannot disagree about layout.
// The points of a proof stand at offsets its shape fixes; they are decompressed before the walk by a backend -- the host's below, or the device's (verify.hip:
// one dehalo_points_decompress_device launch for all proofs of a call) -- and the two sums go through the backend's MSM.  The pairing is pairing_host.hpp's.
// IPA over Pallas / Vesta [UPSTREAM plonk/verifier.rs with QUERY_INSTANCE = true, poly/ipa/multiopen/verifier.rs, poly/ipa/commitment/verifier.rs, poly/ipa/strategy.rs] is
// a third reduction behind the same read: the instance columns enter as commitments (the backend's instance_commitments), the multiopen and the opening argument
// (ipa_reduce_opening) leave ONE term list over the proof's points, the key's and the instance commitments, g[0], U and W, plus per proof k round challenges and
// init = -w c; accept iff  (sum over the list) + sum_idx s[idx] g[idx]  is the identity, s = sum_i compute_s(u_i, init_i) (the backend's g_sum: on the device the
// kernel of ipa.cuh into the MSM over the params' resident g).
// The map.  One proof (verify_walk): walk_read fills a WalkRead (commitments, challenges, evaluations), expected_h evaluates the circuit over it, and one of
// reduce_gwc / reduce_shplonk / reduce_ipa_multiopen appends the proof's terms through a WalkQueries.  One call (verify_proofs_host, after
// verify_check_arguments has made its VerifyInput): stage_points, stage_instances, run_walks, then decide_kzg or decide_ipa into a VerifyVerdict.  A verdict per
// proof (verify_proofs_each_host): the same three stages, then the backend's msm_segments sums each proof's runs apart and blame_search.hpp names the proofs that fail.
// Host only, no HIP header: verify.hip includes it, and tests/native_host/verify_host_check.cpp and verify_ipa_host_check.cpp drive it on the CPU under ASan + UBSan.
#pragma once
#include <chrono>
#include <string>
#include <vector>

#include "../../include/dehalo.h"
#include "blame_search.hpp"
#include "g1_host.hpp"
#include "hostfield.hpp"
#include "key_format.hpp"
#include "opening_plan.hpp"
#include "pairing_host.hpp"
#include "plonk_host.hpp"
#include "transcript_host.hpp"

// Blind::default() of the instance columns' commitments (whole_call.hpp IPA_DEFAULT_BLIND is the prover's twin; this header includes no HIP header)
constexpr uint64_t VERIFY_IPA_DEFAULT_BLIND = 1;

// ---- what decompresses a call's points and sums its two term lists: the host (below) or the device (verify.hip).  A non-zero return is an error of the
// backend (a device error stays an error: nothing falls back to the host)
struct VerifyBackend {
    virtual ~VerifyBackend() {}
    // count x 32 B -> count x {x, y}; a point that is refused is written as (0, 0) (so is the identity's all-zero encoding, which no proof may hold)
    virtual int decompress(const uint8_t* in32, size_t count, uint64_t* xy) = 0;
    // sum_i [scalars_i] xy_i -> one affine point ((0, 0): the identity); scalars Montgomery, canonical words
    virtual int msm(const Fe* scalars, const uint64_t* xy, size_t len, uint64_t out_affine[8]) = 0;
    // segment s < segments: sum over offsets[s] <= i < offsets[s + 1] of [scalars_i] xy_i -> segments affine points; the offsets do not decrease
    virtual int msm_segments(const Fe* scalars, const uint64_t* xy, const uint32_t* offsets, uint32_t segments, uint64_t* out_affine) = 0;
    // IPA only (a backend without ParamsIPA's points refuses both).  commit_lagrange(column, Blind::default()) of `count` instance columns in one batch: column i
    // has lens[i] values (Montgomery, canonical), zero from there on -> count x {x, y}
    virtual int instance_commitments(const Fe* const*, const size_t*, size_t, uint64_t*) { return DEHALO_ERR_UNSUPPORTED; }
    // sum_idx s[idx] g[idx] over the params' 2^k generators, s = sum_i compute_s(challenges[i k .. i k + k), inits[i]) (GuardIPA::compute_s under the inits) -> one
    // affine point
    virtual int g_sum(const Fe*, const Fe*, size_t, uint32_t, uint64_t[8]) { return DEHALO_ERR_UNSUPPORTED; }
    // KZG in device mode only (VerifierKey::pairing): count independent checks e(lr[i][0], s_g2) e(lr[i][1], g2) == 1 in one launch, lr count x 2 affine points ->
    // count bytes, a DEHALO_PAIRING_* status each
    virtual int pairing_checks(const uint64_t*, uint32_t, uint8_t*) { return DEHALO_ERR_UNSUPPORTED; }
};
// compute_s of one proof added into s (2^k scalars): s[idx] += init prod_{bit j of idx set} us[k - 1 - j]
inline void ipa_add_s(const HostField* f, const Fe* us, uint32_t k, const Fe& init, std::vector<Fe>& s) {
    std::vector<Fe> v((size_t)1 << k);
    v[0] = init;
    for (uint32_t j = 0; j < k; j++)
        for (size_t t = 0; t < ((size_t)1 << j); t++) v[((size_t)1 << j) + t] = f->mul(v[t], us[k - 1 - j]);
    for (size_t i = 0; i < v.size(); i++) s[i] = f->add(s[i], v[i]);
}
struct HostVerifyBackend : VerifyBackend {
    const HostField* fr;
    G1Host g1;
    // ParamsIPA's points, borrowed (set_ipa): g and g_lagrange 2^k affine points each, w one
    const uint64_t *g = nullptr, *g_lagrange = nullptr, *w = nullptr;
    uint32_t k = 0;
    HostVerifyBackend(const HostField* fq, const HostField* fr_, uint64_t curve_b) : fr(fr_), g1(fq, curve_b) {}
    void set_ipa(const uint64_t* g_, const uint64_t* g_lagrange_, const uint64_t* w_, uint32_t k_) { g = g_; g_lagrange = g_lagrange_; w = w_; k = k_; }
    int instance_commitments(const Fe* const* cols, const size_t* lens, size_t count, uint64_t* xy) override {
        if (!g_lagrange) return DEHALO_ERR_UNSUPPORTED;
        for (size_t i = 0; i < count; i++) {      // a short MSM over g_lagrange[0 .. len) and [Blind::default()] W
            std::vector<Fe> sc(cols[i], cols[i] + lens[i]);
            std::vector<uint64_t> bs(g_lagrange, g_lagrange + 8 * lens[i]);
            sc.push_back(fr->from_u64(VERIFY_IPA_DEFAULT_BLIND));
            bs.insert(bs.end(), w, w + 8);
            msm(sc.data(), bs.data(), sc.size(), xy + 8 * i);
        }
        return 0;
    }
    int g_sum(const Fe* challenges, const Fe* inits, size_t count, uint32_t k_, uint64_t out_affine[8]) override {
        if (!g || k_ != k) return DEHALO_ERR_UNSUPPORTED;
        std::vector<Fe> s((size_t)1 << k, Fe{});
        for (size_t i = 0; i < count; i++) ipa_add_s(fr, challenges + i * k, k, inits[i], s);
        return msm(s.data(), g, s.size(), out_affine);
    }
    int decompress(const uint8_t* in32, size_t count, uint64_t* xy) override {
        for (size_t i = 0; i < count; i++) g1.decompress(in32 + 32 * i, xy + 8 * i);
        return 0;
    }
    int msm(const Fe* scalars, const uint64_t* xy, size_t len, uint64_t out_affine[8]) override {
        std::vector<Fe> c(len);
        for (size_t i = 0; i < len; i++) c[i] = fr->to_canonical(scalars[i]);
        g1.msm(c.data(), xy, len, out_affine);
        return 0;
    }
    int msm_segments(const Fe* scalars, const uint64_t* xy, const uint32_t* offsets, uint32_t segments, uint64_t* out_affine) override {
        for (uint32_t s = 0; s < segments; s++) msm(scalars + offsets[s], xy + 8 * (size_t)offsets[s], offsets[s + 1] - offsets[s], out_affine + 8 * (size_t)s);
        return 0;
    }
};

// where a call's time went, in milliseconds (dehalo_verifier_last_timings)
struct VerifyStats { double decompress = 0, walk = 0, msm = 0, pairing = 0; };      // (pairing: under IPA the sum over g)
struct VerifyClock {      // lap(): milliseconds since it was made or last read
    typedef std::chrono::steady_clock clk;
    clk::time_point t0 = clk::now();
    double lap() {
        const clk::time_point t = t0;
        t0 = clk::now();
        return std::chrono::duration<double, std::milli>(t0 - t).count();
    }
};

// ---- the verifying half of a key, and of the params: all a verifier keeps
struct VerifierKey {
    int curve = 0;
    const HostField *f = nullptr, *fq = nullptr;
    HostCS cs;
    HostDomain dom;
    uint32_t k = 0, num_selectors = 0;
    std::vector<uint64_t> fixed_commitments, perm_commitments;      // Montgomery affine, 8 u64 each
    std::vector<std::vector<uint8_t>> selectors;                    // packed, as the vk holds them: hashed into the substitute transcript_repr
    Fe transcript_repr{};
    uint64_t g0[8] = {};
    uint8_t g2[128] = {}, s_g2[128] = {};
    int multiopen = DEHALO_MULTIOPEN_GWC;
    int pairing = DEHALO_PAIRING_ON_HOST;      // _ON_DEVICE: the checks go through the backend's pairing_checks (dehalo_verifier_set_pairing)
    int scheme = DEHALO_SCHEME_KZG;      // DEHALO_SCHEME_IPA: the instance columns are committed and queried, the multiopen is the IPA's; g0 = g[0], and u, w below
    uint64_t u[8] = {}, w[8] = {};
    bool unsupported = false;      // init_cs: the message describes a circuit this library does not take

    KeyShape shape() const {
        KeyShape sh;
        sh.nf = cs.num_fixed; sh.npc = cs.perm_cols.size(); sh.nsel = num_selectors; sh.ext_shift = dom.extended_k - dom.k;
        return sh;
    }
    // "" or what is wrong with the circuit / k
    std::string init_cs(int curve_, const dehalo_constraint_system* csd, uint32_t k_) {
        curve = curve_; k = k_;
        f = host_field(curve_scalar_field(curve));
        fq = host_field(curve_base_field(curve));
        const std::string err = cs.load(csd);
        unsupported = cs.unsupported;
        if (!err.empty()) return err;
        if (k > 28 || !dom.init(f, cs.degree(), k)) { unsupported = true; return "extended_k exceeds the field's two-adicity"; }
        if (dom.n < (size_t)cs.blinding_factors() + 3) return "not enough rows available";
        return "";
    }
    // g2 and s_g2: on the twist and in the order-r subgroup
    std::string check_g2() const {
        const PairingHost* ph = pairing_host(curve);
        if (!ph || !ph->ok) return "no pairing on this curve";
        G2Host::Pt Q;
        if (ph->load_g2(g2, Q) != PairingHost::G2_OK || Q.inf) return "g2 is not a point of the order-r subgroup of the twist";
        if (ph->load_g2(s_g2, Q) != PairingHost::G2_OK || Q.inf) return "s_g2 is not a point of the order-r subgroup of the twist";
        return "";
    }
    // vk bytes in any SerdeFormat -> commitments and selectors; "" or what is wrong.  Processed: every commitment decoded (the identity's all-zero encoding is a
    // commitment to the zero column); RawBytes: every stored word below the modulus and every point on the curve or (0, 0); RawBytesUnchecked: copied.
    std::string load_vk(const uint8_t* bytes, size_t len, int format, uint32_t nsel) {
        num_selectors = nsel;
        KeyLayout L;
        const KeyHeaderError he = key_parse_header(bytes, len, format, shape(), k, false, L);
        if (he != KEY_HEADER_OK) return key_header_error_text(he);
        const G1Host g1(fq, curve_b_host(curve));
        const size_t nf = cs.num_fixed, npc = cs.perm_cols.size();
        fixed_commitments.assign(8 * nf, 0);
        perm_commitments.assign(8 * npc, 0);
        for (size_t i = 0; i < nf + npc; i++) {
            const uint8_t* src = bytes + (i < nf ? L.off_fixed_c + L.point * i : L.off_perm_c + L.point * (i - nf));
            uint64_t* dst = i < nf ? &fixed_commitments[8 * i] : &perm_commitments[8 * (i - nf)];
            if (format == DEHALO_SERDE_PROCESSED) {
                const uint32_t st = g1.decompress(src, dst);
                if (st) return point_status_text(st, true);
                continue;
            }
            memcpy(dst, src, 64);
            if (format == DEHALO_SERDE_RAW_BYTES_UNCHECKED) continue;
            const uint32_t st = g1.check_stored(dst);
            if (st && !g1_affine_is_zero(dst)) return point_status_text(st, false);
        }
        selectors.clear();
        for (uint32_t s = 0; s < nsel; s++) selectors.emplace_back(bytes + L.off_selectors + L.sel_bytes * s, bytes + L.off_selectors + L.sel_bytes * (s + 1));
        return "";
    }
    // the substitute transcript_repr keygen gives this key (plonk_host.hpp: the one statement of it)
    void default_transcript_repr() { transcript_repr = substitute_transcript_repr(f, k, cs, fixed_commitments, perm_commitments, selectors); }
    OpeningShape opening_shape(uint32_t circuits) const {
        OpeningShape sh;
        sh.k = k; sh.A = cs.num_advice; sh.num_fixed = cs.num_fixed; sh.I = cs.num_instance; sh.L = (uint32_t)cs.lookups.size(); sh.S = cs.num_sets();
        sh.npc = (uint32_t)cs.perm_cols.size(); sh.bf = cs.blinding_factors(); sh.pieces = dom.quotient_poly_degree;
        sh.query_instance = scheme == DEHALO_SCHEME_IPA;
        sh.circuits = circuits;
        sh.shuffles = (uint32_t)cs.shuffles.size();
        for (auto& q : cs.advice_q) sh.advice_q.push_back({q.index, q.rotation});
        for (auto& q : cs.fixed_q) sh.fixed_q.push_back({q.index, q.rotation});
        for (auto& q : cs.instance_q) sh.instance_q.push_back({q.index, q.rotation});
        return sh;
    }
};

// ---- the two term lists of a call, every proof's appended under its weight
// (IPA has one list, the right one, over the proof's points, the key's and the instance commitments, g[0], U and W; what goes over the params' g is kept as
// each proof's k round challenges and its init = -w c: the backend's g_sum makes the 2^k scalars from them)
struct VerifyTerms {
    std::vector<Fe> ls, rs;
    std::vector<uint64_t> lp, rp;      // 8 u64 a point
    std::vector<Fe> us, inits;         // IPA: k challenges and one init a proof
    // where each walked proof's terms stand (run_walks): its index in the call and the first term of its run in ls and in rs.  The runs are contiguous and in
    // the order of `runs` -- one ends where the next starts, the last at the list's end -- and so are the proofs' challenges (k each) and inits (one each)
    struct Run { uint32_t proof; size_t l0, r0; };
    std::vector<Run> runs;
    void truncate(size_t nl, size_t nr, size_t nu, size_t ni) { ls.resize(nl); lp.resize(8 * nl); rs.resize(nr); rp.resize(8 * nr); us.resize(nu); inits.resize(ni); }
    void left(const Fe& s, const uint64_t* p) { ls.push_back(s); lp.insert(lp.end(), p, p + 8); }
    void right(const Fe& s, const uint64_t* p) { rs.push_back(s); rp.insert(rp.end(), p, p + 8); }
};

// where the points of a proof stand, in the order of the bytes: (byte offset, count) runs.  KZG: every commitment before the evaluations, then the multiopen's at
// the end; IPA: the commitments, f behind the evaluations, then S and the k rounds' (L_j, R_j) behind the q evaluations
inline std::vector<std::pair<size_t, size_t>> verify_point_runs(const OpeningPlan& pl, int scheme, int multiopen) {
    const size_t p0 = (size_t)pl.NC + pl.p_instance - pl.p_hpiece;
    if (scheme != DEHALO_SCHEME_IPA) {
        const size_t p1 = multiopen == DEHALO_MULTIOPEN_SHPLONK ? 2 : pl.groups.size();
        return {{0, p0}, {pl.proof_size(multiopen == DEHALO_MULTIOPEN_SHPLONK ? OpeningPlan::SHPLONK : OpeningPlan::GWC) - 32 * p1, p1}};
    }
    const size_t off_f = 32 * (p0 + pl.instance_write.size() + pl.write.size()), off_s = off_f + 32 * (1 + pl.point_sets.size());
    return {{0, p0}, {off_f, 1}, {off_s, 1 + 2 * (size_t)pl.k}};
}

// what a walk makes of one proof
enum VerifyWalkResult { VERIFY_WALK_OK = 0, VERIFY_WALK_MALFORMED = 1, VERIFY_WALK_OPENING = 2 };

// The IPA opening argument's check [UPSTREAM poly/ipa/commitment/verifier.rs verify_proof, poly/ipa/strategy.rs GuardIPA] on the rest of transcript t, for a commitment
// P whose terms the caller has appended to `out` under `weight` already:  w (P - [v] G_0 + [xi] S + sum_j ([u_j^-1] L_j + [u_j] R_j) - [c b z] U - [f] W) goes to
// out's right list, the k challenges and init = -w c to out.us / out.inits (the sum over g, - w c <s, G>, is the backend's g_sum).  point(): the next 32 bytes as
// a point, absorbed; null when they are none.  The one routine behind a whole proof's last step and dehalo_ipa_verify.
template <class NextPoint>
inline VerifyWalkResult ipa_reduce_opening(const HostField* f, dehalo_transcript& t, NextPoint&& point, uint32_t k, const Fe& weight, const Fe& x3, const Fe& v,
                                           const uint64_t* g0, const uint64_t* U, const uint64_t* W, VerifyTerms& out) {
    const uint64_t* S = point();
    if (!S) return VERIFY_WALK_MALFORMED;
    const Fe xi = t.squeeze(), z = t.squeeze();
    std::vector<const uint64_t*> Ls(k), Rs(k);
    std::vector<Fe> us(k);
    for (uint32_t j = 0; j < k; j++) {
        Ls[j] = point();
        Rs[j] = Ls[j] ? point() : nullptr;
        if (!Rs[j]) return VERIFY_WALK_MALFORMED;
        us[j] = t.squeeze();
    }
    Fe c, fv;
    if (!t.read_scalar(c) || !t.read_scalar(fv) || t.remaining()) return VERIFY_WALK_MALFORMED;
    std::vector<Fe> inv = us;
    if (!f->batch_invert(inv.data(), inv.size())) return VERIFY_WALK_OPENING;      // a round challenge is zero
    Fe b = f->one, cur = x3;      // compute_b: prod_j (1 + u_{k - j} x3^(2^j))
    for (uint32_t j = k; j-- > 0;) {
        b = f->mul(b, f->add(f->one, f->mul(us[j], cur)));
        cur = f->sqr(cur);
    }
    out.right(f->mul(weight, xi), S);
    for (uint32_t j = 0; j < k; j++) {
        out.right(f->mul(weight, inv[j]), Ls[j]);
        out.right(f->mul(weight, us[j]), Rs[j]);
    }
    const Fe wc = f->mul(weight, c);
    out.right(f->neg(f->mul(wc, f->mul(b, z))), U);
    out.right(f->neg(f->mul(weight, fv)), W);
    out.right(f->neg(f->mul(weight, v)), g0);      // what verify_opening subtracts from s[0]
    out.us.insert(out.us.end(), us.begin(), us.end());
    out.inits.push_back(f->neg(wc));
    return VERIFY_WALK_OK;
}

// ---- one proof, a function per phase: walk_read -> expected_h -> reduce_gwc | reduce_shplonk | reduce_ipa_multiopen (verify_walk)
// the instance columns' values of one proof: [circuit][column] -> values (Montgomery, canonical)
typedef std::vector<std::vector<std::vector<Fe>>> InstanceValues;

// what reading a proof up to the end of its evaluations leaves
struct WalkRead {
    dehalo_transcript t;
    const uint64_t* pts = nullptr; size_t next_pt = 0;      // the proof's points, decoded already, in the order of the bytes, and the cursor over them
    std::vector<const uint64_t*> cm;    // polynomial id -> its commitment
    std::vector<Fe> challenges, E;      // the phases' challenges; the evaluations, by the plan's slot
    Fe theta{}, beta{}, gamma{}, y{}, x{}, xn{};      // xn = x^n
    const uint64_t* point() {           // the next 32 bytes are a point: absorbed as the reader would absorb it
        const uint64_t* p = pts + 8 * next_pt++;
        t.write_point(p, false);
        t.pos += 32;
        return p;
    }
};

// The transcript from its start to the last evaluation [UPSTREAM plonk/verifier.rs].  The key's scheme decides how the instance columns enter: KZG their values, as
// scalars; IPA their commitments instance_cm (8 u64 a column), their evaluations read first.  MALFORMED: a scalar is not below r; OPENING (IPA): an identity instance_cm.
inline VerifyWalkResult walk_read(const VerifierKey& vk, const OpeningPlan& pl, const uint8_t* proof, size_t len, const uint64_t* pts, const InstanceValues& instances,
                                  const uint64_t* instance_cm, WalkRead& w) {
    const HostCS& cs = vk.cs;
    dehalo_transcript& t = w.t;
    t.init_read(vk.curve, proof, len);
    w.pts = pts; w.cm.assign(pl.num_polys, nullptr);
    t.common_scalar(vk.transcript_repr);
    if (vk.scheme == DEHALO_SCHEME_IPA) {
        for (uint32_t i = 0; i < cs.num_instance; i++) {
            if (!t.write_point(instance_cm + 8 * i, false)) return VERIFY_WALK_OPENING;
            w.cm[pl.p_instance + i] = instance_cm + 8 * i;
        }
    } else
        for (auto& circuit : instances)
            for (auto& column : circuit)
                for (const Fe& v : column) t.common_scalar(v);
    w.challenges.assign(cs.challenge_phase.size(), Fe{});
    for (uint32_t ph = 0; ph < cs.num_phases; ph++) {
        for (uint32_t c = 0; c < pl.circuits; c++)
            for (uint32_t col = 0; col < pl.A; col++)
                if (cs.advice_phase[col] == ph) w.cm[pl.adv(c) + col] = w.point();
        for (size_t j = 0; j < w.challenges.size(); j++)
            if (cs.challenge_phase[j] == ph) w.challenges[j] = t.squeeze();
    }
    w.theta = t.squeeze();
    for (uint32_t c = 0; c < pl.circuits; c++)
        for (uint32_t l = 0; l < pl.L; l++) {
            w.cm[pl.perm(c) + 2 * l] = w.point();
            w.cm[pl.perm(c) + 2 * l + 1] = w.point();
        }
    w.beta = t.squeeze(); w.gamma = t.squeeze();
    for (uint32_t off : pl.product_order) w.cm[pl.o_pz + off] = w.point();      // every circuit's permutation, lookup, shuffle products; the random polynomial
    w.y = t.squeeze();
    for (uint32_t i = 0; i < vk.dom.quotient_poly_degree; i++) w.cm[pl.p_hpiece + i] = w.point();
    w.x = t.squeeze();
    for (uint32_t i = 0; i < cs.num_fixed; i++) w.cm[pl.p_fixed + i] = &vk.fixed_commitments[8 * i];
    for (size_t j = 0; j < cs.perm_cols.size(); j++) w.cm[pl.p_sigma + j] = &vk.perm_commitments[8 * j];
    w.E.assign(pl.eval_count, Fe{});
    for (int64_t slot : pl.instance_write)      // (none unless the instance columns are queried)
        if (!t.read_scalar(w.E[(size_t)slot])) return VERIFY_WALK_MALFORMED;
    for (int64_t slot : pl.write)
        if (!t.read_scalar(w.E[(size_t)slot])) return VERIFY_WALK_MALFORMED;
    w.xn = w.x;
    for (uint32_t i = 0; i < vk.dom.k; i++) w.xn = vk.f->sqr(w.xn);
    return VERIFY_WALK_OK;
}

// expected_h's working state: the Lagrange values at x every circuit shares, then per circuit c the expression graph's values `val` and the three arguments'
// expressions, each folded into acc with y.  Reads no transcript and makes no term.
struct ExpectedH {
    const OpeningPlan& pl; const WalkRead& w; const InstanceValues& instances;
    const HostField* f; const HostCS& cs; const HostDomain& d;
    const bool ipa; const int32_t last;
    Fe xn1, n_fe, l_0, l_last, active, acc{};
    uint32_t c = 0;
    std::vector<Fe> val;
    ExpectedH(const VerifierKey& vk, const OpeningPlan& pl_, const WalkRead& w_, const InstanceValues& instances_)
        : pl(pl_), w(w_), instances(instances_), f(vk.f), cs(vk.cs), d(vk.dom), ipa(vk.scheme == DEHALO_SCHEME_IPA), last(-(int32_t)(vk.cs.blinding_factors() + 1)) {
        xn1 = f->sub(w.xn, f->one); n_fe = f->from_u64((uint64_t)d.n);
        l_0 = l_i(0); l_last = l_i(last);
        Fe l_blind{};
        for (int32_t i = -1; i > last; i--) l_blind = f->add(l_blind, l_i(i));
        active = f->sub(f->one, f->add(l_last, l_blind));
    }
    Fe l_i(int64_t i) const {      // l_i(x) = omega^i (x^n - 1) / (n (x - omega^i))
        const int64_t m = ((i % (int64_t)d.n) + (int64_t)d.n) % (int64_t)d.n;
        const Fe wi = f->pow_u64(d.omega, (uint64_t)m);
        return f->mul(f->mul(wi, xn1), f->invert(f->mul(n_fe, f->sub(w.x, wi))));
    }
    const Fe& ev(uint32_t poly, int32_t rot) const { return w.E[(size_t)pl.slot(poly, rot)]; }
    Fe instance_eval(uint32_t col, int32_t rot) const {      // QUERY_INSTANCE = false: interpolated from the values; true (IPA): read
        if (ipa) return ev(pl.p_instance + col, rot);
        Fe sum{};
        const std::vector<Fe>& vals = instances[c][col];
        for (size_t j = 0; j < vals.size(); j++)
            if (!vals[j].is_zero()) sum = f->add(sum, f->mul(vals[j], l_i((int64_t)j - rot)));
        return sum;
    }
    void fold(const Fe& term) { acc = f->add(f->mul(acc, w.y), term); }
    Fe compress(const std::vector<uint32_t>& es) const {
        Fe sum{};
        for (uint32_t e : es) sum = f->add(f->mul(sum, w.theta), val[e]);
        return sum;
    }
    void graph() {      // every node of the circuit's expressions at the evaluations: children precede their parents
        val.resize(cs.nodes.size());
        for (size_t i = 0; i < cs.nodes.size(); i++) {
            const dehalo_expr_node& e = cs.nodes[i];
            switch (e.kind) {
                case DEHALO_EXPR_CONSTANT: val[i] = f->mul(cs.constants[e.a], f->one); break;
                case DEHALO_EXPR_FIXED: val[i] = ev(pl.p_fixed + e.a, e.rotation); break;
                case DEHALO_EXPR_ADVICE: val[i] = ev(pl.adv(c) + e.a, e.rotation); break;
                case DEHALO_EXPR_INSTANCE: val[i] = instance_eval(e.a, e.rotation); break;
                case DEHALO_EXPR_CHALLENGE: val[i] = w.challenges[e.a]; break;
                case DEHALO_EXPR_NEGATED: val[i] = f->neg(val[e.a]); break;
                case DEHALO_EXPR_SUM: val[i] = f->add(val[e.a], val[e.b]); break;
                case DEHALO_EXPR_PRODUCT: val[i] = f->mul(val[e.a], val[e.b]); break;
                default: val[i] = f->mul(val[e.a], f->mul(cs.constants[e.b], f->one)); break;      // SCALED
            }
        }
    }
    void permutation() {      // permutation::verifier::Evaluated::expressions
        const uint32_t S = pl.S, chunk = cs.chunk_len();
        auto column_eval = [&](const dehalo_column_query& q) {
            return q.kind == DEHALO_COLUMN_ADVICE ? ev(pl.adv(c) + q.index, 0) : q.kind == DEHALO_COLUMN_FIXED ? ev(pl.p_fixed + q.index, 0) : instance_eval(q.index, 0);
        };
        fold(f->mul(l_0, f->sub(f->one, ev(pl.pz(c), 0))));
        const Fe zl = ev(pl.pz(c) + S - 1, 0);
        fold(f->mul(l_last, f->sub(f->sqr(zl), zl)));
        for (uint32_t s = 1; s < S; s++) fold(f->mul(l_0, f->sub(ev(pl.pz(c) + s, 0), ev(pl.pz(c) + s - 1, last))));
        Fe cur = f->mul(w.beta, w.x);      // beta x delta^j, running across the sets' column chunks
        for (uint32_t s = 0; s < S; s++) {
            Fe left = ev(pl.pz(c) + s, 1), right = ev(pl.pz(c) + s, 0);
            for (size_t j = (size_t)s * chunk; j < std::min<size_t>((size_t)(s + 1) * chunk, cs.perm_cols.size()); j++) {
                const Fe cv = column_eval(cs.perm_cols[j]);
                left = f->mul(left, f->add(f->add(cv, f->mul(w.beta, ev(pl.p_sigma + (uint32_t)j, 0))), w.gamma));
                right = f->mul(right, f->add(f->add(cv, cur), w.gamma));
                cur = f->mul(cur, f->delta);
            }
            fold(f->mul(f->sub(left, right), active));
        }
    }
    void lookup(uint32_t l) {      // lookup::verifier::Evaluated::expressions
        const uint32_t zc = pl.lz(c) + l, ai = pl.perm(c) + 2 * l, ti = ai + 1;
        const Fe &z0 = ev(zc, 0), &z1 = ev(zc, 1), &a0 = ev(ai, 0), &am1 = ev(ai, -1), &s0 = ev(ti, 0);
        const Fe left = f->mul(f->mul(z1, f->add(a0, w.beta)), f->add(s0, w.gamma));
        const Fe right = f->mul(f->mul(z0, f->add(compress(cs.lookups[l].inputs), w.beta)), f->add(compress(cs.lookups[l].tables), w.gamma));
        fold(f->mul(l_0, f->sub(f->one, z0)));
        fold(f->mul(l_last, f->sub(f->sqr(z0), z0)));
        fold(f->mul(f->sub(left, right), active));
        fold(f->mul(l_0, f->sub(a0, s0)));
        fold(f->mul(f->mul(f->sub(a0, s0), f->sub(a0, am1)), active));
    }
    void shuffle(uint32_t j) {      // shuffles: l0 (1 - z), l_last (z^2 - z), l_active (z(wx) (S + gamma) - z(x) (A + gamma))
        const Fe &z0 = ev(pl.sz(c) + j, 0), &z1 = ev(pl.sz(c) + j, 1);
        fold(f->mul(l_0, f->sub(f->one, z0)));
        fold(f->mul(l_last, f->sub(f->sqr(z0), z0)));
        fold(f->mul(f->sub(f->mul(z1, f->add(compress(cs.shuffles[j].tables), w.gamma)), f->mul(z0, f->add(compress(cs.shuffles[j].inputs), w.gamma))), active));
    }
};
// expected_h [UPSTREAM plonk/verifier.rs]: every circuit's gates, then its permutation, lookup and shuffle expressions, at the read evaluations, folded with y
inline Fe expected_h(const VerifierKey& vk, const OpeningPlan& pl, const WalkRead& w, const InstanceValues& instances) {
    ExpectedH h(vk, pl, w, instances);
    for (h.c = 0; h.c < pl.circuits; h.c++) {
        h.graph();
        for (uint32_t g : vk.cs.gates) h.fold(h.val[g]);
        if (pl.S) h.permutation();
        for (uint32_t l = 0; l < pl.L; l++) h.lookup(l);
        for (uint32_t j = 0; j < pl.H; j++) h.shuffle(j);
    }
    return h.acc;
}

// What the three reductions share: the value and the commitment behind a query, and the points x omega^rot of the plan's rotations (points[i]: pl.point_rot[i]).
struct WalkQueries {
    const HostField* f; const OpeningPlan& pl; WalkRead& w; VerifyTerms& out;
    Fe hfold_eval;     // the folded quotient's value, expected_h / (x^n - 1)  (x^n = 1 with negligible probability: the value is then 0 and the check fails)
    std::vector<Fe> points;
    WalkQueries(const VerifierKey& vk, const OpeningPlan& pl_, WalkRead& w_, const Fe& expected_h_, VerifyTerms& out_) : f(vk.f), pl(pl_), w(w_), out(out_) {
        hfold_eval = f->mul(expected_h_, f->invert(f->sub(w.xn, f->one)));
        for (int32_t r : pl.point_rot) points.push_back(vk.dom.rotate_omega(w.x, r));
    }
    const Fe& eval_of(int64_t slot) const { return slot >= 0 ? w.E[(size_t)slot] : hfold_eval; }
    // coef x the commitment of polynomial `poly`, to the right list; the folded quotient h = sum_i x^(n i) h_i goes to its pieces
    void commitment_term(const Fe& coef, uint32_t poly) {
        if (poly != pl.p_hfold) { out.right(coef, w.cm[poly]); return; }
        Fe xp = coef;
        for (uint32_t i = pl.p_hpiece; i < pl.p_instance; i++) {
            out.right(xp, w.cm[i]);
            xp = f->mul(xp, w.xn);
        }
    }
};

// The Lagrange bases of the point sets `sets` (indices into points) at `at`, set after set: per point a of a set  prod_{b != a} (at - z_b) / (z_a - z_b).  The
// denominators are inverted in ONE batch, and with them the caller's own in `also`, in place.  A zero among them (two points coincide, `at` is an opening point:
// negligible probability) has the inverse 0.
inline std::vector<Fe> lagrange_basis_at(const HostField* f, const std::vector<Fe>& points, const std::vector<std::vector<uint32_t>>& sets, const Fe& at, std::vector<Fe>& also) {
    std::vector<Fe> basis, inv = also;
    for (const std::vector<uint32_t>& T : sets)
        for (size_t a = 0; a < T.size(); a++) {
            Fe num = f->one, den = f->one;
            for (size_t b = 0; b < T.size(); b++)
                if (b != a) { num = f->mul(num, f->sub(at, points[T[b]])); den = f->mul(den, f->sub(points[T[a]], points[T[b]])); }
            basis.push_back(num);
            inv.push_back(den);
        }
    if (!f->batch_invert(inv.data(), inv.size())) for (Fe& e : inv) e = f->invert(e);
    std::copy(inv.begin(), inv.begin() + also.size(), also.begin());
    for (size_t i = 0; i < basis.size(); i++) basis[i] = f->mul(basis[i], inv[also.size() + i]);
    return basis;
}

// VerifierGWC::verify_proof.  (Groups and points are numbered alike, by the first appearance of their rotation: group gi opens at points[gi].)
inline VerifyWalkResult reduce_gwc(const VerifierKey& vk, WalkQueries& q, const Fe& weight) {
    const HostField* f = q.f; const OpeningPlan& pl = q.pl;
    const Fe v = q.w.t.squeeze();
    std::vector<const uint64_t*> W;
    for (size_t gi = 0; gi < pl.groups.size(); gi++) W.push_back(q.w.point());
    const Fe u = q.w.t.squeeze();
    Fe pu = weight, eval_multi{};
    for (size_t gi = 0; gi < pl.groups.size(); gi++) {
        const OpeningPlan::Group& g = pl.groups[gi];
        q.out.left(pu, W[gi]);
        q.out.right(f->mul(pu, q.points[gi]), W[gi]);
        Fe pv = pu;
        for (size_t j = 0; j < g.polys.size(); j++) {
            q.commitment_term(pv, g.polys[j]);
            eval_multi = f->add(eval_multi, f->mul(pv, q.eval_of(g.evals[j])));
            pv = f->mul(pv, v);
        }
        pu = f->mul(pu, u);
    }
    q.out.right(f->neg(eval_multi), vk.g0);
    return VERIFY_WALK_OK;
}

// VerifierSHPLONK::verify_proof over the plan's intermediate sets.  (u an opening point, or two points coinciding: inverses taken as 0, and the pairing fails.)
inline VerifyWalkResult reduce_shplonk(const VerifierKey& vk, WalkQueries& q, const Fe& weight) {
    const HostField* f = q.f; const OpeningPlan& pl = q.pl;
    const Fe y = q.w.t.squeeze(), v = q.w.t.squeeze();
    const uint64_t* h = q.w.point();
    const Fe u = q.w.t.squeeze();
    const uint64_t* h2 = q.w.point();
    const size_t ns = pl.point_sets.size();
    std::vector<Fe> zdiff(ns, f->one);      // per set: prod over the points outside it (u - point)
    Fe z_0 = f->one;                        // prod over set 0's points (u - point)
    for (size_t si = 0; si < ns; si++) {
        const std::vector<uint32_t>& T = pl.point_sets[si];
        for (uint32_t pi = 0; pi < q.points.size(); pi++)
            if (std::find(T.begin(), T.end(), pi) == T.end()) zdiff[si] = f->mul(zdiff[si], f->sub(u, q.points[pi]));
            else if (si == 0) z_0 = f->mul(z_0, f->sub(u, q.points[pi]));
    }
    std::vector<Fe> zdiff_0_inv(zdiff.begin(), zdiff.begin() + 1);      // (the quotient's query makes every plan's first set)
    const std::vector<Fe> basis = lagrange_basis_at(f, q.points, pl.point_sets, u, zdiff_0_inv);
    Fe vi = weight, r_total{};
    const Fe* set_basis = basis.data();
    for (size_t si = 0; si < ns; si++) {
        const size_t np = pl.point_sets[si].size();
        Fe yj = f->mul(f->mul(vi, zdiff[si]), zdiff_0_inv[0]);      // c_i = v^i zdiff_i / zdiff_0, then times y^j
        for (uint32_t ci : pl.set_members[si]) {
            const OpeningPlan::Commitment& m = pl.commitments[ci];
            Fe r{};
            for (size_t a = 0; a < np; a++) r = f->add(r, f->mul(set_basis[a], q.eval_of(m.evals[a])));
            q.commitment_term(yj, m.poly);
            r_total = f->add(r_total, f->mul(yj, r));
            yj = f->mul(yj, y);
        }
        vi = f->mul(vi, v);
        set_basis += np;
    }
    q.out.right(f->neg(r_total), vk.g0);
    q.out.right(f->neg(f->mul(weight, z_0)), h);
    q.out.right(f->mul(weight, u), h2);
    q.out.left(weight, h2);
    return VERIFY_WALK_OK;
}

// VerifierIPA::verify_proof over the plan's intermediate sets, then the opening argument's check of the final commitment P (ipa_reduce_opening).  MALFORMED: a
// scalar is not below r; OPENING: x_3 is an opening point, a round challenge is zero.
inline VerifyWalkResult reduce_ipa_multiopen(const VerifierKey& vk, WalkQueries& q, const Fe& weight) {
    const HostField* f = q.f; const OpeningPlan& pl = q.pl;
    dehalo_transcript& t = q.w.t;
    const Fe x1 = t.squeeze(), x2 = t.squeeze();
    const uint64_t* f_commitment = q.w.point();
    const Fe x3 = t.squeeze();
    const size_t ns = pl.point_sets.size();
    std::vector<Fe> q_evals(ns);
    for (Fe& e : q_evals)
        if (!t.read_scalar(e)) return VERIFY_WALK_MALFORMED;
    std::vector<Fe> vanish_inv(ns, f->one);      // per set: prod over its points (x_3 - point), then its inverse
    for (size_t si = 0; si < ns; si++)
        for (uint32_t pi : pl.point_sets[si]) {
            const Fe diff = f->sub(x3, q.points[pi]);
            if (diff.is_zero()) return VERIFY_WALK_OPENING;
            vanish_inv[si] = f->mul(vanish_inv[si], diff);
        }
    const std::vector<Fe> basis = lagrange_basis_at(f, q.points, pl.point_sets, x3, vanish_inv);
    // per set: the x_1-folded evaluations at its points, their interpolant's value at x_3, and (q_eval - that) / prod (x_3 - point), folded with x_2
    Fe f_eval{};
    const Fe* set_basis = basis.data();
    for (size_t si = 0; si < ns; si++) {
        const size_t np = pl.point_sets[si].size();
        std::vector<Fe> evs(np, Fe{});
        for (uint32_t ci : pl.set_members[si])
            for (size_t a = 0; a < np; a++) evs[a] = f->add(f->mul(evs[a], x1), q.eval_of(pl.commitments[ci].evals[a]));
        Fe r{};
        for (size_t a = 0; a < np; a++) r = f->add(r, f->mul(evs[a], set_basis[a]));
        f_eval = f->add(f->mul(f_eval, x2), f->mul(f->sub(q_evals[si], r), vanish_inv[si]));
        set_basis += np;
    }
    const Fe x4 = t.squeeze();
    // P = x_4^ns f + sum_si x_4^(ns - 1 - si) q_si,  q_si = sum_m x_1^(M - 1 - m) C_m: never formed, its scalars go to the commitments; v likewise
    std::vector<Fe> x4p(ns + 1, weight);      // weight x_4^i
    for (size_t i = 1; i <= ns; i++) x4p[i] = f->mul(x4p[i - 1], x4);
    q.out.right(x4p[ns], f_commitment);
    Fe v = f_eval;
    for (size_t si = 0; si < ns; si++) {
        const std::vector<uint32_t>& M = pl.set_members[si];
        Fe coef = x4p[ns - 1 - si];
        for (size_t m = M.size(); m-- > 0;) {
            q.commitment_term(coef, pl.commitments[M[m]].poly);
            coef = f->mul(coef, x1);
        }
        v = f->add(f->mul(v, x4), q_evals[si]);
    }
    return ipa_reduce_opening(f, t, [&] { return q.w.point(); }, pl.k, weight, x3, v, vk.g0, vk.u, vk.w, q.out);
}

// One proof whose length is the shape's and whose points are decoded (none refused): read, expected_h and the reduction of the key's scheme and multiopen, the
// terms appended to `out` under `weight`.  On MALFORMED or OPENING (walk_read, reduce_ipa_multiopen) nothing of `out` is meaningful.
inline VerifyWalkResult verify_walk(const VerifierKey& vk, const OpeningPlan& pl, const uint8_t* proof, size_t len, const uint64_t* pts, const InstanceValues& instances,
                                    const uint64_t* instance_cm, const Fe& weight, VerifyTerms& out) {
    WalkRead w;
    const VerifyWalkResult read = walk_read(vk, pl, proof, len, pts, instances, instance_cm, w);
    if (read != VERIFY_WALK_OK) return read;
    WalkQueries q(vk, pl, w, expected_h(vk, pl, w, instances), out);
    if (vk.scheme == DEHALO_SCHEME_IPA) return reduce_ipa_multiopen(vk, q, weight);
    return vk.multiopen == DEHALO_MULTIOPEN_SHPLONK ? reduce_shplonk(vk, q, weight) : reduce_gwc(vk, q, weight);
}

// ---- one call: `count` proofs under one key.  instances[(i N + c) nic + j] / instance_lens likewise: proof i's circuit c's column j (Montgomery words, any
// residue); weights: count scalars (Montgomery).  verify_check_arguments fills `plan`; the caller sets `weights` after it.
struct VerifyInput {
    const uint8_t* const* proofs = nullptr; const size_t* lens = nullptr; uint32_t count = 0;
    const uint64_t* const* instances = nullptr; const size_t* instance_lens = nullptr;
    uint32_t nic = 0, N = 0;      // instance columns; circuits a proof
    const Fe* weights = nullptr;
    OpeningPlan plan;
};
// What the call found.  accept: every proof is readable and the check holds; first_malformed: the first unreadable proof or -1; reason: a dehalo_reject_reason
struct VerifyVerdict { int accept = 0; int64_t first_malformed = -1; int reason = DEHALO_REJECT_NONE; VerifyStats stats; };
inline int verify_fail(std::string* error, int rc, const std::string& why) { if (error) *error = why; return rc; }

// the caller's errors of a verify call, before anything is read or drawn: 0 -- and in.plan is the call's opening plan --, DEHALO_ERR_INVALID, or
// DEHALO_ERR_UNSUPPORTED for a shape the opening plan refuses
inline int verify_check_arguments(const VerifierKey& vk, VerifyInput& in, std::string* error) {
    if (in.count && (!in.proofs || !in.lens)) return verify_fail(error, DEHALO_ERR_INVALID, "verify_proofs: null argument");
    if (in.N == 0) return verify_fail(error, DEHALO_ERR_INVALID, "verify_proofs: no circuit");
    if (in.count && in.nic != vk.cs.num_instance) return verify_fail(error, DEHALO_ERR_INVALID, "verify_proofs: instances.len() != num_instance_columns");
    if (in.nic && in.count && (!in.instances || !in.instance_lens)) return verify_fail(error, DEHALO_ERR_INVALID, "verify_proofs: null instances");
    in.plan = OpeningPlan(vk.opening_shape(in.N));
    if (!in.plan.error.empty()) return verify_fail(error, DEHALO_ERR_UNSUPPORTED, in.plan.error);
    const size_t usable = vk.dom.n - (vk.cs.blinding_factors() + 1);
    for (size_t e = 0; e < (size_t)in.count * in.N * in.nic; e++) {
        if (in.instance_lens[e] > usable) return verify_fail(error, DEHALO_ERR_INVALID, "verify_proofs: an instance column is longer than the usable rows");
        if (in.instance_lens[e] && !in.instances[e]) return verify_fail(error, DEHALO_ERR_INVALID, "verify_proofs: null instance column");
    }
    return 0;
}

// the proofs of a call whose length is the shape's (`sized` of them, proof i the slot_of[i]-th), their np points each decoded, their instance columns' values and,
// under IPA, those columns' commitments (nic a proof, in the order of the slots)
struct VerifyStaged {
    size_t np = 0, sized = 0;
    std::vector<size_t> slot_of;
    std::vector<uint8_t> malformed;      // per proof: bytes missing or trailing; later a refused point, a scalar not below r
    std::vector<uint8_t> opening;        // per proof: readable and no proof (run_walks)
    std::vector<uint64_t> xy, inst_cm;
    std::vector<InstanceValues> inst_of;
    const uint64_t* points(uint32_t i) const { return xy.data() + 8 * np * slot_of[i]; }
};

// every proof's points, decoded in one call of the backend
inline int stage_points(const VerifierKey& vk, VerifyBackend& be, const VerifyInput& in, VerifyStaged& sg, VerifyStats& st, std::string* error) {
    const int mo = vk.multiopen == DEHALO_MULTIOPEN_SHPLONK ? DEHALO_MULTIOPEN_SHPLONK : DEHALO_MULTIOPEN_GWC;
    const size_t size = in.plan.proof_size(vk.scheme == DEHALO_SCHEME_IPA ? OpeningPlan::IPA : mo == DEHALO_MULTIOPEN_SHPLONK ? OpeningPlan::SHPLONK : OpeningPlan::GWC);
    const std::vector<std::pair<size_t, size_t>> runs = verify_point_runs(in.plan, vk.scheme, mo);
    for (auto& r : runs) sg.np += r.second;
    sg.malformed.assign(in.count, 0);
    sg.opening.assign(in.count, 0);
    sg.slot_of.assign(in.count, 0);
    std::vector<uint8_t> enc;
    for (uint32_t i = 0; i < in.count; i++) {
        if (in.lens[i] != size || !in.proofs[i]) { sg.malformed[i] = 1; continue; }      // bytes missing or trailing
        sg.slot_of[i] = sg.sized++;
        for (auto& r : runs) enc.insert(enc.end(), in.proofs[i] + r.first, in.proofs[i] + r.first + 32 * r.second);
    }
    sg.xy.assign(8 * sg.np * sg.sized + 8, 0);
    VerifyClock clock;
    const int rc = sg.sized ? be.decompress(enc.data(), sg.np * sg.sized, sg.xy.data()) : 0;
    st.decompress = clock.lap();
    return rc ? verify_fail(error, rc, "verify_proofs: point decompression failed") : 0;
}

// the instance columns' values; under IPA their commitments, every column of every proof in one batch of the backend
inline int stage_instances(const VerifierKey& vk, VerifyBackend& be, const VerifyInput& in, VerifyStaged& sg, std::string* error) {
    sg.inst_of.resize(in.count);
    for (uint32_t i = 0; i < in.count; i++) {
        if (sg.malformed[i]) continue;
        sg.inst_of[i].assign(in.N, std::vector<std::vector<Fe>>(in.nic));
        for (uint32_t c = 0; c < in.N; c++)
            for (uint32_t j = 0; j < in.nic; j++) {
                const size_t e = ((size_t)i * in.N + c) * in.nic + j;
                std::vector<Fe>& column = sg.inst_of[i][c][j];
                column.resize(in.instance_lens[e]);
                for (size_t r = 0; r < column.size(); r++) {
                    Fe w;
                    memcpy(w.v, in.instances[e] + 4 * r, 32);
                    column[r] = vk.f->mul(w, vk.f->one);      // a word stands for its residue
                }
            }
    }
    sg.inst_cm.assign(8 * sg.sized * in.nic + 8, 0);
    if (vk.scheme != DEHALO_SCHEME_IPA || !sg.sized || !in.nic) return 0;
    std::vector<const Fe*> cols;      // (N = 1: the plan refuses more)
    std::vector<size_t> col_lens;
    for (uint32_t i = 0; i < in.count; i++)
        for (uint32_t j = 0; j < in.nic && !sg.malformed[i]; j++) { cols.push_back(sg.inst_of[i][0][j].data()); col_lens.push_back(sg.inst_of[i][0][j].size()); }
    const int rc = be.instance_commitments(cols.data(), col_lens.data(), cols.size(), sg.inst_cm.data());
    return rc ? verify_fail(error, rc, "verify_proofs: the instance columns' commitments failed") : 0;
}

// the walks: every staged proof's terms under its weight, and where they stand (terms.runs); a proof the walk rejects leaves nothing in the lists.
// -> some readable proof is no proof (x_3 at an opening point, a zero round challenge: sg.opening says which)
inline bool run_walks(const VerifierKey& vk, const VerifyInput& in, VerifyStaged& sg, VerifyTerms& terms) {
    bool opening_rejected = false;
    for (uint32_t i = 0; i < in.count; i++) {
        if (sg.malformed[i]) continue;
        const uint64_t* pts = sg.points(i);
        for (size_t j = 0; j < sg.np && !sg.malformed[i]; j++)
            if (g1_affine_is_zero(pts + 8 * j)) sg.malformed[i] = 1;      // refused by the decoder, or the identity
        if (sg.malformed[i]) continue;
        const size_t l0 = terms.ls.size(), r0 = terms.rs.size(), u0 = terms.us.size(), i0 = terms.inits.size();
        const VerifyWalkResult wr = verify_walk(vk, in.plan, in.proofs[i], in.lens[i], pts, sg.inst_of[i], sg.inst_cm.data() + 8 * sg.slot_of[i] * in.nic,
                                                vk.f->mul(in.weights[i], vk.f->one), terms);
        if (wr == VERIFY_WALK_OK) terms.runs.push_back({i, l0, r0});
        else terms.truncate(l0, r0, u0, i0);
        if (wr == VERIFY_WALK_MALFORMED) sg.malformed[i] = 1;
        if (wr == VERIFY_WALK_OPENING) { sg.opening[i] = 1; opening_rejected = true; }
    }
    return opening_rejected;
}

// two affine sums cancel: fresh = -(gs), (0, 0) the identity
inline bool ipa_sums_cancel(const HostField* fq, const uint64_t fresh[8], const uint64_t gs[8]) {
    Fe gy;
    memcpy(gy.v, gs + 4, 32);
    gy = fq->neg(gy);      // -(x, y) = (x, -y); (0, 0) stays the identity
    return memcmp(fresh, gs, 32) == 0 && memcmp(fresh + 4, gy.v, 32) == 0;
}

// The IPA acceptance, the one statement of it (a call's last step, and dehalo_ipa_verify's): *accept = 1 iff  sum over the fresh bases + sum over g = the identity
// -- two affine results of the backend, compared here.  Returns the backend's error.
inline int decide_ipa(VerifyBackend& be, const VerifyTerms& terms, size_t count, uint32_t k, const HostField* fq, int* accept, VerifyStats* st = nullptr,
                      std::string* error = nullptr) {
    VerifyClock clock;
    uint64_t fresh[8] = {}, gs[8] = {};      // (no proof: both sums are the identity)
    int rc = count ? be.msm(terms.rs.data(), terms.rp.data(), terms.rs.size(), fresh) : 0;
    if (rc) return verify_fail(error, rc, "verify_proofs: the multi-scalar multiplication failed");
    if (st) st->msm = clock.lap();
    rc = count ? be.g_sum(terms.us.data(), terms.inits.data(), count, k, gs) : 0;
    if (rc) return verify_fail(error, rc, "verify_proofs: the sum over g failed");
    if (st) st->pairing = clock.lap();
    *accept = ipa_sums_cancel(fq, fresh, gs) ? 1 : 0;
    return 0;
}

// The KZG pairing check of two sums L | R (affine): *accept = 1 iff  e(L, s_g2) e(-R, g2) = 1
// L | R -> L | -R ((0, 0) stays the identity)
inline void kzg_negate_right(const VerifierKey& vk, const uint64_t lr[16], uint64_t sums[16]) {
    memcpy(sums, lr, 128);
    Fe ry;
    memcpy(ry.v, sums + 12, 32);
    ry = vk.fq->neg(ry);
    memcpy(sums + 12, ry.v, 32);
}
// In device mode: `count` pairs L_i | R_i, each its own check in ONE launch of the backend; accept[i] = 1 iff the status is DEHALO_PAIRING_ONE (a sum off the
// curve is a rejection, as on the host)
inline int kzg_pairings_device(const VerifierKey& vk, VerifyBackend& be, const uint64_t* lr, uint32_t count, uint8_t* accept, std::string* error) {
    std::vector<uint64_t> sums(16 * (size_t)count);
    for (uint32_t i = 0; i < count; i++) kzg_negate_right(vk, lr + 16 * (size_t)i, sums.data() + 16 * (size_t)i);
    const int rc = be.pairing_checks(sums.data(), count, accept);
    if (rc) return verify_fail(error, rc, "verify_proofs: the pairing checks on the device failed");
    for (uint32_t i = 0; i < count; i++) accept[i] = accept[i] == DEHALO_PAIRING_ONE ? 1 : 0;
    return 0;
}
inline int kzg_pairing(const VerifierKey& vk, VerifyBackend& be, const uint64_t lr[16], int* accept, std::string* error) {
    if (vk.pairing == DEHALO_PAIRING_ON_DEVICE) {
        uint8_t ok = 0;
        const int rc = kzg_pairings_device(vk, be, lr, 1, &ok, error);
        if (rc) return rc;
        *accept = ok;
        return 0;
    }
    uint64_t sums[16];
    kzg_negate_right(vk, lr, sums);
    uint8_t g2s[256];
    memcpy(g2s, vk.s_g2, 128);
    memcpy(g2s + 128, vk.g2, 128);
    const PairingHost* ph = pairing_host(vk.curve);
    if (!ph) return verify_fail(error, DEHALO_ERR_UNSUPPORTED, "verify_proofs: no pairing on this curve");
    // (g2 and s_g2 passed the constructor's checks, a proof's points the decoder's: a sum off the curve can only come from a key's commitment that was read
    // unchecked and is no point.  Nothing such a key verifies is valid: the proof is rejected, the call is not in error.)
    int is_one = 0;
    const int rc = ph->check(sums, g2s, 2, &is_one, /* g2_subgroup_known */ true);
    if (rc == DEHALO_ERR_INVALID) is_one = 0;
    else if (rc) return verify_fail(error, rc, "verify_proofs: the pairing check failed");
    *accept = is_one ? 1 : 0;
    return 0;
}

// The KZG acceptance: the two sums, then the pairing check
inline int decide_kzg(const VerifierKey& vk, VerifyBackend& be, const VerifyTerms& terms, int* accept, VerifyStats& st, std::string* error) {
    VerifyClock clock;
    uint64_t sums[16] = {};      // L | R
    if (!terms.ls.empty()) {
        int rc = be.msm(terms.ls.data(), terms.lp.data(), terms.ls.size(), sums);
        if (!rc) rc = be.msm(terms.rs.data(), terms.rp.data(), terms.rs.size(), sums + 8);
        if (rc) return verify_fail(error, rc, "verify_proofs: the multi-scalar multiplication failed");
    }
    st.msm = clock.lap();
    const int rc = kzg_pairing(vk, be, sums, accept, error);
    if (rc) return rc;
    st.pairing = clock.lap();
    return 0;
}

// `in` as verify_check_arguments left it, with its weights: out.accept = 1 iff every proof is readable and  e(sum_i w_i L_i, s_g2) e(-sum_i w_i R_i, g2) = 1  (IPA:
// decide_ipa's identity).  Returns 0 whenever the check ran; DEHALO_ERR_INVALID without weights or the backend's error, and `out` is then as it was made.
inline int verify_proofs_host(const VerifierKey& vk, VerifyBackend& be, const VerifyInput& in, VerifyVerdict& out, std::string* error) {
    if (in.count && !in.weights) return verify_fail(error, DEHALO_ERR_INVALID, "verify_proofs: null argument");
    VerifyVerdict v;
    VerifyStaged sg;
    int rc = stage_points(vk, be, in, sg, v.stats, error);
    if (!rc) rc = stage_instances(vk, be, in, sg, error);
    if (rc) return rc;
    VerifyClock clock;
    VerifyTerms terms;
    const bool opening_rejected = run_walks(vk, in, sg, terms);
    v.stats.walk = clock.lap();
    for (uint32_t i = 0; i < in.count && v.first_malformed < 0; i++)
        if (sg.malformed[i]) v.first_malformed = i;
    if (v.first_malformed >= 0) v.reason = DEHALO_REJECT_MALFORMED;
    else if (opening_rejected) v.reason = DEHALO_REJECT_OPENING;      // readable, and no proof
    else {
        const bool ipa = vk.scheme == DEHALO_SCHEME_IPA;
        rc = ipa ? decide_ipa(be, terms, in.count, in.plan.k, vk.fq, &v.accept, &v.stats, error) : decide_kzg(vk, be, terms, &v.accept, v.stats, error);
        if (rc) return rc;
        if (!v.accept) v.reason = ipa ? DEHALO_REJECT_OPENING : DEHALO_REJECT_PAIRING;
    }
    out = v;
    return 0;
}

// What dehalo_verify_proofs_each found: reasons[i] = a dehalo_reject_reason, NONE for a valid proof; checks: the subset checks made
struct VerifyEachVerdict { std::vector<int> reasons; uint32_t checks = 0; VerifyStats stats; };

// A verdict per proof from one batch: the staging and the walks of verify_proofs_host; the proofs a walk rejects are named there (MALFORMED, OPENING) and take no
// part in what follows.  ONE msm_segments call of the backend then sums every remaining proof's runs apart -- w_i L_i and w_i R_i (IPA: the weighted fresh sum)
// --, a subset's sums are point additions on the host, and blame_search names the proofs that fail with few checks of subsets: KZG one pairing check on the
// subset's two sums, IPA the subset's fresh sum against the backend's g_sum over the subset's challenges and inits (ipa_sums_cancel).  A proof the search names is
// PAIRING under KZG and OPENING under IPA.  KZG in device mode (vk.pairing): no search -- every live proof's two sums go through ONE pairing_checks call of the
// backend, a check each, and `checks` is the number of live proofs.  Returns 0 whenever the checks ran; DEHALO_ERR_INVALID without weights or the backend's error, and `out` is then as it was.
inline int verify_proofs_each_host(const VerifierKey& vk, VerifyBackend& be, const VerifyInput& in, VerifyEachVerdict& out, std::string* error) {
    if (in.count && !in.weights) return verify_fail(error, DEHALO_ERR_INVALID, "verify_proofs_each: null argument");
    VerifyEachVerdict v;
    VerifyStaged sg;
    int rc = stage_points(vk, be, in, sg, v.stats, error);
    if (!rc) rc = stage_instances(vk, be, in, sg, error);
    if (rc) return rc;
    VerifyClock clock;
    VerifyTerms terms;
    run_walks(vk, in, sg, terms);
    v.stats.walk = clock.lap();
    v.reasons.assign(in.count, DEHALO_REJECT_NONE);
    for (uint32_t i = 0; i < in.count; i++) v.reasons[i] = sg.malformed[i] ? DEHALO_REJECT_MALFORMED : sg.opening[i] ? DEHALO_REJECT_OPENING : DEHALO_REJECT_NONE;
    const bool ipa = vk.scheme == DEHALO_SCHEME_IPA;
    const size_t live = terms.runs.size(), nl = terms.ls.size(), nr = terms.rs.size(), k = in.plan.k;
    if (live) {
        if (nl + nr > DEHALO_MSM_SEGMENTS_MAX_TERMS) return verify_fail(error, DEHALO_ERR_INVALID, "verify_proofs_each: too many terms in one call");
        // one list: every left run, then every right run (IPA has no left list); segment p < live is proof p's left run, live + p its right run
        std::vector<Fe> scalars(terms.ls);
        scalars.insert(scalars.end(), terms.rs.begin(), terms.rs.end());
        std::vector<uint64_t> points(terms.lp);
        points.insert(points.end(), terms.rp.begin(), terms.rp.end());
        std::vector<uint32_t> offsets;
        for (const VerifyTerms::Run& r : terms.runs)
            if (!ipa) offsets.push_back((uint32_t)r.l0);
        for (const VerifyTerms::Run& r : terms.runs) offsets.push_back((uint32_t)(nl + r.r0));
        offsets.push_back((uint32_t)(nl + nr));
        const uint32_t segments = (uint32_t)offsets.size() - 1;
        std::vector<uint64_t> sums(8 * (size_t)segments);
        rc = be.msm_segments(scalars.data(), points.data(), offsets.data(), segments, sums.data());
        if (rc) return verify_fail(error, rc, "verify_proofs_each: the segmented sums failed");
        v.stats.msm = clock.lap();
        const uint64_t* right = sums.data() + (ipa ? 0 : 8 * live);
        const G1Host g1(vk.fq, curve_b_host(vk.curve));
        auto range_sum = [&](const uint64_t* per_proof, size_t first, size_t count, uint64_t out_affine[8]) {
            G1Host::Jac acc = g1.identity();
            for (size_t p = first; p < first + count; p++) {
                Fe x, y;
                memcpy(x.v, per_proof + 8 * p, 32);
                memcpy(y.v, per_proof + 8 * p + 4, 32);
                acc = g1.add_affine(acc, x, y);
            }
            g1.to_affine(acc, out_affine);
        };
        int check_rc = 0;      // an error of a check ends the search: every later check "passes" unasked
        auto check = [&](size_t first, size_t count) -> bool {
            if (check_rc) return true;
            int ok = 0;
            if (ipa) {
                uint64_t fresh[8], gs[8] = {};
                range_sum(right, first, count, fresh);
                check_rc = be.g_sum(terms.us.data() + first * k, terms.inits.data() + first, count, (uint32_t)k, gs);
                if (check_rc) verify_fail(error, check_rc, "verify_proofs_each: the sum over g failed");
                ok = ipa_sums_cancel(vk.fq, fresh, gs);
            } else {
                uint64_t lr[16];
                range_sum(sums.data(), first, count, lr);
                range_sum(right, first, count, lr + 8);
                check_rc = kzg_pairing(vk, be, lr, &ok, error);
            }
            return !check_rc && ok;
        };
        std::vector<uint8_t> bad;
        if (!ipa && vk.pairing == DEHALO_PAIRING_ON_DEVICE) {
            // every live proof's (w_i L_i, -w_i R_i) its own check, all in one launch: no search, and no verdict depends on another proof's weight
            std::vector<uint64_t> lr(16 * live);
            for (size_t p = 0; p < live; p++) {
                memcpy(&lr[16 * p], sums.data() + 8 * p, 64);
                memcpy(&lr[16 * p + 8], right + 8 * p, 64);
            }
            bad.assign(live, 0);
            check_rc = kzg_pairings_device(vk, be, lr.data(), (uint32_t)live, bad.data(), error);
            for (size_t p = 0; p < live; p++) bad[p] = !bad[p];
            v.checks = (uint32_t)live;
        } else v.checks = blame_search(live, check, bad);
        if (check_rc) return check_rc;
        v.stats.pairing = clock.lap();
        for (size_t p = 0; p < live; p++)
            if (bad[p]) v.reasons[terms.runs[p].proof] = ipa ? DEHALO_REJECT_OPENING : DEHALO_REJECT_PAIRING;
    }
    out = std::move(v);
    return 0;
}
