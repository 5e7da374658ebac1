// verify.hip -- verify_proof for KZG and for IPA behind the C ABI: the verifier object, its constructors, dehalo_verify_proof / dehalo_verify_proofs / dehalo_verify_proofs_each, dehalo_ipa_verify.
// The protocol is verify_host.hpp's (host only); this unit adds the device backend -- every point of a call's proofs through one dehalo_points_decompress_device
// launch, the term lists through the fresh-bases MSM (dehalo_best_multiexp), a call's per-proof sums through one dehalo_msm_segments launch; under IPA the instance columns' commitments over the params' Lagrange table and the
// sum over g: dehalo_ipa_s_device (ipa.cuh) into dehalo_msm_device over the params' resident table, the 2^k scalars never leaving the device -- and the batch
// weights' draw.  No kernel of its own.  A verifier made without a context uses the host backend: a mode the caller chose, never a fallback.
#include <memory>

#include "verify_host.hpp"
#include "whole_call.hpp"

struct dehalo_verifier {
    dehalo_ctx* ctx = nullptr;      // null: the host verifier
    const dehalo_params* params = nullptr;      // an IPA verifier with a context: its ParamsIPA, borrowed as a prover borrows them
    std::vector<uint64_t> g, g_lagrange;        // a host IPA verifier: its copies of the 2^k generators and of their Lagrange form
    VerifierKey key;
    VerifyStats stats;
    std::string error;
    std::mutex mu;
    dehalo_pairing_table* pairing_table = nullptr;      // (s_g2, g2) for the device's pairing checks: made when dehalo_verifier_set_pairing first asks for them
    ~dehalo_verifier() { dehalo_pairing_table_release(pairing_table); }
};

namespace {

// why the calling thread's last constructor call failed: a host verifier has no context to keep the text, and a failed constructor no verifier
thread_local std::string t_create_error;
int create_fail(dehalo_ctx* ctx, int code, const std::string& msg) {
    t_create_error = msg;
    return dh_fail(ctx, code, msg);
}

struct DeviceVerifyBackend : VerifyBackend {
    dehalo_ctx* ctx;
    int curve;
    const dehalo_params* params;      // IPA: the tables the two new sums run over; null for KZG
    const dehalo_pairing_table* pairing_table;      // KZG in device mode: the verifier's (s_g2, g2); null otherwise
    DeviceVerifyBackend(dehalo_ctx* c, int cv, const dehalo_params* p = nullptr, const dehalo_pairing_table* t = nullptr) : ctx(c), curve(cv), params(p), pairing_table(t) {}
    // every check in ONE launch (pairing.cuh)
    int pairing_checks(const uint64_t* lr, uint32_t count, uint8_t* status) override {
        if (!pairing_table) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "verify_proofs: no pairing table behind this verifier");
        return dehalo_pairing_checks(pairing_table, lr, count, status, nullptr);
    }
    // (both sums work in the context's grow-only workspace ws_verify: [0] scalars in, [1] points out -- no allocation per call once it has grown)
    int instance_commitments(const Fe* const* cols, const size_t* lens, size_t count, uint64_t* xy) override {
        if (!params) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "verify_proofs: no ParamsIPA behind this verifier");
        size_t len = 1;      // the longest column: the batch's stride (shorter ones are zero from their end on)
        for (size_t i = 0; i < count; i++) len = std::max(len, lens[i]);
        if (len > params->n) return dh_fail(ctx, DEHALO_ERR_INVALID, "verify_proofs: an instance column is longer than the params");
        // ONE MSM for every column of the call; only a call of more than 2^26 instance values (512 columns of 2^17) is split, at what one MSM launch takes
        const size_t per_launch = std::max<size_t>(1, ((size_t)1 << 26) / len);
        const size_t m_max = std::min(count, per_launch);
        TRY(dh_ensure(ctx, ctx->ws_verify[0], 32 * (m_max * len + m_max)));      // columns, then one blind a column
        TRY(dh_ensure(ctx, ctx->ws_verify[1], 32 * 5 * m_max));                   // Jacobian (3 elements a point), then affine (2)
        fe* sc = (fe*)ctx->ws_verify[0].p;
        fe* bl = sc + m_max * len;
        fe* jac = (fe*)ctx->ws_verify[1].p;
        fe* aff = jac + 3 * m_max;
        const std::vector<Fe> blinds(m_max, host_field(curve_scalar_field(curve))->from_u64(IPA_DEFAULT_BLIND));
        TRY(dehalo_upload(ctx, blinds.data(), 32 * m_max, bl));
        for (size_t lo = 0; lo < count; lo += per_launch) {
            const size_t m = std::min(per_launch, count - lo);
            std::vector<Fe> host(m * len, Fe{});
            for (size_t i = 0; i < m; i++) std::copy(cols[lo + i], cols[lo + i] + lens[lo + i], host.begin() + i * len);
            TRY(dehalo_upload(ctx, host.data(), 32 * m * len, sc));
            TRY(dehalo_msm_device(ctx, params->bases_gl.get(), (const uint64_t*)sc, len, m, (uint64_t*)jac, nullptr));
            TRY(dehalo_fixed_base_blind_device(ctx, params->fb_w.get(), (uint64_t*)jac, (const uint64_t*)bl, m, nullptr));
            TRY(dehalo_to_affine_device(ctx, curve, (const uint64_t*)jac, m, (uint64_t*)aff, nullptr));
            TRY(dehalo_download(ctx, aff, 64 * m, xy + 8 * lo));
        }
        return 0;
    }
    int g_sum(const Fe* challenges, const Fe* inits, size_t count, uint32_t k, uint64_t out_affine[8]) override {
        if (!params || params->k != k) return dh_fail(ctx, DEHALO_ERR_UNSUPPORTED, "verify_proofs: no ParamsIPA of this k behind this verifier");
        TRY(dh_ensure(ctx, ctx->ws_verify[0], 32 * (count * (k + 1) + params->n)));      // [count x k challenges | count inits | the 2^k scalars]
        TRY(dh_ensure(ctx, ctx->ws_verify[1], 32 * 5));                                   // the sum: Jacobian (3 elements), then affine (2)
        fe* in = (fe*)ctx->ws_verify[0].p;
        fe* s = in + count * (k + 1);
        fe* pt = (fe*)ctx->ws_verify[1].p;
        TRY(dehalo_upload(ctx, challenges, 32 * count * k, in));
        TRY(dehalo_upload(ctx, inits, 32 * count, in + count * k));
        TRY(dehalo_ipa_s_device(ctx, curve, (const uint64_t*)in, (const uint64_t*)(in + count * k), count, k, (uint64_t*)s, nullptr));
        TRY(dehalo_msm_device(ctx, params->bases_g.get(), (const uint64_t*)s, params->n, 1, (uint64_t*)pt, nullptr));
        TRY(dehalo_to_affine_device(ctx, curve, (const uint64_t*)pt, 1, (uint64_t*)(pt + 3), nullptr));
        return dehalo_download(ctx, pt + 3, 64, out_affine);
    }
    int decompress(const uint8_t* in32, size_t count, uint64_t* xy) override {
        if (count >= ((size_t)1 << 29)) return dh_fail(ctx, DEHALO_ERR_INVALID, "verify_proofs: too many points in one call");
        DevMem in, out;
        TRY(in.alloc(ctx, count, false));
        TRY(out.alloc(ctx, 2 * count, false));
        TRY(dehalo_upload(ctx, in32, 32 * count, in.p));
        uint32_t status = 0;      // the verdict per point is the (0, 0) a refused point is written as
        TRY(dehalo_points_decompress_device(ctx, curve, (const uint8_t*)in.p, count, out.u64(), &status, nullptr));
        return dehalo_download(ctx, out.p, 64 * count, xy);
    }
    int msm(const Fe* scalars, const uint64_t* xy, size_t len, uint64_t out_affine[8]) override {
        uint64_t jac[12];
        TRY(dehalo_best_multiexp(ctx, curve, (const uint64_t*)scalars, xy, len, jac));
        return dehalo_to_affine(ctx, curve, jac, 1, out_affine);
    }
    // every segment in ONE launch (msm_segments.cuh)
    int msm_segments(const Fe* scalars, const uint64_t* xy, const uint32_t* offsets, uint32_t segments, uint64_t* out_affine) override {
        return dehalo_msm_segments(ctx, curve, (const uint64_t*)scalars, xy, offsets, segments, out_affine);
    }
};

int verifier_fail(dehalo_verifier* v, dehalo_ctx* ctx, int code, const std::string& msg) {
    if (v) v->error = msg;
    return dh_fail(ctx, code, msg);
}

// what every constructor ends with
int verifier_finish(dehalo_ctx* ctx, std::unique_ptr<dehalo_verifier>& v, dehalo_verifier** out) {
    const std::string err = v->key.scheme == DEHALO_SCHEME_IPA ? "" : v->key.check_g2();
    if (!err.empty()) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create: " + err);
    const OpeningPlan pl(v->key.opening_shape(1));
    if (!pl.error.empty()) return create_fail(ctx, DEHALO_ERR_UNSUPPORTED, "verifier_create: " + pl.error);
    *out = v.release();
    return 0;
}

// what every verify call does around its work: the caller's errors, the weights' draw, then work(backend, input, error text) on the verifier's backend
template <class Work>
int verify_call(dehalo_verifier* v, const uint8_t* const* proofs, const size_t* lens, uint32_t count, const uint64_t* const* instances, const size_t* instance_lens,
                uint32_t num_instance_columns, uint32_t num_circuits, dehalo_rng* rng, Work&& work) {
    std::lock_guard<std::mutex> lk(v->mu);
    v->error.clear();
    const HostField* f = v->key.f;
    std::string err;
    VerifyInput in{proofs, lens, count, instances, instance_lens, num_instance_columns, num_circuits, nullptr, OpeningPlan()};
    {   // the caller's errors first: a call that is refused has drawn nothing from the caller's generator
        const int bad = verify_check_arguments(v->key, in, &err);
        if (bad) return verifier_fail(v, v->ctx, bad, err);
    }
    std::vector<Fe> weights(std::max<uint32_t>(count, 1), f->one);      // w_0 = 1, then the generator's first count - 1 scalars
    if (count > 1) {
        HostRng hr;
        if (hr.init(rng, f) != 0) return verifier_fail(v, v->ctx, DEHALO_ERR_INVALID, "verify_proofs: unusable rng");
        if (hr.scalars((uint64_t*)(weights.data() + 1), count - 1) != 0) return verifier_fail(v, v->ctx, DEHALO_ERR_INVALID, "verify_proofs: the rng callback failed");
        hr.write_back(rng);
    }
    in.weights = weights.data();
    std::unique_lock<std::recursive_mutex> hold;      // a device verifier's context, for the length of the work
    std::unique_ptr<VerifyBackend> be;
    if (v->ctx) {
        hold = std::unique_lock<std::recursive_mutex>(v->ctx->mu);
        (void)hipSetDevice(v->ctx->device);
        be.reset(new DeviceVerifyBackend(v->ctx, v->key.curve, v->params, v->pairing_table));
    } else {
        std::unique_ptr<HostVerifyBackend> host(new HostVerifyBackend(v->key.fq, v->key.f, curve_b_host(v->key.curve)));
        if (v->key.scheme == DEHALO_SCHEME_IPA) host->set_ipa(v->g.data(), v->g_lagrange.data(), v->key.w, v->key.k);
        be = std::move(host);
    }
    const int rc = work(*be, in, err);
    if (rc && !err.empty()) {
        v->error = err;
        if (v->ctx && (rc == DEHALO_ERR_INVALID || rc == DEHALO_ERR_UNSUPPORTED)) dh_fail(v->ctx, rc, err);      // (a device error has its own text already)
    }
    return rc;
}

// one combined check; the verdict goes to the caller's pointers here and nowhere else
int verify_body(dehalo_verifier* v, const uint8_t* const* proofs, const size_t* lens, uint32_t count, const uint64_t* const* instances, const size_t* instance_lens,
                uint32_t num_instance_columns, uint32_t num_circuits, dehalo_rng* rng, int* accept, int64_t* first_malformed, int* reason) {
    return verify_call(v, proofs, lens, count, instances, instance_lens, num_instance_columns, num_circuits, rng, [&](VerifyBackend& be, const VerifyInput& in, std::string& err) {
        VerifyVerdict verdict;
        verdict.stats = v->stats;      // (a call in error leaves the last call's timings)
        const int rc = verify_proofs_host(v->key, be, in, verdict, &err);
        *accept = verdict.accept;
        if (first_malformed) *first_malformed = verdict.first_malformed;
        if (reason) *reason = verdict.reason;
        v->stats = verdict.stats;
        return rc;
    });
}

// the vk half of a key from the key at hand
void key_from_pk(VerifierKey& key, const dehalo_pk* pk) {
    key.curve = pk->curve; key.k = pk->k;
    key.f = pk->f; key.fq = host_field(curve_base_field(pk->curve));
    key.cs = pk->cs; key.dom = pk->dom;
    key.fixed_commitments = pk->fixed_commitments; key.perm_commitments = pk->perm_commitments;
    key.num_selectors = pk->num_selectors; key.selectors = pk->selectors;
    key.transcript_repr = pk->transcript_repr;
}
// the vk half from the circuit and the vk's bytes; who: the constructor, as its messages name it
int key_from_vk(dehalo_ctx* ctx, const char* who, VerifierKey& key, int scheme, int curve, uint32_t k, const dehalo_constraint_system* cs, const uint8_t* vk_bytes,
                size_t vk_len, int vk_format, uint32_t num_selectors) {
    key.scheme = scheme;
    std::string err = key.init_cs(curve, cs, k);
    if (!err.empty()) return create_fail(ctx, key.unsupported ? DEHALO_ERR_UNSUPPORTED : DEHALO_ERR_INVALID, std::string(who) + ": " + err);
    err = key.load_vk(vk_bytes, vk_len, vk_format, num_selectors);
    if (!err.empty()) return create_fail(ctx, DEHALO_ERR_INVALID, std::string(who) + ": " + err);
    key.default_transcript_repr();
    return 0;
}
// a point of the caller's: both words below the modulus and on the key's curve
bool key_point_ok(const VerifierKey& key, const uint64_t* xy) { return G1Host(key.fq, curve_b_host(key.curve)).check_stored(xy) == 0; }
void ipa_key_points(VerifierKey& key, const uint64_t* g0, const uint64_t* u, const uint64_t* w) {
    memcpy(key.g0, g0, 64);
    memcpy(key.u, u, 64);
    memcpy(key.w, w, 64);
}

}   // namespace

extern "C" int dehalo_verifier_create(dehalo_ctx* ctx, const dehalo_params* params, const dehalo_pk* pk, dehalo_verifier** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !params || !pk || !out) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create: null argument");
        if (params->scheme != DEHALO_SCHEME_KZG || params->curve != DEHALO_CURVE_BN254_G1 || pk->curve != DEHALO_CURVE_BN254_G1)
            return create_fail(ctx, DEHALO_ERR_UNSUPPORTED, "verifier_create: KZG over BN254 only (IPA: dehalo_verifier_create_ipa, _create_ipa_vk, _create_ipa_host)");
        if (params->k != pk->k) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create: k of the key differs from the params'");
        std::unique_ptr<dehalo_verifier> v(new dehalo_verifier);
        v->ctx = ctx;
        VerifierKey& key = v->key;
        key_from_pk(key, pk);
        memcpy(key.g0, params->g.data(), 64);
        memcpy(key.g2, params->g2, 128);
        memcpy(key.s_g2, params->s_g2, 128);
        return verifier_finish(ctx, v, out);
    });
}

extern "C" int dehalo_verifier_create_vk(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t g0[8], const uint8_t g2[128], const uint8_t s_g2[128],
                                         const dehalo_constraint_system* cs, const uint8_t* vk_bytes, size_t vk_len, int vk_format, uint32_t num_selectors, dehalo_verifier** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!g0 || !g2 || !s_g2 || !cs || !vk_bytes || !out) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create_vk: null argument");
        if (curve_scalar_field(curve) < 0) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create_vk: unknown curve");
        if (curve != DEHALO_CURVE_BN254_G1) return create_fail(ctx, DEHALO_ERR_UNSUPPORTED, "verifier_create_vk: KZG over BN254 only (IPA: dehalo_verifier_create_ipa, _create_ipa_vk, _create_ipa_host)");
        std::unique_ptr<dehalo_verifier> v(new dehalo_verifier);
        v->ctx = ctx;
        VerifierKey& key = v->key;
        TRY(key_from_vk(ctx, "verifier_create_vk", key, DEHALO_SCHEME_KZG, curve, k, cs, vk_bytes, vk_len, vk_format, num_selectors));
        memcpy(key.g0, g0, 64);
        memcpy(key.g2, g2, 128);
        memcpy(key.s_g2, s_g2, 128);
        if (!key_point_ok(key, g0)) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create_vk: g0 is not a curve point");
        return verifier_finish(ctx, v, out);
    });
}

// ---- the IPA verifier's constructors
extern "C" int dehalo_verifier_create_ipa(dehalo_ctx* ctx, const dehalo_params* params, const dehalo_pk* pk, dehalo_verifier** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !params || !pk || !out) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create_ipa: null argument");
        if (params->scheme != DEHALO_SCHEME_IPA) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create_ipa: needs ParamsIPA");
        if (params->curve != pk->curve) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create_ipa: the key is over another curve than the params");
        if (params->k != pk->k) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create_ipa: k of the key differs from the params'");
        std::unique_ptr<dehalo_verifier> v(new dehalo_verifier);
        v->ctx = ctx;
        v->params = params;
        VerifierKey& key = v->key;
        key.scheme = DEHALO_SCHEME_IPA;
        key_from_pk(key, pk);
        ipa_key_points(key, params->g.data(), params->u, params->w);
        return verifier_finish(ctx, v, out);
    });
}

extern "C" int dehalo_verifier_create_ipa_vk(dehalo_ctx* ctx, const dehalo_params* params, const dehalo_constraint_system* cs, const uint8_t* vk_bytes, size_t vk_len,
                                             int vk_format, uint32_t num_selectors, dehalo_verifier** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !params || !cs || !vk_bytes || !out) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create_ipa_vk: null argument");
        if (params->scheme != DEHALO_SCHEME_IPA) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create_ipa_vk: needs ParamsIPA");
        std::unique_ptr<dehalo_verifier> v(new dehalo_verifier);
        v->ctx = ctx;
        v->params = params;
        TRY(key_from_vk(ctx, "verifier_create_ipa_vk", v->key, DEHALO_SCHEME_IPA, params->curve, params->k, cs, vk_bytes, vk_len, vk_format, num_selectors));
        ipa_key_points(v->key, params->g.data(), params->u, params->w);
        return verifier_finish(ctx, v, out);
    });
}

extern "C" int dehalo_verifier_create_ipa_host(int curve, uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, const uint64_t w[8], const uint64_t u[8],
                                               const dehalo_constraint_system* cs, const uint8_t* vk_bytes, size_t vk_len, int vk_format, uint32_t num_selectors,
                                               dehalo_verifier** out) {
    return dh_guard(nullptr, [&]() -> int {
        if (!g || !g_lagrange || !w || !u || !cs || !vk_bytes || !out) return create_fail(nullptr, DEHALO_ERR_INVALID, "verifier_create_ipa_host: null argument");
        if (curve_scalar_field(curve) < 0) return create_fail(nullptr, DEHALO_ERR_INVALID, "verifier_create_ipa_host: unknown curve");
        if (curve != DEHALO_CURVE_PALLAS && curve != DEHALO_CURVE_VESTA) return create_fail(nullptr, DEHALO_ERR_UNSUPPORTED, "verifier_create_ipa_host: IPA over Pallas / Vesta only");
        if (k < 1 || k > 28) return create_fail(nullptr, DEHALO_ERR_INVALID, "verifier_create_ipa_host: k out of range");
        std::unique_ptr<dehalo_verifier> v(new dehalo_verifier);
        TRY(key_from_vk(nullptr, "verifier_create_ipa_host", v->key, DEHALO_SCHEME_IPA, curve, k, cs, vk_bytes, vk_len, vk_format, num_selectors));
        const size_t n = (size_t)1 << k;
        v->g.assign(g, g + 8 * n);
        v->g_lagrange.assign(g_lagrange, g_lagrange + 8 * n);
        for (size_t i = 0; i < n; i++)      // (the identity is no generator: the sums would not see its scalar)
            if (!key_point_ok(v->key, &v->g[8 * i]) || !key_point_ok(v->key, &v->g_lagrange[8 * i]))
                return create_fail(nullptr, DEHALO_ERR_INVALID, "verifier_create_ipa_host: g or g_lagrange holds a word that is no curve point");
        if (!key_point_ok(v->key, w) || !key_point_ok(v->key, u)) return create_fail(nullptr, DEHALO_ERR_INVALID, "verifier_create_ipa_host: w or u is not a curve point");
        ipa_key_points(v->key, g, u, w);
        return verifier_finish(nullptr, v, out);
    });
}

// The stand-alone opening check, dehalo_ipa_open's counterpart: the reduction is the whole proof's (ipa_reduce_opening), the sums the device backend's
extern "C" int dehalo_ipa_verify(dehalo_ctx* ctx, const dehalo_params* p, const uint64_t commitment[8], const uint64_t x3_in[4], const uint64_t v_in[4], const uint8_t* proof,
                                 size_t len, int* accept) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !p || !commitment || !x3_in || !v_in || (!proof && len) || !accept) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_verify: null argument");
        if (p->scheme != DEHALO_SCHEME_IPA) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_verify: needs ParamsIPA (dehalo_params_ipa_create)");
        *accept = 0;
        const HostField* f = host_field(curve_scalar_field(p->curve));
        Fe x3, v;
        memcpy(x3.v, x3_in, 32);
        memcpy(v.v, v_in, 32);
        x3 = f->mul(x3, f->one);
        v = f->mul(v, f->one);
        if (g1_affine_is_zero(commitment)) return 0;      // (the identity is no commitment the transcript could have absorbed)
        dehalo_transcript t;
        t.init_read(p->curve, proof, len);
        std::vector<uint64_t> store(8 * (2 * (size_t)p->k + 1));
        size_t next = 0;
        auto point = [&]() -> const uint64_t* {
            uint64_t* dst = store.data() + 8 * next;
            if (8 * next >= store.size() || !t.read_point(dst)) return nullptr;
            next++;
            return dst;
        };
        VerifyTerms terms;
        terms.right(f->one, commitment);
        if (ipa_reduce_opening(f, t, point, p->k, f->one, x3, v, p->g.data(), p->u, p->w, terms) != VERIFY_WALK_OK) return 0;
        std::lock_guard<std::recursive_mutex> hold(ctx->mu);
        (void)hipSetDevice(ctx->device);
        DeviceVerifyBackend be(ctx, p->curve, p);
        return decide_ipa(be, terms, 1, p->k, host_field(curve_base_field(p->curve)), accept);
    });
}

extern "C" int dehalo_verifier_set_transcript_repr(dehalo_verifier* v, const uint64_t repr[4]) {
    return dh_guard(v ? v->ctx : nullptr, [&]() -> int {
        if (!v || !repr) return DEHALO_ERR_INVALID;
        std::lock_guard<std::mutex> lk(v->mu);
        Fe r;
        memcpy(r.v, repr, 32);
        v->key.transcript_repr = v->key.f->mul(r, v->key.f->one);
        return 0;
    });
}
extern "C" int dehalo_verifier_set_multiopen(dehalo_verifier* v, int multiopen) {
    return dh_guard(v ? v->ctx : nullptr, [&]() -> int {
        if (!v || (multiopen != DEHALO_MULTIOPEN_GWC && multiopen != DEHALO_MULTIOPEN_SHPLONK)) return DEHALO_ERR_INVALID;
        if (v->key.scheme == DEHALO_SCHEME_IPA) return verifier_fail(v, v->ctx, DEHALO_ERR_INVALID, "verifier_set_multiopen: an IPA verifier has one multiopen");
        std::lock_guard<std::mutex> lk(v->mu);
        v->key.multiopen = multiopen;
        return 0;
    });
}
extern "C" int dehalo_verifier_set_pairing(dehalo_verifier* v, int mode) {
    return dh_guard(v ? v->ctx : nullptr, [&]() -> int {
        if (!v || (mode != DEHALO_PAIRING_ON_HOST && mode != DEHALO_PAIRING_ON_DEVICE)) return DEHALO_ERR_INVALID;
        std::lock_guard<std::mutex> lk(v->mu);
        if (mode == DEHALO_PAIRING_ON_DEVICE) {
            if (v->key.scheme == DEHALO_SCHEME_IPA) return verifier_fail(v, v->ctx, DEHALO_ERR_INVALID, "verifier_set_pairing: an IPA verifier has no pairing");
            if (!v->ctx) return verifier_fail(v, nullptr, DEHALO_ERR_INVALID, "verifier_set_pairing: a host verifier has no device");
            if (!v->pairing_table) {
                uint8_t g2s[256];
                memcpy(g2s, v->key.s_g2, 128);
                memcpy(g2s + 128, v->key.g2, 128);
                TRY(dehalo_pairing_table_create(v->ctx, v->key.curve, g2s, 2, &v->pairing_table));
            }
        }
        v->key.pairing = mode;
        return 0;
    });
}
extern "C" int dehalo_verifier_release(dehalo_verifier* v) {
    return dh_guard(nullptr, [&]() -> int {
        delete v;
        return 0;
    });
}
extern "C" int dehalo_verifier_create_error(char* out, size_t cap) {
    if (!out || !cap) return DEHALO_ERR_INVALID;
    const size_t n = std::min(cap - 1, t_create_error.size());
    memcpy(out, t_create_error.data(), n);
    out[n] = 0;
    return 0;
}
extern "C" const char* dehalo_verifier_last_error(const dehalo_verifier* v) { return v ? v->error.c_str() : "null verifier"; }
extern "C" int dehalo_verifier_last_timings(const dehalo_verifier* v, double out[4]) {
    if (!v || !out) return DEHALO_ERR_INVALID;
    out[0] = v->stats.decompress; out[1] = v->stats.walk; out[2] = v->stats.msm; out[3] = v->stats.pairing;
    return 0;
}

extern "C" int dehalo_verify_proofs(dehalo_verifier* v, const uint8_t* const* proofs, const size_t* lens, uint32_t count, const uint64_t* const* instances,
                                    const size_t* instance_lens, uint32_t num_instance_columns, uint32_t num_circuits, dehalo_rng* rng, int* accept, int64_t* first_malformed) {
    return dh_guard(v ? v->ctx : nullptr, [&]() -> int {
        if (!v || !accept) return DEHALO_ERR_INVALID;
        return verify_body(v, proofs, lens, count, instances, instance_lens, num_instance_columns, num_circuits, rng, accept, first_malformed, nullptr);
    });
}

// a verdict per proof (verify_host.hpp verify_proofs_each_host); a call in error leaves reasons, checks and the last call's timings as they were
extern "C" int dehalo_verify_proofs_each(dehalo_verifier* v, const uint8_t* const* proofs, const size_t* lens, uint32_t count, const uint64_t* const* instances,
                                         const size_t* instance_lens, uint32_t num_instance_columns, uint32_t num_circuits, dehalo_rng* rng, int* reasons, uint32_t* checks) {
    return dh_guard(v ? v->ctx : nullptr, [&]() -> int {
        if (!v || (!reasons && count)) return DEHALO_ERR_INVALID;
        return verify_call(v, proofs, lens, count, instances, instance_lens, num_instance_columns, num_circuits, rng, [&](VerifyBackend& be, const VerifyInput& in, std::string& err) {
            VerifyEachVerdict verdict;
            const int rc = verify_proofs_each_host(v->key, be, in, verdict, &err);
            if (rc) return rc;
            std::copy(verdict.reasons.begin(), verdict.reasons.end(), reasons);
            if (checks) *checks = verdict.checks;
            v->stats = verdict.stats;
            return 0;
        });
    });
}

// the batch with count = 1: one code path
extern "C" int dehalo_verify_proof(dehalo_verifier* v, const uint64_t* const* instances, const size_t* instance_lens, uint32_t num_instance_columns, uint32_t num_circuits,
                                   const uint8_t* proof, size_t len, int* accept, int* reason) {
    return dh_guard(v ? v->ctx : nullptr, [&]() -> int {
        if (!v || !accept || (!proof && len)) return DEHALO_ERR_INVALID;
        const uint8_t none = 0;
        const uint8_t* one_proof = proof ? proof : &none;
        return verify_body(v, &one_proof, &len, 1, instances, instance_lens, num_instance_columns, num_circuits, nullptr, accept, nullptr, reason);
    });
}
