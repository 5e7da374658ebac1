// verify.hip -- verify_proof for KZG behind the C ABI: the verifier object, its two constructors, dehalo_verify_proof / dehalo_verify_proofs.  The protocol is
// verify_host.hpp's (host only); this unit adds the device backend -- every point of a call's proofs through one dehalo_points_decompress_device launch, the two
// term lists through the fresh-bases MSM (dehalo_best_multiexp) -- and the batch weights' draw.  No kernel of its own.  A verifier made without a context uses
// the host backend: a mode the caller chose, never a fallback.
#include <memory>

#include "verify_host.hpp"
#include "whole_call.hpp"

struct dehalo_verifier {
    dehalo_ctx* ctx = nullptr;      // null: the host verifier
    VerifierKey key;
    VerifyStats stats;
    std::string error;
    std::mutex mu;
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
    DeviceVerifyBackend(dehalo_ctx* c, int cv) : ctx(c), curve(cv) {}
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
};

int verifier_fail(dehalo_verifier* v, dehalo_ctx* ctx, int code, const std::string& msg) {
    if (v) v->error = msg;
    return dh_fail(ctx, code, msg);
}

// what both constructors end with
int verifier_finish(dehalo_ctx* ctx, std::unique_ptr<dehalo_verifier>& v, dehalo_verifier** out) {
    const std::string err = v->key.check_g2();
    if (!err.empty()) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create: " + err);
    const OpeningPlan pl(v->key.opening_shape(1));
    if (!pl.error.empty()) return create_fail(ctx, DEHALO_ERR_UNSUPPORTED, "verifier_create: " + pl.error);
    *out = v.release();
    return 0;
}

int verify_body(dehalo_verifier* v, const uint8_t* const* proofs, const size_t* lens, uint32_t count, const uint64_t* const* instances, const size_t* instance_lens,
                uint32_t num_instance_columns, uint32_t num_circuits, dehalo_rng* rng, int* accept, int64_t* first_malformed, int* reason) {
    std::lock_guard<std::mutex> lk(v->mu);
    v->error.clear();
    const HostField* f = v->key.f;
    std::string err;
    {   // the caller's errors first: a call that is refused has drawn nothing from the caller's generator
        const int bad = verify_check_arguments(v->key, proofs, lens, count, instances, instance_lens, num_instance_columns, num_circuits, &err);
        if (bad) return verifier_fail(v, v->ctx, bad, err);
    }
    std::vector<Fe> weights(std::max<uint32_t>(count, 1), f->one);      // w_0 = 1, then the generator's first count - 1 scalars
    if (count > 1) {
        HostRng hr;
        if (hr.init(rng, f) != 0) return verifier_fail(v, v->ctx, DEHALO_ERR_INVALID, "verify_proofs: unusable rng");
        if (hr.scalars((uint64_t*)(weights.data() + 1), count - 1) != 0) return verifier_fail(v, v->ctx, DEHALO_ERR_INVALID, "verify_proofs: the rng callback failed");
        hr.write_back(rng);
    }
    int rc;
    if (v->ctx) {
        std::lock_guard<std::recursive_mutex> hold(v->ctx->mu);
        (void)hipSetDevice(v->ctx->device);
        DeviceVerifyBackend be(v->ctx, v->key.curve);
        rc = verify_proofs_host(v->key, be, proofs, lens, count, instances, instance_lens, num_instance_columns, num_circuits, weights.data(), accept, first_malformed, reason,
                                &v->stats, &err);
    } else {
        HostVerifyBackend be(v->key.fq, v->key.f, 3);
        rc = verify_proofs_host(v->key, be, proofs, lens, count, instances, instance_lens, num_instance_columns, num_circuits, weights.data(), accept, first_malformed, reason,
                                &v->stats, &err);
    }
    if (rc && !err.empty()) {
        v->error = err;
        if (v->ctx && (rc == DEHALO_ERR_INVALID || rc == DEHALO_ERR_UNSUPPORTED)) dh_fail(v->ctx, rc, err);      // (a device error has its own text already)
    }
    return rc;
}

}   // namespace

extern "C" int dehalo_verifier_create(dehalo_ctx* ctx, const dehalo_params* params, const dehalo_pk* pk, dehalo_verifier** out) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !params || !pk || !out) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create: null argument");
        if (params->scheme != DEHALO_SCHEME_KZG || params->curve != DEHALO_CURVE_BN254_G1 || pk->curve != DEHALO_CURVE_BN254_G1)
            return create_fail(ctx, DEHALO_ERR_UNSUPPORTED, "verifier_create: KZG over BN254 only (IPA verification is not part of this library)");
        if (params->k != pk->k) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create: k of the key differs from the params'");
        std::unique_ptr<dehalo_verifier> v(new dehalo_verifier);
        v->ctx = ctx;
        VerifierKey& key = v->key;
        key.curve = pk->curve; key.k = pk->k;
        key.f = pk->f;
        key.fq = host_field(curve_base_field(pk->curve));
        key.cs = pk->cs;
        key.dom = pk->dom;
        key.num_selectors = pk->num_selectors;
        key.fixed_commitments = pk->fixed_commitments;
        key.perm_commitments = pk->perm_commitments;
        key.selectors = pk->selectors;
        key.transcript_repr = pk->transcript_repr;
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
        if (curve != DEHALO_CURVE_BN254_G1) return create_fail(ctx, DEHALO_ERR_UNSUPPORTED, "verifier_create_vk: KZG over BN254 only (IPA verification is not part of this library)");
        std::unique_ptr<dehalo_verifier> v(new dehalo_verifier);
        v->ctx = ctx;
        VerifierKey& key = v->key;
        std::string err = key.init_cs(curve, cs, k);
        if (!err.empty()) return create_fail(ctx, key.unsupported ? DEHALO_ERR_UNSUPPORTED : DEHALO_ERR_INVALID, "verifier_create_vk: " + err);
        err = key.load_vk(vk_bytes, vk_len, vk_format, num_selectors);
        if (!err.empty()) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create_vk: " + err);
        key.default_transcript_repr();
        memcpy(key.g0, g0, 64);
        memcpy(key.g2, g2, 128);
        memcpy(key.s_g2, s_g2, 128);
        const G1Host g1(key.fq, 3);
        Fe x, y;
        memcpy(x.v, g0, 32);
        memcpy(y.v, g0 + 4, 32);
        if (HostField::geq(x.v, key.fq->p) || HostField::geq(y.v, key.fq->p) || !g1.on_curve(x, y)) return create_fail(ctx, DEHALO_ERR_INVALID, "verifier_create_vk: g0 is not a curve point");
        return verifier_finish(ctx, v, out);
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
        std::lock_guard<std::mutex> lk(v->mu);
        v->key.multiopen = multiopen;
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
