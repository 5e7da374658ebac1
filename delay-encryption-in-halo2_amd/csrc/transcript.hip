// transcript.hip -- the C entry points that are about no params, key or proof: the Blake2b transcript (Blake2bWrite / Blake2bRead; the object: transcript_host.hpp),
// the pairing check (pairing_host.hpp), dehalo_field_info and the scalar draws, on the host and by the one kernel here, the ChaCha20 draw [UPSTREAM halo2_proofs
// @ v2023_04_20: transcript.rs] -- through create_proof, the reference's Blake2bWrite transcript at benches/delay_enc.rs:120-134.
// C entry points run under dh_guard, as in prover.hip.
#include <memory>

#include "pairing_host.hpp"
#include "whole_call.hpp"

namespace {

// The ChaCha20 kinds (DEHALO_RNG_OS, DEHALO_RNG_CHACHA20), the vanishing argument's random polynomial (n scalars: 4 MiB at k = 17): generated ON THE DEVICE from
// the proof's ChaCha20 key (32 bytes of operating-system entropy, or the caller's) instead of being drawn on a host thread and uploaded.  Scalar i = the first of
// ChaCha20 blocks (counter low = i, counter high = attempt 0, 1, ...), nonce = the helper's stream, whose first 256 bits masked to the modulus' length are < p
// (chacha_accept, hostrng.hpp): uniform over the field.  The schedule of all draws: include/dehalo.h, dehalo_rng_kind.
// (the block function: chacha_indexed_block, hostrng.hpp, shared with the generator kernel of gfft.cuh)
__global__ void k_chacha_scalars(ChaKey key, u64 stream, fe p, u32 bits, fe* out, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (u32 attempt = 0;; attempt++) {
        fe v;
        chacha_indexed_block(key.k, stream, i, attempt, v.v);
        if (chacha_accept(v.v, p.v, bits)) {
            out[i] = v;
            return;
        }
    }
}

}   // namespace

// the ChaCha20 kinds' indexed draw: key from the proof's generator, modulus and bit length of its field
int chacha_scalars_device(dehalo_ctx* ctx, const HostRng& rng, uint64_t cha_stream, fe* out, size_t n, hipStream_t s) {
    const HostField* f = rng.f;
    ChaKey ck;
    memcpy(ck.k, rng.key, 32);
    fe pw;
    for (int i = 0; i < 4; i++) { pw.v[2 * i] = (u32)f->p[i]; pw.v[2 * i + 1] = (u32)(f->p[i] >> 32); }
    k_chacha_scalars<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(ck, /* stream of the fork */ cha_stream, pw, f->bits, out, n);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ================================================================================================ transcript
extern "C" int dehalo_transcript_create(int curve, dehalo_transcript** out) {
    return dh_guard(nullptr, [&]() -> int {
        if (!out || curve_scalar_field(curve) < 0) return DEHALO_ERR_INVALID;
        dehalo_transcript* t = new dehalo_transcript;
        t->init(curve);
        *out = t;
        return 0;
    });
}
extern "C" int dehalo_transcript_common_scalar(dehalo_transcript* t, const uint64_t s[4]) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || !s) return DEHALO_ERR_INVALID;
        Fe v;
        memcpy(v.v, s, 32);
        t->common_scalar(v);
        return 0;
    });
}
extern "C" int dehalo_transcript_write_scalar(dehalo_transcript* t, const uint64_t s[4]) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || !s || t->reader) return DEHALO_ERR_INVALID;
        Fe v;
        memcpy(v.v, s, 32);
        t->write_scalar(v);
        return 0;
    });
}
extern "C" int dehalo_transcript_write_point(dehalo_transcript* t, const uint64_t xy[8]) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || !xy || t->reader) return DEHALO_ERR_INVALID;
        return t->write_point(xy) ? 0 : DEHALO_ERR_INVALID;
    });
}
extern "C" int dehalo_transcript_squeeze_challenge(dehalo_transcript* t, uint64_t out[4]) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || !out) return DEHALO_ERR_INVALID;
        const Fe c = t->squeeze();
        memcpy(out, c.v, 32);
        return 0;
    });
}
extern "C" size_t dehalo_transcript_len(const dehalo_transcript* t) { return t ? t->proof.size() : 0; }
extern "C" int dehalo_transcript_finalize(const dehalo_transcript* t, uint8_t* out, size_t cap) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || (!out && !t->proof.empty())) return DEHALO_ERR_INVALID;
        if (cap < t->proof.size()) return DEHALO_ERR_INVALID;
        if (!t->proof.empty()) memcpy(out, t->proof.data(), t->proof.size());
        return 0;
    });
}
extern "C" void dehalo_transcript_release(dehalo_transcript* t) { delete t; }

// ---- Blake2bRead: the same object over a proof's bytes (copied: the caller's buffer is not retained)
extern "C" int dehalo_transcript_create_read(int curve, const uint8_t* proof, size_t len, dehalo_transcript** out) {
    return dh_guard(nullptr, [&]() -> int {
        if (!out || (!proof && len) || curve_scalar_field(curve) < 0) return DEHALO_ERR_INVALID;
        std::unique_ptr<dehalo_transcript> t(new dehalo_transcript);
        t->init_read(curve, proof, len);
        *out = t.release();
        return 0;
    });
}
extern "C" int dehalo_transcript_read_point(dehalo_transcript* t, uint64_t affine_xy[8]) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || !affine_xy || !t->reader) return DEHALO_ERR_INVALID;
        uint64_t xy[8];
        if (!t->read_point(xy)) return DEHALO_ERR_INVALID;
        memcpy(affine_xy, xy, 64);
        return 0;
    });
}
extern "C" int dehalo_transcript_read_scalar(dehalo_transcript* t, uint64_t s[4]) {
    return dh_guard(nullptr, [&]() -> int {
        if (!t || !s || !t->reader) return DEHALO_ERR_INVALID;
        Fe v;
        if (!t->read_scalar(v)) return DEHALO_ERR_INVALID;
        memcpy(s, v.v, 32);
        return 0;
    });
}
extern "C" size_t dehalo_transcript_remaining(const dehalo_transcript* t) { return t && t->reader ? t->remaining() : 0; }

// ================================================================================================ the pairing check (pairing_host.hpp; host only)
extern "C" int dehalo_pairing_check(int curve, const uint64_t* g1_affine_xy, const uint8_t* g2_raw, size_t count, int* is_one) {
    return dh_guard(nullptr, [&]() -> int {
        if (curve_scalar_field(curve) < 0 || !is_one || (count && (!g1_affine_xy || !g2_raw))) return DEHALO_ERR_INVALID;
        const PairingHost* ph = pairing_host(curve);
        if (!ph) return DEHALO_ERR_UNSUPPORTED;      // Pallas and Vesta have no pairing
        return ph->check(g1_affine_xy, g2_raw, count, is_one);
    });
}

// ================================================================================================ fields and scalar draws
extern "C" int dehalo_field_info(int field, uint64_t out[24]) {
    return dh_guard(nullptr, [&]() -> int {
        const HostField* f = host_field(field);
        if (!f || !out) return DEHALO_ERR_INVALID;
        memcpy(out, f->p, 32);
        memcpy(out + 4, f->one.v, 32);
        memcpy(out + 8, f->root_of_unity.v, 32);
        memcpy(out + 12, f->zeta.v, 32);
        memcpy(out + 16, f->delta.v, 32);
        memcpy(out + 20, f->gen.v, 32);
        return 0;
    });
}

extern "C" int dehalo_rng_scalars(dehalo_rng* rng, int field, uint64_t skip, uint64_t* out, size_t count) {
    return dh_guard(nullptr, [&]() -> int {
        const HostField* f = host_field(field);
        if (!f || (!out && count)) return DEHALO_ERR_INVALID;
        HostRng r;
        TRY(r.init(rng, f));
        r.skip(skip);
        return r.scalars(out, count);
    });
}

extern "C" int dehalo_rng_scalars_device(dehalo_ctx* ctx, dehalo_rng* rng, int field, uint64_t cha_stream, uint64_t* d_out, size_t n, void* stream) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx) return DEHALO_ERR_INVALID;
        const HostField* f = host_field(field);
        if (!f) return dh_fail(ctx, DEHALO_ERR_INVALID, "rng_scalars_device: unknown field");
        if (!rng || rng->kind != DEHALO_RNG_CHACHA20) return dh_fail(ctx, DEHALO_ERR_INVALID, "rng_scalars_device: needs a keyed ChaCha20 generator (kind 3)");
        if (n >= ((size_t)1 << 29)) return dh_fail(ctx, DEHALO_ERR_INVALID, "rng_scalars_device: too many scalars");
        if (n == 0) return 0;
        if (!d_out) return dh_fail(ctx, DEHALO_ERR_INVALID, "rng_scalars_device: null output");
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        HostRng r;
        TRY(r.init(rng, f));
        return chacha_scalars_device(ctx, r, cha_stream, (fe*)d_out, n, pick_stream(ctx, stream));
    });
}
