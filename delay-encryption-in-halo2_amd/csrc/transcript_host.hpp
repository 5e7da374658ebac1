// transcript_host.hpp -- the object behind dehalo_transcript: Blake2bWrite and Blake2bRead over Challenge255 [UPSTREAM halo2_proofs @ v2023_04_20 transcript.rs].
// Host only, no HIP header: whole_call.hpp includes it for the prover, verify_host.hpp for the verifier.  The C entry points are transcript.hip's.
#pragma once
#include <vector>

#include "../../include/dehalo.h"
#include "blake2b.hpp"
#include "g1_host.hpp"      // the one host codec of a G1 point
#include "hostfield.hpp"

// ================================================================================================ transcript (C entry points: transcript.hip)
struct dehalo_transcript {
    int curve = 0;
    const HostField *fq = nullptr, *fr = nullptr;      // base field (coordinates), scalar field (challenges)
    Blake2b state;
    std::vector<uint8_t> proof;

    void init(int c) {
        curve = c;
        fq = host_field(curve_base_field(c));
        fr = host_field(curve_scalar_field(c));
        state.init(64, "Halo2-Transcript");
        proof.clear();
    }
    Fe squeeze() {      // Challenge255: Blake2b-512 over everything absorbed + the prefix byte 0 (which stays absorbed), reduced mod r
        const uint8_t z = 0;
        state.update(&z, 1);
        uint8_t d[64];
        state.digest(d);
        return fr->from_u512(d);
    }
    void common_scalar(const Fe& s) {
        uint8_t b[33];
        b[0] = 2;
        fr->to_bytes(s, b + 1);
        state.update(b, 33);
    }
    void write_scalar(const Fe& s) {
        common_scalar(s);
        uint8_t b[32];
        fr->to_bytes(s, b);
        proof.insert(proof.end(), b, b + 32);
    }
    // affine {x, y} Montgomery; false for the identity (upstream: "cannot write points at infinity to the transcript")
    bool write_point(const uint64_t xy[8], bool also_to_proof = true) {
        Fe x, y;
        memcpy(x.v, xy, 32);
        memcpy(y.v, xy + 4, 32);
        if (x.is_zero() && y.is_zero()) return false;
        uint8_t b[65];
        b[0] = 1;
        fq->to_bytes(x, b + 1);
        fq->to_bytes(y, b + 33);
        state.update(b, 65);
        if (also_to_proof) {
            uint8_t c[32];
            g1_compress_host(fq, xy, c);
            proof.insert(proof.end(), c, c + 32);
        }
        return true;
    }

    // ---- Blake2bRead [UPSTREAM halo2_proofs/src/transcript.rs]: the same hash state over a proof's bytes.  A read that fails leaves `pos` and the state as they were.
    bool reader = false;
    std::vector<uint8_t> input;
    size_t pos = 0;
    void init_read(int c, const uint8_t* bytes, size_t len) {
        init(c);
        reader = true;
        if (len) input.assign(bytes, bytes + len);
        pos = 0;
    }
    size_t remaining() const { return input.size() - pos; }
    // 32 bytes little-endian, refused when not below r
    bool read_scalar(Fe& s) {
        if (remaining() < 32) return false;
        Fe c;
        memcpy(c.v, input.data() + pos, 32);
        if (HostField::geq(c.v, fr->p)) return false;
        s = fr->from_canonical(c);
        pos += 32;
        common_scalar(s);
        return true;
    }
    // GroupEncoding::from_bytes: x little-endian, bit 255 = y is odd.  Refused: x not below p, x^3 + b not a square, the all-zero identity.
    bool read_point(uint64_t xy[8]) {
        if (remaining() < 32) return false;
        uint64_t p[8];
        if (g1_decompress_host(fq, fq->from_u64(curve_b_host(curve)), input.data() + pos, p) != 0) return false;
        if (!write_point(p, false)) return false;      // (0, 0): the identity's all-zero encoding
        memcpy(xy, p, 64);
        pos += 32;
        return true;
    }
};

