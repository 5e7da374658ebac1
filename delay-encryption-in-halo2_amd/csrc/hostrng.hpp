// hostrng.hpp -- sources of the prover's random scalars (blinding rows, blinds, the vanishing argument's random polynomial), the
// `rng: R` argument of create_proof [UPSTREAM halo2_proofs/src/plonk/prover.rs; the reference passes OsRng, benches/delay_enc.rs:128].
//   DEHALO_RNG_OS        the default: 32 bytes of operating-system entropy (getrandom) key a ChaCha20 stream per call; every scalar is
//                        256 stream bits masked to the modulus' bit length and rejected when >= p -- uniform over the field (the blinding
//                        rows on the host; the random polynomial's n scalars by a ChaCha20 KERNEL under the same key, transcript.hip);
//   DEHALO_RNG_PCG64     TESTS / BENCHMARKS ONLY (not a CSPRNG): numpy's PCG64 stream from a given state, four 64-bit outputs per scalar,
//                        top word masked to 61 bits -- the stream dehalo2_amd.prover.SeededRng and the CPU restatement consume, so that
//                        proofs can be compared byte for byte;
//   DEHALO_RNG_CALLBACK  the caller's own generator;
//   DEHALO_RNG_CHACHA20  the DEHALO_RNG_OS generator with the caller's key instead of 32 bytes of operating-system entropy: reproducible, and as
//                        strong as the key.  From the key on the two kinds are ONE path (HostRng::chacha()); the schedule of their draws is written
//                        down in include/dehalo.h (dehalo_rng_kind).
// A scalar is handed over as a Montgomery REPRESENTATION (multiplication by R is a bijection of the field: uniform stays uniform).
#pragma once
#include <sys/random.h>

#include <cstdint>
#include <cstring>

#include "../../include/dehalo.h"
#include "hostfield.hpp"

typedef unsigned __int128 u128;

#ifdef __HIPCC__
#define DH_HOST_DEVICE __host__ __device__
#define DH_UNROLL _Pragma("unroll")
#else
#define DH_HOST_DEVICE
#define DH_UNROLL
#endif

// From 256 candidate bits to a scalar -- the one acceptance step of the ChaCha20 kinds, on the host (HostRng::scalars) and in the kernel
// (k_chacha_scalars, transcript.hip): v = eight 32-bit words, least significant first, is masked to the modulus' `bits` (225 .. 256) and accepted iff
// the masked value is < p.  v holds the masked value afterwards either way.
DH_HOST_DEVICE inline bool chacha_accept(uint32_t v[8], const uint32_t p[8], uint32_t bits) {
    if (bits < 256) v[7] &= ((uint32_t)1 << (bits - 224)) - 1;
    bool below = false, decided = false;
    DH_UNROLL
    for (int j = 7; j >= 0; j--)
        if (!decided && v[j] != p[j]) { below = v[j] < p[j]; decided = true; }
    return below;
}

// The ChaCha20 block function (RFC 8439) over the INDEXED schedule, in the two kernels that draw by index (k_chacha_scalars, transcript.hip; k_points_generate,
// gfft.cuh): state = sigma | key | index mod 2^32 | (index >> 32 & 0xffff) | attempt << 16 | stream, low word first.  v = the block's first eight words
// (its first 32 bytes, little-endian): the others are never formed.
struct ChaKey { uint32_t k[8]; };      // a key as a kernel argument
DH_HOST_DEVICE inline uint32_t chacha_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
DH_HOST_DEVICE inline void chacha_indexed_block(const uint32_t key[8], uint64_t stream, uint64_t index, uint32_t attempt, uint32_t v[8]) {
    const uint32_t st[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7],
                             (uint32_t)index, ((uint32_t)(index >> 32) & 0xffffu) | (attempt << 16), (uint32_t)stream, (uint32_t)(stream >> 32)};
    uint32_t x[16];
    DH_UNROLL
    for (int j = 0; j < 16; j++) x[j] = st[j];
#define CHA_QR(a, b, c, d)                                                                                                 \
    x[a] += x[b]; x[d] = chacha_rotl(x[d] ^ x[a], 16); x[c] += x[d]; x[b] = chacha_rotl(x[b] ^ x[c], 12);                  \
    x[a] += x[b]; x[d] = chacha_rotl(x[d] ^ x[a], 8);  x[c] += x[d]; x[b] = chacha_rotl(x[b] ^ x[c], 7);
    for (int r = 0; r < 10; r++) {
        CHA_QR(0, 4, 8, 12) CHA_QR(1, 5, 9, 13) CHA_QR(2, 6, 10, 14) CHA_QR(3, 7, 11, 15)
        CHA_QR(0, 5, 10, 15) CHA_QR(1, 6, 11, 12) CHA_QR(2, 7, 8, 13) CHA_QR(3, 4, 9, 14)
    }
#undef CHA_QR
    DH_UNROLL
    for (int j = 0; j < 8; j++) v[j] = x[j] + st[j];
}

struct Pcg64 {
    u128 state, inc;
    static u128 mult() { return ((u128)0x2360ED051FC65DA4ULL << 64) | 0x4385DF649FCCF645ULL; }
    uint64_t next() {
        state = state * mult() + inc;
        const uint64_t hi = (uint64_t)(state >> 64), lo = (uint64_t)state;
        const uint64_t x = hi ^ lo;
        const unsigned rot = (unsigned)(hi >> 58);
        return (x >> rot) | (x << ((64 - rot) & 63));
    }
    void advance(u128 delta) {
        u128 acc_mult = 1, acc_plus = 0, cur_mult = mult(), cur_plus = inc;
        while (delta) {
            if (delta & 1) {
                acc_mult *= cur_mult;
                acc_plus = acc_plus * cur_mult + cur_plus;
            }
            cur_plus = (cur_mult + 1) * cur_plus;
            cur_mult *= cur_mult;
            delta >>= 1;
        }
        state = acc_mult * state + acc_plus;
    }
};

struct ChaCha20 {
    uint32_t st[16];
    static uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
    void init(const uint8_t key[32], uint64_t stream) {
        static const uint32_t sigma[4] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
        memcpy(st, sigma, 16);
        memcpy(st + 4, key, 32);
        st[12] = st[13] = 0;                        // 64-bit block counter
        st[14] = (uint32_t)stream;
        st[15] = (uint32_t)(stream >> 32);
    }
    void block(uint32_t out[16]) {
        uint32_t x[16];
        memcpy(x, st, 64);
#define CC_QR(a, b, c, d)                                                                                   \
    x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16); x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12);                 \
    x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8);  x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7);
        for (int i = 0; i < 10; i++) {
            CC_QR(0, 4, 8, 12) CC_QR(1, 5, 9, 13) CC_QR(2, 6, 10, 14) CC_QR(3, 7, 11, 15)
            CC_QR(0, 5, 10, 15) CC_QR(1, 6, 11, 12) CC_QR(2, 7, 8, 13) CC_QR(3, 4, 9, 14)
        }
#undef CC_QR
        for (int i = 0; i < 16; i++) out[i] = x[i] + st[i];
        if (++st[12] == 0) ++st[13];
    }
};

// One proof's generator.  `position` counts scalars in upstream's draw order; fork(skip) gives an independent generator positioned
// `skip` scalars further on (the helper thread's: it draws the random polynomial while the earlier phases run).
struct HostRng {
    int kind = DEHALO_RNG_OS;
    const HostField* f = nullptr;
    Pcg64 pcg{};
    ChaCha20 cc{};
    uint32_t ccbuf[16];
    int ccpos = 16;
    uint8_t key[32];
    dehalo_rng_fill_fn fill_fn = nullptr;
    void* user = nullptr;
    uint64_t position = 0;
    dehalo_rng* caller = nullptr;      // PCG64: the caller's state is advanced when the proof is done

    // the two ChaCha20 kinds: they differ in where init takes `key` from and in nothing else
    bool chacha() const { return kind == DEHALO_RNG_OS || kind == DEHALO_RNG_CHACHA20; }

    int init(const dehalo_rng* r, const HostField* field) {
        f = field;
        kind = r ? r->kind : DEHALO_RNG_OS;
        position = 0;
        if (chacha()) {
            if (kind == DEHALO_RNG_OS) {
                size_t got = 0;
                while (got < 32) {
                    const ssize_t n = getrandom(key + got, 32 - got, 0);
                    if (n <= 0) return DEHALO_ERR_UNSUPPORTED;
                    got += (size_t)n;
                }
            } else {      // the caller's key: pcg_state | pcg_inc as they lie in memory
                memcpy(key, r->pcg_state, 16);
                memcpy(key + 16, r->pcg_inc, 16);
            }
            cc.init(key, 0);
            ccpos = 16;
            return 0;
        }
        if (kind == DEHALO_RNG_PCG64) {
            pcg.state = ((u128)r->pcg_state[1] << 64) | r->pcg_state[0];
            pcg.inc = ((u128)r->pcg_inc[1] << 64) | r->pcg_inc[0];
            return 0;
        }
        if (kind == DEHALO_RNG_CALLBACK && r->fill) {
            fill_fn = r->fill;
            user = r->user;
            return 0;
        }
        return DEHALO_ERR_INVALID;
    }
    HostRng fork(uint64_t skip, uint64_t stream) const {
        HostRng o = *this;
        o.position = position + skip;
        if (kind == DEHALO_RNG_PCG64) o.pcg.advance((u128)4 * skip);
        if (chacha()) {      // an independent ChaCha20 stream under the same key
            o.cc.init(key, stream);
            o.ccpos = 16;
        }
        return o;
    }
    void skip(uint64_t count) {      // (ChaCha20 kinds: only `position` moves -- what is skipped is drawn from another stream, and the serial stream stays where it is)
        position += count;
        if (kind == DEHALO_RNG_PCG64) pcg.advance((u128)4 * count);
    }
    void write_back(dehalo_rng* r) const {      // a PCG64 caller's generator moves past the call's draws (upstream's `&mut rng`); a ChaCha20 key stays as it is
        if (!r || r->kind != DEHALO_RNG_PCG64) return;
        r->pcg_state[0] = (uint64_t)pcg.state;
        r->pcg_state[1] = (uint64_t)(pcg.state >> 64);
    }
    void cc_candidate(uint32_t w[8]) {      // the next eight words of the serial stream: half a block, used or rejected
        if (ccpos >= 16) {
            cc.block(ccbuf);
            ccpos = 0;
        }
        memcpy(w, ccbuf + ccpos, 32);
        ccpos += 8;
    }
    int scalars(uint64_t* out, size_t count) {
        if (kind == DEHALO_RNG_PCG64) {
            for (size_t i = 0; i < count; i++) {
                for (int j = 0; j < 4; j++) out[4 * i + j] = pcg.next();
                out[4 * i + 3] &= ((uint64_t)1 << 61) - 1;
            }
        } else if (chacha()) {
            uint32_t pw[8], w[8];
            for (int j = 0; j < 4; j++) { pw[2 * j] = (uint32_t)f->p[j]; pw[2 * j + 1] = (uint32_t)(f->p[j] >> 32); }
            for (size_t i = 0; i < count; i++) {
                do cc_candidate(w);
                while (!chacha_accept(w, pw, f->bits));
                for (int j = 0; j < 4; j++) out[4 * i + j] = (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32);
            }
        } else {
            const int rc = fill_fn(user, out, count, position);
            if (rc != 0) return DEHALO_ERR_INVALID;
        }
        position += count;
        return 0;
    }
};
