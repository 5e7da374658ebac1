// whole_call.hpp -- what the units of the whole call share (host only): params.hip (ParamsKZG / ParamsIPA), transcript.hip (the Blake2b transcript, the scalar
// draws), ipa_open.hip (the IPA opening argument), keygen.hip (keygen_vk / keygen_pk, the key formats) and prover.hip (create_proof).  The objects behind the C ABI's opaque handles
// [UPSTREAM halo2_proofs @ v2023_04_20: poly/kzg/commitment.rs ParamsKZG, poly/ipa/commitment.rs ParamsIPA, transcript.rs Blake2bWrite, plonk.rs
// ProvingKey / VerifyingKey] and the few functions one unit calls in another.  Everything else of a unit stays in its anonymous namespace.
#pragma once
#include "blake2b.hpp"
#include "hostrng.hpp"
#include "internal.hpp"
#include "plonk_host.hpp"
#include "transcript_host.hpp"      // dehalo_transcript: Blake2bWrite / Blake2bRead (C entry points: transcript.hip)

// ================================================================================================ ParamsKZG / ParamsIPA (params.hip)
struct dehalo_params {
    dehalo_ctx* ctx = nullptr;
    int curve = 0;
    uint32_t k = 0;
    size_t n = 0;
    std::vector<uint64_t> g, g_lagrange;      // host copies (write())
    uint8_t g2[128] = {}, s_g2[128] = {};
    BasesPtr bases_g, bases_gl;
    int scheme = DEHALO_SCHEME_KZG;
    // ParamsIPA only: g as plain affine points followed by u, w (n + 2 points, standard Montgomery): the generator vector the opening collapses
    DevMem d_guw;
    BasesPtr bases_uw;                        // [U | W] plain: the extra bases of round 1, whose G' part runs over bases_g
    FixedBasePtr fb_w;                        // W's window table: the [blind] W of every commit / commit_lagrange (dehalo_fixed_base_blind_device)
    uint64_t u[8] = {}, w[8] = {};
};

// Blind::default() of upstream's poly/commitment.rs, the blind of every commitment that is not hiding: the verifying key's fixed and permutation columns and,
// under IPA, the instance columns.  Taken to be Blind(F::ONE) (no upstream source at hand: parity unpinned).  Keygen and the prover
// read this constant only; the CPU restatement and the verifier of the tests have its twin (DEFAULT_BLIND in the reference prover's ipa.py, which INTEGRATION.md names).
constexpr uint64_t IPA_DEFAULT_BLIND = 1;

// ================================================================================================ keys (keygen.hip, which defines the member functions)
struct dehalo_pk {
    dehalo_ctx* ctx = nullptr;
    int curve = 0;
    const HostField* f = nullptr;
    HostCS cs;
    HostDomain dom;
    uint32_t k = 0, num_selectors = 0;
    std::vector<uint64_t> fixed_commitments, perm_commitments;      // Montgomery affine, 8 u64 each
    std::vector<std::vector<uint8_t>> selectors;                    // packed 8 bools per byte, LSB first
    Fe transcript_repr{};
    // device: values / polys in upstream's standard form, extended-domain columns in the kernels' internal form
    DevMem l_ext, fixed_values, fixed_polys, fixed_cosets, perm_values, perm_polys, perm_cosets;
    GraphPtr custom_gates;
    std::vector<GraphPtr> lookup_graphs;
    std::vector<std::pair<GraphPtr, GraphPtr>> compress_graphs;
    std::vector<std::pair<GraphPtr, GraphPtr>> shuffle_graphs;      // per shuffle: compress(inputs) + gamma, compress(shuffle side) + gamma
    GraphPtr check_gates;      // every gate polynomial as a root of its own (dehalo_check_witness)

    size_t vk_size() const;
    void vk_write(uint8_t* o) const;
    size_t size() const;
    void default_transcript_repr();
    int compile_graphs();
};

// ================================================================================================ functions that cross units
// ipa_open.hip: commitment::create_proof of ParamsIPA on `rng` as it stands, into `t` (dehalo_ipa_open; the last step of a ProverIPA proof)
int ipa_open_body(dehalo_ctx* ctx, const dehalo_params* p, const uint64_t* d_poly, const Fe& blind, const Fe& x3, HostRng& rng, uint64_t cha_stream, dehalo_transcript* t);
// transcript.hip: out[0 .. n) = uniform scalars of rng's field from ChaCha20 stream `cha_stream` under rng's key (rng.chacha()), one kernel launch on `s`
int chacha_scalars_device(dehalo_ctx* ctx, const HostRng& rng, uint64_t cha_stream, fe* out, size_t n, hipStream_t s);
// keygen.hip: (n, 4) device column of omega^i
int omega_powers(dehalo_ctx* ctx, const HostDomain& d, fe* col);
