/*
 * dehalo.h -- C ABI of the MI355X (gfx950) MSM / NTT prover backend.
 *
 * Drop-in boundary for the hot path of radiusxyz/delay-encryption-in-halo2: the
 * commitments and FFTs that `create_proof` (reference call sites
 * benches/delay_enc.rs:123-131, benches/mod_pow.rs:201-209, benches/pose_enc.rs:127-135;
 * keygen at benches/delay_enc.rs:86,103) performs through the un-vendored dependency
 * halo2_proofs @ tag v2023_04_20 (Cargo.toml:17).  Each entry point names the upstream
 * function a patched halo2_proofs forwards to it (bindings: INTEGRATION.md).
 *
 * Conventions (all entry points):
 *  - plain pointers and sizes only; caller-owned buffers, never retained after return
 *    (except bases handed to dehalo_bases_register, which are COPIED to the device);
 *  - field element  = 4 x u64 little-endian limbs, MONTGOMERY form, R = 2^256: exactly the
 *    in-memory representation of halo2curves' bn256::{Fr,Fq} / pasta::{Fp,Fq};
 *  - affine point   = {x, y} (64 B), identity encoded as x = y = 0;
 *  - projective out = Jacobian {x, y, z} (96 B), identity z = 0.  Any representative of the
 *    class may be returned (as with rayon's thread-count-dependent summation order
 *    upstream); compare after to_affine();
 *  - return 0 on success, a negative dehalo_status otherwise; never aborts, never throws;
 *  - "host" entry points take host pointers and are synchronous; "_device" entry points
 *    take device pointers and a hipStream_t (as void*; NULL = the context's stream) and
 *    are asynchronous on that stream;
 *  - a context is bound to one device and owns one grow-only workspace in HBM that every call on
 *    it uses: entry points may be called from several threads (a mutex serialises them), but
 *    the device work of one context must be ordered -- use the context's own stream, or one
 *    stream of yours per context.  Work that should overlap (independent proofs, columns of
 *    different phases) goes to DIFFERENT contexts; registered bases and compiled graphs may be
 *    shared between contexts of the same device.  There is NO CPU fallback: without a usable
 *    gfx950 device dehalo_ctx_create fails with DEHALO_ERR_NO_DEVICE.
 *
 * Non-canonical words.  halo2curves only ever stores words below the modulus; a C or Rust caller can hand over anything.  The rules hold for every
 * entry point; tests/test_noncanonical_inputs.py pins them on dehalo_field_op, the NTT family and the domain transforms, dehalo_eval_polynomial (host,
 * device, multi, points), dehalo_kate_division (host, batch) and the vanishing quotient, lincomb, scale, batch inversion, the grand and prefix
 * products, product_terms, graph_evaluate and the permutation / lookup / shuffle terms of h, dehalo_permute_expression_pair (host, device, pointer
 * table), dehalo_check_witness, whole proofs (KZG and IPA, advice and instances), every MSM form, best_multiexp, the fixed-base and blinding calls, the
 * generator collapse, registration, points_check and points_compress (dehalo_msm_segments: in tests/test_msm_segments.py).  Without a row of their own -- they read caller words through the kernels and
 * conversions (f29_from_std / f_from_mont) of the rows above, which is an argument from reading, not a test: dehalo_keygen's fixed columns, dehalo_ipa_open, dehalo_convert_form_device and the *_form_device
 * transforms, dehalo_kate_division_device, dehalo_g_to_lagrange_device, the masked evaluation, the batch / deferred / distinct permute forms and the
 * transcript's common_scalar / write_scalar.  dehalo_points_decompress_device refuses an x not below p (status bit 1), as upstream's from_bytes does.
 *  (1) A field element or scalar READ from caller memory, host or device, is any 256-bit word w and stands for w mod p (w mod r for a scalar): every
 *      result is that of the canonical word, and every "is this zero" or "are these equal" decision -- the elements a batch inversion skips, the
 *      denominators of a grand product, the operand of an inversion, a zero scalar, the keys of a lookup (x and x + p are one key), the two cells of a
 *      copy constraint in dehalo_check_witness -- is made mod p.
 *  (2) A field element the library COMPUTES and writes is canonical, below p.  An element a batch inversion leaves alone because it is zero mod p is
 *      written as 0.  The permuted columns of dehalo_permute_expression_pair* are computed (written back from the sorted canonical keys): canonical too.
 *      A transform of ONE element (log_n = 0) is computed like every other size and stores the canonical word.
 *  (3) The entry points that only MOVE bytes copy the caller's words unchanged, canonical or not: dehalo_upload and dehalo_download, and the copies of a
 *      caller's advice and instance columns that dehalo_create_proof* / dehalo_check_witness make before their kernels read them under rule 1.  (The
 *      prover's own gathers and row placements move values the library made, which are canonical by rule 2.)
 *  (4) The coordinates of a point are field elements under rule 1.  The identity is exactly 64 zero bytes and nothing else: a pair that is (0, 0) mod p
 *      without being zero bytes is not on the curve and what an MSM makes of it is undefined.  Registration does not check; dehalo_points_check_device
 *      reports such a pair, and every other coordinate that is not below p, as status bit 1.  dehalo_points_compress_device writes the canonical encoding.
 *  (5) dehalo_bases_register with stride_bytes > 64: the first 64 bytes of each slot are the point, the rest is ignored (see there).
 */
#ifndef DEHALO_H
#define DEHALO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    DEHALO_OK = 0,
    DEHALO_ERR_INVALID = -1,    /* bad argument: null pointer, length mismatch, log_n out of range */
    DEHALO_ERR_NO_DEVICE = -2,  /* no HIP device / wrong architecture */
    DEHALO_ERR_OOM = -3,        /* device allocation failed */
    DEHALO_ERR_HIP = -4,        /* any other HIP runtime error (see dehalo_last_error) */
    DEHALO_ERR_UNSUPPORTED = -5, /* e.g. NTT over a field whose two-adicity is too small */
    DEHALO_ERR_NOT_IN_TABLE = -6, /* permute_expression_pair: upstream's Error::ConstraintSystemFailure */
    DEHALO_ERR_SHUFFLE = -7       /* create_proof: a shuffle argument's two sides are not a permutation of each other (its product does not end at 1) */
} dehalo_status;

/* halo2curves curve / field identities */
typedef enum { DEHALO_CURVE_BN254_G1 = 0, DEHALO_CURVE_PALLAS = 1, DEHALO_CURVE_VESTA = 2 } dehalo_curve;
typedef enum { DEHALO_FIELD_BN254_FR = 0, DEHALO_FIELD_BN254_FQ = 1, DEHALO_FIELD_PASTA_FP = 2, DEHALO_FIELD_PASTA_FQ = 3 } dehalo_field;

typedef struct dehalo_ctx dehalo_ctx;
typedef struct dehalo_bases dehalo_bases;

/* ---- context --------------------------------------------------------------------------- */
int dehalo_ctx_create(int device, dehalo_ctx** out);
/* The same with a stream priority: > 0 the device's highest (a context of short kernels that must not queue behind another context's
 * long ones -- the prover's side context), < 0 its lowest, 0 the default. */
int dehalo_ctx_create_with_priority(int device, int priority, dehalo_ctx** out);
void dehalo_ctx_destroy(dehalo_ctx* ctx);
/* Human-readable text of the last error on this context (a per-thread copy: valid until the calling thread's next call of this function). */
const char* dehalo_last_error(const dehalo_ctx* ctx);
/* Launch-geometry knobs (results never depend on them).  "msm_acc_points" (default 48): the bucket-accumulation grid of an MSM is 4, 6, 8, ... layers of one wave per SIMD,
 * the fewest that leave a lane at most this many points; 0 selects the older rule, whole rounds of "msm_acc_waves" in [1, 4]
 * waves per SIMD (below 4 the kernel leaves wave slots and registers free for the latency-bound kernels of other contexts).
 * "msm_sort_block" (1024, the default, or 512): threads per workgroup of the MSM sort's two scalar-decoding kernels; 512 halves their LDS (64 + 58 KiB instead of
 * 128 + 115 KiB: the histogram packs two 16-bit counters a word) so that they start on a compute unit another context's NTT tile or bucket reduction occupies.
 * "msm_acc_block" (128 or 768): threads per workgroup of the bucket accumulation.  768 = one
 * 12-wave workgroup per compute unit, three waves per SIMD, which leaves a quarter of every SIMD's registers and all of the LDS to the
 * kernels of other contexts that need at most 128 VGPRs (the bucket reduction, the merge, the NTT's half tiles).
 * "ntt_full_table_log" (default 0, in [0, 30]): transforms of up to 2^value points keep all N powers of omega on the device
 * (32 B x N) so that an inter-pass twiddle is one load; larger ones keep N / 2 and negate (measured equal on MI355X).
 * "host_wait_spin_us" (default 400, in [0, 1000000]): a host wait for the context's stream
 * (dehalo_download and the calls built on it: every transcript round trip of a proof) polls for up to this many microseconds before it
 * blocks in the runtime, whose wake-up comes ~15 us after the stream has drained; 0: block at once (no CPU spent waiting). */
int dehalo_ctx_set_tuning(dehalo_ctx* ctx, const char* key, int value);
/* Environment variables.  The library as shipped reads THREE, all host-side diagnostics; none changes which kernels run or with what geometry:
 *   DEHALO_SYNTH_THREADS    host threads dehalo_synthesize writes the RSA regions of a proving call with (default: 8, or the machine's hardware threads if fewer; 1: none)
 *   DEHALO_SYNTH_TRACE      dehalo_synthesize writes the time of its stages to stderr
 *   DEHALO_PROVER_TRACE     dehalo_create_proof writes the host's timeline inside the phases to stderr
 * Tuning is per context and validated: dehalo_ctx_set_tuning above.  The A/B switches of the measurement scripts (tools/ab_*.sh: DEHALO_MSM_BRED_BLOCK, DEHALO_NTT_SKIP,
 * DEHALO_CU_PARTITION, the *_STAMPS phase stamps, ...) exist only in a library built with `make EXPERIMENTS=1` (-DDEHALO_EXPERIMENTS); in the default build their
 * names are not in the binary (tests/test_abi.py counts them). */
/* The context's own stream (a hipStream_t): lets the caller order its own device work (copies, fills) with the library's
 * kernels by enqueueing it on the same stream. */
void* dehalo_ctx_stream(dehalo_ctx* ctx);
/* Blocks until everything queued on the context's own stream has finished. */
int dehalo_ctx_synchronize(dehalo_ctx* ctx);
/* Copies `bytes` from device memory to the host after everything queued on the context's own stream, and waits for it: the read-back
 * of a phase's commitments / evaluations (what Blake2bWrite::write_point needs on the host, halo2_proofs/src/transcript.rs) in one
 * call instead of a synchronize followed by a separate copy. */
int dehalo_download(dehalo_ctx* ctx, const void* d_src, size_t bytes, void* host_dst);
/* Copies `bytes` from CALLER host memory (a `&[F]`, any ordinary pageable allocation) to device memory on the context's own stream and
 * returns once the source has been read in full and the copy has completed: what a host does with a witness column or a polynomial it
 * wants resident (the `Vec<F>` -> HBM step in front of every `*_device` entry point).  Like every host entry point of this library the
 * transfer never leaves the device holding a mapping of caller memory: the bytes pass through the context's page-locked staging chunks
 * (or move by DMA from pages that are page-locked by the caller / for the duration of the call). */
int dehalo_upload(dehalo_ctx* ctx, const void* host_src, size_t bytes, void* d_dst);

/* ---- SRS / bases ------------------------------------------------------------------------
 * Replaces the `g` / `g_lagrange` vectors of ParamsKZG / ParamsIPA
 * [halo2_proofs/src/poly/kzg/commitment.rs, .../ipa/commitment.rs; built at
 * benches/delay_enc.rs:41-54].  Bases are constant per SRS, so they are uploaded once and
 * stay resident in HBM.
 *   affine_xy     n points, `stride_bytes` apart (>= 64; 64 for halo2curves' {x, y} structs).  With stride_bytes > 64 the FIRST 64 bytes of each slot are
 *                 the point {x, y} and the remaining bytes are ignored: a flag byte kept there (an "is identity" marker, say) is not read, and an identity
 *                 must be x = y = 0 like everywhere else.  Coordinates are words under "Non-canonical words" (4) above.
 *   window_bits   0 = choose from n (with precompute = 1: 17 from 2^20 points, 16 at 2^19, 15 from 2^17, 13 below); otherwise the Pippenger window c in [4, 16], or 17 with precompute = 1
 *   precompute    1 = also store [2^(c*w)]P_i for every window w (n * ceil(256/c) * 64 B of
 *                 HBM): all windows then share one bucket set and the per-window doublings
 *                 vanish.  0 = store the n points only.
 * Limits: n < 2^30; with precompute = 1 also n x windows < 2^30 (30-bit table indices in the sorted list; windows = the signed-digit windows of the
 * scalar field at the chosen c, e.g. 15 for BN254 and the Pasta fields at c = 17): the default window admits tables up to n = 2^26.  Beyond: DEHALO_ERR_INVALID.
 */
int dehalo_bases_register(dehalo_ctx* ctx, int curve, const uint64_t* affine_xy, size_t n, size_t stride_bytes,
                          int window_bits, int precompute, dehalo_bases** out);
/* The same for points that are in device memory already (n x {x, y}, 64 bytes apart, standard Montgomery form): an SRS generated on the device
 * (dehalo_params_setup) or left there by the caller.  The points are read before the call returns. */
int dehalo_bases_register_device(dehalo_ctx* ctx, int curve, const uint64_t* d_affine_xy, size_t n, int window_bits, int precompute, dehalo_bases** out);
int dehalo_bases_release(dehalo_ctx* ctx, dehalo_bases* bases);
size_t dehalo_bases_len(const dehalo_bases* bases);
/* The Pippenger window c chosen for these bases, the number of windows ceil(256 / c) and whether their multiples are stored. */
int dehalo_bases_info(const dehalo_bases* bases, uint32_t* window_bits, uint32_t* windows, int* precomputed);

/* ---- MSM == halo2_proofs::arithmetic::best_multiexp(coeffs, bases) -> C::Curve ------------
 * [halo2_proofs/src/arithmetic.rs; reached from ParamsKZG::commit / commit_lagrange].
 * out = sum_{i < len} scalars[i] * bases[i]; len may be smaller than the registered n
 * (a prefix is used, as commit() does).  scalars: len x 4 u64 (Montgomery).
 * out_jacobian: 12 u64.  upstream's `assert_eq!(coeffs.len(), bases.len())` becomes
 * DEHALO_ERR_INVALID when len > registered n.                                              */
int dehalo_msm(dehalo_ctx* ctx, const dehalo_bases* bases, const uint64_t* scalars, size_t len, uint64_t out_jacobian[12]);
/* `batch` independent MSMs over the same bases (one per committed column):
 * scalars[b] points to len x 4 u64; out_jacobian receives batch x 12 u64.                   */
int dehalo_msm_batch(dehalo_ctx* ctx, const dehalo_bases* bases, const uint64_t* const* scalars, size_t len, size_t batch,
                     uint64_t* out_jacobian);
/* Device-resident form: d_scalars = batch x len x 4 u64 contiguous in HBM, d_out = batch x 12 u64 in HBM. */
int dehalo_msm_device(dehalo_ctx* ctx, const dehalo_bases* bases, const uint64_t* d_scalars, size_t len, size_t batch,
                      uint64_t* d_out_jacobian, void* stream);
/* The same MSMs with the results ALSO (d_out_jacobian may be null: only) written as affine points {x, y} (64 B each, identity =
 * (0, 0), standard Montgomery form): what Blake2bWrite::write_point needs after ParamsKZG::commit_lagrange(..).to_affine()
 * [UPSTREAM halo2_proofs/src/plonk/prover.rs: `C::Curve::batch_normalize`] -- normalised by the kernel that finishes the MSM. */
int dehalo_msm_device_affine(dehalo_ctx* ctx, const dehalo_bases* bases, const uint64_t* d_scalars, size_t len, size_t batch, uint64_t* d_out_jacobian,
                             uint64_t* d_out_affine, void* stream);
/* One-shot best_multiexp over bases that are not registered (uploaded, used, dropped). */
int dehalo_best_multiexp(dehalo_ctx* ctx, int curve, const uint64_t* scalars, const uint64_t* affine_xy, size_t len,
                         uint64_t out_jacobian[12]);
/* Many short independent sums in ONE launch (csrc/msm_segments.cuh):
 *     out[s] = sum over offsets[s] <= i < offsets[s + 1] of scalars[i] * points[i],    s < segments.
 * The per-proof sums of dehalo_verify_proofs_each are its use: about 10^2 terms a segment and 10^2 segments a call, where one dehalo_best_multiexp per segment
 * would be launch latency 10^2 times over.  One workgroup per segment, one quad of lanes per term (a 255-step double-and-add), so the call's time is that of its
 * LONGEST segment in steps of 128 terms; for sums of 2^12 terms and more the Pippenger calls above are the right ones.  All three curves.
 *   scalars    offsets[segments] x 4 u64, Montgomery; words under "Non-canonical words" (1): a word stands for its residue mod r, zero is zero mod r
 *   points     offsets[segments] x {x, y} of 64 B, standard Montgomery, (0, 0) the identity, coordinates under "Non-canonical words" (4).  Both arrays are indexed
 *              by the offsets themselves (entries below offsets[0] are not read)
 *   offsets    segments + 1 words that do not decrease; an empty segment (two equal offsets) sums to the identity
 *   out        segments x {x, y}, affine, canonical, (0, 0) for the identity
 * The group law is exact in every case: equal, opposite and identity operands, zero scalars, one point listed several times in a segment.
 * Limits: segments <= DEHALO_MSM_SEGMENTS_MAX (2^24), offsets[segments] <= DEHALO_MSM_SEGMENTS_MAX_TERMS (2^30).  DEHALO_ERR_INVALID beyond them, for offsets that
 * decrease, an unknown curve, and a null argument (scalars and points may be null when no segment has a term; out when segments = 0, which does nothing).
 * The device form reads the offsets back and checks them BEFORE it launches (one small copy and a wait for the stream), so a refused call has written nothing;
 * the kernel is then queued on the stream and the call returns.  The host form uploads, runs and downloads: for tests and small callers. */
#define DEHALO_MSM_SEGMENTS_MAX (1u << 24)
#define DEHALO_MSM_SEGMENTS_MAX_TERMS (1u << 30)
int dehalo_msm_segments_device(dehalo_ctx* ctx, int curve, const uint64_t* d_scalars, const uint64_t* d_affine_xy, const uint32_t* d_offsets, uint32_t segments,
                               uint64_t* d_out_affine, void* stream);
int dehalo_msm_segments(dehalo_ctx* ctx, int curve, const uint64_t* scalars, const uint64_t* affine_xy, const uint32_t* offsets, uint32_t segments, uint64_t* out_affine);
/* G1::to_affine / batch_normalize of MSM outputs: count x 12 u64 -> count x 8 u64 (host buffers). */
int dehalo_to_affine(dehalo_ctx* ctx, int curve, const uint64_t* jacobian, size_t count, uint64_t* affine_xy);
/* Sum of `count` Jacobian points -> one Jacobian point (identity for count == 0): the combine step when ONE large MSM
 * is split by point range over several GPUs: each rank registers its slice of the bases, runs
 * dehalo_msm_device on its slice of the scalars, the 96-byte partial results are all-gathered (RCCL) and summed here.   */
int dehalo_point_sum_device(dehalo_ctx* ctx, int curve, const uint64_t* d_jacobian, size_t count, uint64_t* d_out_jacobian, void* stream);
/* device-pointer form: `count` Jacobian points (96 B each) -> affine (64 B each), asynchronous on the stream */
int dehalo_to_affine_device(dehalo_ctx* ctx, int curve, const uint64_t* d_jacobian, size_t count, uint64_t* d_affine_xy, void* stream);
/* The generator collapse of the IPA opening argument [UPSTREAM halo2_proofs/src/poly/ipa/commitment/prover.rs: parallel_generator_collapse]:
 * out[i] = g[i] + [challenge] g[len / 2 + i] for i < len / 2, affine {x, y} (64 B, identity = (0, 0), standard Montgomery) in and out, device memory;
 * challenge = one scalar (4 x u64 Montgomery).  len even, < 2^31.  d_out_affine_xy may be d_affine_xy itself (upstream collapses in place), and may
 * overlap it in no other way.  Pallas and Vesta only (DEHALO_ERR_UNSUPPORTED otherwise).  Asynchronous on the stream; no workspace. */
int dehalo_generator_collapse_device(dehalo_ctx* ctx, int curve, const uint64_t* d_affine_xy, size_t len, const uint64_t challenge[4], uint64_t* d_out_affine_xy,
                                     void* stream);
/* The scalars over g of the IPA verifier's one multi-scalar multiplication [UPSTREAM halo2_proofs/src/poly/ipa/strategy.rs: GuardIPA::compute_s, summed over the
 * proofs of a batch under their weights]: for `count` proofs, proof i with round challenges d_challenges[i k .. i k + k) (u_1 .. u_k in the transcript's order) and
 * one scalar d_inits[i] (a verifier passes -w_i c_i),
 *     d_out[idx] = sum_i init_i prod_{j < k, bit j of idx set} u_{i, k - j},    idx < 2^k:
 * bit j of the index selects the j-th challenge from the END, as compute_s does.  All three arrays are device memory, scalars of 4 x u64 Montgomery (any word
 * stands for its residue); the output is canonical.  Two launches, about one multiplication per proof and output; the workspace, count x (2^ceil(k / 2) + 2^floor(k / 2))
 * scalars, is the context's.  1 <= k <= 28 (the largest ParamsIPA), 1 <= count < 2^24, else DEHALO_ERR_INVALID.  Pallas and Vesta only (DEHALO_ERR_UNSUPPORTED otherwise).
 * Asynchronous on the stream. */
int dehalo_ipa_s_device(dehalo_ctx* ctx, int curve, const uint64_t* d_challenges, const uint64_t* d_inits, size_t count, uint32_t k, uint64_t* d_out, void* stream);
/* The blinding term of ParamsIPA::commit / commit_lagrange [UPSTREAM halo2_proofs/src/poly/ipa/commitment.rs: MSM(poly, g) + [blind] W] for the results of
 * one batched MSM: d_jacobian[i] <- d_jacobian[i] + [d_blinds[i]] W for i < count, in place.  Points as dehalo_msm_device leaves them (Jacobian, 96 B,
 * z = 0: the identity), blinds one scalar per point (4 x u64 Montgomery), W one affine point {x, y} (64 B, standard Montgomery): all device memory.
 * One launch for the whole batch, queued behind the MSM on the stream: no host wait between the two.  An identity point gives [b] W, a zero blind
 * leaves the point as it is.  count < 2^29.  Pallas and Vesta only (DEHALO_ERR_UNSUPPORTED otherwise).  Asynchronous on the stream; no workspace. */
int dehalo_blind_commitments_device(dehalo_ctx* ctx, int curve, uint64_t* d_jacobian, const uint64_t* d_blinds, size_t count, const uint64_t* d_w_affine_xy,
                                    void* stream);

/* ---- fixed-base scalar multiplication -----------------------------------------------------
 * [s] P for ONE point P and many scalars, over a window table of P that stays resident: T[w][d] = [d 2^(8 w)] P, 32 byte-windows x 256 entries
 * (512 KB of HBM), so that a multiplication is a sum of at most 32 table entries and no doubling.  One wave per scalar, six dependent group additions:
 * the form for a few dozen scalars at a time (a proof phase's blinds), where the length of the dependent chain is the cost.  All three curves.
 * ParamsIPA keeps such a table of W (every commit / commit_lagrange adds [blind] W); dehalo_blind_commitments_device above is the table-free form. */
typedef struct dehalo_fixed_base dehalo_fixed_base;
/* The table of P = affine_xy ({x, y}, 64 B, standard Montgomery, host memory; (0, 0), the identity, is legal: every product is then the identity).
 * Built on the device (2 launches, about 250 dependent doublings) before the call returns. */
int dehalo_fixed_base_create(dehalo_ctx* ctx, int curve, const uint64_t affine_xy[8], dehalo_fixed_base** out);
int dehalo_fixed_base_release(dehalo_ctx* ctx, dehalo_fixed_base* fb);
/* d_out_affine_xy[i] = [d_scalars[i]] P for i < count: affine {x, y} (64 B, (0, 0) for the identity, standard Montgomery), scalars 4 x u64 Montgomery,
 * both device memory.  count < 2^29; count = 0 returns 0 with the other pointers null.  A null `fb` is DEHALO_ERR_INVALID at every count (the curve comes
 * from the table), here and in dehalo_fixed_base_blind_device.  Asynchronous on the stream; no workspace. */
int dehalo_fixed_base_mul_device(dehalo_ctx* ctx, const dehalo_fixed_base* fb, const uint64_t* d_scalars, size_t count, uint64_t* d_out_affine_xy, void* stream);
/* d_jacobian[i] <- d_jacobian[i] + [d_blinds[i]] P for i < count, in place: the contract of dehalo_blind_commitments_device (Jacobian, 96 B, as
 * dehalo_msm_device leaves it, z = 0: the identity; one launch queued behind the MSM on the stream) with the table in place of W.  count < 2^29.
 * Asynchronous on the stream; no workspace. */
int dehalo_fixed_base_blind_device(dehalo_ctx* ctx, const dehalo_fixed_base* fb, uint64_t* d_jacobian, const uint64_t* d_blinds, size_t count, void* stream);

/* g_to_lagrange [UPSTREAM halo2_proofs/src/poly/commitment.rs, poly/ipa/commitment.rs: best_fft(&mut g, omega_inv, k); g[i] *= n_inv; batch_normalize]:
 * out[i] = [n^-1] sum_j [omega^(-i j)] g[j] over n = 2^k points, omega the 2^k-th root of unity of the curve's scalar field -- the group FFT that takes a
 * commitment key to its Lagrange basis.  Affine {x, y} (64 B, identity = (0, 0), standard Montgomery) in and out, device memory; the output is the
 * canonical affine point, whatever the order of evaluation.  All three curves; 0 <= k <= 28 (k = 0: the output is the input).  d_out_affine_xy may be
 * d_g_affine_xy itself (in place) or disjoint from it; any partial overlap is DEHALO_ERR_INVALID.  About k 2^(k-1) + 2^k variable-base scalar
 * multiplications, k + 2 launches.  Asynchronous on the stream; workspace: 32 B x 2^(k-1) of twiddles, kept by the context. */
int dehalo_g_to_lagrange_device(dehalo_ctx* ctx, int curve, const uint64_t* d_g_affine_xy, uint32_t k, uint64_t* d_out_affine_xy, void* stream);

/* The point codec: vectors of points between their in-memory form (affine {x, y}, 64 B, standard Montgomery, (0, 0) = the identity; 16-byte aligned) and the
 * two forms they take on disk [UPSTREAM halo2curves 0.3.x GroupEncoding, SerdeObject::from_raw_bytes; restated from memory: INTEGRATION.md section 7].  Streaming
 * maps, one lane per point, device memory in and out, all three curves (an unknown curve is DEHALO_ERR_INVALID); count < 2^29, and count = 0 returns 0 without a
 * launch (status 0).  The 32-byte encodings are 4-byte aligned.  Asynchronous on the stream except for a status word's download; no workspace beyond that word.
 *   compress    GroupEncoding::to_bytes: x little-endian canonical, bit 255 = y is odd, (0, 0) -> 32 zero bytes.
 *   decompress  GroupEncoding::from_bytes: y = sqrt(x^3 + b) with the encoded parity.  *status_out (host) collects, over all points, 1 = an x not below the
 *               modulus, 2 = an x that is not on the curve, 4 = x = 0 with the sign bit set (x = 0 belongs to the identity, whose only encoding is
 *               all zero).  A point that raises a bit is written as (0, 0); the call still returns 0: the status is the verdict.
 *   check       what a checked from_raw_bytes does per point; reads only.  *status_out collects 1 = a coordinate whose stored Montgomery word is not below the
 *               modulus, 2 = a point that is neither on y^2 = x^3 + b nor (0, 0). */
int dehalo_points_compress_device(dehalo_ctx* ctx, int curve, const uint64_t* d_affine_xy, size_t count, uint8_t* d_out32, void* stream);
int dehalo_points_decompress_device(dehalo_ctx* ctx, int curve, const uint8_t* d_in32, size_t count, uint64_t* d_affine_xy, uint32_t* status_out, void* stream);
int dehalo_points_check_device(dehalo_ctx* ctx, int curve, const uint64_t* d_affine_xy, size_t count, uint32_t* status_out, void* stream);

/* Generated points: curve points with no known relation between them, derived by a public rule -- what a caller without a ParamsIPA file builds its
 * generators from (dehalo_params_ipa_generate).  They are NOT upstream's ParamsIPA::new generators (hash-to-curve: see dehalo_params_ipa_create).
 * THE RULE.  A point is named by (curve, key, stream, index), index < 2^48.
 *   Block       For attempt = 0, 1, ... the ChaCha20 block (RFC 8439 block function) over the state
 *                   sigma | key | w12 = index mod 2^32 | w13 = (index >> 32 & 0xffff) | attempt << 16 | w14 | w15 = stream, low word first
 *               -- the indexed schedule of the prover's device draws (dehalo_rng_kind, INDEXED).
 *   Candidate   The block's first 32 bytes, read as a GroupEncoding: x = the little-endian integer of the low 255 bits, s = bit 255.
 *   Acceptance  The candidate is accepted iff 0 < x < p (p the curve's base-field modulus) and x^3 + b is a non-zero square; the point is (x, y) with y the root
 *               whose canonical value has parity s.  That is: the first candidate that dehalo_points_decompress_device's rules decode to a point other than
 *               the identity.  The result is uniform over the curve's affine points with x != 0.
 *   Attempt cap Attempts stop at DEHALO_GENERATORS_MAX_ATTEMPTS = 256.  The cap is not part of the mathematics: it bounds the kernel's loop, so that a defect in
 *               the acceptance test cannot spin a wave.  For Pasta (3/4)^256 is about 1e-32.  An index that exhausts the cap is written as (0, 0) and the
 *               call fails with DEHALO_ERR_INVALID and a message.
 *   Key         32 bytes from the caller; NULL selects DEHALO_GENERATORS_DEFAULT_KEY, the 30 ASCII bytes "dehalo ParamsIPA generators v1" followed by two
 *               zero bytes.
 *   ParamsIPA   g[i] = (stream 0, index i); W = (stream 1, index 0); U = (stream 1, index 1).  So g at k is a prefix of g at k' > k, and W, U do not depend
 *               on k, as upstream's do not.
 * What is claimed: nobody knows a relation between the points, provided ChaCha20 under a public key behaves as a random function of (stream, index, attempt) --
 * the usual nothing-up-my-sleeve argument.  Every input is public, so nothing here runs in constant time.
 * dehalo_points_generate_device: d_affine_xy[i] = the point (curve, key, chacha_stream, first_index + i), i < count: affine {x, y} (64 B, standard Montgomery,
 * canonical words, 16-byte aligned: the point codec's layout), device memory.  All three curves.  Asynchronous on the stream except for the download of a status
 * word; no workspace beyond that word.  count = 0 returns 0 without a launch.  DEHALO_ERR_INVALID: a null context or output, an unknown curve, count >= 2^29,
 * first_index + count > 2^48. */
#define DEHALO_GENERATORS_DEFAULT_KEY "dehalo ParamsIPA generators v1\0"
#define DEHALO_GENERATORS_MAX_ATTEMPTS 256
int dehalo_points_generate_device(dehalo_ctx* ctx, int curve, const uint8_t* key32, uint64_t chacha_stream, uint64_t first_index, uint64_t* d_affine_xy, size_t count,
                                  void* stream);

/* The scalar codec, the point codec's twin: vectors of field elements between their in-memory form (4 x u64 Montgomery limbs, 16-byte aligned) and the two forms
 * they take in a key on disk [UPSTREAM halo2curves 0.3.x PrimeField::from_repr, SerdeObject::from_raw_bytes; restated from memory: INTEGRATION.md section 7].
 * Streaming maps, one lane per element, device memory in and out, every field id (an unknown field is DEHALO_ERR_INVALID); count < 2^29, and count = 0 returns 0
 * without a launch, with status 0 and first_bad 0.  Asynchronous on the stream except for the download of the two result words; no workspace beyond them.
 *   from_repr  `count` 32-byte little-endian integers (4-byte aligned) -> Montgomery words.  *status_out (host) collects 1 = an element not below the modulus;
 *              such an element is written as 0 and the call still returns 0: the status is the verdict.  *first_bad_out (host) = the lowest offending index,
 *              `count` if there is none.  d_out may be d_in32 itself (in place) and may overlap it in no other way (DEHALO_ERR_INVALID).
 *   check      what a checked from_raw_bytes does per element; reads only.  Status 1 = a stored Montgomery word not below the modulus; first_bad as above.
 * The other direction, to_repr, is dehalo_field_op_device op 5. */
int dehalo_scalars_from_repr_device(dehalo_ctx* ctx, int field, const uint8_t* d_in32, size_t count, uint64_t* d_out, uint32_t* status_out, uint64_t* first_bad_out,
                                    void* stream);
int dehalo_scalars_check_device(dehalo_ctx* ctx, int field, const uint64_t* d_words, size_t count, uint32_t* status_out, uint64_t* first_bad_out, void* stream);

/* ---- NTT == halo2_proofs::arithmetic::best_fft(a, omega, log_n) ---------------------------
 * [halo2_proofs/src/arithmetic.rs].  In place, natural order in and out,
 * a'[i] = sum_j a[j] * omega^(i*j), no scaling.  a: 2^log_n x 4 u64.  omega must be a
 * primitive 2^log_n-th root of unity (forward or inverse), Montgomery form.
 * upstream's `assert_eq!(a.len(), 1 << log_n)` is the caller's contract here.              */
int dehalo_ntt(dehalo_ctx* ctx, int field, uint64_t* a, uint32_t log_n, const uint64_t omega[4]);
int dehalo_ntt_device(dehalo_ctx* ctx, int field, uint64_t* d_a, uint32_t log_n, const uint64_t omega[4], size_t batch,
                      void* stream);

/* ---- EvaluationDomain conveniences [halo2_proofs/src/poly/domain.rs] ----------------------
 * lagrange_to_coeff:  best_fft(a, omega_inv, k); a[i] *= n_inv                              */
int dehalo_intt_scaled(dehalo_ctx* ctx, int field, uint64_t* a, uint32_t log_n, const uint64_t omega_inv[4], const uint64_t n_inv[4]);
/* coeff_to_extended:  ext[i] = coeffs[i] * [1, zeta, zeta^2][i % 3] for i < 2^log_n, zero
 * above; best_fft(ext, omega_ext, log_ext).  coeffs and ext_out may not alias.              */
int dehalo_coset_ntt(dehalo_ctx* ctx, int field, const uint64_t* coeffs, uint32_t log_n, uint64_t* ext_out, uint32_t log_ext,
                     const uint64_t omega_ext[4], const uint64_t zeta[4]);
/* extended_to_coeff:  best_fft(a, omega_ext_inv, log_ext); a[i] *= ext_n_inv * [1, zeta^2, zeta][i % 3].
 * (The caller truncates to n * quotient_poly_degree, as upstream does.)                     */
int dehalo_coset_intt(dehalo_ctx* ctx, int field, uint64_t* a, uint32_t log_ext, const uint64_t omega_ext_inv[4],
                      const uint64_t ext_n_inv[4], const uint64_t zeta[4]);
/* Device-resident forms (batch polynomials contiguous in HBM). */
int dehalo_intt_scaled_device(dehalo_ctx* ctx, int field, uint64_t* d_a, uint32_t log_n, const uint64_t omega_inv[4],
                              const uint64_t n_inv[4], size_t batch, void* stream);
/* The same out of place: d_coeffs = lagrange_to_coeff(d_values) for `batch` contiguous columns; d_values is left as it is (the prover keeps the
 * Lagrange values it has committed to and needs the coefficients beside them).  d_coeffs == d_values is allowed. */
int dehalo_lagrange_to_coeff_device(dehalo_ctx* ctx, int field, const uint64_t* d_values, uint64_t* d_coeffs, uint32_t log_n, const uint64_t omega_inv[4],
                                    const uint64_t n_inv[4], size_t batch, void* stream);
int dehalo_coset_ntt_device(dehalo_ctx* ctx, int field, const uint64_t* d_coeffs, uint32_t log_n, uint64_t* d_ext_out,
                            uint32_t log_ext, const uint64_t omega_ext[4], const uint64_t zeta[4], size_t batch, void* stream);
int dehalo_coset_intt_device(dehalo_ctx* ctx, int field, uint64_t* d_a, uint32_t log_ext, const uint64_t omega_ext_inv[4],
                             const uint64_t ext_n_inv[4], const uint64_t zeta[4], size_t batch, void* stream);

/* ---- element-wise field ops (halo2curves Fr/Fq/Fp::{add,sub,mul,invert,to_repr,from_repr})
 * Used by the parity tests to pin the device field arithmetic directly (e.g. against the
 * reference's Poseidon known-answer vectors).  Host buffers, n elements each.
 * op: 0 add, 1 sub, 2 mul, 3 invert, 4 canonical->Montgomery, 5 Montgomery->canonical,
 *     6 mul evaluated through the kernels' internal carry-free 29-bit-limb representation.
 * Operands are words under "Non-canonical words" (1): the outputs are canonical whatever multiples of p the operands carry, and the inverse of a word
 * that is zero mod p is 0.                                                                      */
int dehalo_field_op(dehalo_ctx* ctx, int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* device-pointer form (d_b may be NULL for the unary ops; d_out may alias d_a): e.g. canonical -> Montgomery of a column uploaded as raw integers */
int dehalo_field_op_device(dehalo_ctx* ctx, int field, int op, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, size_t n, void* stream);

/* ---- field-vector primitives around the path ---------------------------
 * Everything create_proof does between two commitments that is a scan over a column of field
 * elements, so that columns can stay in HBM from one MSM / NTT to the next.  Elements are
 * upstream's in-memory form (4 x u64 Montgomery limbs, canonical).
 *
 * dehalo_eval_polynomial: out = sum_i coeffs[i] * point^i; 0 for len == 0.  Replaces
 *   halo2_proofs::arithmetic::eval_polynomial (halo2_proofs/src/arithmetic.rs @ v2023_04_20;
 *   called for every opened polynomial in plonk/prover.rs after the challenge x is squeezed).
 *   The device form evaluates `batch` polynomials (stride_elems apart) at the same point into
 *   d_out[batch][4].
 * dehalo_batch_invert: values[i] <- values[i]^-1 in place, zero elements left zero -- zero mod p: an element stored as p or another multiple of p is
 *   skipped like a stored 0 and written back as 0 ("Non-canonical words" (1), (2) at the top; the other elements are inverted all the same).  Replaces
 *   ff::BatchInvert::batch_invert as used on the denominators of the permutation and lookup
 *   grand products (plonk/permutation/prover.rs, plonk/lookup/prover.rs).
 * dehalo_prefix_product_device: out[0] = 1, out[i] = in[0] * ... * in[i-1]  (in == out allowed).
 * dehalo_grand_product: z[0] = 1, z[i] = prod_{j<i} num[j] / den[j] -- the running product
 *   upstream builds after its batch_invert ("z.push(one); for row in 1..n { tmp *= product[row-1] }");
 *   the caller appends upstream's blinding rows.  A zero denominator behaves like upstream's
 *   batch_invert (left zero), so the product is zero from that row on; "zero" is zero mod p ("Non-canonical words" (1)).   */
/* dehalo_permute_expression_pair: the lookup argument's permuted columns, replacing
 *   plonk/lookup/prover.rs permute_expression_pair: permuted_input = the `usable_rows` input values
 *   sorted ascending by canonical value; permuted_table[row] = permuted_input[row] at every first
 *   occurrence, the table's remaining values (ascending) in the repeated rows taken from the end.
 *   Only the table is sorted (merge sort on the 256-bit keys); every input value finds its table position by binary search and the
 *   outputs are written from the position counts (csrc/lookup_permute.hip).
 *   Keys are compared mod p and both outputs are canonical words ("Non-canonical words" (1), (2)): not the caller's words moved.
 *   DEHALO_ERR_NOT_IN_TABLE when an input value does not occur in the table.  The caller appends
 *   upstream's random blinding rows.  The device form synchronises its stream (it has to return
 *   that error).                                                                                 */
int dehalo_permute_expression_pair(dehalo_ctx* ctx, int field, const uint64_t* input, const uint64_t* table, size_t usable_rows,
                                   uint64_t* permuted_input, uint64_t* permuted_table);
int dehalo_permute_expression_pair_device(dehalo_ctx* ctx, int field, const uint64_t* d_input, const uint64_t* d_table, size_t usable_rows,
                                          uint64_t* d_permuted_input, uint64_t* d_permuted_table, void* stream);
/* `batch` lookup arguments in one call (a proof's five): column y of each of the four arrays starts y * stride_elems elements in.
 * All key columns share the sort passes, so the cost barely grows with the batch.                                                */
int dehalo_permute_expression_pair_batch_device(dehalo_ctx* ctx, int field, const uint64_t* d_inputs, const uint64_t* d_tables, size_t usable_rows, size_t batch,
                                                size_t stride_elems, uint64_t* d_permuted_inputs, uint64_t* d_permuted_tables, void* stream);
/* The same with the columns given as HOST arrays of DEVICE pointers.  Lookups whose table pointers are EQUAL share one table sort (the five
 * range lookups of the reference's circuit compress the same (tag, value) table expressions: one sort per proof instead of five). */
int dehalo_permute_expression_pair_ptrs_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_inputs, const uint64_t* const* d_tables, size_t usable_rows, size_t batch,
                                               uint64_t* const* d_permuted_inputs, uint64_t* const* d_permuted_tables, void* stream);
/* The same without the synchronisation: d_status (DEVICE, `batch` int32) receives one flag per lookup -- non-zero: an input value is not in the table, the call
 * above would have returned DEHALO_ERR_NOT_IN_TABLE -- for the caller to read back with whatever it reads next (the prover: with the permuted columns' commitments),
 * so that the stream runs from the permutation straight into the commitment. */
int dehalo_permute_expression_pair_ptrs_deferred_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_inputs, const uint64_t* const* d_tables, size_t usable_rows,
                                                        size_t batch, uint64_t* const* d_permuted_inputs, uint64_t* const* d_permuted_tables, int32_t* d_status, void* stream);
/* The same for tables of FIXED columns (every table expression of the lookup reads fixed columns only -- the reference circuit's range tables): which rows of such
 * a table are equal does not depend on theta, only the order of the compressed values does.  Per lookup y the caller passes one representative row (an index
 * < usable_rows) of every distinct table tuple and how many of the usable rows hold that tuple (DEVICE arrays of distinct_count[y] uint32 each; the multiplicities add
 * up to usable_rows -- otherwise the outputs are unspecified, never an out-of-bounds access; lookups that share a table pass the same arrays).  Then only the distinct compressed values are sorted -- 339 instead of 131,066 for the
 * delay-encryption circuit at k = 17 -- and the sorted table is written out from (value, multiplicity): the same A' and S'.  distinct_count[y] == 0 or > 2048 for any
 * lookup of the call: the general path.  d_status as above, or null: the call synchronises and returns DEHALO_ERR_NOT_IN_TABLE itself. */
int dehalo_permute_expression_pair_distinct_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_inputs, const uint64_t* const* d_tables, size_t usable_rows, size_t batch,
                                                   uint64_t* const* d_permuted_inputs, uint64_t* const* d_permuted_tables, const uint32_t* const* d_rep_rows,
                                                   const uint32_t* const* d_multiplicities, const uint32_t* distinct_count, int32_t* d_status, void* stream);
int dehalo_eval_polynomial(dehalo_ctx* ctx, int field, const uint64_t* coeffs, size_t len, const uint64_t point[4], uint64_t out[4]);
int dehalo_eval_polynomial_device(dehalo_ctx* ctx, int field, const uint64_t* d_coeffs, size_t len, size_t stride_elems, size_t batch,
                                  const uint64_t point[4], uint64_t* d_out, void* stream);
/* `count` polynomials (d_polys: HOST array of DEVICE pointers, len coefficients each) at 1..4 points in one pass over the coefficients
 * (create_proof opens its columns at x, omega x, omega^-1 x and omega^last x): points = num_points x 4 u64 (host),
 * d_out[point][polynomial][4]. */
int dehalo_eval_polynomial_multi_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_polys, size_t count, size_t len, const uint64_t* points,
                                        uint32_t num_points, uint64_t* d_out, void* stream);
/* The same for a caller that needs only some (polynomial, point) pairs: wanted[j] (host, one byte per polynomial; NULL = everything) has bit i set when polynomial j
 * is wanted at point i.  The other entries of d_out are written as zero and cost nothing (a proof asks for about 60 of its 47 x 4 values). */
int dehalo_eval_polynomial_multi_masked_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_polys, size_t count, size_t len, const uint64_t* points,
                                               uint32_t num_points, const uint8_t* wanted, uint64_t* d_out, void* stream);
/* Any set of rotations a circuit queries: 1..32 points, wanted[j] (host, one 32-bit mask per polynomial; NULL = everything) with bit i set when polynomial j is
 * wanted at point i.  d_out[point][polynomial][4], the pairs nobody wants written as zero.  Every polynomial's coefficients are read once however many points
 * its mask holds (a block keeps its tile in registers and takes the points four at a time).  DEHALO_ERR_INVALID for 0 or more than 32 points. */
int dehalo_eval_polynomial_points_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_polys, size_t count, size_t len, const uint64_t* points,
                                         uint32_t num_points, const uint32_t* wanted, uint64_t* d_out, void* stream);
int dehalo_batch_invert(dehalo_ctx* ctx, int field, uint64_t* values, size_t len);
int dehalo_batch_invert_device(dehalo_ctx* ctx, int field, uint64_t* d_values, size_t len, void* stream);
int dehalo_prefix_product_device(dehalo_ctx* ctx, int field, const uint64_t* d_in, size_t len, uint64_t* d_out, void* stream);
int dehalo_grand_product(dehalo_ctx* ctx, int field, const uint64_t* num, const uint64_t* den, size_t len, uint64_t* z);
int dehalo_grand_product_device(dehalo_ctx* ctx, int field, const uint64_t* d_num, const uint64_t* d_den, size_t len, uint64_t* d_z, void* stream);
/* `batch` columns, stride_elems apart in num, den and z alike: the denominators of the whole batch share one inversion
 * (a proof's 2 permutation + 5 lookup products are one call).                                                            */
int dehalo_grand_product_batch_device(dehalo_ctx* ctx, int field, const uint64_t* d_num, const uint64_t* d_den, size_t len, size_t batch,
                                      size_t stride_elems, uint64_t* d_z, void* stream);

/* ---- the remaining element-wise steps of create_proof (so that a proof's columns never leave HBM) ----------
 * dehalo_lincomb_device: out[i] = sum_j coefs[j] * cols[j][i]; sub_const (may be NULL) is subtracted from out[0].
 *   d_cols = HOST array of `count` DEVICE column pointers (len elements each), coefs = host, count x 4 u64.
 *   Replaces the polynomial folds of plonk/prover.rs / vanishing::Constructed::evaluate (h pieces with x^n) and
 *   poly/kzg/multiopen/gwc/prover.rs ("poly_batch = sum v^i poly_i; poly_batch - eval_batch").  out may alias no column.
 * dehalo_scale_device: a[i] *= pattern[i mod period] (host pattern, period in {0 (none), 1, 2, 4, 8}) and, if
 *   d_factor != NULL, *= *d_factor (one element in DEVICE memory).  Replaces EvaluationDomain::divide_by_vanishing_poly
 *   (poly/domain.rs: t_evaluations has 2^(extended_k - k) entries) and the "z = vec![last_z]" carry between the
 *   permutation argument's product columns (plonk/permutation/prover.rs).
 * dehalo_kate_division: q = (a(X) - a(point)) / (X - point), len - 1 coefficients; replaces
 *   halo2_proofs::arithmetic::kate_division (called once per opening point by ProverGWC::create_proof).          */
int dehalo_lincomb_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_cols, const uint64_t* coefs, size_t count, size_t len, uint64_t* d_out,
                          const uint64_t* sub_const, void* stream);
int dehalo_scale_device(dehalo_ctx* ctx, int field, uint64_t* d_a, size_t len, const uint64_t* pattern, uint32_t period, const uint64_t* d_factor, void* stream);
int dehalo_kate_division(dehalo_ctx* ctx, int field, const uint64_t* a, size_t len, const uint64_t point[4], uint64_t* q);
int dehalo_kate_division_device(dehalo_ctx* ctx, int field, const uint64_t* d_a, size_t len, const uint64_t point[4], uint64_t* d_q, void* stream);
/* up to 8 divisions of equal length (<= 2^22 coefficients) in one set of launches: d_a / d_q = HOST arrays of DEVICE pointers,
 * points = count x 4 u64 (ProverGWC::create_proof: one division per distinct opening point) */
int dehalo_kate_division_batch_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_a, size_t len, const uint64_t* points, uint64_t* const* d_q,
                                      size_t count, void* stream);
/* Division by a point set's vanishing polynomial: d_q[y] = d_a[y] div prod_t (X - points[y][t]), the remainder dropped, for up to 8 polynomials of `len`
 * (<= 2^22) coefficients, polynomial y with its own 1 <= num_points[y] <= 32 DISTINCT points (points = HOST array of host pointers, num_points[y] x 4 u64
 * each; d_a / d_q = HOST arrays of DEVICE pointers, no d_q[y] equal to d_a[y]).  d_q[y] receives all `len` coefficients: the top num_points[y] are written as
 * zero, so a buffer of 2^k coefficients can go to a commitment as it is.  One pass over d_a[y] by partial fractions -- sum_t w_t kate_division(a, z_t) with
 * w_t = 1 / prod_{s != t} (z_t - z_s), the weights computed on the host -- not num_points[y] dependent divisions (ProverSHPLONK::create_proof: one quotient
 * per rotation set).  DEHALO_ERR_INVALID, before anything is launched, for count > 8, a null pointer, no or more than 32 points, or two equal points in a set. */
int dehalo_vanishing_quotient_batch_device(dehalo_ctx* ctx, int field, const uint64_t* const* d_a, size_t len, const uint64_t* const* points,
                                           const uint32_t* num_points, uint64_t* const* d_q, size_t count, void* stream);

/* ---- quotient numerator: evaluate_h --------------------------------------
 * The row loops of halo2_proofs/src/plonk/evaluation.rs @ v2023_04_20 on device-resident
 * extended-domain columns (each `rows = 1 << log_rows` elements, standard Montgomery form), so the
 * cosets produced by dehalo_coset_ntt_device never leave HBM before dehalo_coset_intt_device.
 *
 * A dehalo_graph is upstream's GraphEvaluator { constants, rotations, calculations,
 * num_intermediates } handed over verbatim: ValueSource -> dehalo_source (kind, index, rotation
 * = index into rotations[]), Calculation -> dehalo_calculation (Horner(start, parts, factor):
 * a = start, b = factor, parts = horner_parts[parts_begin .. parts_begin + parts_len]),
 * CalculationInfo.target -> target.  dehalo_graph_evaluate_device computes, for every row idx,
 *   out[idx] = GraphEvaluator::evaluate(.., previous_value = previous[idx] (0 if NULL), idx, rot_scale, isize = rows)
 * i.e. the value of the LAST calculation (0 for an empty graph); a column source reads
 * column[(idx + rotations[rotation] * rot_scale) mod rows].  previous == out is allowed (custom
 * gates: values[idx] = evaluate(.., values[idx], ..)).
 *
 * dehalo_permutation_h_device / dehalo_lookup_h_device fold upstream's hard-coded argument terms
 * into `values` in place (value = value * y + term, in upstream's order):
 *   permutation: l0 (1 - z_0); l_last (z_last^2 - z_last); for sets s >= 1: l0 (z_s - z_{s-1}(w^last X));
 *                for every set: l_active (z_s(wX) prod_j (col_j + beta sigma_j + gamma)
 *                                         - z_s(X) prod_j (col_j + delta^j beta X + gamma)),
 *                X = zeta * extended_omega^idx, delta^j running across the sets' column chunks;
 *   lookup:      l0 (1 - z); l_last (z^2 - z); l_active (z(wX)(a' + beta)(s' + gamma) - z(X) table_value);
 *                l0 (a' - s'); l_active (a' - s')(a' - a'(w^-1 X)),
 *                table_value = the lookup's GraphEvaluator output for the row.                    */
/* Optional device-internal element form.  Every `_device` entry point above takes and returns
 * upstream's standard form; converting it costs the evaluate_h kernels one multiplication per
 * column load.  Columns that only travel between this library's kernels can stay in the kernels'
 * own form instead (x * 2^261 mod p, canonical, 32 B -- opaque to the caller):
 *   dehalo_convert_form_device             standard <-> internal, element-wise (proving-key columns, once);
 *   dehalo_coset_ntt_form_device           coeff_to_extended emitting the internal form (DEHALO_FORM_OUT_INTERNAL);
 *   dehalo_coset_intt_form_device          extended_to_coeff consuming it (DEHALO_FORM_IN_INTERNAL);
 *   form_flags of the three *_inputs structs below: DEHALO_EVAL_COLUMNS_INTERNAL (every column pointer of the
 *   struct), DEHALO_EVAL_VALUES_INTERNAL (d_previous / d_out / d_values / table_value).              */
enum { DEHALO_FORM_OUT_INTERNAL = 1, DEHALO_FORM_IN_INTERNAL = 2 };
enum { DEHALO_EVAL_COLUMNS_INTERNAL = 1, DEHALO_EVAL_VALUES_INTERNAL = 2 };
int dehalo_convert_form_device(dehalo_ctx* ctx, int field, const uint64_t* d_in, uint64_t* d_out, size_t n, int to_internal, void* stream);
int dehalo_coset_ntt_form_device(dehalo_ctx* ctx, int field, const uint64_t* d_coeffs, uint32_t log_n, uint64_t* d_ext_out, uint32_t log_ext,
                                 const uint64_t omega_ext[4], const uint64_t zeta[4], size_t batch, uint32_t form_flags, void* stream);
int dehalo_coset_intt_form_device(dehalo_ctx* ctx, int field, uint64_t* d_a, uint32_t log_ext, const uint64_t omega_ext_inv[4],
                                  const uint64_t ext_n_inv[4], const uint64_t zeta[4], size_t batch, uint32_t form_flags, void* stream);

typedef enum {
    DEHALO_SRC_CONSTANT = 0, DEHALO_SRC_INTERMEDIATE = 1, DEHALO_SRC_FIXED = 2, DEHALO_SRC_ADVICE = 3, DEHALO_SRC_INSTANCE = 4,
    DEHALO_SRC_CHALLENGE = 5, DEHALO_SRC_BETA = 6, DEHALO_SRC_GAMMA = 7, DEHALO_SRC_THETA = 8, DEHALO_SRC_Y = 9, DEHALO_SRC_PREVIOUS = 10
} dehalo_source_kind;
typedef struct { uint32_t kind, index, rotation; } dehalo_source;
typedef enum {
    DEHALO_CALC_ADD = 0, DEHALO_CALC_SUB = 1, DEHALO_CALC_MUL = 2, DEHALO_CALC_SQUARE = 3, DEHALO_CALC_DOUBLE = 4, DEHALO_CALC_NEGATE = 5,
    DEHALO_CALC_HORNER = 6, DEHALO_CALC_STORE = 7
} dehalo_calc_op;
typedef struct {
    uint32_t op;
    dehalo_source a, b;
    uint32_t parts_begin, parts_len;
    uint32_t target;
} dehalo_calculation;
typedef struct dehalo_graph dehalo_graph;
int dehalo_graph_create(dehalo_ctx* ctx, int field, const uint64_t* constants, uint32_t num_constants, const int32_t* rotations, uint32_t num_rotations,
                        const dehalo_calculation* calcs, uint32_t num_calcs, const dehalo_source* horner_parts, uint32_t num_horner_parts,
                        uint32_t num_intermediates, dehalo_graph** out);
int dehalo_graph_release(dehalo_ctx* ctx, dehalo_graph* graph);
typedef struct {
    const uint64_t* const* fixed; uint32_t num_fixed;        /* host arrays of DEVICE column pointers */
    const uint64_t* const* advice; uint32_t num_advice;
    const uint64_t* const* instance; uint32_t num_instance;
    const uint64_t* challenges; uint32_t num_challenges;     /* host, 4 u64 each */
    const uint64_t *beta, *gamma, *theta, *y;                /* host, 4 u64 each; NULL = 0 */
    uint32_t form_flags;                                     /* 0, or DEHALO_EVAL_* */
} dehalo_eval_inputs;
int dehalo_graph_evaluate_device(dehalo_ctx* ctx, const dehalo_graph* graph, const dehalo_eval_inputs* in, uint32_t log_rows, uint32_t rot_scale,
                                 const uint64_t* d_previous, uint64_t* d_out, void* stream);
/* `count` programs over the SAME inputs (no previous value), program i into d_outs[i]: the theta-compressed input and table expressions
 * of every lookup [UPSTREAM plonk/lookup/prover.rs commit_permuted: compress_expressions], one call from the host instead of `count`. */
int dehalo_graph_evaluate_batch_device(dehalo_ctx* ctx, const dehalo_graph* const* graphs, uint32_t count, const dehalo_eval_inputs* in, uint32_t log_rows,
                                       uint32_t rot_scale, uint64_t* const* d_outs, void* stream);
typedef struct {
    const uint64_t* const* z; uint32_t num_sets;             /* permutation_product_coset per set (device pointers) */
    const uint64_t* const* columns; const uint64_t* const* sigma; uint32_t num_columns;   /* column cosets / pk.permutation.cosets */
    uint32_t chunk_len;                                      /* cs.degree() - 2 */
    int32_t last_rotation;                                   /* -(blinding_factors + 1) */
    const uint64_t *l0, *l_last, *l_active_row;              /* device */
    const uint64_t *beta, *gamma, *y, *delta, *beta_zeta, *extended_omega;   /* host, 4 u64 each */
    uint32_t form_flags;                                     /* 0, or DEHALO_EVAL_* */
} dehalo_perm_inputs;
int dehalo_permutation_h_device(dehalo_ctx* ctx, int field, const dehalo_perm_inputs* in, uint32_t log_rows, uint32_t rot_scale, uint64_t* d_values,
                                void* stream);
typedef struct {
    const uint64_t *product_coset, *permuted_input_coset, *permuted_table_coset, *table_value;   /* device */
    const uint64_t *l0, *l_last, *l_active_row;              /* device */
    const uint64_t *beta, *gamma, *y;                        /* host */
    uint32_t form_flags;                                     /* 0, or DEHALO_EVAL_*; table_value counts as a value */
} dehalo_lookup_inputs;
int dehalo_lookup_h_device(dehalo_ctx* ctx, int field, const dehalo_lookup_inputs* in, uint32_t log_rows, uint32_t rot_scale, uint64_t* d_values,
                           void* stream);
/* The same terms for `count` <= 8 lookups (in[0], in[1], ... in upstream's order: evaluate_h's `for lookup in lookups` loop) in ONE pass
 * over the rows: d_values and the three Lagrange columns are read once instead of once per lookup.  The lookups of one call share
 * l0 / l_last / l_active_row, beta / gamma / y and form_flags (checked); each brings its own cosets and table_value column. */
int dehalo_lookup_h_batch_device(dehalo_ctx* ctx, int field, const dehalo_lookup_inputs* in, uint32_t count, uint32_t log_rows, uint32_t rot_scale,
                                 uint64_t* d_values, void* stream);

/* The shuffle argument's terms for `count` <= 8 shuffles (in[0], in[1], ... in the constraint system's order) in ONE pass over the rows, folded into d_values
 * in place (value = value * y + term):
 *   l0 (1 - z); l_last (z^2 - z); l_active (z(wX) shuffle_value - z(X) input_value),
 * input_value = compressed input + gamma and shuffle_value = compressed shuffle side + gamma: the outputs of the shuffle's two GraphEvaluator programs for the
 * row.  d_values and the three Lagrange columns are read once; each shuffle reads z[row], z[row + rot_scale] and its two value columns.  The shuffles of one
 * call share l0 / l_last / l_active_row, y and form_flags (checked).  form_flags: product_coset and the Lagrange columns are columns, input_value /
 * shuffle_value and d_values are values. */
typedef struct {
    const uint64_t *product_coset, *input_value, *shuffle_value;   /* device */
    const uint64_t *l0, *l_last, *l_active_row;                    /* device */
    const uint64_t* y;                                             /* host */
    uint32_t form_flags;                                           /* 0, or DEHALO_EVAL_* */
} dehalo_shuffle_inputs;
int dehalo_shuffle_h_batch_device(dehalo_ctx* ctx, int field, const dehalo_shuffle_inputs* in, uint32_t count, uint32_t log_rows, uint32_t rot_scale,
                                  uint64_t* d_values, void* stream);

/* ==== the whole call: halo2_proofs::plonk::{keygen_vk, keygen_pk, create_proof} over KZG / GWC =====================================
 * The reference's timed call is
 *     create_proof::<KZGCommitmentScheme<Bn256>, ProverGWC<_>, Challenge255<_>, _, Blake2bWrite<_, _, _>, _>(&params, &pk, &[circuit],
 *                                                                                                          &[&[&[]]], &mut OsRng, &mut transcript)
 * (benches/delay_enc.rs:123-131, mod_pow.rs:201-209, pose_enc.rs:127-135) over objects it builds once and caches on disk (params
 * :41-54, vk / pk :84-115).  The entry points below are that call and those objects, one C function each: every column stays in HBM
 * from the witness upload to the last opening; the host hashes the transcript (Blake2b-512) and orders the phases, in C++.
 * What arrives from the caller is what halo2 holds at that point: the constraint system as data, the fixed columns and the permutation
 * assembly keygen produced, the advice columns `synthesize` filled (witness generation stays the front-end's).
 */
typedef struct dehalo_params dehalo_params;         /* ParamsKZG<E>: k, g, g_lagrange (resident MSM tables), g2, s_g2; or ParamsIPA<C>: k, g, g_lagrange, w, u */
typedef struct dehalo_pk dehalo_pk;                 /* ProvingKey<C> incl. its VerifyingKey and the compiled GraphEvaluator programs */
typedef struct dehalo_prover dehalo_prover;         /* device buffers of ONE proof in flight (reused by every create_proof on it) */
typedef struct dehalo_transcript dehalo_transcript; /* Blake2bWrite<Vec<u8>, C, Challenge255<C>>, or Blake2bRead over a proof's bytes (dehalo_transcript_create_read) */

/* ParamsKZG [UPSTREAM halo2_proofs/src/poly/kzg/commitment.rs].  g / g_lagrange: 2^k affine points each ({x, y} Montgomery, 64 B);
 * g2 / s_g2: 128 raw bytes each (kept for write() and for a verifier made from these params, dehalo_verifier_create, whose pairing check reads them; the prover never uses them).  read / write: SerdeFormat::RawBytes --
 * k: u32 LE | g | g_lagrange | g2 | s_g2  (what benches/delay_enc.rs:45,54 write and read). */
int dehalo_params_create(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, const uint8_t* g2, const uint8_t* s_g2,
                         dehalo_params** out);
/* ParamsKZG::setup(k, rng) with the rng's draw handed over: `s` is the toxic waste as a Montgomery scalar (what `<E::Scalar>::random(rng)` returns).  g[i] = [s^i] G
 * and g_lagrange[i] = [L_i(s)] G are made on the device (fixed-base table multiplication, one batch inversion), g2 / s_g2 on the host: the reference's
 * `ParamsKZG::<Bn256>::setup(K, OsRng)` (benches/delay_enc.rs:43).  BN254 only (a KZG SRS needs the pairing); k <= 25 (checked before any device work: k = 26, whose two tables
 * would take 128 GB, is DEHALO_ERR_INVALID). */
int dehalo_params_setup(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t s[4], dehalo_params** out);
/* ParamsIPA<C> [UPSTREAM halo2_proofs/src/poly/ipa/commitment.rs] from its parts, as the caller's ParamsIPA holds them: g / g_lagrange = 2^k affine
 * points each, w and u one point each ({x, y} Montgomery, 64 B, the layout of dehalo_params_create).  Pallas or Vesta (IPACommitmentScheme<EqAffine>
 * is Vesta; its scalar field is pasta::Fp); any other curve is DEHALO_ERR_UNSUPPORTED.  g and g_lagrange are registered with precomputed tables
 * as for KZG, so dehalo_keygen works on them: under these params the verifying key's fixed and permutation commitments are commit_lagrange with
 * Blind::default(), taken to be Blind(F::ONE) -- MSM + W (parity with upstream unpinned); under KZG params keygen is unchanged.
 * dehalo_params_commit_device is the bare MSM under either scheme.  g, u and w also stay on the device as plain points for the opening argument.
 * Not provided: ParamsIPA::new.  Its generators are hash-to-curve outputs ("Halo2-Parameters"), and the simplified SWU map of the Pasta curves needs the
 * constants of their 3-isogenies, which this library has no checked source for and will not restate from memory: the caller passes params.g, params.w and
 * params.u (dehalo_params_ipa_from_g) or a written ParamsIPA (dehalo_params_ipa_read), or asks for generators of the library's own public rule
 * (dehalo_params_ipa_generate).
 * Whole proofs: dehalo_prover_create / dehalo_create_proof with these params write a ProverIPA proof (below). */
int dehalo_params_ipa_create(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, const uint64_t w[8], const uint64_t u[8],
                             dehalo_params** out);
/* ParamsIPA from g alone, as upstream builds it: g_lagrange = g_to_lagrange(g) on the device (dehalo_g_to_lagrange_device), then exactly
 * dehalo_params_ipa_create(g, g_lagrange, w, u).  Host pointers; the same range checks and return codes as dehalo_params_ipa_create. */
int dehalo_params_ipa_from_g(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t* g, const uint64_t w[8], const uint64_t u[8], dehalo_params** out);
/* ParamsIPA at any k without a file: g, W and U are generated points ("Generated points" above: g[i] = (stream 0, index i), W = (stream 1, index 0),
 * U = (stream 1, index 1) under key32, NULL = DEHALO_GENERATORS_DEFAULT_KEY), made on the device; g_lagrange = dehalo_g_to_lagrange_device on the points where
 * they lie; then as dehalo_params_ipa_from_g, W's fixed-base table included.  The same range checks and return codes as dehalo_params_ipa_create.  The result is
 * an ordinary ParamsIPA: write, downsize, keygen and the provers take it as any other.  These are not upstream's generators: a proof made under generated
 * params verifies against the same params only, which an upstream verifier gets from dehalo_params_ipa_write's bytes through ParamsIPA::read. */
int dehalo_params_ipa_generate(dehalo_ctx* ctx, int curve, uint32_t k, const uint8_t* key32, dehalo_params** out);
/* ParamsIPA::{write, read} [UPSTREAM halo2_proofs/src/poly/ipa/commitment.rs]: k: u32 LE | g (2^k x 32 B) | g_lagrange (2^k x 32 B) | w (32 B) | u (32 B), every
 * point GroupEncoding::to_bytes -- x little-endian, bit 255 = y & 1, the identity all zeros: the encoding dehalo_transcript_write_point appends to a proof.
 * size = 4 + 64 x 2^k + 64; for ParamsKZG size is 0 and write DEHALO_ERR_UNSUPPORTED.  These are entry points of their own, beside dehalo_params_size /
 * dehalo_params_write, because those two are pinned for IPA params (0 and DEHALO_ERR_UNSUPPORTED: callers tell the schemes apart by them) and stay so.
 * read decompresses the 2 x 2^k + 2 points on the device (y = sqrt(x^3 + b), sign from bit 255) and then does what dehalo_params_ipa_create does;
 * DEHALO_ERR_INVALID, with nothing allocated left behind, for a length other than 4 + 64 x 2^k + 64 for the k in the first four bytes, an x coordinate
 * not below the modulus, an x that is not on the curve, and the encoding "x = 0 with the sign bit set". */
size_t dehalo_params_ipa_size(const dehalo_params* params);
int dehalo_params_ipa_write(const dehalo_params* params, uint8_t* out, size_t cap);
int dehalo_params_ipa_read(dehalo_ctx* ctx, int curve, const uint8_t* bytes, size_t len, dehalo_params** out);
/* The commitment scheme of params: DEHALO_SCHEME_KZG (dehalo_params_create / _setup / _read) or DEHALO_SCHEME_IPA (dehalo_params_ipa_create / _from_g / _read); < 0 for null. */
typedef enum { DEHALO_SCHEME_KZG = 0, DEHALO_SCHEME_IPA = 1 } dehalo_scheme;
int dehalo_params_scheme(const dehalo_params* params);
/* ParamsIPA's fixed-base table of W (dehalo_fixed_base_*: [blind] W of every commit / commit_lagrange), built once by whichever call made the params; null for
 * ParamsKZG and for null.  It belongs to the params: valid until dehalo_params_release, never passed to dehalo_fixed_base_release. */
const dehalo_fixed_base* dehalo_params_fixed_base(const dehalo_params* params);
int dehalo_params_read(dehalo_ctx* ctx, int curve, const uint8_t* bytes, size_t len, dehalo_params** out);
size_t dehalo_params_size(const dehalo_params* params);
int dehalo_params_write(const dehalo_params* params, uint8_t* out, size_t cap);
/* ParamsKZG from any SRS [UPSTREAM halo2_proofs/src/poly/kzg/commitment.rs write_custom / read_custom / from_parts, Params::downsize; halo2curves 0.3.x SerdeFormat;
 * restated from memory: INTEGRATION.md section 7].  The file is k: u32 LE | g | g_lagrange | g2 | s_g2 in every format:
 *   DEHALO_SERDE_PROCESSED            compressed points: G1 32 B (the point codec above), G2 64 B (x.c0 | x.c1 little-endian canonical, bit 7 of byte 63 = y.c0 is
 *                                     odd, the identity all zero): 4 + 64 x 2^k + 128 bytes;
 *   DEHALO_SERDE_RAW_BYTES            Montgomery limbs, G1 64 B, G2 128 B: 4 + 128 x 2^k + 256 bytes; every point is checked when read;
 *   DEHALO_SERDE_RAW_BYTES_UNCHECKED  the same bytes, copied in unseen: what dehalo_params_read / _write above have always read and written.
 * size_custom / write_custom: ParamsKZG only (ParamsIPA, which has one format upstream: 0 / DEHALO_ERR_UNSUPPORTED); both raw formats write dehalo_params_write's
 * bytes; Processed compresses g and g_lagrange on the device.
 * read_custom with downsize_k = DEHALO_KEEP_K reads the whole file: RAW_BYTES checks all 2 x 2^k points on the device (dehalo_points_check_device) and the two G2
 * points on the host, PROCESSED decompresses them, RAW_BYTES_UNCHECKED is dehalo_params_read.  With downsize_k <= k it is read + Params::downsize(downsize_k) in one
 * step, for a large SRS and a small circuit: only g[0 .. 2^downsize_k) is taken from the file (checked or decompressed as the format says), g_lagrange comes from
 * dehalo_g_to_lagrange_device, and tables of the small size alone are registered; the file's g_lagrange section is never read, so a checked format then vouches only
 * for what was kept (and for the two G2 points).  downsize_k above the file's k is DEHALO_ERR_INVALID.  Every failure is DEHALO_ERR_INVALID with a message naming its
 * kind -- the length, k, an x not below the modulus, an x not on the curve, x = 0 with the sign bit set, a stored coordinate word not below the modulus, a point
 * off the curve -- leaves nothing allocated and the context usable.  Processed and the checked G2 points are BN254's (other curves: DEHALO_ERR_UNSUPPORTED).
 * from_g: ParamsKZG from g, g2 and s_g2 alone (host pointers as dehalo_params_create takes them): g_lagrange = g_to_lagrange(g) on the device -- the KZG twin of
 * dehalo_params_ipa_from_g.
 * downsize: Params::downsize(k) as a NEW object (the caller keeps and releases `params`), under either scheme: the first 2^k of g, g_lagrange by the group FFT; KZG
 * keeps g2 / s_g2, IPA keeps w / u and gets its own table of W.  k above the params' is DEHALO_ERR_INVALID; k equal to it gives an equal copy. */
typedef enum { DEHALO_SERDE_PROCESSED = 0, DEHALO_SERDE_RAW_BYTES = 1, DEHALO_SERDE_RAW_BYTES_UNCHECKED = 2 } dehalo_serde_format;
#define DEHALO_KEEP_K 0xffffffffu
size_t dehalo_params_size_custom(const dehalo_params* params, int format);
int dehalo_params_write_custom(const dehalo_params* params, int format, uint8_t* out, size_t cap);
int dehalo_params_read_custom(dehalo_ctx* ctx, int curve, const uint8_t* bytes, size_t len, int format, uint32_t downsize_k, dehalo_params** out);
int dehalo_params_from_g(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t* g, const uint8_t* g2, const uint8_t* s_g2, dehalo_params** out);
int dehalo_params_downsize(dehalo_ctx* ctx, const dehalo_params* params, uint32_t k, dehalo_params** out);
int dehalo_params_release(dehalo_ctx* ctx, dehalo_params* params);
/* ParamsKZG::{commit, commit_lagrange} of `batch` device-resident columns of 2^k elements (n apart) -> affine points in HBM. */
int dehalo_params_commit_device(dehalo_ctx* ctx, const dehalo_params* params, const uint64_t* d_polys, size_t batch, int lagrange, uint64_t* d_out_affine, void* stream);

/* The circuit as data: the fields of halo2_proofs::plonk::ConstraintSystem that keygen and the prover read
 * [UPSTREAM halo2_proofs/src/plonk/circuit.rs].  Expressions are a flat array of nodes, children before parents:
 *   CONSTANT  a = index into `constants`;     FIXED / ADVICE / INSTANCE  a = column index, rotation;
 *   NEGATED   a = child;  SUM / PRODUCT  a, b = children;  SCALED  a = child, b = index into `constants`;
 *   CHALLENGE a = challenge index (Expression::Challenge: degree 0, its value squeezed from the transcript during the proof).
 * The Challenge API [cs.advice_column_phase, cs.challenge_phase; advice_column_in(SecondPhase), challenge_usable_after(FirstPhase)]:
 *   advice_phases     num_advice entries, the phase 0 / 1 / 2 of every advice column; NULL = all 0.  The phases in use are 0 ..= the largest, each with at least
 *                     one column (DEHALO_ERR_INVALID otherwise); more than three phases: DEHALO_ERR_UNSUPPORTED
 *   challenge_phases  num_challenges entries: challenge j is squeezed after the advice commitments of phase challenge_phases[j] (a phase in use)
 * A circuit with one phase and no challenge is described, encoded (the substitute transcript_repr) and proved exactly as before these fields existed.
 * The shuffle argument [cs.shuffle(name, |meta| vec![(input_i, shuffle_i)]); halo2_proofs v0.3.0 plonk/shuffle]: the rows' input tuples are a permutation of
 * the rows' shuffle tuples over the usable rows.  Both sides are compressed with theta as a lookup's are (the first expression carries the highest power);
 * the argument is one grand product z with z[0] = 1, z[i + 1] = z[i] (A[i] + gamma) / (S[i] + gamma), committed behind the lookups' products, three
 * quotient terms -- l0 (1 - z), l_last (z^2 - z), l_active (z(wX)(S + gamma) - z(X)(A + gamma)) -- behind the lookups' terms, and z(x), z(wx) behind every
 * circuit's lookup evaluations.  It requires degree max(2 + deg input, 2 + deg shuffle), either at least 1.  A constraint system with num_shuffles = 0 is
 * described, encoded and proved exactly as before these fields existed.       */
typedef enum {
    DEHALO_EXPR_CONSTANT = 0, DEHALO_EXPR_FIXED = 1, DEHALO_EXPR_ADVICE = 2, DEHALO_EXPR_INSTANCE = 3, DEHALO_EXPR_NEGATED = 4, DEHALO_EXPR_SUM = 5,
    DEHALO_EXPR_PRODUCT = 6, DEHALO_EXPR_SCALED = 7, DEHALO_EXPR_CHALLENGE = 8
} dehalo_expr_kind;
typedef struct { uint32_t kind, a, b; int32_t rotation; } dehalo_expr_node;
typedef enum { DEHALO_COLUMN_ADVICE = 0, DEHALO_COLUMN_FIXED = 1, DEHALO_COLUMN_INSTANCE = 2 } dehalo_column_kind;
typedef struct { uint32_t kind, index; int32_t rotation; } dehalo_column_query;          /* (Column, Rotation); rotation unused for permutation columns */
typedef struct {
    uint32_t num_advice, num_fixed, num_instance, minimum_degree;
    const dehalo_expr_node* nodes; uint32_t num_nodes;
    const uint64_t* constants; uint32_t num_constants;              /* 4 x u64 Montgomery each (Expression::Constant(F)) */
    const uint32_t* gates; uint32_t num_gates;                      /* root node of every gate polynomial, in order (gates.flat_map(polynomials)) */
    const uint32_t* lookup_lens; uint32_t num_lookups;              /* lookup l has lookup_lens[l] (input, table) expression pairs ...          */
    const uint32_t* lookup_inputs; const uint32_t* lookup_tables;   /* ... their root nodes, lookups concatenated                                */
    const dehalo_column_query* permutation_columns; uint32_t num_permutation_columns;      /* cs.permutation.columns, enable_equality order */
    const dehalo_column_query* advice_queries; uint32_t num_advice_queries;                /* first-use order: the order of the evaluations in the proof */
    const dehalo_column_query* fixed_queries; uint32_t num_fixed_queries;
    const dehalo_column_query* instance_queries; uint32_t num_instance_queries;
    const uint8_t* advice_phases;                                   /* num_advice entries; NULL = every column in phase 0 */
    const uint8_t* challenge_phases; uint32_t num_challenges;       /* the phase after which each challenge is squeezed */
    const uint32_t* shuffle_lens;                                   /* shuffle j has shuffle_lens[j] >= 1 (input, shuffle) expression pairs ...    */
    const uint32_t* shuffle_inputs; const uint32_t* shuffle_tables; /* ... their root nodes, shuffles concatenated; NULL / 0: no shuffle argument  */
    uint32_t num_shuffles;
} dehalo_constraint_system;

/* keygen_vk + keygen_pk [UPSTREAM halo2_proofs/src/plonk/keygen.rs; benches/delay_enc.rs:86,103] on the device: commit_lagrange,
 * lagrange_to_coeff and coeff_to_extended of every fixed and permutation column, l0 / l_last / l_active_row.
 *   fixed               num_fixed x 2^k x 4 u64, host; Montgomery unless DEHALO_KEYGEN_FIXED_CANONICAL (selectors already compressed into them)
 *   permutation_mapping num_permutation_columns x 2^k u64, host: cell (column j, row i) is mapped to cell value / 2^k, value % 2^k
 *                       (permutation::keygen::Assembly::mapping flattened); identity = j * 2^k + i
 *   selectors           num_selectors arrays of 2^k bytes (0 / 1): only serialised with the verifying key (vk.selectors)              */
enum { DEHALO_KEYGEN_FIXED_CANONICAL = 1 };
int dehalo_keygen(dehalo_ctx* ctx, const dehalo_params* params, const dehalo_constraint_system* cs, const uint64_t* fixed, const uint64_t* permutation_mapping,
                  const uint8_t* const* selectors, uint32_t num_selectors, uint32_t flags, dehalo_pk** out);
/* ProvingKey::{read, write} / VerifyingKey::write with SerdeFormat::RawBytes [UPSTREAM halo2_proofs/src/plonk.rs; benches/delay_enc.rs:
 * 88-115]: reading needs the circuit's constraint system, as upstream's read::<_, ConcreteCircuit> does. */
int dehalo_pk_read(dehalo_ctx* ctx, int curve, const dehalo_constraint_system* cs, const uint8_t* bytes, size_t len, uint32_t num_selectors, dehalo_pk** out);
size_t dehalo_pk_size(const dehalo_pk* pk);
int dehalo_pk_write(dehalo_ctx* ctx, const dehalo_pk* pk, uint8_t* out, size_t cap);
size_t dehalo_vk_size(const dehalo_pk* pk);
int dehalo_vk_write(const dehalo_pk* pk, uint8_t* out, size_t cap);
/* Keys in every SerdeFormat [UPSTREAM halo2_proofs/src/plonk.rs VerifyingKey / ProvingKey::{write, read}(.., SerdeFormat), poly.rs, helpers.rs; restated from memory:
 * INTEGRATION.md sections 7 and 15].  The formats are dehalo_serde_format's (declared with the params above; plain int here):
 *   vk   = k: u32 BE | num_fixed: u32 BE | fixed commitments | permutation commitments | selectors (2^k bits each, packed LSB first)
 *   pk   = vk | l0 | l_last | l_active_row | slice(fixed_values) | slice(fixed_polys) | slice(fixed_cosets) | slice(perm values) | slice(perm polys) | slice(perm cosets)
 *   poly = len: u32 BE | len elements          slice = count: u32 BE | count polys
 *   DEHALO_SERDE_PROCESSED            a commitment is 32 B (the point codec's compressed form), an element its canonical integer, 32 B little-endian (to_repr).
 *                                     Read: every point is decompressed on the device (status 1 / 2 / 4 fail), every element must be below p (from_repr).
 *   DEHALO_SERDE_RAW_BYTES            a commitment is 64 B, an element 32 B, Montgomery limbs.  Read: every point goes through dehalo_points_check_device (status
 *                                     1 / 2 fail; (0, 0) is legal), every element's stored word must be below p (dehalo_scalars_check_device).
 *   DEHALO_SERDE_RAW_BYTES_UNCHECKED  the same bytes, copied in unseen: dehalo_pk_read itself, giving an equal key.
 * Both raw formats write dehalo_pk_write's / dehalo_vk_write's bytes; the Processed vk and pk are each 32 x (num_fixed + permutation columns) bytes shorter.  All
 * three curves.  Extended-domain columns leave in upstream's standard form.  size_custom returns 0 for null or an unknown format.  A null ctx in a write means the
 * key's own.  The read uploads one slice at a time and runs one conversion or check launch per slice (one
 * per 2^28 elements of a slice that holds more: the scalar codec's count limit is not the key's).
 * Every failure of a read is DEHALO_ERR_INVALID, with a message that names its kind -- the length, k, the fixed-column count, a polynomial length or count, an x
 * not below the modulus, an x not on the curve, x = 0 with the sign bit set, a stored coordinate word not below the modulus, a point off the curve, an element (or
 * its stored word) not below the modulus -- and the section (which commitment list, which polynomial slice), for an element also the lowest offending index
 * within that section; it leaves nothing allocated and the context usable.  An unknown format is DEHALO_ERR_INVALID from every call. */
size_t dehalo_vk_size_custom(const dehalo_pk* pk, int format);
int dehalo_vk_write_custom(dehalo_ctx* ctx, const dehalo_pk* pk, int format, uint8_t* out, size_t cap);
size_t dehalo_pk_size_custom(const dehalo_pk* pk, int format);
int dehalo_pk_write_custom(dehalo_ctx* ctx, const dehalo_pk* pk, int format, uint8_t* out, size_t cap);
int dehalo_pk_read_custom(dehalo_ctx* ctx, int curve, const dehalo_constraint_system* cs, const uint8_t* bytes, size_t len, int format, uint32_t num_selectors,
                          dehalo_pk** out);
/* VerifyingKey::read + keygen_pk(params, vk, circuit) [UPSTREAM halo2_proofs/src/plonk/keygen.rs; benches/delay_enc.rs:96-103]: the proving key of `fixed` /
 * `permutation_mapping` UNDER the given verifying key.  The vk is parsed in vk_format (a checked format checks its commitments as above); its commitments and packed
 * selectors become the key's, and fixed_values / polys / cosets, the permutation's three column sets and l0 / l_last / l_active_row are built exactly as
 * dehalo_keygen builds them -- without launching an MSM.  The vk's commitments are NOT compared with the columns, as upstream does not: a vk that belongs to other
 * columns gives a key whose proofs a verifier rejects.  DEHALO_ERR_INVALID when the vk's k differs from the params', its num_fixed from the circuit's, or the length
 * does not fit.  flags: dehalo_keygen's.  Both schemes; under ParamsIPA the vk's commitments already carry [Blind::default()] W.  The substitute transcript_repr is
 * the one dehalo_keygen would give for the same vk bytes. */
int dehalo_keygen_pk(dehalo_ctx* ctx, const dehalo_params* params, const dehalo_constraint_system* cs, const uint8_t* vk_bytes, size_t vk_len, int vk_format,
                     uint32_t num_selectors, const uint64_t* fixed, const uint64_t* permutation_mapping, uint32_t flags, dehalo_pk** out);
/* vk.transcript_repr, the first thing create_proof absorbs.  Upstream derives it from the Debug text of the pinned verifying key, which
 * cannot be reproduced outside the crate: an integrator passes upstream's value (4 x u64 Montgomery).  Until set, the key carries a
 * substitute: Blake2b-512("Halo2-Verify-Key") over the key's RawBytes and a binary encoding of the constraint system. */
int dehalo_pk_set_transcript_repr(dehalo_pk* pk, const uint64_t repr[4]);
int dehalo_pk_get_transcript_repr(const dehalo_pk* pk, uint64_t repr[4]);
/* out[0..7] = k, extended_k, blinding_factors, degree, permutation sets, commitments before the evaluations (advice + 3 lookups + sets + shuffles + 1 +
 * (degree - 1)), evaluations (advice queries + fixed queries + 1 + permutation columns + 3 sets - 1 + 5 lookups + 2 shuffles), opening points */
int dehalo_pk_info(const dehalo_pk* pk, uint32_t out[8]);
/* out[0] = advice phases in use (1 .. 3), out[1] = challenges of the key's constraint system */
int dehalo_pk_phases(const dehalo_pk* pk, uint32_t out[2]);
int dehalo_pk_release(dehalo_ctx* ctx, dehalo_pk* pk);

/* Random scalars of one proof (see csrc/hostrng.hpp).  DEHALO_RNG_OS is what a NULL pointer selects.
 * DEHALO_RNG_CHACHA20 is the DEHALO_RNG_OS generator with the caller's key instead of 32 bytes of operating-system entropy: reproducible, and as strong as
 * the key.  The key is the 32 bytes of pcg_state[2] | pcg_inc[2], read as they lie in memory; it is never written back, so two calls with the same key give
 * the same proof -- a key must not be used for two different proofs.  From the key on the two kinds are one code path, and their schedule is:
 *   - ChaCha20 (RFC 8439's block function) over the state words sigma | key | w12 w13 | w14 w15, where w14 | w15 is a 64-bit stream id, low word first;
 *   - a scalar is 256 candidate bits (eight 32-bit words, least significant first) masked to the modulus' bit length and accepted iff the result is < p,
 *     handed over as a Montgomery representation;
 *   - stream 0, the SERIAL stream, serves every small draw on the host (blinding rows, blinds, l_rand / r_rand), in upstream's order: consecutive blocks
 *     with a 64-bit block counter in w12 | w13 from 0, each block two candidates; a rejected candidate consumes its half block;
 *   - a draw of n = 2^k scalars is INDEXED and made by a kernel: scalar i is the first accepted candidate among the first halves of the blocks
 *     w12 = i mod 2^32, w13 = (i >> 32 & 0xffff) | attempt << 16 for attempt = 0, 1, ...; it consumes nothing of the serial stream.  Stream 1: the vanishing
 *     argument's random polynomial, and s_poly of a stand-alone dehalo_ipa_open; stream 2: s_poly of the opening inside an IPA proof. */
typedef enum { DEHALO_RNG_OS = 0, DEHALO_RNG_PCG64 = 1, DEHALO_RNG_CALLBACK = 2, DEHALO_RNG_CHACHA20 = 3 } dehalo_rng_kind;
/* fills `count` scalars (4 x u64 Montgomery representations, < p); `position` = index of the first one in upstream's draw order.  May be
 * called from a helper thread of the library, never concurrently for one proof.  Returns 0. */
typedef int (*dehalo_rng_fill_fn)(void* user, uint64_t* out, size_t count, uint64_t position);
typedef struct {
    int kind;
    uint64_t pcg_state[2], pcg_inc[2];     /* DEHALO_RNG_PCG64: numpy PCG64 state / increment, low word first; advanced past the proof's draws on return.
                                            * DEHALO_RNG_CHACHA20: the 32-byte key, left as it is */
    dehalo_rng_fill_fn fill; void* user;   /* DEHALO_RNG_CALLBACK */
} dehalo_rng;
/* `count` scalars of the field from a generator (what create_proof draws): lets a test pin the kinds without a device.  `skip`: PCG64 is advanced past
 * that many scalars and a callback sees it as `position`; under the ChaCha20 kinds it moves no stream (what a proof skips there is an indexed draw, which
 * consumes nothing of the serial stream), so any `skip` returns the scalars of skip = 0. */
int dehalo_rng_scalars(dehalo_rng* rng, int field, uint64_t skip, uint64_t* out, size_t count);
/* An indexed draw of the schedule above on the device: d_out[0 .. n) = n scalars of `field` (a dehalo_field id) from ChaCha20 stream `cha_stream` under rng's
 * key, one kernel launch on `stream` (NULL: the context's) -- the launch create_proof makes for its random polynomial.  Only DEHALO_RNG_CHACHA20 is taken:
 * DEHALO_ERR_INVALID for a NULL rng, any other kind (DEHALO_RNG_OS as well: its output could not be checked), an unknown field or n >= 2^29; n = 0 does
 * nothing and returns 0. */
int dehalo_rng_scalars_device(dehalo_ctx* ctx, dehalo_rng* rng, int field, uint64_t cha_stream, uint64_t* d_out, size_t n, void* stream);

/* Blake2bWrite / Challenge255 [UPSTREAM halo2_proofs/src/transcript.rs; benches/delay_enc.rs:120,134]. */
int dehalo_transcript_create(int curve, dehalo_transcript** out);
int dehalo_transcript_common_scalar(dehalo_transcript* t, const uint64_t scalar[4]);                 /* Montgomery */
int dehalo_transcript_write_scalar(dehalo_transcript* t, const uint64_t scalar[4]);
int dehalo_transcript_write_point(dehalo_transcript* t, const uint64_t affine_xy[8]);                /* Montgomery; identity rejected */
int dehalo_transcript_squeeze_challenge(dehalo_transcript* t, uint64_t out[4]);                      /* Montgomery */
size_t dehalo_transcript_len(const dehalo_transcript* t);
int dehalo_transcript_finalize(const dehalo_transcript* t, uint8_t* out, size_t cap);                /* the proof bytes written so far */
void dehalo_transcript_release(dehalo_transcript* t);
/* Blake2bRead<_, C, Challenge255<C>>: the same object over the `len` bytes of a proof (copied; `proof` may be NULL when len = 0).  common_scalar and
 * squeeze_challenge work on both kinds; the write_* calls on a reader and the read_* calls on a writer return DEHALO_ERR_INVALID, and a reader's _len is 0.
 * A read takes the next 32 bytes, absorbs what it decoded exactly as the writer absorbed it, and returns it (Montgomery words, canonical).  It fails with
 * DEHALO_ERR_INVALID, leaving the position and the hash state where they were, when fewer than 32 bytes are left; for a scalar, when the integer is not below
 * r; for a point (GroupEncoding::from_bytes: x little-endian, bit 255 = y is odd), when x is not below p, when x^3 + b is not a square, or when the bytes
 * are all zero (the identity, which no writer can have written).  All three curves.  _remaining: the bytes not read yet (0 for a writer). */
int dehalo_transcript_create_read(int curve, const uint8_t* proof, size_t len, dehalo_transcript** out);
int dehalo_transcript_read_point(dehalo_transcript* t, uint64_t affine_xy[8]);
int dehalo_transcript_read_scalar(dehalo_transcript* t, uint64_t scalar[4]);
size_t dehalo_transcript_remaining(const dehalo_transcript* t);

/* The pairing check a KZG verifier ends with [UPSTREAM halo2_proofs/src/poly/kzg/strategy.rs; halo2curves bn256: multi_miller_loop, final_exponentiation]:
 * prod_i e(P_i, Q_i) == 1 in GT.  P_i: affine x | y, 8 u64 Montgomery ((0, 0) = the identity, whose factor is 1); Q_i: the 128-byte raw form dehalo_params_create takes
 * for g2 / s_g2 (all zero = the identity).  A P_i or Q_i off its curve, or a Q_i outside the order-r subgroup: DEHALO_ERR_INVALID.  count = 0: *is_one = 1.  Host only, no context.
 * BN254 only: DEHALO_ERR_UNSUPPORTED for Pallas and Vesta.  Optimal ate over 6x + 2 and one final exponentiation for the whole product (csrc/pairing_host.hpp: every
 * derived constant is computed at first use); a two-pair check takes milliseconds.  Nothing here runs in constant time: every input of a verifier is public. */
int dehalo_pairing_check(int curve, const uint64_t* g1_affine_xy, const uint8_t* g2_raw, size_t count, int* is_one);

/* Many INDEPENDENT pairing checks against FIXED G2 points, on the device in one launch (csrc/pairing.cuh): what a KZG verifier of many proofs needs, whose
 * s_g2 and g2 are fixed when it is made.  For check c < checks and the table's `pairs` points Q_j:
 *     gt[c] = (prod_j miller(P[c][j], Q_j)) ^ ((q^12 - 1) / r),    status[c] = DEHALO_PAIRING_ONE iff gt[c] = 1.
 * A table is made once from `pairs` G2 points in dehalo_pairing_check's 128-byte raw form: all the Miller loop does on the twist -- the 64 doublings, the 36
 * additions of 6x + 2, the two Frobenius steps, an Fq2 inversion each -- depends on Q alone and is done then, on the host; the table keeps the two line
 * coefficients of each of the 102 steps (128 B a step).  An all-zero Q is the identity: its factor is 1.  A Q that dehalo_pairing_check would refuse (off the
 * twist, outside the order-r subgroup, a word not below q) is DEHALO_ERR_INVALID, and so are pairs = 0 or > DEHALO_PAIRING_MAX_PAIRS and a null argument;
 * DEHALO_ERR_UNSUPPORTED for Pallas and Vesta.  ctx = NULL makes a HOST table: dehalo_pairing_checks then runs on the host through the same table (a mode the
 * caller chooses, never a fallback), and dehalo_pairing_checks_device refuses it with DEHALO_ERR_INVALID.
 *   g1_affine_xy  checks x pairs x {x, y}, 8 u64 standard Montgomery a point; (0, 0) words = the identity, whose factor is 1; a coordinate word not below q
 *                 stands for its residue ("Non-canonical words" (4) at the top)
 *   status        checks bytes: DEHALO_PAIRING_NOT_ONE, _ONE, or _OFF_CURVE for a check one of whose P is not on y^2 = x^3 + 3 (its gt is zero words, and no
 *                 other check is affected)
 *   gt            optional, checks x 12 x 4 u64: the Fq2 coefficients of w^0 .. w^5 in that order, each as a | b (a + b i), canonical words, standard
 *                 Montgomery.  In the tower Fq12 = Fq6[w] / (w^2 - v), Fq6 = Fq2[v] / (v^3 - (9 + i)), an element a + b w with a, b = (a, b, c) in Fq6 has
 *                 w^0, w^2, w^4 = a.a, a.b, a.c and w^1, w^3, w^5 = b.a, b.b, b.c.  The value is the host pairing's, bit for bit.
 * checks = 0 does nothing and accepts null arrays; checks > DEHALO_PAIRING_MAX_CHECKS is DEHALO_ERR_INVALID.  dehalo_pairing_checks takes host arrays: with a
 * device table it uploads, runs the kernel on the context's stream and downloads.  One wave per check, the running product in LDS, no workspace; nothing here
 * runs in constant time. */
#define DEHALO_PAIRING_MAX_PAIRS 8
#define DEHALO_PAIRING_MAX_CHECKS (1u << 20)
enum { DEHALO_PAIRING_NOT_ONE = 0, DEHALO_PAIRING_ONE = 1, DEHALO_PAIRING_OFF_CURVE = 2 };
typedef struct dehalo_pairing_table dehalo_pairing_table;
int dehalo_pairing_table_create(dehalo_ctx* ctx, int curve, const uint8_t* g2_raw /* pairs x 128 */, uint32_t pairs, dehalo_pairing_table** out);
void dehalo_pairing_table_release(dehalo_pairing_table* t);
int dehalo_pairing_checks_device(dehalo_ctx* ctx, const dehalo_pairing_table* t, const uint64_t* d_g1_affine_xy, uint32_t checks, uint8_t* d_status, uint64_t* d_gt,
                                 void* stream);
int dehalo_pairing_checks(const dehalo_pairing_table* t, const uint64_t* g1_affine_xy, uint32_t checks, uint8_t* status, uint64_t* gt);
/* the number of checks one block of the kernel holds for this table's launches (ceil(checks / this) blocks a launch; t may be NULL: the same for every
 * table today): for tests of the launch's edges */
uint32_t dehalo_pairing_checks_per_block(const dehalo_pairing_table* t);

/* The IPA opening of ONE polynomial [UPSTREAM halo2_proofs/src/poly/ipa/commitment/prover.rs: create_proof(params, rng, transcript, p_poly, p_blind,
 * x_3)]: proves that the commitment P = MSM(p, g) + [blind] W opens to p(x_3) -- what ProverIPA's multiopen ends with, and what a test or an integrator
 * can call on its own.  params: dehalo_params_ipa_create; d_poly: 2^k coefficients in device memory (Montgomery, read only); blind, x3: Montgomery.
 * Neither P nor p(x_3) is written: the caller's transcript holds them already, as upstream's does.
 * Draws, in upstream's order: s_poly (2^k scalars), s_poly_blind, then (l_rand, r_rand) for each of the k rounds.  s_poly is the call's large draw and
 * comes from the generator forked at its position, as create_proof's random polynomial does: with DEHALO_RNG_OS / DEHALO_RNG_CHACHA20 a ChaCha20 kernel (stream 1) under
 * the call's key, with PCG64 / a callback exactly the scalars a serial draw would give.  A PCG64 rng is advanced past all of them.
 * Writes: the point S = commit(s_poly, s_poly_blind); squeezes xi, z; per round j < k the points L_j, R_j and squeezes u_j; then the scalars c, f.
 * Proof bytes: 32 (S) + k x 64 (L_j | R_j) + 64 (c | f).  Each round queues its launches on the context's stream and waits once (L_j, R_j): round 1
 * runs over the precomputed table of g, later rounds over one plain registration of [G' | U | W] that is rebuilt on the stream (no allocation, no wait). 
 * Errors: DEHALO_ERR_INVALID for KZG params / null arguments / a point at infinity that the transcript cannot take. */
int dehalo_ipa_open(dehalo_ctx* ctx, const dehalo_params* params, const uint64_t* d_poly, const uint64_t blind[4], const uint64_t x3[4], dehalo_rng* rng,
                    dehalo_transcript* transcript);

/* A prover = the device buffers of one proof for a given key, on `ctx` (stream + workspace).  `side_ctx` (may be NULL): a second context of
 * the same device; work no transcript challenge waits for (lagrange_to_coeff / coeff_to_extended of a phase's columns, the random
 * polynomial's commitment, the gate and table-value passes of evaluate_h) is queued there and runs beside the commitment phases.
 * Several provers over one key, each on its own context(s), may run concurrently from different threads (batch proving).
 * `params` decides the scheme: ParamsKZG -> ProverGWC (or ProverSHPLONK: dehalo_prover_set_multiopen), ParamsIPA (Pallas / Vesta) -> ProverIPA.  DEHALO_ERR_UNSUPPORTED: more than 32 distinct
 * rotations among the circuit's queries and the prover's own {0, 1, -1, -(blinding_factors + 1)} (either scheme). */
int dehalo_prover_create(dehalo_ctx* ctx, dehalo_ctx* side_ctx, const dehalo_params* params, const dehalo_pk* pk, dehalo_prover** out);
/* A prover whose proofs are over `num_circuits` witnesses of the one key [UPSTREAM create_proof(&params, &pk, &[circuit_0, .., circuit_{N-1}], &[instances_0, ..], ..)]:
 * one transcript, one random polynomial, one quotient, one set of fixed and sigma evaluations and one multiopen for all of them (dehalo_create_proof_multi).
 * dehalo_prover_create is its num_circuits = 1 case.  Every per-circuit buffer is num_circuits times a single prover's; the quotient's and the multiopen's are not.
 * DEHALO_ERR_INVALID for num_circuits = 0; with num_circuits > 1 DEHALO_ERR_UNSUPPORTED for ParamsIPA and for a key with more than one advice phase;
 * DEHALO_ERR_OOM when the buffers do not fit.  No cap on num_circuits is set here; the batched entry points a phase goes through take num_circuits x lookups
 * < 4096 pairs (the permutation), < 65536 columns per transform or grand-product call and columns x 2^k x windows < 2^32 per MSM launch, and refuse more
 * with DEHALO_ERR_INVALID at the proof. */
int dehalo_prover_create_multi(dehalo_ctx* ctx, dehalo_ctx* side_ctx, const dehalo_params* params, const dehalo_pk* pk, uint32_t num_circuits, dehalo_prover** out);
int dehalo_prover_release(dehalo_prover* prover);
/* Which KZG multiopen a prover over ParamsKZG writes [UPSTREAM poly/kzg/multiopen/{gwc,shplonk}]: ProverGWC (the default: one witness commitment per distinct
 * opening point) or ProverSHPLONK (two commitments, h and h', whatever the circuit's rotations are).  Everything before the multiopen is the same proof.
 * Takes the prover's lock (it waits for a proof in flight) and may be called again with either value; the SHPLONK buffers are allocated at the first switch
 * to it.  Followed by dehalo_prover_proof_size, dehalo_create_proof(s)(_circuit) and a sharded prover alike (both commitments are single columns: nothing to
 * split).  DEHALO_ERR_UNSUPPORTED for a prover over ParamsIPA, DEHALO_ERR_INVALID for any other value or a null prover. */
typedef enum { DEHALO_MULTIOPEN_GWC = 0, DEHALO_MULTIOPEN_SHPLONK = 1 } dehalo_multiopen;
int dehalo_prover_set_multiopen(dehalo_prover* prover, int multiopen);
/* Byte length of one proof of this prover (its params' scheme, instance commitments and evaluations included); 0 for null.
 *   KZG / GWC: 32 x (advice + 3 lookups + permutation sets + shuffles + 1 + (degree - 1) + opening points) + 32 x evaluations
 *   KZG / SHPLONK: the same with 2 in the place of the opening points
 *   IPA: 32 x (advice + 3 lookups + permutation sets + shuffles + 1 + (degree - 1) + 1 (f) + 1 (S) + 2 k) + 32 x (instance queries + evaluations + point sets + 2)
 * A shuffle adds one commitment and two evaluations (its product at x and at omega x). */
size_t dehalo_prover_proof_size(const dehalo_prover* prover);
/* create_proof: one circuit (of a prover made for one: DEHALO_ERR_INVALID on a prover of dehalo_prover_create_multi with num_circuits > 1), its instance columns,
 * the caller's rng and transcript.
 *   advice     num_advice x 2^k x 4 u64 Montgomery (rows >= usable are overwritten by blinding), host memory, or device memory when
 *              DEHALO_PROOF_ADVICE_ON_DEVICE
 *   instances  num_instance_columns arrays of instance_lens[i] scalars (Montgomery); the reference passes none (&[&[&[]]])
 * Errors follow upstream's: DEHALO_ERR_INVALID for instances.len() != num_instance_columns / an instance column longer than the usable
 * rows / a commitment at infinity; DEHALO_ERR_NOT_IN_TABLE when a lookup input is missing from its table; DEHALO_ERR_SHUFFLE when the two sides of a shuffle
 * argument are not a permutation of each other over the usable rows (its product does not come back to 1; upstream only debug-asserts this).  The flag is read
 * with the products' commitments, at the wait the proof makes there anyway; the prover is usable for the next proof.
 * Under ParamsIPA (create_proof::<IPACommitmentScheme<_>, ProverIPA<_>, ..>) every commitment carries its blind ([blind] W from the table of W, dehalo_fixed_base_blind_device: one
 * launch per phase), the instance columns are committed with Blind::default() and absorbed as points, their evaluations are written first, and the proof ends
 * with ProverIPA's multiopen (x_1, x_2, f, x_3, the q evaluations, x_4) and the opening argument of dehalo_ipa_open on the same transcript and generator.
 * Advice and instance values are words under "Non-canonical words" (1), (3) at the top: a value given as x + j p proves what x proves, byte for byte (the
 * instance values a KZG proof hashes are hashed as their canonical encodings). */
enum { DEHALO_PROOF_ADVICE_ON_DEVICE = 1, DEHALO_PROOF_ADVICE_CANONICAL = 2 /* plain integers < p: converted on the device */ };
int dehalo_create_proof(dehalo_prover* prover, const uint64_t* advice, const uint64_t* const* instances, const size_t* instance_lens, uint32_t num_instance_columns,
                        dehalo_rng* rng, dehalo_transcript* transcript, uint32_t flags);
/* create_proof over the N = num_circuits witnesses of a prover made by dehalo_prover_create_multi: ONE proof [UPSTREAM plonk/prover.rs, the loops over `circuits`].
 *   advice      N pointers, each a buffer of dehalo_create_proof's layout (all on the host, or all on the device with DEHALO_PROOF_ADVICE_ON_DEVICE)
 *   instances   N x num_instance_columns arrays, circuit-major (circuit c's column i is entry c * num_instance_columns + i); instance_lens likewise
 * Order of the transcript: the key's representation; every circuit's instance values (circuit after circuit, column after column); every circuit's advice
 * commitments; theta; every circuit's permuted lookup pairs; beta, gamma; every circuit's permutation products, THEN every circuit's lookup products, THEN every
 * circuit's shuffle products, then the random polynomial; y; the pieces of the one quotient, whose numerator is one running value v = v y + term over circuit 0's gates, permutation, lookup and shuffle terms,
 * circuit 1's, ...; x; the evaluations -- every circuit's advice queries | fixed | random | sigma | every circuit's permutation products | every circuit's
 * lookups | every circuit's shuffles -- and the multiopen over the queries of circuit 0, circuit 1, ..., then once fixed, sigma, h, random.  The generator's draws are circuit-major the
 * same way: the blinding rows of circuit c's advice columns, then its columns' blinds, then circuit c + 1's.  A PCG64 generator is advanced past all of them.
 * Proof bytes (GWC; SHPLONK: 2 for `points`): 32 x (N (advice + 3 lookups + sets + shuffles) + 1 + (degree - 1) + points)
 *                                             + 32 x (N (advice queries + (3 sets - 1 if sets) + 5 lookups + 2 shuffles) + fixed queries + 1 + permutation columns).
 * With N = 1 the proof is dehalo_create_proof's, byte for byte.  Each commitment phase is one MSM launch over all circuits' columns.
 * Errors: dehalo_create_proof's for every circuit (DEHALO_ERR_NOT_IN_TABLE when any circuit's lookup input is missing from its table, DEHALO_ERR_SHUFFLE when
 * any circuit's shuffle does not close; the prover stays usable); DEHALO_ERR_INVALID for num_circuits = 0 or other than the prover's.  A prover with num_circuits > 1 proves through this call only:
 * dehalo_create_proofs, dehalo_create_proof_circuit, dehalo_create_proofs_circuit, dehalo_create_proof_phased and dehalo_prover_set_shard (world > 1)
 * return DEHALO_ERR_UNSUPPORTED on it. */
int dehalo_create_proof_multi(dehalo_prover* prover, const uint64_t* const* advice, const uint64_t* const* instances, const size_t* instance_lens,
                              uint32_t num_instance_columns, uint32_t num_circuits, dehalo_rng* rng, dehalo_transcript* transcript, uint32_t flags);
/* create_proof of a circuit with later-phase advice [UPSTREAM plonk/prover.rs: `for current_phase in phases`]: the witness of phase p may depend on the challenges
 * squeezed after the commitments of the phases before it, so the caller supplies it through a callback, one call per phase.  After the instances are absorbed,
 * for each phase in order: fn(user, phase, challenges, num_challenges, &advice); the blinding rows of that phase's columns (column order), one blind per column;
 * commit_lagrange of each, written to the transcript in column order; one squeeze per challenge of that phase, in challenge-index order.  theta follows the
 * last phase.  So the advice commitments stand phase-major in the proof and the generator's draws are phase-major; with one phase both are dehalo_create_proof's.
 *   fn          called on the proving thread, once per phase; for phase p > 0 after the commitments of phase p - 1 are in the transcript.  It may call nothing
 *               on this prover (the prover's lock is held) or on the prover's contexts' streams
 *   challenges  num_challenges x 4 u64 Montgomery (the key's challenges, by index); those not squeezed yet are zero.  Valid during the callback only
 *   *advice     set by fn: a buffer of dehalo_create_proof's layout (num_advice x 2^k x 4 u64) under this call's `flags` (host, or device memory with
 *               DEHALO_PROOF_ADVICE_ON_DEVICE; DEHALO_PROOF_ADVICE_CANONICAL).  Only the columns of `phase` are read from it.  It must stay valid and unchanged until
 *               the next callback or the return of this call
 * A non-zero return of fn ends the proof with DEHALO_ERR_INVALID (the code is in dehalo_last_error's text); the prover is usable for the next proof.
 * On a key with one phase fn is called once and the proof is dehalo_create_proof's, byte for byte.
 * dehalo_create_proof on a key with more than one phase returns DEHALO_ERR_INVALID (its advice would have to exist before the first commitment).  On such a
 * key dehalo_create_proofs, dehalo_create_proof_circuit, dehalo_create_proofs_circuit and dehalo_prover_set_shard (world > 1) return DEHALO_ERR_UNSUPPORTED. */
typedef int (*dehalo_advice_fn)(void* user, uint32_t phase, const uint64_t* challenges, uint32_t num_challenges, const uint64_t** advice);
int dehalo_create_proof_phased(dehalo_prover* prover, dehalo_advice_fn fn, void* user, const uint64_t* const* instances, const size_t* instance_lens,
                               uint32_t num_instance_columns, dehalo_rng* rng, dehalo_transcript* transcript, uint32_t flags);
/* ---- MockProver::verify over a proving key [UPSTREAM halo2_proofs/src/dev.rs MockProver::verify] (csrc/check.hip) ----------------------------------
 * dehalo_create_proof proves whatever advice it is handed; this call says WHERE a witness breaks the circuit of `pk`, on the device, before anything is proved.
 *   advice, instances, instance_lens, num_instance_columns, flags   exactly dehalo_create_proof's (DEHALO_PROOF_ADVICE_ON_DEVICE and DEHALO_PROOF_ADVICE_CANONICAL
 *                       included; the same instance checks, DEHALO_ERR_INVALID in the same cases); nothing is blinded: the rows beyond the usable ones are read as given
 *   permutation_mapping dehalo_keygen's argument of that name (host memory).  NULL: the copy constraints are not checked (copy_failures = cells_in_cycles = 0).  An
 *                       entry >= num_permutation_columns x 2^k is DEHALO_ERR_INVALID, decided by a kernel that only reads the mapping, before any kernel follows it.
 *                       Whether the mapping is a bijection is NOT checked.
 * What is checked (usable rows = [0, 2^k - (blinding_factors + 1))):
 *   GATE    every gate polynomial on every usable row; rotations wrap mod 2^k; unusable rows are read, never checked
 *   LOOKUP  the input tuple of every usable row must equal the table tuple of some usable row.  Tuples are compared through the lookup argument's compression
 *           sum_i theta^i e_i with a theta fixed per key (Blake2b-512, personalisation "Dehalo-CheckTheta" cut to BLAKE2b's 16 bytes, over transcript_repr, reduced as
 *           a transcript challenge is): the report of a key and a witness is reproducible, and two different tuples collide with probability ~ tuple length / p.
 *           A debugging aid, not a verifier.
 *   COPY    every cell c of a permutation column, all 2^k rows, with m = mapping[c] != c: value(c) == value(m).  Each end of a broken constraint is its own failure.
 *   SHUFFLE the input tuples of the usable rows must be a permutation of the shuffle tuples of the usable rows.  Both sides are compressed with the LOOKUP check's
 *           theta and sorted; a usable row fails when its input value occurs another number of times among the inputs than on the shuffle side.  Both lists hold
 *           as many values, so no row fails exactly when the two multisets are equal; a value of the shuffle side that no input has shows through the input rows
 *           whose values it displaces.
 * The failures come ordered by (kind, index, row) ascending; the first `cap` are stored; the totals are exact however small `cap` is.  Returns 0 whenever the check
 * ran: the witness satisfies the circuit when the four totals are 0.  `failures` may be NULL when cap is 0.  DEHALO_ERR_INVALID: null ctx / pk / report, a key of
 * another device.  Allocates from the context's workspace only; everything is queued on the context's stream, which the call waits for once, before it returns.
 * Upstream's failure NAMING (gate names, region offsets, cell values) is the front-end's: it maps (kind, index, row) back through its own ConstraintSystem. */
typedef enum { DEHALO_CHECK_GATE = 0, DEHALO_CHECK_LOOKUP = 1, DEHALO_CHECK_COPY = 2, DEHALO_CHECK_SHUFFLE = 3 } dehalo_check_kind;
typedef struct { uint32_t kind, index, row, reserved; } dehalo_check_failure;
/*  GATE:   index = position in cs.gates (gates.flat_map(polynomials) order), row = the row whose polynomial is non-zero
    LOOKUP: index = lookup, row = the row whose input tuple is no row of the table
    COPY:   index = position j in cs.permutation_columns, row = i: cell (j, i) differs from the cell the mapping sends it to
    SHUFFLE: index = shuffle, row = the row whose input tuple occurs another number of times among the inputs than on the shuffle side */
/* (The struct GREW by its last two members when the shuffle argument came: a caller built against the older header passes a shorter struct and must be rebuilt.) */
typedef struct {
    uint64_t gate_failures, lookup_failures, copy_failures;   /* totals, however small `cap` is */
    uint64_t rows, lookup_inputs, cells_in_cycles;            /* what was checked: usable rows; usable rows x lookups; cells with mapping[c] != c */
    uint64_t written;                                         /* entries stored in `failures` = min(cap, total) */
    uint64_t shuffle_failures, shuffle_inputs;                /* total; usable rows x shuffles */
} dehalo_check_report;
/* Advice and instance values are words under "Non-canonical words" (1) at the top: gates and lookups are judged on the residues, and the two cells of a copy
 * constraint are equal when their words are equal mod p. */
int dehalo_check_witness(dehalo_ctx* ctx, const dehalo_pk* pk, const uint64_t* advice, const uint64_t* const* instances, const size_t* instance_lens, uint32_t num_instance_columns,
                         const uint64_t* permutation_mapping, uint32_t flags, dehalo_check_failure* failures, size_t cap, dehalo_check_report* report);
/* The same checks for a key whose expressions read challenges, under the caller's values for them: challenges = num_challenges x 4 u64 Montgomery, num_challenges =
 * the key's (dehalo_pk_phases; anything else is DEHALO_ERR_INVALID).  All advice columns, of every phase, are taken from `advice`.  dehalo_check_witness itself
 * returns DEHALO_ERR_INVALID on a key one of whose expressions holds a challenge; on a key without one the two calls are the same. */
int dehalo_check_witness_challenges(dehalo_ctx* ctx, const dehalo_pk* pk, const uint64_t* advice, const uint64_t* const* instances, const size_t* instance_lens,
                                    uint32_t num_instance_columns, const uint64_t* permutation_mapping, uint32_t flags, const uint64_t* challenges, uint32_t num_challenges,
                                    dehalo_check_failure* failures, size_t cap, dehalo_check_report* report);

/* ONE proof on several GPUs ("single-proof mode -- round-robin columns of the current phase across GPUs"): every one of `world` processes runs
 * the same dehalo_create_proof on its own GPU with the same inputs and the same seeded random stream (DEHALO_RNG_PCG64, or a callback that hands every process the
 * same scalars); of every commitment phase with more than one column (advice, permuted lookup columns, the grand products, the quotient's pieces, the openings) a
 * process runs the MSM of columns [count * rank / world, count * (rank + 1) / world) only, and `gather` -- called on the proving thread with `points` = count affine
 * points (8 u64 each, Montgomery) of which this process's own slots [first[rank], first[rank] + num[rank]) are filled -- must fill in the others (an all-gather of
 * num[r] points from process r, e.g. ncclAllGather over xGMI: at most ten points a phase) and return 0.  Every process then writes the same points to its transcript,
 * squeezes the same challenges and ends with the same proof bytes as a lone prover.  Everything that is not an MSM is computed by every process (no column travels).
 * world = 1 (or gather = NULL with world = 1) switches it off. */
typedef int (*dehalo_gather_fn)(void* user, uint64_t* points, uint32_t count, const uint32_t* first, const uint32_t* num, uint32_t world);
int dehalo_prover_set_shard(dehalo_prover* prover, uint32_t rank, uint32_t world, dehalo_gather_fn gather, void* user);
/* Host wall-clock milliseconds the last create_proof on this prover spent per phase (advice, lookups, products, random, quotient, evaluations,
 * openings, total): out[8]. */
int dehalo_prover_last_timings(const dehalo_prover* prover, double out[8]);
/* `count` proofs of the same circuit on `num_provers` provers, one host thread each (proof i -> prover i mod num_provers), no interpreter
 * in the loop: advice[i] / rngs[i] / proofs_out[i] (capacity proof_cap bytes each, length into proof_lens[i]) per proof; every proof starts
 * a fresh transcript.  Batch / throughput mode (BASELINE configs[4]). */
int dehalo_create_proofs(dehalo_prover* const* provers, uint32_t num_provers, const uint64_t* const* advice, uint32_t count, dehalo_rng* rngs, uint32_t flags,
                         uint8_t* const* proofs_out, size_t proof_cap, size_t* proof_lens);

/* ---- Circuit::synthesize of the reference's circuits, as values (csrc/witness.hip) --------------------------------------------------
 * What the reference's timed create_proof does BEFORE its first commitment: DelayEncryptCircuit::synthesize (src/lib.rs:164-318: RSA
 * time-lock x^e mod n over BigIntChip rows, Poseidon sponge of the packed result, Poseidon cipher of the message under the hash's two
 * outputs), benches/mod_pow.rs:63-110's RSACircuit (the RSA region alone) and PoseidonEncCircuit (src/encryption/chip.rs:114-204, the
 * cipher region alone) -- laid out over MainGate + RangeChip instruction by instruction the way halo2wrong lays them out (row counts: the ones the reference
 * publishes, benches/README.md:56-99; cell for cell identity with upstream's synthesize is unverified -- the crates are not in the tree), so the columns belong
 * with a key made by dehalo_keygen from THIS call's fixed columns and mapping.  The reference's circuit is satisfiable only for x < n, e < 2^exp_bits and the
 * all-zero message its benches encrypt (its in-circuit cipher adds the message twice, its native one never to the state it permutes): other inputs are refused.
 *   advice     out, 5 x 2^k x 4 u64, CANONICAL values (pass DEHALO_PROOF_ADVICE_CANONICAL to dehalo_create_proof), rows beyond the
 *              circuit zero; NULL = not wanted
 *   fixed      out, (15 | 9 for pose_enc) x 2^k x 4 u64 canonical (DEHALO_KEYGEN_FIXED_CANONICAL), range table included; NULL = not wanted
 *   mapping    out, 6 x 2^k u64: the permutation assembly for dehalo_keygen; NULL = not wanted
 *   selectors  out, two arrays of 2^k bytes (s_composition, s_overflow; none for pose_enc); NULL = not wanted
 * Per proof only `advice` is needed; the other three are keygen's.  DEHALO_ERR_INVALID when the circuit does not fit 2^k rows or a constraint cannot hold. */
typedef enum { DEHALO_CIRCUIT_DELAY_ENC = 0, DEHALO_CIRCUIT_MOD_POW = 1, DEHALO_CIRCUIT_POSE_ENC = 2 } dehalo_circuit_kind;
typedef struct {
    uint32_t circuit, k;
    uint32_t bits_len, exp_bits;        /* RSA: modulus bits (the reference's BITS_LEN = 2048; any multiple of 64 -- the RangeChip table follows compute_range_lens(bits_len / 64)), exponent bits (<= 64) */
    const uint64_t *n, *x;              /* modulus and base, bits_len / 64 limbs, little-endian */
    uint64_t e;                         /* exponent */
    const uint64_t* message; uint32_t message_len;   /* <= 2 canonical field elements (4 u64 each) */
    const uint64_t* key;                /* pose_enc: 2 canonical field elements */
    uint32_t t, rate, r_f, r_p;         /* Poseidon; 0 = the reference's (5, 4, 8, 57) */
} dehalo_circuit_inputs;
typedef struct {
    uint64_t rsa_rows, total_rows;
    uint64_t rsa_result[128];           /* x^e mod n, little-endian limbs */
    uint64_t cipher[12]; uint32_t cipher_len;   /* the ciphertext (canonical), message_len + 1 elements */
} dehalo_synthesis_info;
int dehalo_synthesize(const dehalo_circuit_inputs* in, uint64_t* advice, uint64_t* fixed, uint64_t* mapping, uint8_t* const* selectors, dehalo_synthesis_info* info);
/* create_proof of a CIRCUIT -- the call the reference makes (benches/delay_enc.rs:123-131, benches/mod_pow.rs:201-209, benches/pose_enc.rs:127-135:
 * create_proof(&params, &pk, &[circuit], instances, rng, &mut transcript) synthesizes the circuit inside): dehalo_synthesize into a page-locked buffer the
 * prover keeps, upload, and the proof; the random polynomial's draw, upload and commitment (side context) run on the otherwise idle device meanwhile.
 * Same proof bytes as dehalo_synthesize + dehalo_create_proof with DEHALO_PROOF_ADVICE_CANONICAL.  `info` (optional): rows, x^e mod n, ciphertext. */
int dehalo_create_proof_circuit(dehalo_prover* prover, const dehalo_circuit_inputs* in, dehalo_synthesis_info* info, const uint64_t* const* instances,
                                const size_t* instance_lens, uint32_t num_instance_columns, dehalo_rng* rng, dehalo_transcript* transcript);
/* dehalo_create_proofs with every proof's circuit synthesized inside its call: inputs[i] -> proof i on prover i mod num_provers, one library thread per
 * prover (witness generation of one proof runs beside the device work of the others). */
int dehalo_create_proofs_circuit(dehalo_prover* const* provers, uint32_t num_provers, const dehalo_circuit_inputs* inputs, uint32_t count, dehalo_rng* rngs,
                                 uint8_t* const* proofs_out, size_t proof_cap, size_t* proof_lens);

/* ---- verify_proof for KZG: GWC and SHPLONK, one proof or a batch (csrc/verify_host.hpp, verify.hip) ----------------------------------------------------------
 * [UPSTREAM halo2_proofs plonk/verifier.rs verify_proof::<KZGCommitmentScheme<Bn256>, VerifierGWC | VerifierSHPLONK, Challenge255, Blake2bRead, SingleStrategy |
 * AccumulatorStrategy>; benches/delay_enc.rs:147-165].  Everything the KZG prover proves is verified: N circuits in one proof, up to three advice phases with
 * challenges, lookups, shuffles, up to 32 rotations, both multiopens.  A verifier holds the verifying half of the params (g[0], g2, s_g2, k) and of the key (the
 * commitments, the constraint system, transcript_repr): no proving key, no SRS table.
 * The host reads the proof through the Blake2bRead transcript, evaluates the gate, permutation, lookup and shuffle expressions at the read evaluations and
 * reduces either multiopen to two sums L and R over the proof's points, the key's commitments and g[0]; accept iff e(L, s_g2) e(-R, g2) = 1
 * (dehalo_pairing_check's code, on the host).  With a context the points of all proofs of a call are decompressed in ONE dehalo_points_decompress_device launch and
 * the two sums are fresh-bases MSMs on the device (dehalo_best_multiexp); with ctx = NULL -- a HOST verifier, a mode the caller chooses, for machines without a
 * GPU -- both run on the host (a plain double-and-add).  It is never a fallback: a verifier made with a context reports a device error as that error.
 *
 * IPA over Pallas / Vesta [UPSTREAM plonk/verifier.rs with QUERY_INSTANCE = true, poly/ipa/multiopen/verifier.rs, poly/ipa/commitment/verifier.rs, poly/ipa/strategy.rs
 * GuardIPA / AccumulatorStrategy]: the SAME verifier type and verify calls, made by the three _ipa constructors below (the two constructors above the line keep
 * refusing ParamsIPA and the Pasta curves with DEHALO_ERR_UNSUPPORTED).  Everything the IPA prover proves is verified: phases and challenges, lookups, shuffles, up
 * to 32 rotations, committed instance columns; one circuit a proof (num_circuits != 1 is DEHALO_ERR_UNSUPPORTED, as for the prover).  The same walk reads the proof
 * -- the instance columns enter as commitments (commit_lagrange + [Blind::default()] W, every column of every proof of a call in one batch) and their evaluations are
 * read first -- and the IPA multiopen and opening argument are reduced to one term list over the proof's points, the key's and the instance commitments, g[0], U and
 * W, plus per proof its k round challenges and init = -w c.  Accept iff  (sum over the term list) + sum_idx s[idx] g[idx] = the identity,  s = sum_i compute_s(u_i, init_i):
 * with a context s is built on the device (dehalo_ipa_s_device) and summed by dehalo_msm_device over the params' resident table -- one kernel pass and one MSM over
 * g whatever the number of proofs; a host verifier (dehalo_verifier_create_ipa_host) builds s and both sums on the host.
 * Still not provided: ParamsIPA::new's hash-to-curve generators (a ParamsIPA is read, made from g, or generated by this library's own rule), and several circuits
 * in one IPA proof. */
typedef struct dehalo_verifier dehalo_verifier;
/* from objects the caller already has: g[0], g2, s_g2, k of the params; the vk half of the key (commitments, constraint system, transcript_repr) */
int dehalo_verifier_create(dehalo_ctx* ctx, const dehalo_params* params, const dehalo_pk* pk, dehalo_verifier** out);
/* ParamsVerifierKZG + VerifyingKey::read: vk bytes in any dehalo_serde_format, parsed as dehalo_keygen_pk parses them; transcript_repr = the substitute dehalo_keygen
 * gives for the same vk bytes until set.  ctx may be NULL: a HOST verifier (above). */
int dehalo_verifier_create_vk(dehalo_ctx* ctx, int curve, uint32_t k, const uint64_t g0[8], const uint8_t g2[128], const uint8_t s_g2[128],
                              const dehalo_constraint_system* cs, const uint8_t* vk_bytes, size_t vk_len, int vk_format, uint32_t num_selectors, dehalo_verifier** out);
/* Both constructors check g2 and s_g2: on the twist, in the order-r subgroup, not the identity; otherwise DEHALO_ERR_INVALID. */
/* IPA, from a ParamsIPA and a key made under it.  The params are borrowed as a prover borrows them: they must outlive the verifier.  DEHALO_ERR_INVALID for
 * ParamsKZG, a key over another curve or of another k. */
int dehalo_verifier_create_ipa(dehalo_ctx* ctx, const dehalo_params* params, const dehalo_pk* pk, dehalo_verifier** out);
/* IPA, the verifier's side: ParamsIPA::read + VerifyingKey::read, no proving key.  vk bytes in any dehalo_serde_format, read as dehalo_verifier_create_vk reads them
 * (the commitments are the blinded ones a key made under ParamsIPA holds); curve and k are the params'. */
int dehalo_verifier_create_ipa_vk(dehalo_ctx* ctx, const dehalo_params* params, const dehalo_constraint_system* cs, const uint8_t* vk_bytes, size_t vk_len, int vk_format,
                                  uint32_t num_selectors, dehalo_verifier** out);
/* IPA, a HOST verifier over points the caller holds (g, g_lagrange: 2^k affine {x, y} of 8 u64 each, standard Montgomery; w, u: one each; all copied), without a
 * context.  Every verify call costs on the order of 380 x 2^k group operations on one thread (256 doublings and about 128 additions per generator's scalar, and as
 * much again per instance value): meant for small k and for machines without a GPU.  A mode the caller chooses, never a fallback. */
int dehalo_verifier_create_ipa_host(int curve, uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, const uint64_t w[8], const uint64_t u[8],
                                    const dehalo_constraint_system* cs, const uint8_t* vk_bytes, size_t vk_len, int vk_format, uint32_t num_selectors, dehalo_verifier** out);
int dehalo_verifier_set_transcript_repr(dehalo_verifier* v, const uint64_t repr[4]);
int dehalo_verifier_set_multiopen(dehalo_verifier* v, int multiopen);      /* DEHALO_MULTIOPEN_GWC (default) | _SHPLONK; DEHALO_ERR_INVALID on an IPA verifier */
/* Where a KZG verifier's pairing checks run: DEHALO_PAIRING_ON_HOST (the default: every call is what it was before this mode existed) or DEHALO_PAIRING_ON_DEVICE
 * (dehalo_pairing_checks_device over the verifier's table of (s_g2, g2), built when the mode is first set).  On the device dehalo_verify_proof and
 * dehalo_verify_proofs make their one check through the kernel (checks = 1), and dehalo_verify_proofs_each puts EVERY live proof's (w_i L_i, -w_i R_i) through ONE
 * launch after the dehalo_msm_segments sums: each proof is checked by itself, there is no search over subsets, *checks is the number of live proofs, out[3] of
 * dehalo_verifier_last_timings is that launch, and a verdict no longer depends on the weights.  A status of NOT_ONE or OFF_CURVE is DEHALO_REJECT_PAIRING.  A mode
 * the caller switches on, never a fallback: a device error is that error.  DEHALO_ERR_INVALID for ON_DEVICE on a verifier made without a context, for an IPA
 * verifier, and for any other value. */
enum { DEHALO_PAIRING_ON_HOST = 0, DEHALO_PAIRING_ON_DEVICE = 1 };
int dehalo_verifier_set_pairing(dehalo_verifier* v, int mode);
int dehalo_verifier_release(dehalo_verifier* v);
/* Why the calling thread's last dehalo_verifier_create / _create_vk failed (a bad g2, the vk's header, a point's status, ...): a host verifier has no context
 * whose dehalo_last_error could say, and a failed constructor leaves no verifier.  The text is copied into out[0 .. cap), cut to cap - 1 bytes, NUL-terminated. */
int dehalo_verifier_create_error(char* out, size_t cap);
/* Text of the last error of a call on this verifier (a host verifier has no context to keep it); valid until the next call on it. */
const char* dehalo_verifier_last_error(const dehalo_verifier* v);
/* Where the last dehalo_verify_proof(s) call spent its time, milliseconds: out[0] point decompression, out[1] the transcript walks (hashing, expected_h, the
 * term lists), out[2] the two MSMs (IPA: the one over the term list), out[3] the pairing check (IPA: the sum over g -- kernel, MSM, download).  After
 * dehalo_verify_proofs_each: out[2] the per-proof sums (one dehalo_msm_segments call), out[3] the total of the subset checks. */
int dehalo_verifier_last_timings(const dehalo_verifier* v, double out[4]);

typedef enum {
    DEHALO_REJECT_NONE = 0, DEHALO_REJECT_MALFORMED = 1 /* a read failed, bytes missing or trailing */, DEHALO_REJECT_PAIRING = 2,
    DEHALO_REJECT_OPENING = 3 /* IPA: the proof was readable and the final sum is not the identity, x_3 hit an opening point, or a round challenge was zero */
} dehalo_reject_reason;
/* instances / instance_lens / num_instance_columns / num_circuits: dehalo_create_proof_multi's layout.  Returns 0 whenever the check ran; *accept = 1 or 0, *reason (may be
 * NULL) why not.  A wrong number of instance columns or a column longer than the usable rows is the caller's error: DEHALO_ERR_INVALID. */
int dehalo_verify_proof(dehalo_verifier* v, const uint64_t* const* instances, const size_t* instance_lens, uint32_t num_instance_columns, uint32_t num_circuits,
                        const uint8_t* proof, size_t len, int* accept, int* reason);
/* `count` proofs under one verifier (upstream's BatchVerifier / AccumulatorStrategy): every proof is read as above, then sum_i w_i L_i and sum_i w_i R_i are checked with
 * ONE pairing check.  w_0 = 1; w_1 .. w_{count-1} are the first count - 1 scalars of `rng` (NULL = DEHALO_RNG_OS), in order.  instances: proof i's circuit c's column j at
 * [(i * num_circuits + c) * num_instance_columns + j], instance_lens likewise.  *accept = 1 iff every proof was readable and the combined check holds; *first_malformed = index of the first
 * unreadable proof or -1 (a pairing failure does not say which proof: dehalo_verify_proofs_each below does).  With a context: all proofs' points in one decompress launch, the term lists
 * concatenated into one MSM pair.
 * THE WEIGHTS MUST BE UNPREDICTABLE TO WHOEVER MADE THE PROOFS: someone who knows w_i before choosing the proofs can make invalid proofs whose errors cancel in the
 * weighted sums (two copies of one invalid proof under w_1 = -1 pass).  Use DEHALO_RNG_OS (rng = NULL) outside tests. */
int dehalo_verify_proofs(dehalo_verifier* v, const uint8_t* const* proofs, const size_t* lens, uint32_t count, const uint64_t* const* instances, const size_t* instance_lens,
                         uint32_t num_instance_columns, uint32_t num_circuits, dehalo_rng* rng, int* accept, int64_t* first_malformed);
/* A verdict PER PROOF from one batch verification: what a verifier of untrusted proofs needs, since whoever submits one invalid proof otherwise turns a batch call
 * into `count` single calls.  Arguments, argument errors and the weights' draw are dehalo_verify_proofs's (w_0 = 1, the rest from `rng`, NULL = DEHALO_RNG_OS), and so is
 * the warning: THE WEIGHTS MUST BE UNPREDICTABLE TO WHOEVER MADE THE PROOFS -- under known weights invalid proofs can cancel each other and all be reported valid.
 *   reasons   count x int, a dehalo_reject_reason each: DEHALO_REJECT_NONE for a valid proof, otherwise what dehalo_verify_proof says of that proof alone
 *             (MALFORMED; PAIRING under KZG; OPENING under IPA).  May be NULL only when count = 0
 *   checks    optional: the number of subset checks made (KZG: pairing checks; IPA: sums over g)
 * Every proof is read ONCE, as in the batch call.  Proofs the read rejects (MALFORMED, or IPA's OPENING for x_3 at an opening point or a zero round challenge) get
 * their reason there and take no part in what follows.  One dehalo_msm_segments launch then sums each remaining proof's weighted term lists apart (w_i L_i and w_i R_i;
 * IPA: the weighted sum over the fresh bases), a subset's sums are point additions on the host, and a search over subsets names the proofs that fail (csrc/blame_search.hpp:
 * a set that fails and whose first half passes has its second half bad without a check of it): 0 checks when no proof is left, 1 when all of them are valid, at most
 * 1 + 2 b ceil(log2 n) for b >= 1 invalid among n -- 13 for one invalid proof among 64, 127 when all 64 are invalid.  Two copies of one invalid proof are both named.
 * A check is one pairing check on the host (KZG) or one dehalo_ipa_s_device + MSM over g (IPA; a host verifier: 2^k group operations each).
 * Returns 0 whenever the checks ran; on an error `reasons` and `checks` are not written.  dehalo_verifier_last_timings: out[2] the dehalo_msm_segments call, out[3] the
 * total of the subset checks.  dehalo_verify_proof and dehalo_verify_proofs are what they were.  A KZG verifier switched to DEHALO_PAIRING_ON_DEVICE
 * (dehalo_verifier_set_pairing above) makes no search: every live proof gets its own check in one launch, and *checks is the number of live proofs. */
int dehalo_verify_proofs_each(dehalo_verifier* v, const uint8_t* const* proofs, const size_t* lens, uint32_t count, const uint64_t* const* instances,
                              const size_t* instance_lens, uint32_t num_instance_columns, uint32_t num_circuits, dehalo_rng* rng, int* reasons, uint32_t* checks);
/* The IPA opening argument's check alone, the counterpart of dehalo_ipa_open: *accept = 1 iff `proof` (S, the k rounds' L_j, R_j, then c and f: 32 (2 k + 3) bytes,
 * read through a fresh transcript) opens `commitment` (affine {x, y}, standard Montgomery) to v at x3 (4 x u64 Montgomery each) under the ParamsIPA `params`.  The
 * reduction is the whole proof's; the two sums run on the device.  Returns 0 whenever the check ran. */
int dehalo_ipa_verify(dehalo_ctx* ctx, const dehalo_params* params, const uint64_t commitment[8], const uint64_t x3[4], const uint64_t v[4], const uint8_t* proof, size_t len,
                      int* accept);

/* The grand products' per-row factors, every product of a proof in one launch [UPSTREAM plonk/permutation/prover.rs Argument::commit:
 * per set of columns  den = prod_j (value_j + beta sigma_j + gamma),  num = prod_j (value_j + delta^j beta omega^i + gamma);
 * plonk/lookup/prover.rs Permuted::commit_product:  den = (a' + beta)(s' + gamma),  num = (A + beta)(S + gamma)] over the `n` rows of the
 * ORIGINAL domain.  Product p (permutation sets first, then lookups) is written to d_num / d_den + p * stride_elems; all columns and
 * results in upstream's standard form: the inputs of dehalo_grand_product_batch_device. */
typedef struct {
    const uint64_t* const* columns; const uint64_t* const* sigma; uint32_t num_columns, chunk_len;   /* the permutation's columns (values) and sigma_j values */
    const uint64_t* omega_powers;                    /* device column: omega^i */
    const uint64_t *beta, *gamma, *delta;            /* host, 4 u64 each */
    const uint64_t* set_factors;                     /* host, one per set: beta * delta^(chunk_len * set) */
    const uint64_t* const* compressed_input; const uint64_t* const* compressed_table;     /* per lookup: A, S (theta-compressed) ... */
    const uint64_t* const* permuted_input; const uint64_t* const* permuted_table;         /* ... a', s' */
    uint32_t num_lookups;
} dehalo_product_inputs;
int dehalo_product_terms_device(dehalo_ctx* ctx, int field, const dehalo_product_inputs* in, size_t n, uint64_t* d_num, uint64_t* d_den, size_t stride_elems, void* stream);

/* ---- measurement ---------------------------------------------------------------------------
 * Per-kernel device time measured with HIP events on the launching stream (bench.py's
 * roofline leg).  kernel ids: see dehalo_kernel_id.                                          */
typedef enum {
    DEHALO_K_MSM_ACCUMULATE = 0, /* bucket accumulation (the dominant MSM kernel) */
    DEHALO_K_MSM_SORT = 1,       /* digit histogram + scatter                       */
    DEHALO_K_MSM_REDUCE = 2,     /* partial merge + bucket reduction                */
    DEHALO_K_NTT_PASS = 3,       /* all NTT passes of one transform                 */
    DEHALO_K_POLY = 4,           /* eval_polynomial / batch_invert / prefix product */
    DEHALO_K_EVAL_H = 5,         /* quotient-numerator kernels (graph, permutation, lookup) */
    DEHALO_K_COUNT = 6
} dehalo_kernel_id;
int dehalo_timing_enable(dehalo_ctx* ctx, int on);
int dehalo_timing_reset(dehalo_ctx* ctx);
/* Synchronises the context, then returns total milliseconds and number of timed regions. */
int dehalo_timing_get(dehalo_ctx* ctx, int kernel_id, double* total_ms, uint64_t* count);

/* Shape of the context's most recent MSM launch, for tuning (synchronises): out[0..3] = buckets whose partial sums were merged by one
 * lane or quad / 32 lanes / one wave / a whole block, out[4] = points per lane of the accumulation, out[5] = (bucket, point) pairs sorted. */
int dehalo_msm_last_shape(dehalo_ctx* ctx, uint32_t out[6]);

/* The host-side constants of a field as the library computed them (4 x u64 Montgomery each): out[0] = modulus (plain integer), out[1] = R mod p (one),
 * out[2] = ROOT_OF_UNITY, out[3] = ZETA, out[4] = DELTA, out[5] = MULTIPLICATIVE_GENERATOR [UPSTREAM halo2curves / pasta_curves PrimeField, WithSmallOrderMulGroup]. */
int dehalo_field_info(int field, uint64_t out[24]);

/* Library / build info, e.g. "dehalo 0.1 gfx950". */
const char* dehalo_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DEHALO_H */
