// ipa_open.hip -- the IPA opening argument behind the C ABI: commitment::create_proof of ParamsIPA [UPSTREAM halo2_proofs @ v2023_04_20:
// poly/ipa/commitment/prover.rs] -- dehalo_ipa_open, and through ipa_open_body the last step of a ProverIPA proof (prover.hip).  The params it reads
// (d_guw, bases_uw, fb_w): params.hip.
// The C entry point runs under dh_guard and the column work goes through the library's device entry points, as in prover.hip; no kernel is defined here.
#include "whole_call.hpp"

namespace {

// commit(poly, blind) of ParamsIPA = MSM(poly, g) + [blind] W, affine into d_pts[0 .. 8) (d_pts: 8 field elements of scratch = 32 u64; the Jacobian
// result sits in [8, 20), the blind in [20, 24)): the MSM, [blind] W from W's table on top of it, one normalisation -- all on the stream
int ipa_commit_blinded(dehalo_ctx* ctx, const dehalo_params* p, const uint64_t* d_poly, const Fe& blind, uint64_t* d_pts, hipStream_t s) {
    TRY(dh_h2d(ctx, d_pts + 20, blind.v, 32, s));
    TRY(dehalo_msm_device(ctx, p->bases_g.get(), d_poly, p->n, 1, d_pts + 8, s));
    TRY(dehalo_fixed_base_blind_device(ctx, p->fb_w.get(), d_pts + 8, d_pts + 20, 1, s));
    return dehalo_to_affine_device(ctx, p->curve, d_pts + 8, 1, d_pts, s);
}

}   // namespace

// commitment::create_proof on `rng` as it stands (dehalo_ipa_open: a fresh generator; a whole proof: the proof's generator, right behind f's blind).
// cha_stream: the ChaCha20 stream of the n-scalar draw under the ChaCha20 kinds -- within one proof it must differ from the random polynomial's (1).
int ipa_open_body(dehalo_ctx* ctx, const dehalo_params* p, const uint64_t* d_poly, const Fe& blind, const Fe& x3, HostRng& rng, uint64_t cha_stream, dehalo_transcript* t) {
        const hipStream_t s = ctx->stream.get();
        const int fid = curve_scalar_field(p->curve);
        const HostField* f = host_field(fid);
        const IpaOps* ops = ipa_ops(p->curve);
        const size_t n = p->n;
        const uint32_t k = p->k;
        DevMem s_poly, s_adj, pa, pb, guw, sc, ev, rr, pts, uwsc;
        TRY(s_poly.alloc(ctx, n, false));
        TRY(s_adj.alloc(ctx, n, false));
        TRY(pa.alloc(ctx, n, false));
        TRY(pb.alloc(ctx, n, false));
        TRY(guw.alloc(ctx, n + 4, false));           // G' of rounds 2.., then U, W: n / 2 + 2 points of 2 elements
        TRY(sc.alloc(ctx, 2 * n, false));
        TRY(ev.alloc(ctx, 2, false));
        TRY(rr.alloc(ctx, 2 * (size_t)k, false));
        TRY(pts.alloc(ctx, 8, false));
        TRY(uwsc.alloc(ctx, 4, false));
        // ---- draws, in upstream's order: s_poly (n), s_poly_blind, (l_rand, r_rand) per round.  The n scalars are the proof's large draw and come, as
        // the prover's random polynomial does, from the generator forked at their position: for the ChaCha20 kinds a ChaCha20 kernel under the call's key
        // (stream 1); for PCG64 / a callback the fork yields exactly the scalars a serial draw would, drawn on the host and uploaded.
        HostRng rng_poly = rng.fork(0, cha_stream);
        rng.skip(n);
        Fe s_blind;
        std::vector<uint64_t> rands(8 * (size_t)k);
        TRY(rng.scalars(s_blind.v, 1));
        TRY(rng.scalars(rands.data(), 2 * (size_t)k));
        if (rng.chacha()) TRY(chacha_scalars_device(ctx, rng, cha_stream, s_poly.p, n, s));
        else {
            std::vector<uint64_t> s_host(4 * n);
            TRY(rng_poly.scalars(s_host.data(), n));
            TRY(dh_h2d(ctx, s_poly.p, s_host.data(), 32 * n, s));
        }
        TRY(dh_h2d(ctx, rr.p, rands.data(), 64 * (size_t)k, s));
        // ---- s(x3) and p(x3); s_poly[0] -= s(x3)
        TRY(dehalo_eval_polynomial_device(ctx, fid, s_poly.u64(), n, n, 1, x3.v, ev.u64(0), s));
        TRY(dehalo_eval_polynomial_device(ctx, fid, d_poly, n, n, 1, x3.v, ev.u64(1), s));
        Fe at[2];
        TRY(dehalo_download(ctx, ev.p, 64, at));
        const uint64_t* one_col[1] = {s_poly.u64()};
        TRY(dehalo_lincomb_device(ctx, fid, one_col, f->one.v, 1, n, s_adj.u64(), at[0].v, s));
        // ---- S = commit(s_poly, s_poly_blind)
        TRY(ipa_commit_blinded(ctx, p, s_adj.u64(), s_blind, pts.u64(), s));
        uint64_t S[8];
        TRY(dehalo_download(ctx, pts.p, 64, S));
        if (!t->write_point(S)) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_open: s_poly commitment at infinity");
        const Fe xi = t->squeeze();
        const Fe z = t->squeeze();
        // ---- p' = p + xi s, p'[0] -= p'(x3) (= p(x3): s(x3) = 0 now); f = s_poly_blind xi + blind
        {
            const uint64_t* cols[2] = {d_poly, s_adj.u64()};
            Fe coefs[2] = {f->one, xi};
            TRY(dehalo_lincomb_device(ctx, fid, cols, coefs[0].v, 2, n, pa.u64(), at[1].v, s));
        }
        Fe fsum = f->add(f->mul(s_blind, xi), blind);
        // ---- k rounds; b stays geometric: b^(j)[i] = c_j x3^i.  Round 1 runs over the resident precomputed table of g (its [U | W] terms over
        // bases_uw, added by a collapse with u = 1); rounds 2.. over one plain registration of [G' | U | W], rebuilt on the stream each round.
        BasesPtr breg;
        TRY(dh_bases_plain_alloc(ctx, p->curve, n / 2 + 2, breg));
        std::vector<Fe> x3_pow(k + 1);           // x3^(2^i)
        x3_pow[0] = x3;
        for (uint32_t i = 1; i <= k; i++) x3_pow[i] = f->sqr(x3_pow[i - 1]);
        Fe c = f->one;
        DevMem* cur = &pa;
        DevMem* nxt = &pb;
        for (uint32_t j = 0; j < k; j++) {
            const size_t nj = n >> j, half = nj / 2, m = j == 0 ? nj : nj + 2;
            const Fe x3h = x3_pow[k - 1 - j];                  // x3^half
            // scalars: L = [p'_hi | 0 | z value_l | l_rand], R = [0 | p'_lo | z value_r | r_rand] (round 1: the [U | W] slots in uwsc)
            fe* sl = sc.at(0);
            fe* sr = sc.at(m);
            HIP_TRY(ctx, hipMemcpyAsync(sl, cur->at(half), 32 * half, hipMemcpyDeviceToDevice, s));
            HIP_TRY(ctx, hipMemsetAsync(sl + half, 0, 32 * half, s));
            HIP_TRY(ctx, hipMemsetAsync(sr, 0, 32 * half, s));
            HIP_TRY(ctx, hipMemcpyAsync(sr + half, cur->p, 32 * half, hipMemcpyDeviceToDevice, s));
            TRY(dehalo_eval_polynomial_device(ctx, fid, cur->u64(), half, half, 2, x3.v, ev.u64(), s));      // p'_lo(x3), p'_hi(x3)
            const Fe zc = f->mul(z, c), zch = f->mul(zc, x3h);
            if (j == 0) {
                TRY(ops->slots(ctx, ev.p, zc.v, zch.v, rr.at(0), uwsc.at(0), uwsc.at(2), s));
                TRY(dehalo_msm_device_affine(ctx, p->bases_g.get(), sc.u64(), n, 2, nullptr, pts.u64(0), s));       // L_g, R_g
                TRY(dehalo_msm_device_affine(ctx, p->bases_uw.get(), uwsc.u64(), 2, 2, nullptr, pts.u64(4), s));    // L_uw, R_uw (points 2, 3)
                const uint64_t one_m[4] = {f->one.v[0], f->one.v[1], f->one.v[2], f->one.v[3]};
                TRY(dehalo_generator_collapse_device(ctx, p->curve, pts.u64(), 4, one_m, pts.u64(), s));      // [L_g + L_uw, R_g + R_uw]
            } else {
                TRY(ops->slots(ctx, ev.p, zc.v, zch.v, rr.at(2 * j), sl + nj, sr + nj, s));
                HIP_TRY(ctx, hipMemcpyAsync(guw.at(2 * nj), p->d_guw.at(2 * n), 128, hipMemcpyDeviceToDevice, s));     // U, W behind G'
                TRY(dh_bases_plain_rebuild(ctx, breg.get(), (const affine_t*)guw.p, m, s));
                TRY(dehalo_msm_device_affine(ctx, breg.get(), sc.u64(), m, 2, nullptr, pts.u64(), s));
            }
            uint64_t LR[16];
            TRY(dehalo_download(ctx, pts.p, 128, LR));      // the round's one host wait
            if (!t->write_point(LR) || !t->write_point(LR + 8)) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_open: L_j or R_j at infinity");
            const Fe u = t->squeeze();
            const Fe u_inv = f->invert(u);
            Fe lr, rrnd;
            memcpy(lr.v, &rands[8 * j], 32);
            memcpy(rrnd.v, &rands[8 * j + 4], 32);
            fsum = f->add(fsum, f->add(f->mul(lr, u_inv), f->mul(rrnd, u)));
            c = f->mul(c, f->add(f->one, f->mul(u, x3h)));
            // p' <- p'_lo + u^-1 p'_hi (into the other buffer: lincomb's out may alias no column); G' <- G'_lo + [u] G'_hi (round 1 reads g, later
            // rounds collapse in place; the last round's G' would never be read)
            const uint64_t* cols[2] = {cur->u64(), cur->u64(half)};
            Fe coefs[2] = {f->one, u_inv};
            TRY(dehalo_lincomb_device(ctx, fid, cols, coefs[0].v, 2, half, nxt->u64(), nullptr, s));
            if (j + 1 < k) TRY(dehalo_generator_collapse_device(ctx, p->curve, j == 0 ? p->d_guw.u64() : guw.u64(), nj, u.v, guw.u64(), s));
            std::swap(cur, nxt);
        }
        Fe cfin;
        TRY(dehalo_download(ctx, cur->p, 32, cfin.v));
        t->write_scalar(cfin);
        t->write_scalar(fsum);
        return 0;
}

extern "C" int dehalo_ipa_open(dehalo_ctx* ctx, const dehalo_params* p, const uint64_t* d_poly, const uint64_t blind_in[4], const uint64_t x3_in[4], dehalo_rng* rng_in,
                               dehalo_transcript* t) {
    return dh_guard(ctx, [&]() -> int {
        if (!ctx || !p || !d_poly || !blind_in || !x3_in || !t) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_open: null argument");
        if (p->scheme != DEHALO_SCHEME_IPA) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_open: needs ParamsIPA (dehalo_params_ipa_create)");
        if (t->curve != p->curve) return dh_fail(ctx, DEHALO_ERR_INVALID, "ipa_open: transcript and params disagree on the curve");
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        (void)hipSetDevice(ctx->device);
        Fe blind, x3;
        memcpy(blind.v, blind_in, 32);
        memcpy(x3.v, x3_in, 32);
        HostRng rng;
        TRY(rng.init(rng_in, host_field(curve_scalar_field(p->curve))));
        TRY(ipa_open_body(ctx, p, d_poly, blind, x3, rng, 1, t));
        rng.write_back(rng_in);
        return 0;
    });
}
