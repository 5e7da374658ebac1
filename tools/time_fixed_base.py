"""Times the fixed-base table path (csrc/fixed_base.cuh) on Vesta: the blinding kernel against the one it replaces, the table's one-time cost, and
whole ProverIPA proofs by phase.

    python tools/time_fixed_base.py kernels [--counts 1 8 32] [--reps 5]
        dehalo_blind_commitments_device (k_ipa_blind) against dehalo_fixed_base_blind_device over the same points and blinds: a warm-up of each,
        then `reps` alternating pairs between device events on the context's stream, the median of each reported; then the table build alone
        (dehalo_fixed_base_create between the same events) and dehalo_params_ipa_create as a whole at two sizes (host clock: the call is synchronous).
    python tools/time_fixed_base.py proof --k 14 17 [--proofs 10] [--warmup 3]
        whole proofs of the delay_enc shape (MainGate with range lookups) with a warm prover and a side context: every phase of last_timings() and the
        total, the median of `proofs` proofs after `warmup`.  The A/B of two trees: a copy of this file in the other tree's tools/, alternating processes.

Every mode prints one JSON line per row.  Needs a gfx950 device: no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def event_ms(ctx, fn):
    import torch
    st = ctx.torch_stream_obj()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def points_on_device(ctx, cs, co, count, seed):
    """`count` Jacobian points as an MSM leaves them and as many blinds, both on the device; W on the host and on the device"""
    r = cs.scalar.p
    rng = np.random.default_rng(seed)
    bases = co.synth_bases(cs.id, 3)
    jac = np.stack([co.best_multiexp(cs.id, cs.scalar.encode_many([int.from_bytes(rng.bytes(32), "little") % r for _ in range(2)]), bases[:2], 1) for _ in range(count)])
    blinds = cs.scalar.encode_many([int.from_bytes(rng.bytes(32), "little") % r for _ in range(count)])
    return ctx.upload(jac.reshape(count, 12)), ctx.upload(blinds), bases[2], ctx.upload(bases[2].reshape(1, 8))


def kernels(a):
    pkg = entry.load_package()
    _, co = entry.load_oracle()
    cs = pkg.fields.VESTA
    with pkg.Context(0) as ctx:
        for count in a.counts:
            d, b, w, dw = points_on_device(ctx, cs, co, count, 7 + count)
            fb = ctx.fixed_base(cs.id, w)
            # (both kernels work in place: each timed call blinds the previous call's output again, a point as generic as the first)
            old = lambda: ctx.blind_commitments_device(cs.id, d.data_ptr(), b.data_ptr(), count, dw.data_ptr())
            new = lambda: fb.blind_device(d.data_ptr(), b.data_ptr(), count)
            old(); new()
            ctx.synchronize()                                  # warm-up: code objects loaded
            t_old, t_new = [], []
            for _ in range(a.reps):
                t_old.append(event_ms(ctx, old))
                t_new.append(event_ms(ctx, new))
            print(json.dumps({"count": count, "k_ipa_blind_ms": round(float(np.median(t_old)), 4), "fixed_base_blind_ms": round(float(np.median(t_new)), 4),
                              "ratio": round(float(np.median(t_old) / np.median(t_new)), 1), "k_ipa_blind_ms_all": [round(x, 4) for x in t_old],
                              "fixed_base_blind_ms_all": [round(x, 4) for x in t_new]}), flush=True)
            fb.release()
        # the one-time cost: the table alone, then the params that own one
        w = co.synth_bases(cs.id, 3)[2]
        ctx.fixed_base(cs.id, w).release()
        ms = []
        for _ in range(a.reps):
            box = []
            ms.append(event_ms(ctx, lambda: box.append(ctx.fixed_base(cs.id, w))))
            box[0].release()
        print(json.dumps({"table_build_ms": round(float(np.median(ms)), 3), "table_build_ms_all": [round(x, 3) for x in ms]}), flush=True)
        from dehalo2_amd import native
        for k in a.params_k:
            g, uw = srs_points(ctx, cs, co, k)
            native.ParamsIPA.from_g(ctx, cs, k, g, uw[1], uw[0]).release()
            gl = g                                             # (any 2^k points do for the timing: the call registers them as they are)
            ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                p = native.ParamsIPA.create(ctx, cs, k, g, gl, uw[1], uw[0])
                ms.append(1e3 * (time.perf_counter() - t0))
                p.release()
            print(json.dumps({"k": k, "params_ipa_create_ms": round(float(np.median(ms)), 3), "params_ipa_create_ms_all": [round(x, 3) for x in ms]}), flush=True)


def srs_points(ctx, cs, co, k):
    """2^k distinct non-identity points (the transform of (G, 2 G, O, ...): tools/time_g_to_lagrange.py) on the host, and (u, w)"""
    b = cs.base
    G = (b.p - 1, 2)
    lam = 3 * G[0] * G[0] * pow(2 * G[1], -1, b.p) % b.p
    x2 = (lam * lam - 2 * G[0]) % b.p
    G2 = (x2, (lam * (G[0] - x2) - G[1]) % b.p)
    seed = np.zeros((1 << k, 8), dtype=np.uint64)
    for i, P in enumerate((G, G2)):
        seed[i, :4], seed[i, 4:] = b.encode(P[0]), b.encode(P[1])
    d = ctx.upload(seed)
    ctx.g_to_lagrange(cs.id, d.data_ptr(), k)
    g = ctx.download_tensor(d)
    return g, co.fixed_base_mul(cs.id, co.fill_scalars(cs.scalar.id, "uniform", 2, 7))


def proof(a):
    pkg = entry.load_package()
    _, co = entry.load_oracle()
    from dehalo2_amd import circuits, keygen, native, prover
    cs = pkg.fields.VESTA
    with pkg.Context(0) as ctx, pkg.Context(0) as side:
        for k in a.k:
            circ = circuits.synthesize(cs.scalar.p, k, True, seed=3)
            g, uw = srs_points(ctx, cs, co, k)
            params = native.ParamsIPA.from_g(ctx, cs, k, g, uw[1], uw[0])
            pk = native.ProvingKey.keygen(ctx, params, circ.cs, circ.fixed, circ.assembly, circ.selectors)
            with ctx.torch_stream():
                advice = keygen.to_device(circ.advice)
                ctx.field_op_device(cs.scalar.id, "to_mont", advice.data_ptr(), 0, advice.data_ptr(), advice.numel() // 4, 0)
            ctx.synchronize()
            P = native.Prover(params, pk, ctx, side)
            rows = []
            for i in range(a.warmup + a.proofs):
                P.create_proof(advice, [[]], prover.SeededRng(100 + i)).finalize()
                if i >= a.warmup:
                    rows.append(P.last_timings())
            med = {ph: round(float(np.median([r[ph] for r in rows])), 3) for ph in native.PHASES}
            print(json.dumps({"k": k, "proofs": a.proofs, "median_ms": med,
                              "total_ms_all": [round(r["total"], 3) for r in rows]}), flush=True)
            P.release(); pk.release(); params.release()


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("--counts", type=int, nargs="+", default=[1, 8, 32])
    k.add_argument("--reps", type=int, default=5)
    k.add_argument("--params-k", type=int, nargs="+", default=[10, 14])
    p = sub.add_parser("proof")
    p.add_argument("--k", type=int, nargs="+", default=[14, 17])
    p.add_argument("--proofs", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    kernels(a) if a.mode == "kernels" else proof(a)


if __name__ == "__main__":
    main()
