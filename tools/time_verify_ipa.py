"""Times verify_proof for IPA on one MI355X: a native maingate proof (range lookups) over Vesta at k = 14 and k = 17 -- one proof on the device verifier with
its four timing slots (point decompression, the transcript walk, the fresh-bases MSM, the sum over g), the per-proof time in batches of 8 and 64 (one
dehalo_verify_proofs call each) -- beside the same commit's create_proof of that proof and the oracle's verify_proof_ipa (Python integers) on it in the same run.
Then the kernel alone (dehalo_ipa_s_device, 2^17 outputs at count 1 and 64) beside the MSM over g it feeds (dehalo_params_commit_device over the same 2^17
scalars): the number that says whether the kernel matters.  Upstream's Rust verifier cannot be run here.

One process; whole host calls through ctypes on the host clock after one warm-up call, the device drained before the clock is read.  Needs a gfx950 device: no
fallback.  No threshold is attached to these figures: DESIGN.md section 6 quotes them.

    python tools/time_verify_ipa.py [out file, default profiles/verify_ipa_times.txt]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "verify_ipa_times.txt")
import __graft_entry__ as entry      # noqa: E402

pkg = entry.load_package()
po, co = entry.load_oracle()
import ipa      # noqa: E402
import verifier as V      # noqa: E402
from dehalo2_amd import circuits, native, prover      # noqa: E402

F = pkg.fields
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def timed_verify(call, verifier, runs, per=1):
    """-> 'wall (split)' of `runs` calls after one warm-up: medians, milliseconds, divided by `per`"""
    assert call() is True
    wall, split = [], []
    for _ in range(runs):
        t = time.perf_counter()
        ok = call()
        wall.append(1e3 * (time.perf_counter() - t))
        assert ok is True
        split.append(verifier.last_timings())
    parts = {name: median([s[name] for s in split]) / per for name in ("walk", "decompress", "msm", "g_sum")}
    return "%9.3f ms  (decompress %7.3f  walk %8.3f  fresh-bases msm %7.3f  sum over g %7.3f; %d runs, medians)" % (
        median(wall) / per, parts["decompress"], parts["walk"], parts["msm"], parts["g_sum"], runs)


def timed_device(ctx, call, reps):
    """median milliseconds of one call, the device drained around it"""
    call()
    ctx.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ctx.synchronize()
        out.append(1e3 * (time.perf_counter() - t))
    return median(out)


say("# one MI355X, one process; whole host calls through ctypes on the host clock, one warm-up call each; maingate with range lookups over Vesta (IPA)")
spec, curve = F.VESTA, po.VESTA
with pkg.Context(0) as ctx:
    for K in (14, 17):
        circ = circuits.synthesize(curve.scalar.p, K, True, seed=3)
        n = 1 << K
        pts = co.fixed_base_mul(po.CURVE_IDS["vesta"], co.fill_scalars(po.FIELD_IDS[curve.scalar.name], "uniform", n + 2, 7))
        g, w, u = pts[2:], pts[1], pts[0]
        params = native.ParamsIPA.from_g(ctx, spec, K, g, w, u)
        pk = native.ProvingKey.keygen(ctx, params, circ.cs, circ.fixed, circ.assembly, circ.selectors)
        inst = [[] for _ in range(circ.cs.num_instance)]
        P = native.Prover(params, pk)
        P.create_proof(circ.advice, inst, prover.KeyedRng(b"\x01" * 32), canonical=True)      # warm
        t_prove = []
        for i in range(5):
            ctx.synchronize()
            t = time.perf_counter()
            proof = P.create_proof(circ.advice, inst, prover.KeyedRng(bytes([i + 2]) * 32), canonical=True).finalize()
            t_prove.append(1e3 * (time.perf_counter() - t))
        say("k = %d: proof of %d bytes" % (K, len(proof)))
        dev = native.Verifier.from_ipa(params, pk)
        say("  one proof, device verifier          " + timed_verify(lambda: dev.verify(proof, inst), dev, 9))
        for B in (8, 64):
            batch = [P.create_proof(circ.advice, inst, prover.KeyedRng(bytes([100 + i]) * 32), canonical=True).finalize() for i in range(B)]
            insts = [[inst]] * B
            say("  batch of %2d, device, per proof      " % B + timed_verify(lambda: dev.verify_batch(batch, insts, num_circuits=1), dev, 5, B))
            bad = bytearray(batch[B // 2])
            bad[len(bad) - 40] ^= 1
            assert dev.verify_batch(batch[:B // 2] + [bytes(bad)] + batch[B // 2 + 1:], insts, num_circuits=1) is False and dev.verify(bytes(bad), inst) is False
        vk, nf = pk.vk_bytes(), circ.cs.num_fixed
        ncm = (len(vk) - 8 - len(circ.selectors) * (n // 8)) // 64
        cms = [ipa.dec_point(curve, np.frombuffer(vk[8 + 64 * i:8 + 64 * i + 64], dtype=np.uint64)) for i in range(ncm)]
        t = time.perf_counter()      # (the instance column holds no value: g_lagrange is not read, g stands in for it)
        ok = V.verify_proof_ipa(curve, circ.cs.description(), K, cms[:nf], cms[nf:], pk.transcript_repr, g, g, u, w, inst, proof)
        t_oracle = 1e3 * (time.perf_counter() - t)
        assert ok is True
        say("  the oracle's verifier, same proof   %9.3f ms  (Python integers and the C restatement's multiexp; one run)" % t_oracle)
        say("  create_proof, same commit           %9.3f ms  (median of 5, advice on the host)" % median(t_prove))
        if K == 17:
            import torch
            lib = pkg.load_library()
            out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
            aff = torch.zeros((1, 8), dtype=torch.int64, device="cuda")
            for count in (1, 64):
                ch = ctx.upload(co.fill_scalars(po.FIELD_IDS[curve.scalar.name], "uniform", count * K, 11))
                ini = ctx.upload(co.fill_scalars(po.FIELD_IDS[curve.scalar.name], "uniform", count, 12))
                ms = timed_device(ctx, lambda: ctx.ipa_s_device(spec.id, ch.data_ptr(), ini.data_ptr(), count, K, out.data_ptr()), 20)
                say("  dehalo_ipa_s_device, 2^17 outputs, count = %2d   %7.3f ms  (two launches; median of 20, host clock, device drained)" % (count, ms))
            ms = timed_device(ctx, lambda: ctx._check(lib.dehalo_params_commit_device(ctx.handle, params.handle, out.data_ptr(), 1, 0, aff.data_ptr(), None)), 20)
            say("  the MSM over g it feeds, 2^17 scalars           %7.3f ms  (dehalo_params_commit_device on the kernel's output; median of 20)" % ms)
        dev.release(); P.release(); pk.release(); params.release()
say("# upstream's Rust verifier (halo2_proofs verify_proof with VerifierIPA) cannot be built or run here: no figure for it")

with open(OUT, "w") as fh:
    fh.write("\n".join(lines) + "\n")
