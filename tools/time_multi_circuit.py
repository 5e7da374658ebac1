"""Times one proof over N circuits (dehalo_create_proof_multi) against batch mode's N proofs (dehalo_create_proofs) of the PARENT commit's build, and the single
proof (dehalo_create_proof) of both builds against each other.

    python tools/time_multi_circuit.py [--parent tools/ab/parent] [--k 17] [--ns 1,2,4,8] [--pairs 5] [--reps 6] [--out profiles/multi_circuit_times.txt]

The parent's tree is made as tools/ab_parent.sh says (`git archive HEAD~ | tar -x -C tools/ab/parent`, then `make` in it).  This process never opens the device: it
starts one worker process per leg, alternating (parent, this) `pairs` times, each with its own time limit; the first failure ends the run.  A worker imports the
package of ITS tree, builds the bench's k = 17 delay_enc witness through dehalo_synthesize, the SRS and the key once, then per measurement makes 2 warm-up calls
and `reps` timed ones: host clock around the whole call, which returns the proof's bytes -- every stream has been waited for by then.  Legs:

    single   native.Prover(ctx, side).create_proof                                               both builds
    batch    native.create_proofs of N proofs on min(N, 4) provers (one context each, as bench.py's batch mode)      both builds; the parent's is the comparison
    multi    native.Prover(ctx, side, num_circuits=N).create_proof_multi over N copies of the witness               this build

Medians per worker, then the median and the spread (max - min) over the `pairs` workers of a build.  No thresholds.  Needs a gfx950 device: no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(root, k, ns, reps, multi):
    import random

    import numpy as np
    sys.path.insert(0, root)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    from dehalo2_amd import native, plonk, prover, witness as W
    rnd = random.Random(2048)
    n_big, x = rnd.getrandbits(2048) | (1 << 2047) | 1, rnd.getrandbits(2000)
    tail = W.hash_region_rows() + W.cipher_region_rows(2, True)
    bits = max(b for b in range(1, 16) if W.rsa_region_rows(b) + tail + 1 <= (1 << k) - 6)
    e = rnd.getrandbits(bits) | (1 << (bits - 1))
    nat = native.synthesize(native.CIRCUIT_DELAY_ENC, k, n_big=n_big, e=e, x=x, exp_bits=bits, message=[0, 0], keygen=True)
    cs = plonk.maingate_cs(True)
    asm = plonk.Assembly(6, 1 << k)
    asm.mapping = nat["mapping"].astype(np.int64)
    out = {}

    def timed(fn):
        for _ in range(2):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ts), 3)

    with pkg.Context(0) as ctx, pkg.Context(0) as side:
        params = native.ParamsKZG.setup(ctx, pkg.fields.BN254, k, 0x5EED)
        pk = native.ProvingKey.keygen(ctx, params, cs, nat["fixed"], asm, nat["selectors"])
        adv = ctx.upload(np.ascontiguousarray(nat["advice"]))
        P = native.Prover(params, pk, ctx, side)
        out["single_ms"] = timed(lambda: P.create_proof(adv, [[]], prover.SeededRng(7), canonical=True))
        out["single_bytes"] = len(P.create_proof(adv, [[]], prover.SeededRng(7), canonical=True).finalize())
        P.release()
        for N in ns:
            if multi:
                PM = native.Prover(params, pk, ctx, side, num_circuits=N)
                out["multi_ms_%d" % N] = timed(lambda: PM.create_proof_multi([adv] * N, [[[]]] * N, prover.SeededRng(7), canonical=True))
                out["multi_bytes_%d" % N] = len(PM.create_proof_multi([adv] * N, [[[]]] * N, prover.SeededRng(7), canonical=True).finalize())
                PM.release()
        # (batch mode takes Montgomery advice: converted once on the device, outside the timed calls -- what DEHALO_PROOF_ADVICE_CANONICAL runs inside a proof)
        mont = adv.clone()
        ctx.field_op_device(pkg.fields.BN254.scalar.id, "to_mont", mont.data_ptr(), 0, mont.data_ptr(), mont.numel() // 4)
        ctx.synchronize()
        for N in ns:
            prios = (1, 0, -1)
            ctxs = [pkg.Context(0, priority=prios[i % 3]) for i in range(min(N, 4))]
            provers = [native.Prover(params, pk, c) for c in ctxs]
            out["batch_ms_%d" % N] = timed(lambda: native.create_proofs(provers, mont, [prover.SeededRng(100 + i) for i in range(N)]))
            for p in provers:
                p.release()
            for c in ctxs:
                c.close()
        pk.release(); params.release()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(HERE, "tools", "ab", "parent"))
    ap.add_argument("--k", type=int, default=17)
    ap.add_argument("--ns", default="1,2,4,8")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "multi_circuit_times.txt"))
    ap.add_argument("--worker", default="")
    ap.add_argument("--multi", type=int, default=0)
    a = ap.parse_args()
    ns = [int(v) for v in a.ns.split(",") if v]
    if a.worker:
        return worker(a.worker, a.k, ns, a.reps, bool(a.multi))
    runs = {"parent": [], "this": []}
    for pair in range(a.pairs):
        for build, root in (("parent", a.parent), ("this", HERE)):
            cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--worker", root, "--k", str(a.k), "--ns", a.ns, "--reps", str(a.reps),
                   "--multi", "1" if build == "this" else "0"]
            res = subprocess.run(cmd, cwd=root, capture_output=True, text=True)
            lines = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
            if res.returncode != 0 or not lines:
                sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
                sys.exit("pair %d, %s build: the worker failed (exit %d); nothing further is started" % (pair, build, res.returncode))
            runs[build].append(json.loads(lines[-1][7:]))
            print("pair %d %-6s %s" % (pair, build, lines[-1][7:]), flush=True)

    def stat(build, key):
        v = [r[key] for r in runs[build] if key in r]
        return (round(statistics.median(v), 3), round(max(v) - min(v), 3)) if v else (None, None)

    text = ["One proof over N circuits against N proofs in batch mode, delay_enc at k = %d, MI355X (tools/time_multi_circuit.py): %d alternating (parent build, this build)" % (a.k, a.pairs),
            "worker processes, each 2 warm-up + %d timed calls per figure (host clock around the whole call; median), then median [spread = max - min] over the workers." % a.reps,
            "multi: one prover with a side context, the same witness N times.  batch: dehalo_create_proofs on min(N, 4) provers, one context each.", ""]
    text.append("%3s | %-26s | %-26s | %-26s | %-22s | %s" % ("N", "multi, this: ms per proof", "ms per circuit", "batch, parent: ms for N", "ms per proof", "proof bytes multi | batch"))
    for N in ns:
        mm, ms_ = stat("this", "multi_ms_%d" % N)
        bm, bs = stat("parent", "batch_ms_%d" % N)
        mb = runs["this"][0]["multi_bytes_%d" % N]
        text.append("%3d | %10.3f [%6.3f]        | %10.3f                 | %10.3f [%6.3f]        | %10.3f             | %d | %d" %
                    (N, mm, ms_, mm / N, bm, bs, bm / N, mb, N * runs["this"][0]["single_bytes"]))
    text.append("")
    for N in ns:
        bm, bs = stat("this", "batch_ms_%d" % N)
        text.append("batch, this build, N = %d: %.3f ms [%.3f]" % (N, bm, bs))
    sp, ss = stat("parent", "single_ms")
    st, st_s = stat("this", "single_ms")
    text += ["", "single proof (native.Prover.create_proof, side context), %d pairs: parent %.3f ms [spread %.3f], this %.3f ms [spread %.3f]; this - parent = %+.3f ms" %
             (a.pairs, sp, ss, st, st_s, st - sp),
             "  parent: %s" % [r["single_ms"] for r in runs["parent"]], "  this:   %s" % [r["single_ms"] for r in runs["this"]]]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(text) + "\n")
    print("\n".join(text))


if __name__ == "__main__":
    main()
