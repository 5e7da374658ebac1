"""The cost of one single-column shuffle argument at k = 17: the bench's delay_enc circuit with a sixth advice column (column 0's usable rows reversed, queried
at rotation 0), proved without and with the shuffle [a0] ~ [a5] -- the same columns, commitments and queries but for the argument itself.

    python tools/time_shuffle.py [--k 17] [--pairs 5] [--reps 6] [--out profiles/shuffle_cost.txt]

One process; per pair the two provers alternate, each figure the median of `reps` timed calls after 2 warm-up calls (host clock around the whole call, which
returns the proof's bytes).  Prints and writes the medians, the spreads over the pairs and the difference.  No thresholds.  Needs a gfx950 device: no fallback."""
import argparse
import json
import os
import random
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=17)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "shuffle_cost.txt"))
    a = ap.parse_args()
    import numpy as np
    sys.path.insert(0, HERE)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    from dehalo2_amd import native, plonk, prover, witness as W
    k, n = a.k, 1 << a.k
    rnd = random.Random(2048)
    n_big, x = rnd.getrandbits(2048) | (1 << 2047) | 1, rnd.getrandbits(2000)
    tail = W.hash_region_rows() + W.cipher_region_rows(2, True)
    bits = max(b for b in range(1, 16) if W.rsa_region_rows(b) + tail + 1 <= n - 6)
    e = rnd.getrandbits(bits) | (1 << (bits - 1))
    nat = native.synthesize(native.CIRCUIT_DELAY_ENC, k, n_big=n_big, e=e, x=x, exp_bits=bits, message=[0, 0], keygen=True)

    def circuit(with_shuffle):
        cs = plonk.maingate_cs(True)
        cs.num_advice = 6
        a5 = cs.query_advice(5)
        if with_shuffle:
            cs.shuffle([(("advice", 0, 0), a5)])
        return cs

    usable = n - (circuit(True).blinding_factors() + 1)
    advice = np.zeros((6, n, 4), dtype=np.uint64)
    advice[:5] = nat["advice"]
    advice[5, :usable] = nat["advice"][0, :usable][::-1]
    asm = plonk.Assembly(6, n)
    asm.mapping = nat["mapping"].astype(np.int64)

    def timed(fn):
        for _ in range(2):
            fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ts), 3)

    runs = {False: [], True: []}
    with pkg.Context(0) as ctx, pkg.Context(0) as side:
        params = native.ParamsKZG.setup(ctx, pkg.fields.BN254, k, 0x5EED)
        adv = ctx.upload(np.ascontiguousarray(advice))
        made = {}
        for ws in (False, True):
            pk = native.ProvingKey.keygen(ctx, params, circuit(ws), nat["fixed"], asm, nat["selectors"])
            made[ws] = (pk, native.Prover(params, pk, ctx, side))
        sizes = {ws: len(made[ws][1].create_proof(adv, [[]], prover.SeededRng(7), canonical=True).finalize()) for ws in made}
        for _ in range(a.pairs):
            for ws in (False, True):
                P = made[ws][1]
                runs[ws].append(timed(lambda: P.create_proof(adv, [[]], prover.SeededRng(7), canonical=True)))
        phases = {ws: [round(float(v), 3) for v in made[ws][1].last_timings().values()] for ws in made}
        for pk, P in made.values():
            P.release(); pk.release()
        params.release()
    med = {ws: round(statistics.median(v), 3) for ws, v in runs.items()}
    spread = {ws: round(max(v) - min(v), 3) for ws, v in runs.items()}
    text = ["One single-column shuffle at k = %d, MI355X (tools/time_shuffle.py): delay_enc with a sixth advice column, without and with the shuffle [a0] ~ [a5];" % k,
            "%d alternating pairs in one process, each figure the median of %d timed create_proof calls after 2 warm-up calls (host clock, side context)." % (a.pairs, a.reps),
            "without: %.3f ms [spread %.3f]  %s   proof bytes %d" % (med[False], spread[False], runs[False], sizes[False]),
            "with:    %.3f ms [spread %.3f]  %s   proof bytes %d" % (med[True], spread[True], runs[True], sizes[True]),
            "the shuffle costs %+.3f ms (one more column in the products' commitment, transforms and evaluation; two programs on the original and on the extended domain;" % (med[True] - med[False]),
            "one pass of k_shuffle_h_batch over the 4n extended rows; three more opening queries: a0 is queried by the circuit already, z at x and at omega x)."]
    if phases:
        text.append("last proof's phases (advice, lookups, products, random, quotient, evaluations, openings, total), ms: without %s; with %s" % (phases[False], phases[True]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(text) + "\n")
    print("\n".join(text))
    print("RESULT " + json.dumps({"without_ms": med[False], "with_ms": med[True]}))


if __name__ == "__main__":
    main()
