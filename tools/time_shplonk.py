"""Times the SHPLONK multiopen against GWC, and the one-pass vanishing-polynomial quotient against the chain of kate divisions it stands for.

    python tools/time_shplonk.py [--ks 14,17] [--lens 17,20] [--pairs 5] [--out profiles/shplonk_times.txt]

(a) proofs: the library's own delay_enc witness (2048-bit modulus, as many exponent bits as 2^k rows hold) on ONE prover with a side context, switched between the two
    multiopens (dehalo_prover_set_multiopen).  One warm-up proof under each, then `pairs` alternating (GWC, SHPLONK) pairs in this process; the `openings` phase and
    the total of dehalo_prover_last_timings (host clock around the phase, read-backs included), medians.  GWC is the yardstick: the same code as before the switch existed.
(b) quotients: dehalo_vanishing_quotient_batch_device for m = 2, 3, 4 points at 2^17 and 2^20 coefficients, one polynomial and eight a call, against m chained
    dehalo_kate_division_batch_device calls on the same inputs; device events on the context's stream around each, one warm-up, medians of `pairs` alternating pairs.
Raw JSON lines go to stdout and --out.  No thresholds.  Needs a gfx950 device: no fallback."""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def delay_enc(native, W, k):
    rnd = random.Random(2048)
    n_big, x = rnd.getrandbits(2048) | (1 << 2047) | 1, rnd.getrandbits(2000)
    tail = W.hash_region_rows() + W.cipher_region_rows(2, True)
    bits = max(b for b in range(1, 16) if W.rsa_region_rows(b) + tail + 1 <= (1 << k) - 6)
    e = rnd.getrandbits(bits) | (1 << (bits - 1))
    return native.synthesize(native.CIRCUIT_DELAY_ENC, k, n_big=n_big, e=e, x=x, exp_bits=bits, message=[0, 0], keygen=True), bits


def time_proofs(pkg, k, pairs):
    from dehalo2_amd import native, plonk, prover, witness as W
    nat, bits = delay_enc(native, W, k)
    cs = plonk.maingate_cs(True)
    asm = plonk.Assembly(6, 1 << k)
    asm.mapping = nat["mapping"].astype(np.int64)
    with pkg.Context(0) as ctx, pkg.Context(0) as side:
        params = native.ParamsKZG.setup(ctx, pkg.fields.BN254, k, 0x5EED)
        pk = native.ProvingKey.keygen(ctx, params, cs, nat["fixed"], asm, nat["selectors"])
        P = native.Prover(params, pk, ctx, side)
        adv = ctx.upload(np.ascontiguousarray(nat["advice"]))
        res = {"gwc": [], "shplonk": []}
        sizes = {}

        def one(mo, keep):
            P.set_multiopen(mo)
            proof = P.create_proof(adv, [[]], prover.SeededRng(7), canonical=True).finalize()
            sizes[mo] = len(proof)
            if keep:
                t = P.last_timings()
                res[mo].append((t["openings"], t["total"]))

        for mo in ("gwc", "shplonk"):
            one(mo, False)
        for _ in range(pairs):
            for mo in ("gwc", "shplonk"):
                one(mo, True)
        P.release(); pk.release(); params.release()
    rows = []
    for mo in ("gwc", "shplonk"):
        rows.append({"what": "create_proof, delay_enc", "k": k, "exponent_bits": bits, "multiopen": mo, "proof_bytes": sizes[mo], "pairs": pairs,
                     "openings_ms_median": round(statistics.median(o for o, _ in res[mo]), 3), "total_ms_median": round(statistics.median(t for _, t in res[mo]), 3),
                     "openings_ms": [round(o, 3) for o, _ in res[mo]], "total_ms": [round(t, 3) for _, t in res[mo]]})
    return rows


def time_quotients(pkg, log_lens, pairs):
    import torch
    f = pkg.fields.FIELDS["bn254_fr"]
    rows = []
    with pkg.Context(0) as ctx:
        st = ctx.torch_stream_obj()
        gen = np.random.Generator(np.random.PCG64(5))

        def scalars(count):      # raw 253-bit values taken as Montgomery representations: below the modulus
            a = gen.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
            a[:, 3] &= np.uint64((1 << 61) - 1)
            return a

        pts = scalars(4)
        for lg in log_lens:
            n = 1 << lg
            d = ctx.upload(scalars(8 * n).reshape(8, n, 4))
            out = torch.zeros((8, n, 4), dtype=torch.int64, device="cuda")
            tmp = torch.zeros((2, 8, n, 4), dtype=torch.int64, device="cuda")
            for count in (1, 8):
                ins = [d[i].data_ptr() for i in range(count)]
                outs = [out[i].data_ptr() for i in range(count)]
                for m in (2, 3, 4):
                    def one_pass():
                        ctx.vanishing_quotient_batch_device(f.id, ins, n, [pts[:m]] * count, outs)

                    def chain():
                        cur = ins
                        for t in range(m):
                            dst = [tmp[t & 1, i].data_ptr() for i in range(count)]
                            ctx.kate_division_batch_device(f.id, cur, n, np.tile(pts[t], (count, 1)), dst)
                            cur = dst

                    def timed(fn):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        fn()
                        e1.record(st)
                        e1.synchronize()
                        return e0.elapsed_time(e1)

                    one_pass(); chain(); ctx.synchronize()
                    a, b = [], []
                    for _ in range(pairs):
                        a.append(timed(chain))
                        b.append(timed(one_pass))
                    rows.append({"what": "quotient by a vanishing polynomial", "log_len": lg, "polynomials": count, "points": m, "pairs": pairs,
                                 "chain_ms_median": round(statistics.median(a), 4), "one_pass_ms_median": round(statistics.median(b), 4),
                                 "chain_ms": [round(v, 4) for v in a], "one_pass_ms": [round(v, 4) for v in b]})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="14,17")
    ap.add_argument("--lens", default="17,20")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shplonk_times.txt"))
    a = ap.parse_args()
    pkg = entry.load_package()
    rows = time_quotients(pkg, [int(v) for v in a.lens.split(",") if v], a.pairs)
    for k in [int(v) for v in a.ks.split(",") if v]:
        rows += time_proofs(pkg, k, a.pairs)
    with open(a.out, "w") as fh:
        fh.write("SHPLONK against GWC and the one-pass quotient against the chained division (tools/time_shplonk.py), MI355X; one warm-up, then medians of alternating\n"
                 "pairs in one process.  Proofs: dehalo_prover_last_timings (host clock, read-backs included); quotients: device events on the context's stream.\n")
        for r in rows:
            line = json.dumps(r)
            print(line)
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
