"""Times verify_proof on one MI355X: the delay_enc circuit at k = 17 (2048-bit modulus, 15-bit exponent), BN254 / KZG, under GWC and SHPLONK -- one proof on the
device verifier, one proof on the host verifier (ctx = NULL), a batch of 64 proofs in one dehalo_verify_proofs call (reported per proof) -- each split into point
decompression, the transcript walk, the two MSMs and the pairing check (dehalo_verifier_last_timings), beside the two comparison points there are: the oracle's
verifier (Python integers) on the same proof in the same run, and the same commit's create_proof of that proof.  Upstream's Rust verifier cannot be run here.

One process; whole host calls through ctypes on the host clock after one warm-up call.  Needs a gfx950 device: no fallback.  No threshold is attached to these
figures: DESIGN.md section 6 quotes them.

    python tools/time_verify.py [out file, default profiles/verify_times.txt]
"""
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "verify_times.txt")
import __graft_entry__ as entry      # noqa: E402

pkg = entry.load_package()
po, co = entry.load_oracle()
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pairing as pr      # noqa: E402
import shapes      # noqa: E402
import shplonk_oracle      # noqa: E402
import verifier as V      # noqa: E402
from dehalo2_amd import keygen, native, plonk, prover      # noqa: E402

F = pkg.fields
K, S, BATCH = 17, 0x5EED5EED, 64
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
    parts = {name: median([s[name] for s in split]) / per for name in ("walk", "decompress", "msm", "pairing")}
    return "%9.3f ms  (walk %8.3f  decompress %7.3f  msm %8.3f  pairing %7.3f; %d runs, medians)" % (median(wall) / per, parts["walk"], parts["decompress"], parts["msm"],
                                                                                                    parts["pairing"], runs)


say("# one MI355X, one process; whole host calls through ctypes on the host clock, one warm-up call each; delay_enc at k = %d, 2048-bit modulus, 15-bit exponent" % K)
rnd = random.Random(5)
inputs = dict(n_big=rnd.getrandbits(2048) | (1 << 2047) | 1, x=rnd.getrandbits(2040), e=rnd.getrandbits(15) | (1 << 14), exp_bits=15, message=[0, 0])
with pkg.Context(0) as ctx:
    curve = F.BN254
    nat = native.synthesize(native.CIRCUIT_DELAY_ENC, K, keygen=True, **inputs)
    cs = plonk.maingate_cs(True)
    asm = plonk.Assembly(6, 1 << K)
    asm.mapping = nat["mapping"].astype(np.int64)
    params = native.ParamsKZG.setup(ctx, curve, K, S)
    pk = native.ProvingKey.keygen(ctx, params, cs, nat["fixed"], asm, nat["selectors"])
    raw = params.write()
    g0, g2, s_g2 = np.frombuffer(raw[4:68], dtype=np.uint64), raw[-256:-128], raw[-128:]
    vk = pk.vk_bytes()
    nf, npc = cs.num_fixed, len(cs.permutation_columns)
    pts = keygen.decode_points(curve, np.frombuffer(vk[8:8 + 64 * (nf + npc)], dtype=np.uint64).reshape(-1, 8))
    adv = np.stack([co.field_op(0, "to_mont", nat["advice"][i]) for i in range(cs.num_advice)])
    for multiopen in ("gwc", "shplonk"):
        P = native.Prover(params, pk, multiopen=multiopen)
        P.create_proof(adv, [[]], prover.KeyedRng(b"\x01" * 32))      # warm
        t_prove = []
        for i in range(5):
            ctx.synchronize()
            t = time.perf_counter()
            proof = P.create_proof(adv, [[]], prover.KeyedRng(bytes([i + 2]) * 32)).finalize()
            t_prove.append(1e3 * (time.perf_counter() - t))
        say("%s: proof of %d bytes" % (multiopen.upper(), len(proof)))
        dev = native.Verifier.from_pk(params, pk, multiopen)
        host = native.Verifier.from_vk(curve, K, g0, g2, s_g2, cs, vk, num_selectors=len(nat["selectors"]), ctx=None, multiopen=multiopen, transcript_repr=pk.transcript_repr)
        if multiopen == "gwc":      # the constructors (both check g2 and s_g2: on the twist, in the subgroup), medians of 5; the same for either multiopen
            t_pk, t_vk = [], []
            for _ in range(5):
                t = time.perf_counter()
                native.Verifier.from_pk(params, pk, multiopen).release()
                t_pk.append(1e3 * (time.perf_counter() - t))
                t = time.perf_counter()
                native.Verifier.from_vk(curve, K, g0, g2, s_g2, cs, vk, num_selectors=len(nat["selectors"]), ctx=None, multiopen=multiopen).release()
                t_vk.append(1e3 * (time.perf_counter() - t))
            say("  Verifier.from_pk (device verifier)  %9.3f ms   Verifier.from_vk (host verifier, RawBytesUnchecked vk of %d bytes)  %9.3f ms" % (median(t_pk), len(vk), median(t_vk)))
        say("  one proof, device verifier          " + timed_verify(lambda: dev.verify(proof, [[]]), dev, 9))
        say("  one proof, host verifier            " + timed_verify(lambda: host.verify(proof, [[]]), host, 5))
        batch = native.create_proofs([P], adv, [prover.KeyedRng(bytes([100 + i]) * 32) for i in range(BATCH)])
        inst = [[[[]]]] * BATCH      # per proof: one circuit, whose one instance column holds no value
        say("  batch of %d, device, per proof      " % BATCH + timed_verify(lambda: dev.verify_batch(batch, inst, num_circuits=1), dev, 5, BATCH))
        say("  batch of %d, host, per proof        " % BATCH + timed_verify(lambda: host.verify_batch(batch, inst, num_circuits=1), host, 3, BATCH))
        bad = bytearray(batch[5])
        bad[len(bad) // 2 + 7] ^= 1
        assert dev.verify_batch(batch[:5] + [bytes(bad)] + batch[6:], inst, num_circuits=1) is False and dev.verify(bytes(bad), [[]]) is False
        oracle = shplonk_oracle.verify_proof_shplonk if multiopen == "shplonk" else V.verify_proof
        t = time.perf_counter()
        ok = oracle(po.BN254, shapes.maingate_description(True), K, pts[:nf], pts[nf:], pk.transcript_repr, (1, 2), pr.G2, pr.g2_mul(S, pr.G2), [[]], proof)
        t_oracle = 1e3 * (time.perf_counter() - t)
        assert ok is True
        say("  the oracle's verifier, same proof   %9.3f ms  (Python integers; one run)" % t_oracle)
        say("  create_proof, same commit           %9.3f ms  (median of 5, advice on the host)" % median(t_prove))
        dev.release(); host.release(); P.release()
    pk.release()
    params.release()
say("# upstream's Rust verifier (halo2_proofs verify_proof) cannot be built or run here: no figure for it")

with open(OUT, "w") as fh:
    fh.write("\n".join(lines) + "\n")
