"""Times dehalo_verify_proofs_each on one MI355X against what there was before it.

KZG: the delay_enc circuit at k = 17 (2048-bit modulus, 15-bit exponent), BN254, batches of 64 proofs, under GWC and SHPLONK, on the device verifier and on the host
verifier (ctx = NULL).
  all valid   verify_each against verify_batch (dehalo_verify_proofs: unchanged code, so it is the parent) on the same batch in the same process, alternating; the
              difference of the medians is reported beside the spread of the repeated verify_batch runs
  bad proofs  one, eight and all 64 proofs with one evaluation byte flipped: verify_each against the loop of 64 dehalo_verify_proof calls that the header
              prescribed for a batch that fails; `checks` beside each time, and the call's four timing slots
IPA: the maingate circuit with range lookups over Vesta at k = 17 (tools/time_verify_ipa.py's case), batches of 64, device verifier (a host IPA verifier at k = 17
is 380 x 2^17 group operations a check on one thread: not timed).
Then the kernel's call alone: dehalo_msm_segments_device on 128 segments of 100 terms, the device drained around it.

One process; whole host calls through ctypes on the host clock, ending in the download the call itself waits for; one warm-up call each; medians.  Needs a gfx950
device: no fallback.  No threshold is attached to these figures: DESIGN.md section 6 quotes them.

    python tools/time_verify_each.py [out file, default profiles/verify_each_times.txt]
"""
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "verify_each_times.txt")
import __graft_entry__ as entry      # noqa: E402

pkg = entry.load_package()
po, co = entry.load_oracle()
from dehalo2_amd import circuits, native, plonk, prover      # noqa: E402

F = pkg.fields
K, S, BATCH = 17, 0x5EED5EED, 64
out_file = open(OUT, "w")


def say(s):
    print(s, flush=True)
    out_file.write(s + "\n")
    out_file.flush()


def median(xs):
    return sorted(xs)[len(xs) // 2]


def clock(call):
    t = time.perf_counter()
    result = call()
    return 1e3 * (time.perf_counter() - t), result


def flipped(proof, at):
    bad = bytearray(proof)
    bad[at] ^= 1
    return bytes(bad)


def all_valid(v, batch, inst, runs):
    """verify_each and verify_batch on the same valid batch, alternating"""
    each = lambda: v.verify_each(batch, inst, num_circuits=1)
    both = lambda: v.verify_batch(batch, inst, num_circuits=1)
    assert each() == [0] * len(batch) and v.last_checks == 1 and both() is True      # warm
    t_each, t_batch = [], []
    for _ in range(runs):
        ms, ok = clock(both)
        assert ok is True
        t_batch.append(ms)
        ms, reasons = clock(each)
        assert reasons == [0] * len(batch)
        t_each.append(ms)
    slots = v.last_timings()
    say("    all valid       verify_each %9.3f ms   verify_batch %9.3f ms   difference %+8.3f ms   (verify_batch's %d runs: %.3f .. %.3f ms; medians; checks = %d)" % (
        median(t_each), median(t_batch), median(t_each) - median(t_batch), runs, min(t_batch), max(t_batch), v.last_checks))
    say("                    verify_each's slots: " + "  ".join("%s %.3f" % kv for kv in slots.items()))


def bad_proofs(v, batch, inst, one_inst, at, reason, runs):
    """verify_each on a batch with 1, 8 and 64 bad proofs against the loop of single calls over the same batch"""
    for count in (1, 8, len(batch)):
        where = set(range(len(batch))) if count == len(batch) else set(random.Random(count).sample(range(len(batch)), count))
        mixed = [flipped(p, at) if i in where else p for i, p in enumerate(batch)]
        each = lambda: v.verify_each(mixed, inst, num_circuits=1)
        loop = lambda: [0 if v.verify(p, one_inst) else v.last_reject for p in mixed]
        want = loop()      # warm; the single calls say what each proof is
        assert [i for i, r in enumerate(want) if r] == sorted(where) and set(want) <= {0, reason} and each() == want
        t_each, t_loop = [], []
        for _ in range(runs):
            ms, got = clock(loop)
            assert got == want
            t_loop.append(ms)
            ms, got = clock(each)
            assert got == want
            t_each.append(ms)
        slots = v.last_timings()
        say("    %2d bad          verify_each %9.3f ms   checks %3d   loop of %d verify calls %9.3f ms   (medians of %d; slots: %s)" % (
            count, median(t_each), v.last_checks, len(batch), median(t_loop), runs, "  ".join("%s %.3f" % kv for kv in slots.items())))


say("# one MI355X, one process; whole host calls through ctypes on the host clock, one warm-up call each, medians; batches of %d" % BATCH)
rnd = random.Random(5)
inputs = dict(n_big=rnd.getrandbits(2048) | (1 << 2047) | 1, x=rnd.getrandbits(2040), e=rnd.getrandbits(15) | (1 << 14), exp_bits=15, message=[0, 0])
with pkg.Context(0) as ctx:
    say("# KZG: delay_enc at k = %d, 2048-bit modulus, 15-bit exponent, BN254" % K)
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
    adv = np.stack([co.field_op(0, "to_mont", nat["advice"][i]) for i in range(cs.num_advice)])
    inst = [[[[]]]] * BATCH      # per proof: one circuit, whose one instance column holds no value
    for multiopen in ("gwc", "shplonk"):
        P = native.Prover(params, pk, multiopen=multiopen)
        batch = native.create_proofs([P], adv, [prover.KeyedRng(bytes([100 + i]) * 32) for i in range(BATCH)])
        at = len(batch[0]) // 2 + 7      # a byte of an evaluation: the proof stays readable and fails the pairing
        dev = native.Verifier.from_pk(params, pk, multiopen)
        host = native.Verifier.from_vk(curve, K, g0, g2, s_g2, cs, vk, num_selectors=len(nat["selectors"]), ctx=None, multiopen=multiopen, transcript_repr=pk.transcript_repr)
        for label, v, runs in (("device verifier", dev, 7), ("host verifier", host, 3)):
            say("  %s, %s: proofs of %d bytes" % (multiopen.upper(), label, len(batch[0])))
            all_valid(v, batch, inst, runs)
            bad_proofs(v, batch, inst, [[]], at, 2, runs)
        dev.release(); host.release(); P.release()
    pk.release()
    params.release()

    say("# IPA: maingate with range lookups over Vesta at k = %d, device verifier" % K)
    spec, pcurve = F.VESTA, po.VESTA
    circ = circuits.synthesize(pcurve.scalar.p, K, True, seed=3)
    n = 1 << K
    pts = co.fixed_base_mul(po.CURVE_IDS["vesta"], co.fill_scalars(po.FIELD_IDS[pcurve.scalar.name], "uniform", n + 2, 7))
    params = native.ParamsIPA.from_g(ctx, spec, K, pts[2:], pts[1], pts[0])
    pk = native.ProvingKey.keygen(ctx, params, circ.cs, circ.fixed, circ.assembly, circ.selectors)
    one_inst = [[] for _ in range(circ.cs.num_instance)]
    P = native.Prover(params, pk)
    batch = [P.create_proof(circ.advice, one_inst, prover.KeyedRng(bytes([100 + i]) * 32), canonical=True).finalize() for i in range(BATCH)]
    dev = native.Verifier.from_ipa(params, pk)
    say("  IPA, device verifier: proofs of %d bytes" % len(batch[0]))
    all_valid(dev, batch, [[one_inst]] * BATCH, 5)
    bad_proofs(dev, batch, [[one_inst]] * BATCH, one_inst, len(batch[0]) - 40, 3, 3)
    dev.release(); P.release(); pk.release(); params.release()

    say("# the kernel's call alone: dehalo_msm_segments_device, 128 segments of 100 terms (a GWC batch of 64), uniform scalars, the device drained around the call")
    import torch
    lib = pkg.load_library()
    segments, terms = 128, 100
    for name in ("bn254", "pallas", "vesta"):
        c = F.CURVES[name]
        sc = ctx.upload(co.fill_scalars(c.scalar.id, "uniform", segments * terms, 3))
        pt = ctx.upload(np.ascontiguousarray(np.tile(co.synth_bases(c.id, terms), (segments, 1))))
        off = ctx.upload(np.arange(0, segments * terms + 1, terms, dtype=np.uint32))
        res = torch.zeros((segments, 8), dtype=torch.int64, device=off.device)
        call = lambda: ctx._check(lib.dehalo_msm_segments_device(ctx.handle, c.id, sc.data_ptr(), pt.data_ptr(), off.data_ptr(), segments, res.data_ptr(), None))
        call()
        ctx.synchronize()
        ms = []
        for _ in range(20):
            t = time.perf_counter()
            call()
            ctx.synchronize()
            ms.append(1e3 * (time.perf_counter() - t))
        say("  %-6s %7.3f ms  (median of 20: the offsets' copy back, their check, one launch, the wait; %.3f .. %.3f)" % (name, median(ms), min(ms), max(ms)))
out_file.close()
