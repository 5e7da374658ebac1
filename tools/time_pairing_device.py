"""Times the device pairing checks (csrc/pairing.cuh) on one MI355X: the kernel's call alone, and the KZG verifier in host mode and device mode
(dehalo_verifier_set_pairing) in the same run.

  kernel   dehalo_pairing_checks_device at pairs = 2 (a verifier's s_g2, g2), checks in 1, 2, 64, 128, 1024, 4096: the median of 20 with the device drained around
           each call, as tools/time_verify_each.py times dehalo_msm_segments_device
  verifier tools/time_verify_each.py's KZG rows -- 64 delay_enc proofs at k = 17 under GWC and SHPLONK with 0, 1, 8 and 64 invalid, beside the loop of 64 single
           calls -- on ONE device verifier switched between the modes; then one proof alone in both modes
The one condition: with all 64 invalid, device mode's verify_each takes less than the loop of 64 single calls in host mode, by more than the spread of the
two medians' own runs.  It is asserted at the end, after every figure is written.  Everything else is recorded, not required.

One process; whole host calls through ctypes on the host clock, ending in the download the call itself waits for; one warm-up call each; medians.  Needs a gfx950
device: no fallback.

    python tools/time_pairing_device.py [out file, default profiles/pairing_device_times.txt]
"""
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pairing_device_times.txt")
import __graft_entry__ as entry      # noqa: E402

pkg = entry.load_package()
po, co = entry.load_oracle()
from dehalo2_amd import native, plonk, prover      # noqa: E402

F = pkg.fields
K, S, BATCH, RUNS = 17, 0x5EED5EED, 64, 5
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


def timed(call, want, runs=RUNS):
    assert call() == want      # warm
    ms = []
    for _ in range(runs):
        t, got = clock(call)
        assert got == want
        ms.append(t)
    return ms


say("# one MI355X, one process; host clock around whole calls, one warm-up call each, medians")
condition = []
with pkg.Context(0) as ctx:
    import torch
    lib = pkg.load_library()
    curve = F.BN254
    params = native.ParamsKZG.setup(ctx, curve, K, S)
    raw = params.write()
    g0, g2, s_g2 = np.frombuffer(raw[4:68], dtype=np.uint64), raw[-256:-128], raw[-128:]

    table = pkg.PairingTable(ctx, curve.id, [s_g2, g2])
    say("# the kernel's call alone: dehalo_pairing_checks_device, pairs = 2 (s_g2, g2 of the k = %d params), %d checks a block, the device drained around the call" % (
        K, lib.dehalo_pairing_checks_per_block(table.handle)))
    f = curve.base
    pts = [po.ec_mul(po.BN254, a, (1, 2)) for a in range(1, 9)]
    rows = np.stack([np.concatenate([f.encode(P[0]), f.encode(P[1])]) for P in pts])
    for checks in (1, 2, 64, 128, 1024, 4096):
        g1 = ctx.upload(np.ascontiguousarray(rows[np.arange(2 * checks) % len(rows)]))      # valid points, no check cancels: the whole walk every time
        st = torch.zeros((checks,), dtype=torch.uint8, device=g1.device)
        call = lambda: ctx.pairing_checks_device(table, g1.data_ptr(), checks, st.data_ptr())
        call()
        ctx.synchronize()
        assert not st.cpu().numpy().any()
        ms = []
        for _ in range(20):
            t = time.perf_counter()
            call()
            ctx.synchronize()
            ms.append(1e3 * (time.perf_counter() - t))
        say("  checks %5d   %8.3f ms  (median of 20: one launch, the wait; %.3f .. %.3f)" % (checks, median(ms), min(ms), max(ms)))
    table.release()

    say("# KZG: delay_enc at k = %d, 2048-bit modulus, 15-bit exponent, BN254, batches of %d, one device verifier in host mode and in device mode" % (K, BATCH))
    rnd = random.Random(5)
    inputs = dict(n_big=rnd.getrandbits(2048) | (1 << 2047) | 1, x=rnd.getrandbits(2040), e=rnd.getrandbits(15) | (1 << 14), exp_bits=15, message=[0, 0])
    nat = native.synthesize(native.CIRCUIT_DELAY_ENC, K, keygen=True, **inputs)
    cs = plonk.maingate_cs(True)
    asm = plonk.Assembly(6, 1 << K)
    asm.mapping = nat["mapping"].astype(np.int64)
    pk = native.ProvingKey.keygen(ctx, params, cs, nat["fixed"], asm, nat["selectors"])
    adv = np.stack([co.field_op(0, "to_mont", nat["advice"][i]) for i in range(cs.num_advice)])
    inst = [[[[]]]] * BATCH
    for multiopen in ("gwc", "shplonk"):
        P = native.Prover(params, pk, multiopen=multiopen)
        batch = native.create_proofs([P], adv, [prover.KeyedRng(bytes([100 + i]) * 32) for i in range(BATCH)])
        at = len(batch[0]) // 2 + 7      # a byte of an evaluation: the proof stays readable and fails the pairing
        v = native.Verifier.from_pk(params, pk, multiopen)
        loop_host_all_bad = None
        for mode in ("host", "device"):
            v.set_pairing(mode)
            say("  %s, pairing on the %s: proofs of %d bytes" % (multiopen.upper(), mode, len(batch[0])))
            for count in (0, 1, 8, BATCH):
                where = set(range(BATCH)) if count == BATCH else set(random.Random(count).sample(range(BATCH), count))
                mixed = [flipped(p, at) if i in where else p for i, p in enumerate(batch)]
                want = [2 if i in where else 0 for i in range(BATCH)]
                t_each = timed(lambda: v.verify_each(mixed, inst, num_circuits=1), want)
                checks, slots = v.last_checks, v.last_timings()
                t_loop = timed(lambda: [0 if v.verify(p, [[]]) else v.last_reject for p in mixed], want)
                say("    %2d bad   verify_each %9.3f ms (%.3f .. %.3f)   checks %3d   loop of %d verify calls %9.3f ms (%.3f .. %.3f)   (medians of %d; slots: %s)" % (
                    count, median(t_each), min(t_each), max(t_each), checks, BATCH, median(t_loop), min(t_loop), max(t_loop), RUNS, "  ".join("%s %.3f" % kv for kv in slots.items())))
                if count == 0:
                    t_batch = timed(lambda: v.verify_batch(batch, inst, num_circuits=1), True)
                    say("             verify_batch %8.3f ms (%.3f .. %.3f)" % (median(t_batch), min(t_batch), max(t_batch)))
                if count == BATCH and mode == "host":
                    loop_host_all_bad = t_loop
                if count == BATCH and mode == "device":
                    condition.append((multiopen, t_each, loop_host_all_bad))
            t_one = timed(lambda: v.verify(batch[0], [[]]), True, 9)
            say("    one proof alone   verify %8.3f ms (%.3f .. %.3f; median of 9; slots: %s)" % (
                median(t_one), min(t_one), max(t_one), "  ".join("%s %.3f" % kv for kv in v.last_timings().items())))
        v.release(); P.release()
    pk.release()
    params.release()

say("# the condition: all %d invalid, verify_each in device mode against the loop of %d single calls in host mode, same run" % (BATCH, BATCH))
ok = True
for multiopen, t_each, t_loop in condition:
    spread = (max(t_each) - min(t_each)) + (max(t_loop) - min(t_loop))
    margin = median(t_loop) - median(t_each)
    say("  %-8s device-mode verify_each %9.3f ms   host-mode loop %9.3f ms   margin %9.3f ms   spread of the two medians' runs %.3f ms   %s" % (
        multiopen.upper(), median(t_each), median(t_loop), margin, spread, "holds" if margin > spread else "FAILS"))
    ok = ok and margin > spread
out_file.close()
assert ok, "device mode does not beat the loop of single calls on the all-invalid batch"
