"""Times one dehalo_check_witness of the library's own k = 17 delay_enc witness (2048-bit modulus, 15-bit exponent: the metric's shape).

    python tools/time_check_witness.py [--k 17] [--reps 5] [--out profiles/check_witness_times.txt]

The key is made once; one warm-up check (code objects loaded, workspace grown), then `reps` checks, each between two device events on the context's stream
(the call's uploads, kernels and its one download) and under the host clock; the medians are printed as one JSON line and appended to --out.  The advice is
uploaded from host memory each time, as a front-end's first call would; a second row times the same check with the advice already on the device.
Needs a gfx950 device: no fallback."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=17)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_witness_times.txt"))
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    from dehalo2_amd import native, plonk
    rnd = random.Random(2048)
    n_big, x = rnd.getrandbits(2048) | (1 << 2047) | 1, rnd.getrandbits(2000)
    nat = native.synthesize(native.CIRCUIT_DELAY_ENC, a.k, n_big=n_big, e=0b101101110010111, x=x, exp_bits=15, message=[0, 0], keygen=True)
    cs = plonk.maingate_cs(True)
    asm = plonk.Assembly(6, 1 << a.k)
    asm.mapping = nat["mapping"].astype(np.int64)
    rows = []
    with pkg.Context(0) as ctx:
        params = native.ParamsKZG.setup(ctx, pkg.fields.BN254, a.k, 0x5EED)
        pk = native.ProvingKey.keygen(ctx, params, cs, nat["fixed"], asm, nat["selectors"])
        st = ctx.torch_stream_obj()
        d_adv = ctx.upload(np.ascontiguousarray(nat["advice"]))
        for label, adv in (("advice on the host", nat["advice"]), ("advice on the device", d_adv)):
            rep = pk.check_witness(adv, [[]], assembly=asm, canonical=True)      # warm-up
            assert rep.ok, rep
            dev, host = [], []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(st)
                rep = pk.check_witness(adv, [[]], assembly=asm, canonical=True)
                e1.record(st)
                e1.synchronize()
                host.append((time.perf_counter() - t0) * 1e3)
                dev.append(e0.elapsed_time(e1))
            rows.append({"what": "dehalo_check_witness, delay_enc", "k": a.k, "advice": label, "witness_rows": nat["rows"], "usable_rows": rep.rows,
                         "lookup_inputs": rep.lookup_inputs, "cells_in_cycles": rep.cells_in_cycles, "reps": a.reps,
                         "device_ms_median": round(statistics.median(dev), 3), "host_ms_median": round(statistics.median(host), 3),
                         "device_ms": [round(v, 3) for v in dev]})
        pk.release(); params.release()
    with open(a.out, "w") as fh:
        fh.write("dehalo_check_witness: one check of the library's own delay_enc witness (tools/time_check_witness.py), MI355X; events on the context's stream\n"
                 "around the whole call (uploads, kernels, the one download) after one warm-up check, medians of `reps`.  No target, no comparison: a first figure.\n")
        for r in rows:
            line = json.dumps(r)
            print(line)
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
