"""Times dehalo_g_to_lagrange_device (csrc/gfft.cuh) on Vesta against the single-challenge scalar multiplication the project already runs.

For each k: the transform of 2^k points (warm-up, then `--reps` calls between device events on the context's stream, the median reported), and
one generator collapse over 2^k points (2^(k-1) scalar multiplications by ONE challenge, wave-uniform digits: k_ipa_collapse), timed the same
way and scaled to the transform's k 2^(k-1) butterfly multiplications.  The ratio of the two says what the per-butterfly twiddles, the
normalisation per stage, the [n^-1] pass and the launches cost over the kernel whose digits are uniform.  Needs a gfx950 device: no fallback.

    python tools/time_g_to_lagrange.py [--k 14 17 20] [--reps 5] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def device_points(ctx, cs, k):
    """2^k distinct non-identity points on the device, no two related in a way a butterfly would notice: the transform of (G, 2 G, O, O, ...),
    whose output i is [(1 + 2 omega^-i) / n] G."""
    b = cs.base
    G = (b.p - 1, 2)                                           # the generator of both Pasta curves
    lam = 3 * G[0] * G[0] * pow(2 * G[1], -1, b.p) % b.p       # 2 G by the tangent rule
    x2 = (lam * lam - 2 * G[0]) % b.p
    G2 = (x2, (lam * (G[0] - x2) - G[1]) % b.p)
    seed = np.zeros((1 << k, 8), dtype=np.uint64)
    for i, P in enumerate((G, G2)):
        seed[i, :4], seed[i, 4:] = b.encode(P[0]), b.encode(P[1])
    d = ctx.upload(seed)
    ctx.g_to_lagrange(cs.id, d.data_ptr(), k)
    ctx.synchronize()
    return d


def timed(ctx, fn, reps):
    import torch
    st = ctx.torch_stream_obj()
    fn()
    ctx.synchronize()                                          # warm-up: code objects loaded, workspace grown
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[14, 17, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    cs = pkg.fields.VESTA
    rows = []
    with pkg.Context(0) as ctx:
        u = cs.scalar.encode(0x1D2C3B4A59687766554433221100FFEEDDCCBBAA998877665544332211 % cs.scalar.p)
        for k in a.k:
            n = 1 << k
            g = device_points(ctx, cs, k)
            out = torch.empty_like(g)
            half = torch.empty((n // 2, 8), dtype=torch.int64, device=g.device)
            t_fft, all_fft = timed(ctx, lambda: ctx.g_to_lagrange(cs.id, g.data_ptr(), k, out.data_ptr()), a.reps)
            t_col, all_col = timed(ctx, lambda: ctx.generator_collapse_device(cs.id, g.data_ptr(), n, u, half.data_ptr()), a.reps)
            muls = k * (n // 2)
            yard = t_col * muls / (n // 2)                     # = k collapses over 2^k points
            row = {"k": k, "g_to_lagrange_ms": round(t_fft, 3), "collapse_2^k_ms": round(t_col, 4), "butterfly_muls": muls,
                   "collapse_style_ms_for_the_same_muls": round(yard, 3), "ratio": round(t_fft / yard, 3), "launches": k + 2,
                   "g_to_lagrange_ms_all": [round(x, 3) for x in all_fft], "collapse_ms_all": [round(x, 4) for x in all_col]}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
