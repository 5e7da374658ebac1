"""Times dehalo_params_ipa_generate and its two device parts on Vesta: the generated points (k_points_generate, csrc/gfft.cuh) and the group FFT.

For each k, warm (one untimed call of each first: code objects loaded, workspace grown, clocks up), `--reps` samples, the median and every sample:
  points_ms         dehalo_points_generate_device over 2^k indices of stream 0, between device events on the context's stream;
  g_to_lagrange_ms  dehalo_g_to_lagrange_device over those points, the same way;
  whole_call_ms     dehalo_params_ipa_generate + dehalo_params_release on the host clock (the call ends in host waits: downloads of g and g_lagrange, two
                    table registrations, W's fixed-base table), release outside the timed span.
And, counted on the CPU from the rule itself (tests/generator_reference.py, the first `--waves` x 64 indices): square roots per lane (mean) and per wave (the
slowest lane's, which is what a wave runs), i.e. the share of the points kernel that lanes spend waiting for their wave -- what a restructured kernel could
save at most.  Needs a gfx950 device: no fallback.

    python tools/time_params_ipa_generate.py [--k 14 17 20] [--reps 5] [--waves 256] [--out profiles/params_ipa_generate_times.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as entry  # noqa: E402


def timed(ctx, fn, reps):
    import torch
    st = ctx.torch_stream_obj()
    fn()
    ctx.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [round(x, 4) for x in ms]


def wave_statistics(waves):
    """square roots (candidates with 0 < x < p) and blocks per lane over the first waves x 64 indices of stream 0 on Vesta, and the per-wave maxima"""
    import generator_reference as G
    roots, blocks = [], []
    for i in range(64 * waves):
        tries = G.attempts("vesta", None, 0, i)
        blocks.append(len(tries))
        roots.append(sum(1 for t in tries if t[1] in (G.ACCEPTED, G.NOT_A_NONZERO_SQUARE)))
    roots, blocks = np.array(roots).reshape(waves, 64), np.array(blocks).reshape(waves, 64)
    return {"indices": 64 * waves, "blocks_per_lane_mean": round(float(blocks.mean()), 3), "blocks_per_lane_max": int(blocks.max()),
            "square_roots_per_lane_mean": round(float(roots.mean()), 3), "square_roots_per_lane_max": int(roots.max()), "square_roots_per_wave_mean": round(float(roots.max(axis=1).mean()), 3),
            "lane_share_of_wave_square_roots": round(float(roots.mean() / roots.max(axis=1).mean()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[14, 17, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--waves", type=int, default=256)      # 2^14 indices: the k = 14 launch
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "params_ipa_generate_times.txt"))
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    from dehalo2_amd import native
    cs = pkg.fields.VESTA
    lines = []
    with pkg.Context(0) as ctx:
        for k in a.k:
            n = 1 << k
            g = torch.empty((n, 8), dtype=torch.int64, device=torch.device("cuda", ctx.device))
            out = torch.empty_like(g)
            t_pts, all_pts = timed(ctx, lambda: ctx.points_generate(cs.id, g.data_ptr(), n), a.reps)
            t_fft, all_fft = timed(ctx, lambda: ctx.g_to_lagrange(cs.id, g.data_ptr(), k, out.data_ptr()), a.reps)
            native.ParamsIPA.generate(ctx, cs, k).release()
            whole = []
            for _ in range(a.reps):
                ctx.synchronize()
                t0 = time.perf_counter()
                prm = native.ParamsIPA.generate(ctx, cs, k)
                whole.append((time.perf_counter() - t0) * 1e3)
                prm.release()
            row = {"k": k, "points_ms": round(t_pts, 4), "g_to_lagrange_ms": round(t_fft, 3), "whole_call_ms": round(float(np.median(whole)), 3),
                   "points_over_g_to_lagrange": round(t_pts / t_fft, 4), "points_ns_per_point": round(t_pts * 1e6 / n, 2),
                   "points_ms_all": all_pts, "g_to_lagrange_ms_all": [round(x, 3) for x in all_fft], "whole_call_ms_all": [round(x, 3) for x in whole]}
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    lines.append(json.dumps({"rule_counts_vesta_stream0": wave_statistics(a.waves)}))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
