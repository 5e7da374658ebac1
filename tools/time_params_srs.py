"""Times ParamsKZG from an SRS file on one MI355X: dehalo_params_read_custom in the three formats, the prefix read, dehalo_params_downsize and
dehalo_params_write_custom(Processed) (csrc/params.hip; the kernels: csrc/gfft.cuh).

One process.  Every step is a whole host call (upload, kernels, table registration, download), so it is timed on the host clock: a warm-up call, then `--reps`
calls, the median and every sample printed as one JSON line and appended to `--out`.  Each step runs under its own time limit (`--limit` seconds, a
watchdog thread: the library calls release the interpreter lock): a step that overruns it ends the process with status 124 at once -- nothing is started on
the device after a step that hung.  Needs a gfx950 device: no fallback.
No threshold is attached to these figures (there is no upstream binary to compare with): DESIGN.md section 6 quotes them.

    python tools/time_params_srs.py [--k 20] [--small 17] [--reps 5] [--limit 120] [--out profiles/params_srs_times.txt]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def _overrun():
    sys.stderr.write("time_params_srs: a step overran its time limit\n")
    sys.stderr.flush()
    os._exit(124)


class limit_of:
    """with limit_of(seconds): the process ends with status 124 if the block is still running after `seconds`"""

    def __init__(self, seconds):
        self.timer = threading.Timer(seconds, _overrun)
        self.timer.daemon = True

    def __enter__(self):
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()


def timed(name, fn, reps, limit, extra, out):
    """fn() makes and returns something with .release() (or bytes); warm-up + reps calls under one time limit"""
    ms = []
    with limit_of(limit):
        for i in range(reps + 1):
            t0 = time.perf_counter()
            r = fn()
            t1 = time.perf_counter()
            if hasattr(r, "release"):
                r.release()
            if i:
                ms.append((t1 - t0) * 1e3)
    row = dict({"step": name, "ms": round(float(np.median(ms)), 3), "ms_all": [round(x, 3) for x in ms]}, **extra)
    line = json.dumps(row)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--small", type=int, default=17)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "params_srs_times.txt"))
    a = ap.parse_args()
    pkg = entry.load_package()
    from dehalo2_amd import native
    cs = pkg.fields.BN254
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out, pkg.Context(0) as ctx:
        with limit_of(a.limit):
            big = native.ParamsKZG.setup(ctx, cs, a.k, 0x5EED5EED5EED5EED1234567)
            files = {fmt: big.write(fmt) for fmt in ("processed", "raw", "raw-unchecked")}
        for fmt, data in files.items():
            timed("read_custom", lambda: native.ParamsKZG.read(ctx, cs, data, format=fmt), a.reps, a.limit, {"k": a.k, "format": fmt, "bytes": len(data)}, out)
        for fmt, data in files.items():
            timed("read_custom_downsize", lambda: native.ParamsKZG.read(ctx, cs, data, format=fmt, downsize=a.small), a.reps, a.limit,
                  {"k": a.k, "downsize_k": a.small, "format": fmt, "bytes": len(data)}, out)
        timed("downsize", lambda: big.downsize(a.small), a.reps, a.limit, {"k": a.k, "to_k": a.small}, out)
        timed("write_custom", lambda: big.write("processed"), a.reps, a.limit, {"k": a.k, "format": "processed", "bytes": len(files["processed"])}, out)
        big.release()


if __name__ == "__main__":
    main()
