"""Times the key calls on one MI355X: dehalo_keygen against dehalo_keygen_pk, dehalo_pk_write and dehalo_pk_write_custom in the three formats, dehalo_pk_read and
dehalo_pk_read_custom in the three formats (csrc/keygen.hip; the kernels: csrc/scalar_codec.cuh, csrc/gfft.cuh), at k = 14 and k = 17.

One process, the maingate circuit with range lookups over BN254 / KZG, params from dehalo_params_setup.  Every step is a whole host call through ctypes, timed on
the host clock after one warm-up call; host buffers are pageable and touched beforehand.  dehalo_pk_read and read_custom(RawBytesUnchecked) of the same bytes
alternate: they are the same path, and their agreement within dehalo_pk_read's own spread is the check that the new plumbing added no copy.  Needs a gfx950
device: no fallback.  No threshold is attached to these figures: DESIGN.md section 6 quotes them.

    python tools/time_key_formats.py [out file, default profiles/key_format_times.txt]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "key_format_times.txt")
import __graft_entry__ as entry      # noqa: E402

pkg = entry.load_package()
from dehalo2_amd import circuits, native      # noqa: E402

F = pkg.fields
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(ts):
    ts = sorted(ts)
    return "min %8.2f  median %8.2f  max %8.2f ms (%d runs)" % (1e3 * ts[0], 1e3 * ts[len(ts) // 2], 1e3 * ts[-1], len(ts))


def timed(fn, runs, release=True):
    out = []
    for _ in range(runs):
        ctx.synchronize()
        t = time.perf_counter()
        r = fn()
        ctx.synchronize()
        out.append(time.perf_counter() - t)
        if release and hasattr(r, "release"):
            r.release()
    return out


say("# one MI355X, one process; whole host calls through ctypes on the host clock, one warm-up call each; pageable host buffers, touched beforehand")
with pkg.Context(0) as ctx:
    for k in (14, 17):
        curve = F.BN254
        circ = circuits.synthesize(curve.scalar.p, k, True, seed=3)
        cs, nsel = circ.cs, len(circ.selectors)
        params = native.ParamsKZG.setup(ctx, curve, k, 0x5EED)
        pk = native.ProvingKey.keygen(ctx, params, cs, circ.fixed, circ.assembly, circ.selectors)
        blobs = {fmt: pk.write(fmt) for fmt in ("processed", "raw", "raw-unchecked")}
        vk = pk.vk_bytes()
        say("k = %d: maingate with range lookups, BN254 / KZG; pk %d bytes (RawBytes), %d (Processed); vk %d bytes" % (k, len(blobs["raw"]), len(blobs["processed"]), len(vk)))
        runs = 5
        import ctypes as C
        lib = pkg.load_library()
        desc = native.ConstraintSystemDescriptor(cs, curve.scalar)
        fixed = np.ascontiguousarray(circ.fixed, dtype=np.uint64)
        mapping = np.ascontiguousarray(circ.assembly.mapping, dtype=np.uint64)
        sels = [np.ascontiguousarray(np.asarray(s, dtype=np.uint8)) for s in circ.selectors]
        sel_ptrs = (C.c_void_p * max(1, len(sels)))(*[s.ctypes.data for s in sels])
        vkb = np.frombuffer(vk, dtype=np.uint8)

        def c_keygen():
            h = C.c_void_p()
            t = time.perf_counter()
            rc = lib.dehalo_keygen(ctx.handle, params.handle, desc.ref(), fixed.ctypes.data, mapping.ctypes.data, sel_ptrs, len(sels), 1, C.byref(h))
            dt = time.perf_counter() - t
            assert rc == 0
            lib.dehalo_pk_release(ctx.handle, h)
            return dt

        def c_keygen_pk():
            h = C.c_void_p()
            t = time.perf_counter()
            rc = lib.dehalo_keygen_pk(ctx.handle, params.handle, desc.ref(), vkb.ctypes.data, vkb.size, 2, nsel, fixed.ctypes.data, mapping.ctypes.data, 1, C.byref(h))
            dt = time.perf_counter() - t
            assert rc == 0
            lib.dehalo_pk_release(ctx.handle, h)
            return dt

        out = np.empty(len(blobs["raw"]), dtype=np.uint8)
        out[:] = 0      # touched: no page faults inside the timed calls

        def c_write(fmt_id):
            t = time.perf_counter()
            rc = lib.dehalo_pk_write(ctx.handle, pk.handle, out.ctypes.data, out.size) if fmt_id is None else lib.dehalo_pk_write_custom(ctx.handle, pk.handle, fmt_id, out.ctypes.data, out.size)
            dt = time.perf_counter() - t
            assert rc == 0
            return dt

        c_keygen(); c_keygen_pk(); c_write(None)      # warm
        a, b = [], []
        for _ in range(runs):
            a.append(c_keygen())
            b.append(c_keygen_pk())
        say("  dehalo_keygen                          " + spread(a))
        say("  dehalo_keygen_pk (vk raw-unchecked)    " + spread(b))
        say("  dehalo_pk_write                        " + spread([c_write(None) for _ in range(runs)]))
        for name, fmt_id in (("processed", 0), ("raw", 1), ("raw-unchecked", 2)):
            say("  write_custom %-14s            " % name + spread([c_write(fmt_id) for _ in range(runs)]))
        # reads; the unchecked format alternates with dehalo_pk_read of the same bytes

        def read_c(data, fmt_id):
            buf = np.frombuffer(data, dtype=np.uint8)
            h = C.c_void_p()
            t = time.perf_counter()
            if fmt_id is None:
                rc = lib.dehalo_pk_read(ctx.handle, curve.id, desc.ref(), buf.ctypes.data, buf.size, nsel, C.byref(h))
            else:
                rc = lib.dehalo_pk_read_custom(ctx.handle, curve.id, desc.ref(), buf.ctypes.data, buf.size, fmt_id, nsel, C.byref(h))
            dt = time.perf_counter() - t
            assert rc == 0
            lib.dehalo_pk_release(ctx.handle, h)
            return dt

        read_c(blobs["raw"], None)      # warm
        a, b = [], []
        for _ in range(7):
            a.append(read_c(blobs["raw-unchecked"], None))
            b.append(read_c(blobs["raw-unchecked"], 2))
        say("  dehalo_pk_read                         " + spread(a))
        say("  read_custom raw-unchecked (alternating)" + spread(b))
        say("  read_custom raw                        " + spread([read_c(blobs["raw"], 1) for _ in range(runs)]))
        say("  read_custom processed                  " + spread([read_c(blobs["processed"], 0) for _ in range(runs)]))
        pk.release()
        params.release()

with open(OUT, "w") as fh:
    fh.write("\n".join(lines) + "\n")
