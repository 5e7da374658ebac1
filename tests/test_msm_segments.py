"""Many short independent sums in one launch (dehalo_msm_segments / dehalo_msm_segments_device, csrc/msm_segments.cuh) on all three curves, against the C
restatement of best_multiexp per segment and closed forms.

CPU: both entry points refuse a null context; the Python wrapper refuses offsets that reach past the terms.
GPU: segment lengths 0, 1, 2, 3, 63, 64, 65, 100, 257 (a block has 128 quads, one per term: below, at and above one and two strides, and an empty segment) in one
call; 1, 2 and 129 segments; a first offset above zero; a call whose every segment is empty; the device form on an output filled beforehand.  The group law's
exceptional cases, which a proof's points can bring about at will: one point listed many times with scalars that sum to 0 mod r; P next to -P; identity points
inside a segment; zero scalars and the scalar r - 1; equal points under equal scalars in 2, 64, 128 and 256 terms, so that the addition inside a quad, every level
of the fold inside a wave and the fold across waves each meet a doubling; scalar words not below r, against their residues.  The refusals: an unknown curve, null
arguments, offsets that decrease (the device form leaves the output untouched), more segments and more terms than the limits."""
import ctypes as C

import numpy as np
import pytest

CURVES = ["bn254", "pallas", "vesta"]
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 100, 257]
POOL = sum(LENGTHS) + 5


def offsets_of(lengths, first=0):
    return np.concatenate([[first], first + np.cumsum(lengths)]).astype(np.uint32)


def expected(co, cs, scalars, points, offsets):
    """the C restatement's best_multiexp of every segment, affine; an empty segment is the identity"""
    out = np.zeros((len(offsets) - 1, 8), dtype=np.uint64)
    for s in range(len(offsets) - 1):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        if hi > lo:
            out[s] = co.to_affine(cs.id, co.best_multiexp(cs.id, np.ascontiguousarray(scalars[lo:hi]), np.ascontiguousarray(points[lo:hi]), 1))
    return out


def negated(cs, point):
    f = cs.base
    out = np.array(point, dtype=np.uint64).reshape(8)
    out[4:] = f.encode((f.p - f.decode(out[4:])) % f.p)
    return out


def device_form(ctx, cs, scalars, points, offsets):
    """dehalo_msm_segments_device on uploaded inputs and an output filled with ones beforehand -> (return code, the output)"""
    import torch
    segments = len(offsets) - 1
    ds = ctx.upload(np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4))
    dp = ctx.upload(np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8))
    do = ctx.upload(np.ascontiguousarray(offsets, dtype=np.uint32))
    out = torch.empty((segments, 8), dtype=torch.int64, device=do.device)
    with ctx.torch_stream():
        out.fill_(-1)
    rc = ctx.lib.dehalo_msm_segments_device(ctx.handle, cs.id, ds.data_ptr(), dp.data_ptr(), do.data_ptr(), segments, out.data_ptr(), None)
    return rc, ctx.download_tensor(out)


@pytest.fixture(scope="module")
def pool(pkg, co):
    """curve name -> (curve, POOL uniform scalars, POOL points, best_multiexp of the LENGTHS segments over them): computed once, read by every test"""
    cache = {}

    def get(name):
        if name not in cache:
            cs = pkg.fields.CURVES[name]
            scalars = co.fill_scalars(cs.scalar.id, "uniform", POOL, 77)
            points = co.synth_bases(cs.id, POOL)
            want = expected(co, cs, scalars, points, offsets_of(LENGTHS))
            for a in (scalars, points, want):
                a.setflags(write=False)
            cache[name] = (cs, scalars, points, want)
        return cache[name]
    return get


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def test_msm_segments_is_refused_without_a_context(pkg):
    lib = pkg.load_library()
    off = (C.c_uint32 * 2)(0, 0)
    out = (C.c_uint64 * 8)()
    assert lib.dehalo_msm_segments(None, 0, None, None, off, 1, out) == -1
    assert lib.dehalo_msm_segments_device(None, 0, None, None, off, 1, out, None) == -1


# ------------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", CURVES)
def test_segment_lengths_and_counts(ctx, co, pool, curve_name):
    cs, scalars, points, want = pool(curve_name)
    off = offsets_of(LENGTHS)
    got = ctx.msm_segments(cs.id, scalars, points, off)
    assert np.array_equal(got, want)
    assert not want[0].any() and want[1:].any(axis=1).all()      # the empty segment is (0, 0), no other sum is
    rc, dev = device_form(ctx, cs, scalars, points, off)
    assert rc == 0 and np.array_equal(dev, want)                  # the device form writes every output, the empty segment's too
    # one segment; two; a first offset above zero (what stands below it is not read: here it is not even a point)
    assert np.array_equal(ctx.msm_segments(cs.id, scalars, points, [off[7], off[8]]), want[7:8])
    assert np.array_equal(ctx.msm_segments(cs.id, scalars, points, off[5:8]), want[5:7])
    junk = np.array(points)
    junk[:int(off[4])] = 1
    assert np.array_equal(ctx.msm_segments(cs.id, scalars, junk, off[4:]), want[4:])
    # 129 segments of 0 .. 4 terms: more blocks than one launch wave of a CU, most of them with idle quads
    lens = [(3 * i + 1) % 5 for i in range(129)]
    off = offsets_of(lens)
    assert np.array_equal(ctx.msm_segments(cs.id, scalars, points, off), expected(co, cs, scalars, points, off))


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", CURVES)
def test_every_segment_empty(ctx, pool, curve_name):
    cs, scalars, points, _ = pool(curve_name)
    for off in ([0, 0], [5, 5, 5, 5], [0] * 130):
        assert not ctx.msm_segments(cs.id, scalars, points, off).any()
        rc, dev = device_form(ctx, cs, scalars, points, off)
        assert rc == 0 and not dev.any()
    assert not ctx.msm_segments(cs.id, np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 8), dtype=np.uint64), [0, 0, 0]).any()      # no term at all
    assert ctx.msm_segments(cs.id, scalars, points, [3]).shape == (0, 8)                                                          # no segment at all


def exceptional_segments(co, cs, scalars, points):
    """-> (scalars, points, offsets, closed forms: {segment: the affine point it must be}) of one call that meets every exceptional case of the group law"""
    f, r = cs.scalar, cs.scalar.p
    P, Q = points[0], points[1]
    ints = [int(f.decode(scalars[i])) for i in range(140)]
    mul = lambda k, pt: co.to_affine(cs.id, co.best_multiexp(cs.id, f.encode_many([k % r]), np.ascontiguousarray(pt).reshape(1, 8), 1))
    zero = np.zeros(8, dtype=np.uint64)
    segs, closed = [], {}

    def add(terms, want=None):
        if want is not None:
            closed[len(segs)] = want
        segs.append(terms)
    add([(k, P) for k in ints[:3]] + [(-sum(ints[:3]), P)], zero)                     # one point, scalars summing to 0 mod r
    add([(k, P) for k in ints[:129]] + [(-sum(ints[:129]), P)], zero)                 # the same over 130 terms: two strides of the block
    add([(ints[3], P), (ints[3], negated(cs, P))], zero)                              # P next to -P
    add([(ints[4], Q), (ints[3], P), (ints[3], negated(cs, P))], mul(ints[4], Q))     # ... beside another term
    add([(ints[5], zero), (ints[6], Q), (ints[7], zero)], mul(ints[6], Q))            # identity points inside a segment
    add([(ints[5], zero)] * 3, zero)
    add([(0, P), (ints[8], Q), (0, Q)], mul(ints[8], Q))                              # zero scalars
    add([(0, P), (0, Q)], zero)
    add([(r - 1, P)], negated(cs, P))                                                 # [r - 1] P = -P
    add([(r - 1, P), (1, P)], zero)
    add([(r - 1, P), (2, P)], np.array(P))
    for copies in (2, 64, 128, 256):                                                  # equal points under equal scalars: the fold meets doublings
        add([(ints[9], P)] * copies, mul(copies * ints[9], P))
    add([(ints[10], P)] * 3 + [(ints[11], Q)] * 2, None)                              # (checked against best_multiexp alone)
    sc = f.encode_many([k % r for seg in segs for k, _ in seg])
    pt = np.stack([np.asarray(p, dtype=np.uint64).reshape(8) for seg in segs for _, p in seg])
    return sc, pt, offsets_of([len(seg) for seg in segs]), closed


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", CURVES)
def test_exceptional_cases_of_the_group_law(ctx, co, pool, curve_name):
    cs, scalars, points, _ = pool(curve_name)
    sc, pt, off, closed = exceptional_segments(co, cs, scalars, points)
    want = expected(co, cs, sc, pt, off)
    for s, point in closed.items():      # the reference agrees with the closed forms before the kernel is asked
        assert np.array_equal(want[s], point), s
    got = ctx.msm_segments(cs.id, sc, pt, off)
    for s in range(len(off) - 1):
        assert np.array_equal(got[s], want[s]), "segment %d" % s
    rc, dev = device_form(ctx, cs, sc, pt, off)
    assert rc == 0 and np.array_equal(dev, want)


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", CURVES)
def test_scalar_words_not_below_r_stand_for_their_residue(ctx, pool, curve_name):
    cs, scalars, points, want = pool(curve_name)
    r = cs.scalar.p
    words = [int.from_bytes(np.ascontiguousarray(row).tobytes(), "little") for row in scalars]
    top = lambda w: w + r * (((1 << 256) - 1 - w) // r)
    lifted = [top(w) if i % 3 == 0 else w + r if i % 3 == 1 else w for i, w in enumerate(words)]      # the largest word of the residue, one r above it, the word itself
    assert all(v < 1 << 256 and v % r == w for v, w in zip(lifted, words)) and sum(v >= r for v in lifted) >= 2 * len(words) // 3
    raw = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in lifted), dtype=np.uint64).reshape(-1, 4)
    assert np.array_equal(ctx.msm_segments(cs.id, raw, points, offsets_of(LENGTHS)), want)
    zero_mod_r = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in (r, 2 * r, 0)), dtype=np.uint64).reshape(-1, 4)      # zero is zero mod r
    assert not ctx.msm_segments(cs.id, zero_mod_r, points[:3], [0, 3]).any()


@pytest.mark.gpu
def test_refusals(pkg, ctx, pool):
    cs, scalars, points, want = pool("bn254")
    lib = ctx.lib
    s, p = np.ascontiguousarray(scalars[:8]), np.ascontiguousarray(points[:8])
    out = np.full((4, 8), 7, dtype=np.uint64)

    def host(curve, sc, pt, off, segments, o):
        off = None if off is None else np.asarray(off, dtype=np.uint32)
        return lib.dehalo_msm_segments(ctx.handle, curve, None if sc is None else sc.ctypes.data, None if pt is None else pt.ctypes.data,
                                       None if off is None else off.ctypes.data, segments, None if o is None else o.ctypes.data)
    assert host(3, s, p, [0, 8], 1, out) == -1 and host(-1, s, p, [0, 8], 1, out) == -1      # an unknown curve
    assert host(0, s, p, None, 1, out) == -1 and host(0, s, p, [0, 8], 1, None) == -1          # no offsets, nowhere to write
    assert host(0, None, p, [0, 8], 1, out) == -1 and host(0, s, None, [0, 8], 1, out) == -1   # terms without scalars or points
    assert host(0, s, p, [0, 5, 3], 2, out) == -1 and host(0, s, p, [8, 0], 1, out) == -1      # offsets that decrease
    assert "decrease" in lib.dehalo_last_error(ctx.handle).decode()
    assert host(0, s, p, [0, 8], (1 << 24) + 1, out) == -1                                     # refused before an offset is read
    assert host(0, s, p, [0, (1 << 30) + 1], 1, out) == -1                                     # refused before a term is read
    assert (out == 7).all()
    assert host(0, None, None, [4, 4], 1, out) == 0 and not out[0].any()                       # no term: scalars and points may be null
    with pytest.raises(pkg.DehaloError) as e:
        ctx.msm_segments(cs.id, s, p, [0, 6, 2])
    assert e.value.code == -1
    with pytest.raises(ValueError):
        ctx.msm_segments(cs.id, s, p, [0, 9])      # the offsets reach past the terms
    with pytest.raises(ValueError):
        ctx.msm_segments(cs.id, s, p[:7], [0, 7])
    rc, dev = device_form(ctx, cs, s, p, [0, 5, 3])      # the device form checks before it launches: the output is as it was
    assert rc == -1 and (dev == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    rc, dev = device_form(ctx, cs, s, p, [0, 3])         # ... and the context still works
    assert rc == 0 and np.array_equal(dev[0], ctx.msm_segments(cs.id, s, p, [0, 3])[0]) and dev.any()
