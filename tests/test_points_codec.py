"""GPU suite: the point codec -- dehalo_points_compress_device, dehalo_points_decompress_device, dehalo_points_check_device (csrc/gfft.cuh k_compress,
k_decompress, k_points_check) on all three curves, at counts around one block of 128 lanes.

compress equals the Python closed form (transcript.compress); decompress(compress(P)) == P, identities included; each status bit of decompress is raised by one
planted encoding at the first and at the last index and by nothing else; check passes good points with (0, 0) among them and names a stored word equal to p
(1) and the point (x, y + 1) (2)."""
import ctypes as C

import numpy as np
import pytest

CURVES = ["bn254", "pallas", "vesta"]
COUNTS = [1, 127, 128, 129, 300]      # 128 is one block
IDENTITIES = (1, 5, 126, 128, 299)    # rows made (0, 0) where the count reaches them


@pytest.fixture(scope="module")
def pts(pkg, co):
    """curve name -> (300 affine points as (300, 8) u64 Montgomery with identities at IDENTITIES, their GroupEncoding from transcript.compress): made once"""
    from dehalo2_amd import keygen, transcript
    out = {}
    for name in CURVES:
        cs = pkg.fields.CURVES[name]
        a = np.array(co.synth_bases(cs.id, 300), dtype=np.uint64).reshape(300, 8)
        for i in IDENTITIES:
            a[i] = 0
        dec = keygen.decode_points(cs, a)
        assert len({P[1] & 1 for P in dec if P is not None}) == 2      # both parities of y occur
        out[name] = (a, [transcript.compress(cs, P) for P in dec])
    return out


def _compress(ctx, cs, a):
    import torch
    d_in = ctx.upload(a)
    d_out = torch.full((a.shape[0], 4), -1, dtype=torch.int64, device=d_in.device)
    torch.cuda.synchronize()      # the library works on its own stream
    ctx.points_compress(cs.id, d_in.data_ptr(), a.shape[0], d_out.data_ptr())
    return ctx.download_tensor(d_out).tobytes()


def _decompress(ctx, cs, enc: bytes):
    import torch
    count = len(enc) // 32
    d_in = ctx.upload(np.frombuffer(enc, dtype=np.uint64).reshape(count, 4))
    d_out = torch.full((count, 8), -1, dtype=torch.int64, device=d_in.device)
    torch.cuda.synchronize()      # the library works on its own stream
    status = ctx.points_decompress(cs.id, d_in.data_ptr(), count, d_out.data_ptr())
    return status, ctx.download_tensor(d_out)


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", CURVES)
def test_compress_is_the_closed_form(pkg, ctx, pts, name, count):
    cs = pkg.fields.CURVES[name]
    a, enc = pts[name]
    assert _compress(ctx, cs, a[:count]) == b"".join(enc[:count])


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", CURVES)
def test_decompress_inverts_compress(pkg, ctx, pts, name, count):
    cs = pkg.fields.CURVES[name]
    a, enc = pts[name]
    status, back = _decompress(ctx, cs, b"".join(enc[:count]))
    assert status == 0 and np.array_equal(back, a[:count])


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", CURVES)
def test_decompress_status_bits(pkg, ctx, pts, name, count):
    from dehalo2_amd import transcript
    cs = pkg.fields.CURVES[name]
    p = cs.base.p
    a, enc = pts[name]
    off_curve = next(x for x in range(2, 1000) if transcript.sqrt_mod((x * x * x + cs.b) % p, p) is None)
    planted = {1: p.to_bytes(32, "little"), 2: off_curve.to_bytes(32, "little"), 4: (1 << 255).to_bytes(32, "little")}
    for bit, bad in planted.items():
        for at in sorted({0, count - 1}):
            e = list(enc[:count])
            e[at] = bad
            status, back = _decompress(ctx, cs, b"".join(e))
            assert status == bit, (bit, at)
            want = a[:count].copy()
            want[at] = 0                                         # the refused encoding is written as (0, 0), every other point as before
            assert np.array_equal(back, want), (bit, at)
    # the sign bit on an x that is not on the curve is still "not on the curve"; x = p + 1 with the sign bit is still "not below p"
    e = list(enc[:count])
    e[0] = (off_curve | (1 << 255)).to_bytes(32, "little")
    assert _decompress(ctx, cs, b"".join(e))[0] == 2
    if p + 1 < 1 << 255:
        e[0] = ((p + 1) | (1 << 255)).to_bytes(32, "little")
        assert _decompress(ctx, cs, b"".join(e))[0] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", CURVES)
def test_check_status_bits(pkg, ctx, pts, name, count):
    from dehalo2_amd import keygen
    cs = pkg.fields.CURVES[name]
    p = cs.base.p
    a, _ = pts[name]
    good = a[:count]
    assert ctx.points_check(cs.id, ctx.upload(good).data_ptr(), count) == 0      # (0, 0) among them from count 127 on
    live = [i for i in range(count) if good[i].any()]
    p_word = np.frombuffer(p.to_bytes(32, "little"), dtype=np.uint64)
    for at in sorted({0, count - 1}):
        for half in (0, 4):                                      # x's stored word = p, then y's
            bad = good.copy()
            bad[at, half:half + 4] = p_word
            assert ctx.points_check(cs.id, ctx.upload(bad).data_ptr(), count) == 1, (at, half)
    for at in sorted({live[0], live[-1]}) if live else []:
        x, y = keygen.decode_points(cs, good[at])[0]
        bad = good.copy()
        bad[at] = keygen.encode_points(cs, [(x, (y + 1) % p)])[0]
        assert ctx.points_check(cs.id, ctx.upload(bad).data_ptr(), count) == 2, at
        # and the two kinds together are reported together
        bad[0, :4] = p_word
        assert ctx.points_check(cs.id, ctx.upload(bad).data_ptr(), count) == (3 if at != 0 else 1), at


@pytest.mark.gpu
def test_argument_checks(pkg, ctx, pts):
    import torch
    lib = pkg.load_library()
    a, enc = pts["bn254"]
    d = ctx.upload(a[:4])
    e = torch.zeros((4, 4), dtype=torch.int64, device=d.device)
    torch.cuda.synchronize()
    st = C.c_uint32(9)
    # count = 0 returns 0 without a launch, whatever the pointers
    assert lib.dehalo_points_compress_device(ctx.handle, 0, None, 0, None, None) == 0
    assert lib.dehalo_points_decompress_device(ctx.handle, 0, None, 0, None, C.byref(st), None) == 0 and st.value == 0
    st.value = 9
    assert lib.dehalo_points_check_device(ctx.handle, 0, None, 0, C.byref(st), None) == 0 and st.value == 0
    for curve in (-1, 3):
        assert lib.dehalo_points_compress_device(ctx.handle, curve, d.data_ptr(), 4, e.data_ptr(), None) == -1
        assert lib.dehalo_points_decompress_device(ctx.handle, curve, e.data_ptr(), 4, d.data_ptr(), C.byref(st), None) == -1
        assert lib.dehalo_points_check_device(ctx.handle, curve, d.data_ptr(), 4, C.byref(st), None) == -1
    assert lib.dehalo_points_compress_device(ctx.handle, 0, d.data_ptr(), 1 << 29, e.data_ptr(), None) == -1
    assert lib.dehalo_points_check_device(ctx.handle, 0, d.data_ptr(), 1 << 29, C.byref(st), None) == -1
    assert lib.dehalo_points_decompress_device(ctx.handle, 0, e.data_ptr(), 4, d.data_ptr(), None, None) == -1      # no status word
    assert lib.dehalo_points_check_device(ctx.handle, 0, d.data_ptr() + 8, 3, C.byref(st), None) == -1               # points not 16-byte aligned
    assert ctx.points_check(0, d.data_ptr(), 4) == 0                                                                  # the context still works
