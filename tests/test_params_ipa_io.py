"""ParamsIPA from g alone and on disk: dehalo_params_ipa_from_g, dehalo_params_ipa_size / _write / _read and their Python mirror
(keygen.params_ipa_bytes / params_ipa_from_bytes).

CPU: the mirror round-trips (an identity point and a point with odd y included) and lays the bytes out as ParamsIPA::write does; the header
declares the five entry points; without a device each of them is an error, not a crash.
GPU: a whole ProverIPA proof under ParamsIPA.from_g(g, w, u) is byte for byte the proof under ParamsIPA.create(g, g_lagrange, w, u) with the
oracle's g_lagrange, and is accepted; write() equals the mirror's bytes; read(write()) writes the same bytes and proves the same proof; malformed
input is refused with DEHALO_ERR_INVALID and the context keeps working."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT
from test_ipa_proof import F, accepts, ipa_chain      # noqa: F401  (fixtures and the verifier call of the ProverIPA tests)

NEW_SYMBOLS = ["dehalo_g_to_lagrange_device", "dehalo_params_ipa_from_g", "dehalo_params_ipa_size", "dehalo_params_ipa_write", "dehalo_params_ipa_read"]


def _points(pkg, curve, count, seed):
    """`count` affine points (canonical ints) found by decompressing x = seed, seed + 1, ...; both parities of y occur"""
    from dehalo2_amd import transcript
    out, x = [], seed
    while len(out) < count:
        try:
            P = transcript.decompress(curve, (x | ((len(out) & 1) << 255)).to_bytes(32, "little"))
            if P is not None:
                out.append(P)
        except ValueError:
            pass
        x += 1
    return out


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def test_mirror_round_trips(pkg):
    from dehalo2_amd import keygen
    curve = pkg.fields.VESTA
    k = 3
    pts = _points(pkg, curve, 18, 1000)
    pts[2] = None                                                # an identity point
    assert any(P is not None and P[1] & 1 for P in pts) and any(P is not None and not P[1] & 1 for P in pts)
    enc = keygen.encode_points(curve, pts)
    g, gl, w, u = enc[:8], enc[8:16], enc[16], enc[17]
    data = keygen.params_ipa_bytes(curve, k, g, gl, w, u)
    assert len(data) == 4 + 64 * 8 + 64
    k2, g2, gl2, w2, u2 = keygen.params_ipa_from_bytes(curve, data)
    assert k2 == k and np.array_equal(g2, g) and np.array_equal(gl2, gl) and np.array_equal(w2, w) and np.array_equal(u2, u)
    assert keygen.params_ipa_bytes(curve, k2, g2, gl2, w2, u2) == data
    with pytest.raises(ValueError):
        keygen.params_ipa_from_bytes(curve, data[:-1])
    with pytest.raises(ValueError):
        keygen.params_ipa_from_bytes(curve, data + b"\0")


def test_mirror_layout_at_k1(pkg):
    from dehalo2_amd import keygen
    curve = pkg.fields.PALLAS
    P = _points(pkg, curve, 6, 2000)
    P[1] = None

    def comp(Q):      # GroupEncoding::to_bytes by hand
        if Q is None:
            return bytes(32)
        b = bytearray(Q[0].to_bytes(32, "little"))
        b[31] |= (Q[1] & 1) << 7
        return bytes(b)

    enc = keygen.encode_points(curve, P)
    want = struct.pack("<I", 1) + comp(P[0]) + comp(P[1]) + comp(P[2]) + comp(P[3]) + comp(P[4]) + comp(P[5])      # k | g[0] g[1] | gl[0] gl[1] | w | u
    assert keygen.params_ipa_bytes(curve, 1, enc[0:2], enc[2:4], enc[4], enc[5]) == want
    assert len(want) == 4 + 64 * 2 + 64 and want[:4] == b"\x01\x00\x00\x00"


def test_header_declares_the_new_entry_points(pkg):
    txt = open(os.path.join(ROOT, "include", "dehalo.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(lib, s), s


def test_no_device_means_error_not_fallback(pkg):
    lib = pkg.load_library()
    h = C.c_void_p()
    buf = (C.c_uint64 * 16)()
    raw = (C.c_uint8 * 196)()
    raw[0] = 1
    assert lib.dehalo_g_to_lagrange_device(None, 2, buf, 1, buf, None) == -1
    assert lib.dehalo_params_ipa_from_g(None, 2, 1, buf, buf, buf, C.byref(h)) == -1 and not h.value
    assert lib.dehalo_params_ipa_read(None, 2, raw, 196, C.byref(h)) == -1 and not h.value
    assert lib.dehalo_params_ipa_size(None) == 0
    assert lib.dehalo_params_ipa_write(None, raw, 196) == -1


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _prove(pkg, ctx, c, params):
    from dehalo2_amd import native, prover
    pk = native.ProvingKey.keygen(ctx, params, c["circ"].cs, c["circ"].fixed, c["circ"].assembly, c["circ"].selectors)
    pk.transcript_repr = c["rep"]
    P = native.Prover(params, pk)
    try:
        return P.create_proof(c["adv"], [[]], prover.SeededRng(7)).finalize()
    finally:
        P.release()
        pk.release()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 11])
def test_from_g_write_read(pkg, po, co, F, ctx, ipa_chain, k):
    from dehalo2_amd import keygen, native
    c = ipa_chain(k, False)
    cs = pkg.fields.VESTA
    g, gl = c["srs"]["g"], c["srs"]["g_lagrange"]
    lib = pkg.load_library()
    made = native.ParamsIPA.from_g(ctx, cs, k, g, c["w"], c["u"])
    given = native.ParamsIPA.create(ctx, cs, k, g, gl, c["w"], c["u"])
    back = None
    try:
        # from_g == create with the oracle's g_lagrange: the same proof, accepted
        proof = _prove(pkg, ctx, c, made)
        assert proof == _prove(pkg, ctx, c, given)
        assert accepts(po, c, proof)
        # write() is the mirror's bytes; dehalo_params_size stays 0 for IPA params
        data = made.write()
        assert len(data) == 4 + 64 * (1 << k) + 64 == lib.dehalo_params_ipa_size(made.handle)
        assert data == keygen.params_ipa_bytes(cs, k, g, gl, c["w"], c["u"])
        assert data == given.write()
        assert lib.dehalo_params_size(made.handle) == 0
        # read(write()) writes the same bytes and proves the same proof
        back = native.ParamsIPA.read(ctx, cs, data)
        assert lib.dehalo_params_scheme(back.handle) == 1
        assert back.write() == data
        assert _prove(pkg, ctx, c, back) == proof
    finally:
        for prm in (made, given, back):
            if prm is not None:
                prm.release()


@pytest.mark.gpu
def test_sizes_across_schemes(pkg, ctx):
    from dehalo2_amd import native
    lib = pkg.load_library()
    kzg = native.ParamsKZG.setup(ctx, pkg.fields.BN254, 4, 12345)
    try:
        assert lib.dehalo_params_size(kzg.handle) == 4 + 2 * 64 * 16 + 256
        assert lib.dehalo_params_ipa_size(kzg.handle) == 0
        out = np.zeros(4096, dtype=np.uint8)
        assert lib.dehalo_params_ipa_write(kzg.handle, out.ctypes.data, out.size) == -5
    finally:
        kzg.release()


@pytest.mark.gpu
def test_malformed_input_is_refused(pkg, ctx, co):
    from dehalo2_amd import native, transcript
    cs, k = pkg.fields.VESTA, 4
    n, p = 1 << k, pkg.fields.VESTA.base.p
    lib = pkg.load_library()
    g = co.synth_bases(cs.id, n)
    uw = co.fixed_base_mul(cs.id, cs.scalar.encode_many([3, 5]))
    prm = native.ParamsIPA.from_g(ctx, cs, k, g, uw[0], uw[1])
    good = prm.write()
    prm.release()

    def rc_of(data):
        h = C.c_void_p()
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        rc = lib.dehalo_params_ipa_read(ctx.handle, cs.id, buf.ctypes.data, buf.size, C.byref(h))
        assert rc == 0 or not h.value
        if rc == 0:
            lib.dehalo_params_release(ctx.handle, h)
        return rc

    def with_point(i, enc):
        return good[:4 + 32 * i] + enc + good[4 + 32 * (i + 1):]

    off_curve = next(x for x in range(2, 1000) if transcript.sqrt_mod((x * x * x + cs.b) % p, p) is None)
    with pytest.raises(ValueError):
        transcript.decompress(cs, off_curve.to_bytes(32, "little"))
    cases = {
        "truncated": good[:-1],
        "truncated to the header": good[:4],
        "one byte too many": good + b"\0",
        "k does not match the length": struct.pack("<I", k + 1) + good[4:],
        "x not below p (g)": with_point(3, p.to_bytes(32, "little")),
        "x not below p (u)": with_point(2 * n + 1, (p + 5).to_bytes(32, "little")),
        "x off the curve (g_lagrange)": with_point(n + 2, off_curve.to_bytes(32, "little")),
        "x off the curve, sign set (w)": with_point(2 * n, (off_curve | (1 << 255)).to_bytes(32, "little")),
        "x = 0 with the sign bit set": with_point(5, (1 << 255).to_bytes(32, "little")),
    }
    for name, data in cases.items():
        assert rc_of(data) == -1, name
        assert lib.dehalo_last_error(ctx.handle).decode().startswith("params_ipa_read:"), name
        assert rc_of(good) == 0, "a valid read after: " + name
    # an identity point is an encoding (all zeros) and reads back
    ident = with_point(1, bytes(32))
    back = native.ParamsIPA.read(ctx, cs, ident)
    assert back.write() == ident
    back.release()
