"""Every route to the same params gives the same object (csrc/params.hip: every constructor ends in one tail).

KZG over BN254 at k = 0, 1, 3 (k = 0: the one-point group FFT): from one setup(s), the params rebuilt by create, read, read_custom in the three formats, from_g,
downsize of a k = 4 setup and the prefix read of the k = 4 file write the same bytes in every format and commit one fixed polynomial to the same point in
both bases.
IPA over Pallas and Vesta at k = 1, 3 (k = 1: the smallest ParamsIPA, round 1 of the opening is the last): from generate, the params rebuilt by ipa_create,
ipa_from_g, ipa_read and downsize of generate(4) write the same bytes, commit to the same points and, under one seed, open the same polynomial to the same
transcript bytes -- the opening reads d_guw, bases_uw and W's fixed-base table, the parts only ParamsIPA's constructors build."""
import ctypes as C

import numpy as np
import pytest

S_TOXIC = 0x5EED5EED5EED5EED1234567
FORMATS = ["processed", "raw", "raw-unchecked"]


def _poly(scalar, n):
    """n distinct non-zero coefficients, Montgomery words"""
    return scalar.encode_many([(0x9E3779B97F4A7C15 * (i + 1) + 7) % scalar.p for i in range(n)])


def _commits(pkg, ctx, prm, d_poly):
    """dehalo_params_commit_device of the polynomial in the coefficient and the Lagrange basis: (2, 8) u64"""
    import torch
    out = torch.zeros((2, 8), dtype=torch.int64, device="cuda")
    lib = pkg.load_library()
    for lagrange in (0, 1):
        assert lib.dehalo_params_commit_device(ctx.handle, prm.handle, d_poly.data_ptr(), 1, lagrange, out[lagrange].data_ptr(), None) == 0
    got = ctx.download_tensor(out)
    assert got[0].any() and got[1].any()
    return got


def _files(pkg, ctx, prm):
    """dehalo_params_write's bytes and dehalo_params_write_custom's in each of the three formats"""
    from dehalo2_amd import native
    lib = pkg.load_library()
    out = {"write": prm.write()}
    for fmt in FORMATS:
        buf = np.empty(lib.dehalo_params_size_custom(prm.handle, native.SERDE_FORMATS[fmt]), dtype=np.uint8)
        native._check(ctx, lib.dehalo_params_write_custom(prm.handle, native.SERDE_FORMATS[fmt], buf.ctypes.data, buf.size))
        out[fmt] = buf.tobytes()
    return out


@pytest.fixture(scope="module")
def setup4(pkg, ctx):
    from dehalo2_amd import native
    prm = native.ParamsKZG.setup(ctx, pkg.fields.BN254, 4, S_TOXIC)
    yield prm, {fmt: prm.write(fmt) for fmt in FORMATS}
    prm.release()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 3])
def test_kzg_routes(pkg, ctx, setup4, k):
    from dehalo2_amd import keygen, native
    cs = pkg.fields.BN254
    big, big_files = setup4
    made = native.ParamsKZG.setup(ctx, cs, k, S_TOXIC)
    routes = {}
    try:
        files = _files(pkg, ctx, made)
        assert files["write"] == files["raw"] == files["raw-unchecked"] and len(files["processed"]) == 4 + 64 * (1 << k) + 128
        _, g, gl, g2, s_g2 = keygen.params_from_bytes(cs, files["raw-unchecked"], "raw-unchecked")
        d_poly = ctx.upload(_poly(cs.scalar, 1 << k))
        want = _commits(pkg, ctx, made, d_poly)
        routes["create"] = native.ParamsKZG.create(ctx, cs, k, g, gl, g2, s_g2)
        routes["read"] = native.ParamsKZG.read(ctx, cs, files["raw-unchecked"])
        for fmt in FORMATS:
            h = C.c_void_p()
            buf = np.frombuffer(files[fmt], dtype=np.uint8)
            native._check(ctx, pkg.load_library().dehalo_params_read_custom(ctx.handle, cs.id, buf.ctypes.data, buf.size, native.SERDE_FORMATS[fmt], native.KEEP_K, C.byref(h)))
            routes["read_custom " + fmt] = native.ParamsKZG(ctx, cs, h)
            routes["prefix read " + fmt] = native.ParamsKZG.read(ctx, cs, big_files[fmt], format=fmt, downsize=k)
        routes["from_g"] = native.ParamsKZG.from_g(ctx, cs, k, g, g2, s_g2)
        routes["downsize"] = big.downsize(k)
        for name, prm in routes.items():
            assert _files(pkg, ctx, prm) == files, name
            assert np.array_equal(_commits(pkg, ctx, prm, d_poly), want), name
    finally:
        for prm in [made] + list(routes.values()):
            prm.release()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_ipa_routes(pkg, ctx, curve, k):
    from dehalo2_amd import keygen, native
    from dehalo2_amd.prover import SeededRng
    cs = pkg.fields.CURVES[curve]
    made = native.ParamsIPA.generate(ctx, cs, k)
    big = native.ParamsIPA.generate(ctx, cs, 4)
    routes = {}
    try:
        data = made.write()
        _, g, gl, w, u = keygen.params_ipa_from_bytes(cs, data)
        d_poly = ctx.upload(_poly(cs.scalar, 1 << k))
        blind, x3 = 0xB11D + k, 0x1234567 + k

        def observed(prm):
            return prm.write(), _commits(pkg, ctx, prm, d_poly), prm.open(d_poly.data_ptr(), blind, x3, rng=SeededRng(11)).finalize()

        want = observed(made)
        assert want[0] == data and len(want[2]) == 32 + 64 * k + 64
        routes["ipa_create"] = native.ParamsIPA.create(ctx, cs, k, g, gl, w, u)
        routes["ipa_from_g"] = native.ParamsIPA.from_g(ctx, cs, k, g, w, u)
        routes["ipa_read"] = native.ParamsIPA.read(ctx, cs, data)
        routes["downsize"] = big.downsize(k)      # (generated points: g of k = 4 starts with g of k, W and U do not depend on k)
        for name, prm in routes.items():
            got = observed(prm)
            assert got[0] == want[0], name
            assert np.array_equal(got[1], want[1]), name
            assert got[2] == want[2], name
    finally:
        for prm in [made, big] + list(routes.values()):
            prm.release()
