"""GPU suite: ParamsKZG from any SRS -- dehalo_params_from_g, dehalo_params_downsize, dehalo_params_size_custom / _write_custom / _read_custom.

The results have closed forms: setup(k', s) is what downsize(setup(k, s), k') and from_g(setup(k', s).g) must equal, byte for byte -- two independent device
computations of g_lagrange, [L_i(s)] G and the group FFT, set against each other.  The formats are pinned by the Python mirror (keygen.params_bytes) and by round
trips; the prefix read by a file whose g_lagrange section is overwritten; malformed input by DEHALO_ERR_INVALID and a good read on the same context afterwards.
BN254 unless said; `write` is dehalo_params_write throughout."""
import ctypes as C
import struct

import numpy as np
import pytest

from test_ipa_proof import F, ipa_chain      # noqa: F401  (the IPA fixtures: the k = 6 params)

S_TOXIC = 0x5EED5EED5EED5EED1234567
FORMATS = ["processed", "raw", "raw-unchecked"]
INVALID, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def srs(pkg, ctx):
    """k -> (write(setup(k, s)), its parts (k, g, g_lagrange, g2, s_g2)): each size set up once, its bytes kept, the params released"""
    from dehalo2_amd import keygen, native
    cache = {}

    def get(k):
        if k not in cache:
            prm = native.ParamsKZG.setup(ctx, pkg.fields.BN254, k, S_TOXIC)
            data = prm.write()
            prm.release()
            cache[k] = (data, keygen.params_from_bytes(pkg.fields.BN254, data, "raw-unchecked"))
        return cache[k]
    return get


@pytest.fixture(scope="module")
def setup8(pkg, ctx):
    from dehalo2_amd import native
    prm = native.ParamsKZG.setup(ctx, pkg.fields.BN254, 8, S_TOXIC)
    yield prm
    prm.release()


def _written(prm):
    try:
        return prm.write()
    finally:
        prm.release()


def _rc_read(pkg, ctx, data, fmt, downsize=None):
    """dehalo_params_read_custom's return code; whatever it made is released"""
    from dehalo2_amd import native
    lib = pkg.load_library()
    h = C.c_void_p()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    rc = lib.dehalo_params_read_custom(ctx.handle, 0, buf.ctypes.data, buf.size, native.SERDE_FORMATS[fmt], native.KEEP_K if downsize is None else downsize, C.byref(h))
    assert rc == 0 or not h.value
    if rc == 0:
        lib.dehalo_params_release(ctx.handle, h)
    return rc


# ------------------------------------------------------------------------------------------------------------------------------ from_g, downsize
@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2, 5, 8])
def test_from_g_equals_setup(pkg, ctx, srs, k):
    """[L_i(s)] G against the group FFT of [s^i] G; k = 0 has no FFT stage"""
    from dehalo2_amd import native
    data, (_, g, _, g2, s_g2) = srs(k)
    assert _written(native.ParamsKZG.from_g(ctx, pkg.fields.BN254, k, g, g2, s_g2)) == data


@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, 5, 1, 0])
def test_downsize_kzg_equals_setup(pkg, ctx, srs, setup8, k):
    assert _written(setup8.downsize(k)) == srs(k)[0]
    assert setup8.write() == srs(8)[0]                           # the params that were downsized stay as they were


@pytest.mark.gpu
def test_downsize_above_k_is_refused(pkg, ctx, setup8):
    lib = pkg.load_library()
    h = C.c_void_p()
    assert lib.dehalo_params_downsize(ctx.handle, setup8.handle, 9, C.byref(h)) == INVALID and not h.value
    assert lib.dehalo_last_error(ctx.handle).decode().startswith("params_downsize:")


@pytest.mark.gpu
def test_downsize_ipa(pkg, ctx, F, ipa_chain):
    from dehalo2_amd import native
    c = ipa_chain(6, False)
    g, gl = c["srs"]["g"], c["srs"]["g_lagrange"]
    P6 = native.ParamsIPA.create(ctx, F.VESTA, 6, g, gl, c["w"], c["u"])
    try:
        small = P6.downsize(3)
        assert isinstance(small, native.ParamsIPA) and pkg.load_library().dehalo_params_scheme(small.handle) == 1
        assert small.fixed_base.handle                           # its own table of W
        got = _written(small)
        assert got == _written(native.ParamsIPA.from_g(ctx, F.VESTA, 3, np.asarray(g).reshape(-1, 8)[:8], c["w"], c["u"]))
        assert len(got) == 4 + 64 * 8 + 64
        assert _written(P6.downsize(6)) == P6.write()            # k equal to the params': an equal copy
    finally:
        P6.release()


@pytest.mark.gpu
def test_proof_under_downsized_params(pkg, ctx, setup8):
    """One seeded proof at k = 6: the tables registered by downsize(setup(8), 6) are the small ones, those of setup(6)"""
    import test_rotations
    from dehalo2_amd import native, prover
    k = 6
    cs, fixed, advice, asm = test_rotations.build_circuit(pkg, "R9all", k)

    def prove(params):
        pk = native.ProvingKey.keygen(ctx, params, cs, fixed, asm, ())
        P = native.Prover(params, pk)
        try:
            return P.create_proof(advice, [], prover.SeededRng(7), canonical=True).finalize()
        finally:
            P.release(); pk.release(); params.release()

    want = prove(native.ParamsKZG.setup(ctx, pkg.fields.BN254, k, S_TOXIC))
    assert len(want) > 0 and prove(setup8.downsize(k)) == want


# ------------------------------------------------------------------------------------------------------------------------------ formats
@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 7])
def test_formats(pkg, ctx, srs, k):
    from dehalo2_amd import keygen, native
    lib = pkg.load_library()
    cs = pkg.fields.BN254
    raw, (_, g, gl, g2, s_g2) = srs(k)
    prm = native.ParamsKZG.read(ctx, cs, raw)
    try:
        assert prm.write("raw") == raw and prm.write("raw-unchecked") == raw
        processed = prm.write("processed")
        assert processed == keygen.params_bytes(cs, k, g, gl, g2, s_g2, "processed")
        for fmt, data in (("processed", processed), ("raw", raw), ("raw-unchecked", raw)):
            assert lib.dehalo_params_size_custom(prm.handle, native.SERDE_FORMATS[fmt]) == len(data) == keygen.params_size(k, fmt)
            back = native.ParamsKZG.read(ctx, cs, data, format=fmt)
            try:
                assert back.write(fmt) == data
                assert back.write() == raw                       # Processed read back and written raw is the original raw file
            finally:
                back.release()
        assert lib.dehalo_params_size_custom(prm.handle, 3) == 0
        out = np.zeros(len(raw), dtype=np.uint8)
        assert lib.dehalo_params_write_custom(prm.handle, 3, out.ctypes.data, out.size) == INVALID
        assert lib.dehalo_params_write_custom(prm.handle, 0, out.ctypes.data, len(processed) - 1) == INVALID      # buffer too small
    finally:
        prm.release()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_prefix_read(pkg, ctx, srs, setup8, fmt):
    """read_custom(file at k = 8, downsize_k = 5) is setup(5, s) -- also when the file's g_lagrange section is 0xff throughout: only the prefix of g is read"""
    from dehalo2_amd import native
    cs = pkg.fields.BN254
    data = setup8.write(fmt)
    n, g1 = 256, 32 if fmt == "processed" else 64
    assert _written(native.ParamsKZG.read(ctx, cs, data, format=fmt, downsize=5)) == srs(5)[0]
    scribbled = data[:4 + g1 * n] + b"\xff" * (g1 * n) + data[4 + 2 * g1 * n:]
    assert len(scribbled) == len(data) and scribbled != data
    assert _written(native.ParamsKZG.read(ctx, cs, scribbled, format=fmt, downsize=5)) == srs(5)[0]
    # ... and beyond the prefix of g itself
    beyond = data[:4 + g1 * 32] + b"\xff" * (g1 * (2 * n - 32)) + data[4 + 2 * g1 * n:]
    assert _written(native.ParamsKZG.read(ctx, cs, beyond, format=fmt, downsize=5)) == srs(5)[0]
    assert _written(native.ParamsKZG.read(ctx, cs, data, format=fmt, downsize=8)) == srs(8)[0]      # downsize_k = k: g_lagrange from the FFT, equal to the file's
    assert _written(native.ParamsKZG.read(ctx, cs, data, format=fmt, downsize=0)) == srs(0)[0]
    assert _rc_read(pkg, ctx, data, fmt, 9) == INVALID
    if fmt != "raw-unchecked":      # the whole file is read without downsize_k: the scribble is found
        assert _rc_read(pkg, ctx, scribbled, fmt) == INVALID


# ------------------------------------------------------------------------------------------------------------------------------ malformed input
@pytest.mark.gpu
def test_malformed_input_is_refused(pkg, ctx, srs):
    from dehalo2_amd import keygen, native, transcript
    lib = pkg.load_library()
    cs, k = pkg.fields.BN254, 3
    n, p = 1 << k, cs.base.p
    raw, (_, g, gl, g2, s_g2) = srs(k)
    files = {"processed": keygen.params_bytes(cs, k, g, gl, g2, s_g2, "processed"), "raw": raw, "raw-unchecked": raw}

    def refused(name, data, fmt, kind):
        assert _rc_read(pkg, ctx, data, fmt) == INVALID, name
        msg = lib.dehalo_last_error(ctx.handle).decode()
        assert msg.startswith("params_read") and kind in msg, (name, msg)
        assert _rc_read(pkg, ctx, files[fmt], fmt) == 0, "a good read after: " + name

    for fmt in FORMATS:
        good = files[fmt]
        refused("one byte short", good[:-1], fmt, "length")
        refused("one byte long", good + b"\0", fmt, "length")
        refused("k field 29", struct.pack("<I", 29) + good[4:], fmt, "k out of range")
    assert _rc_read(pkg, ctx, raw, "raw", None) == 0 and _rc_read(pkg, ctx, raw[:3], "raw", None) == INVALID

    # Processed: the three bad encodings at g[0], g[n - 1] and inside g_lagrange
    off_curve = next(x for x in range(2, 1000) if transcript.sqrt_mod((x * x * x + cs.b) % p, p) is None)
    bad = {"not below the modulus": p.to_bytes(32, "little"), "not on the curve": off_curve.to_bytes(32, "little"), "sign bit": (1 << 255).to_bytes(32, "little")}
    good = files["processed"]
    for kind, enc in bad.items():
        for i in (0, n - 1, n + 2):
            refused("%s at %d" % (kind, i), good[:4 + 32 * i] + enc + good[4 + 32 * (i + 1):], "processed", kind)
    refused("G2 x.c1 = q", good[:-32] + p.to_bytes(32, "little"), "processed", "G2")

    # RAW_BYTES: (x, y + 1), a stored word equal to p, a G2 point off the curve; RAW_BYTES_UNCHECKED takes the same (x, y + 1) bytes as they are
    x, y = keygen.decode_points(cs, g[1])[0]
    moved = keygen.encode_points(cs, [(x, (y + 1) % p)])[0].tobytes()
    for i in (1, n + 1):
        shifted = raw[:4 + 64 * i] + moved + raw[4 + 64 * (i + 1):]
        refused("(x, y + 1) at %d" % i, shifted, "raw", "neither on the curve")
        assert _written(native.ParamsKZG.read(ctx, cs, shifted, format="raw-unchecked")) == shifted
        assert _written(native.ParamsKZG.read(ctx, cs, shifted)) == shifted
    for i, half in ((0, 0), (2 * n - 1, 32)):
        refused("word = p at %d" % i, raw[:4 + 64 * i + half] + p.to_bytes(32, "little") + raw[4 + 64 * i + half + 32:], "raw", "stored word")
    g2_off = bytearray(raw)
    g2_off[4 + 128 * n + 64] ^= 1                                # g2's y.c0
    refused("G2 off the curve", bytes(g2_off), "raw", "G2")
    assert _rc_read(pkg, ctx, bytes(g2_off), "raw-unchecked") == 0

    # an identity point inside g is a point in every format and round-trips
    ident = keygen.params_bytes(cs, k, np.concatenate([g[:2], np.zeros((1, 8), dtype=np.uint64), g[3:]]), gl, g2, s_g2, "raw")
    for fmt in FORMATS:
        data = ident if fmt != "processed" else files["processed"][:4 + 64] + bytes(32) + files["processed"][4 + 96:]
        back = native.ParamsKZG.read(ctx, cs, data, format=fmt)
        try:
            assert back.write(fmt) == data and back.write() == ident
        finally:
            back.release()


@pytest.mark.gpu
def test_params_ipa_has_one_format(pkg, ctx, F, ipa_chain):
    from dehalo2_amd import native
    lib = pkg.load_library()
    c = ipa_chain(6, False)
    prm = native.ParamsIPA.create(ctx, F.VESTA, 6, c["srs"]["g"], c["srs"]["g_lagrange"], c["w"], c["u"])
    try:
        out = np.zeros(1 << 16, dtype=np.uint8)
        for fmt in (0, 1, 2):
            assert lib.dehalo_params_size_custom(prm.handle, fmt) == 0
            assert lib.dehalo_params_write_custom(prm.handle, fmt, out.ctypes.data, out.size) == UNSUPPORTED
    finally:
        prm.release()
