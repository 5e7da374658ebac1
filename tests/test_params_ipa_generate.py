"""GPU suite: the generated points and ParamsIPA built from them -- dehalo_points_generate_device (csrc/gfft.cuh k_points_generate) and
dehalo_params_ipa_generate -- against the judge of tests/generator_reference.py, which restates the rule of include/dehalo.h on Python integers.

Points: word for word the judge's, on all three curves, at counts around one block of 128 lanes and at 300 (tests/test_generator_reference.py shows that
indices 0..299 hold an index accepted at once and one that needs at least 16 attempts), with the index crossing into the second counter word, on another
stream and under another key; canonical words, dehalo_points_check_device status 0, no (0, 0), nothing written past `count`.  Integer arithmetic: no tolerance.
Params: write() is byte for byte ParamsIPA.from_g(judge's g, w, u).write() (from_g's g_lagrange is the path tests/test_params_ipa_io.py checks);
generate(7).downsize(5) writes generate(5); write -> read -> write is unchanged; a call repeats; another key moves g[0]; the refusals.
One whole proof at k = 5 on Vesta under generated params equals the CPU restatement's and is accepted; a tampered one is rejected.
Not tested: an index that uses up its 256 attempts -- no key that reaches it is known and the library has no hook to force it."""
import ctypes as C

import numpy as np
import pytest

import generator_reference as G

CURVE_NAMES = ["bn254", "pallas", "vesta"]
COUNTS = [1, 127, 128, 129, 300]      # 128 is one block of k_points_generate
OTHER_KEY = bytes(range(100, 132))
INVALID, UNSUPPORTED = -1, -5


def mont_words(curve, pts):
    """[(x, y)] canonical integers -> (len, 8) u64: x R | y R mod p, R = 2^256, least significant word first (plain integers: nothing from the package)"""
    p = G.CURVES[curve]["p"]
    out = np.zeros((len(pts), 8), dtype=np.uint64)
    for i, (x, y) in enumerate(pts):
        for half, v in enumerate(((x << 256) % p, (y << 256) % p)):
            for j in range(4):
                out[i, 4 * half + j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


@pytest.fixture(scope="module")
def judged():
    """(curve, key, stream, first, count) -> (count, 8) u64, the judge's points; indices 0..299 of stream 0 under the default key are computed once per curve"""
    cache = {}

    def get(curve, key, stream, first, count):
        if key is None and stream == 0 and first + count <= 300:
            if curve not in cache:
                cache[curve] = mont_words(curve, [G.point(curve, None, 0, i)[:2] for i in range(300)])
            return cache[curve][first:first + count]
        return mont_words(curve, [G.point(curve, key, stream, first + i)[:2] for i in range(count)])

    return get


def generate(ctx, curve, count, first=0, stream=0, key=None):
    """-> (count, 8) u64 from dehalo_points_generate_device, after checking that the row behind the last point was left alone"""
    import torch
    cid = G.CURVES[curve]["id"]
    d = torch.full((count + 1, 8), -1, dtype=torch.int64, device=torch.device("cuda", ctx.device))
    torch.cuda.synchronize()      # the library works on its own stream
    ctx.points_generate(cid, d.data_ptr(), count, first, stream, key)
    assert ctx.points_check(cid, d.data_ptr(), count) == 0
    out = ctx.download_tensor(d)
    assert (out[count] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "written past count"
    return out[:count]


def check_points(curve, got, want):
    p = G.CURVES[curve]["p"]
    for row in got:      # canonical words, and no (0, 0)
        x, y = (sum(int(w) << (64 * j) for j, w in enumerate(row[h:h + 4])) for h in (0, 4))
        assert x < p and y < p and (x or y)
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_points_are_the_judges(ctx, judged, curve, count):
    check_points(curve, generate(ctx, curve, count), judged(curve, None, 0, 0, count))


@pytest.mark.gpu
@pytest.mark.parametrize("first,count,stream,key", [((1 << 32) - 2, 4, 0, None), (1 << 47, 2, 0, None), ((1 << 48) - 1, 1, 0, None), (0, 5, 1, None), (3, 5, 0, OTHER_KEY),
                                                    (0, 2, (1 << 32) + 1, None)],
                         ids=["index crosses into w13", "index 2^47", "the last index", "stream 1", "another key", "a stream id above 2^32"])
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_points_at_other_indices_streams_and_keys(ctx, judged, curve, first, count, stream, key):
    got = generate(ctx, curve, count, first, stream, key)
    check_points(curve, got, judged(curve, key, stream, first, count))
    if stream == 1 or key is not None:      # and they are other points than stream 0's under the default key
        assert not np.array_equal(got, judged(curve, None, 0, first, count))


@pytest.mark.gpu
def test_argument_table(pkg, ctx, judged):
    import torch
    lib = pkg.load_library()
    d = torch.full((4, 8), -1, dtype=torch.int64, device=torch.device("cuda", ctx.device))
    torch.cuda.synchronize()
    gen = lambda h, curve, first, ptr, count: lib.dehalo_points_generate_device(h, curve, None, 0, first, ptr, count, None)
    assert gen(None, 2, 0, d.data_ptr(), 4) == INVALID                        # a null context
    assert gen(ctx.handle, 2, 0, None, 4) == INVALID                          # a null output
    assert gen(ctx.handle, 2, 0, d.data_ptr() + 8, 3) == INVALID              # points not 16-byte aligned
    for curve in (3, -1):
        assert gen(ctx.handle, curve, 0, d.data_ptr(), 4) == INVALID          # an unknown curve
    assert gen(ctx.handle, 2, 0, d.data_ptr(), 1 << 29) == INVALID            # count >= 2^29
    assert gen(ctx.handle, 2, (1 << 48) - 3, d.data_ptr(), 4) == INVALID      # first_index + count > 2^48
    assert gen(ctx.handle, 2, (1 << 48) + 1, d.data_ptr(), 0) == INVALID
    assert gen(ctx.handle, 2, (1 << 64) - 2, d.data_ptr(), 4) == INVALID      # (the sum wraps)
    assert lib.dehalo_last_error(ctx.handle).decode().startswith("points_generate:")
    assert (ctx.download_tensor(d) == np.uint64(0xFFFFFFFFFFFFFFFF)).all()    # no refusal wrote anything
    for curve in (0, 1, 2):                                                   # count = 0: 0 without a launch, null pointers allowed
        assert gen(ctx.handle, curve, 0, None, 0) == 0 and gen(ctx.handle, curve, 1 << 48, None, 0) == 0
    assert (ctx.download_tensor(d) == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    with pytest.raises(ValueError):
        ctx.points_generate(2, d.data_ptr(), 4, key=b"short")
    # the context is usable afterwards
    check_points("vesta", generate(ctx, "vesta", 4), judged("vesta", None, 0, 0, 4))


# ------------------------------------------------------------------------------------------------------------------------------ ParamsIPA
def _curve_spec(pkg, curve):
    return pkg.fields.CURVES[curve]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_params_are_from_g_of_the_judges_points(pkg, ctx, judged, curve, k):
    from dehalo2_amd import native
    cs, n = _curve_spec(pkg, curve), 1 << k
    g = judged(curve, None, 0, 0, n)
    wu = mont_words(curve, [G.point(curve, None, 1, 0)[:2], G.point(curve, None, 1, 1)[:2]])
    made = native.ParamsIPA.generate(ctx, cs, k)
    want = native.ParamsIPA.from_g(ctx, cs, k, g, wu[0], wu[1])
    back = again = None
    try:
        data = made.write()
        assert len(data) == 4 + 64 * n + 64 and data == want.write()
        lib = pkg.load_library()
        assert lib.dehalo_params_scheme(made.handle) == 1 and lib.dehalo_params_fixed_base(made.handle)
        back = native.ParamsIPA.read(ctx, cs, data)      # write -> read -> write
        assert back.write() == data
        again = native.ParamsIPA.generate(ctx, cs, k, key=G.DEFAULT_KEY)      # a second call, the default key spelled out
        assert again.write() == data
    finally:
        for prm in (made, want, back, again):
            if prm is not None:
                prm.release()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_prefix_property_and_another_key(pkg, ctx, judged, curve):
    from dehalo2_amd import native
    cs = _curve_spec(pkg, curve)
    p7 = native.ParamsIPA.generate(ctx, cs, 7)
    p5 = native.ParamsIPA.generate(ctx, cs, 5)
    down = other = None
    try:
        down = p7.downsize(5)
        data5 = p5.write()
        assert down.write() == data5
        assert p7.write()[4:4 + 32 * 32] == data5[4:4 + 32 * 32] and p7.write()[-64:] == data5[-64:]      # g is a prefix; W, U do not depend on k
        other = native.ParamsIPA.generate(ctx, cs, 5, key=OTHER_KEY)
        odata = other.write()
        assert odata[4:36] != data5[4:36] and odata[-64:] != data5[-64:]
        from dehalo2_amd import keygen
        _, g, _, w, u = keygen.params_ipa_from_bytes(cs, odata)
        assert np.array_equal(g, mont_words(curve, [G.point(curve, OTHER_KEY, 0, i)[:2] for i in range(32)]))
        assert np.array_equal(np.stack([w, u]), mont_words(curve, [G.point(curve, OTHER_KEY, 1, 0)[:2], G.point(curve, OTHER_KEY, 1, 1)[:2]]))
    finally:
        for prm in (p7, p5, down, other):
            if prm is not None:
                prm.release()


@pytest.mark.gpu
def test_params_refusals(pkg, ctx):
    from dehalo2_amd import native
    lib = pkg.load_library()
    h = C.c_void_p()
    assert lib.dehalo_params_ipa_generate(ctx.handle, 0, 5, None, C.byref(h)) == UNSUPPORTED and not h.value      # BN254
    for k in (0, 29):
        for curve in (1, 2):
            assert lib.dehalo_params_ipa_generate(ctx.handle, curve, k, None, C.byref(h)) == INVALID and not h.value
            assert lib.dehalo_last_error(ctx.handle).decode().startswith("params_ipa_generate:")
    assert lib.dehalo_params_ipa_generate(ctx.handle, 2, 5, None, None) == INVALID
    assert lib.dehalo_params_ipa_generate(None, 2, 5, None, C.byref(h)) == INVALID and not h.value
    with pytest.raises(ValueError):
        native.ParamsIPA.generate(ctx, pkg.fields.VESTA, 5, key=b"short")
    with pytest.raises(NotImplementedError):      # upstream's ParamsIPA::new is still not provided
        native.ParamsIPA.setup(ctx, pkg.fields.VESTA, 5)
    prm = native.ParamsIPA.generate(ctx, pkg.fields.VESTA, 1)      # the context still works
    assert len(prm.write()) == 4 + 128 + 64
    prm.release()


# ------------------------------------------------------------------------------------------------------------------------------ a whole proof
@pytest.mark.gpu
def test_proof_under_generated_params(pkg, po, co, ctx, judged):
    """maingate_k5 on Vesta: the chain of tests/proof_chains.py built over the generated g, g_lagrange, w, u"""
    import ipa
    import plonk_oracle as PO
    import proof_chains as PC
    import shapes
    from dehalo2_amd import circuits, keygen, native, prover

    cs, k = pkg.fields.VESTA, 5
    circ = circuits.synthesize(po.VESTA.scalar.p, k, False, seed=3)
    desc = shapes.maingate_description(False)
    assert desc == circ.cs.description()
    params = native.ParamsIPA.generate(ctx, cs, k)
    pk = P = None
    try:
        k2, g, gl, w, u = keygen.params_ipa_from_bytes(cs, params.write())
        assert k2 == k and np.array_equal(g, judged("vesta", None, 0, 0, 1 << k))
        assert np.array_equal(np.stack([w, u]), mont_words("vesta", [G.point("vesta", None, 1, 0)[:2], G.point("vesta", None, 1, 1)[:2]]))
        srs = dict(g=g, g_lagrange=gl)
        key = PO.keygen(po.VESTA, srs, desc, k, circ.fixed, circ.assembly.mapping, PC.THREADS)
        adv = np.stack([co.field_op(PO.Fld(po.VESTA.scalar).id, "to_mont", circ.advice[i]) for i in range(desc[0])])
        fc, pc = ipa.blinded_key_commitments(po.VESTA, key, w)
        ipa_key = dict(key, fixed_commitments=fc, perm_commitments=pc)
        c = dict(desc=desc, k=k, srs=srs, key=key, adv=adv, u=u, w=w, fc=fc, pc=pc, ipa_key=ipa_key, rep=PO.transcript_repr(po.VESTA, ipa_key, circ.selectors))
        pk = native.ProvingKey.keygen(ctx, params, circ.cs, circ.fixed, circ.assembly, circ.selectors)
        pk.transcript_repr = c["rep"]
        P = native.Prover(params, pk)
        proof = P.create_proof(adv, [[]], prover.SeededRng(7)).finalize()
        assert proof == PC.prove(po, c, [[]], seed=7)[0]
        assert PC.accepts(po, c, proof, [[]])
        assert not PC.accepts(po, c, PC.tampered(c, proof), [[]])
    finally:
        if P is not None:
            P.release()
        if pk is not None:
            pk.release()
        params.release()
