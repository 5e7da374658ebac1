"""Fixed-base scalar multiplication over a resident window table (dehalo_fixed_base_*, csrc/fixed_base.cuh).

CPU: the four entry points refuse a null context.
GPU: [s] P against the C restatement of best_multiexp on all three curves for a non-generator base, the generator and the identity, over scalars that
exercise every window boundary and counts that straddle one block (the kernel takes one wave per scalar, four to a block); the blinding form against the
kernel it replaces (dehalo_blind_commitments_device, Pasta) and against best_multiexp (all three curves; the old kernel refuses BN254), the exceptional
group-law cases of the final addition included; ParamsIPA's own table of W and a whole k = 6 proof through it; the argument checks."""
import numpy as np
import pytest

from test_ipa_proof import F, accepts, ipa_chain, native_ipa  # noqa: F401  (fixtures and helpers of the IPA proof tests, reused as they are)

CURVES = ["bn254", "pallas", "vesta"]
COUNTS = [1, 2, 3, 4, 5, 63, 64, 65, 257]      # 4 scalars per block: one block short, full, one over; a wave's worth of blocks; many blocks


def edge_scalars(r):
    """every digit pattern the windows can meet: small values, both sides of byte-window boundaries (low, middle, the 128-bit word boundary, top),
    the largest scalars, one whose only non-zero byte is the top one, and 16 random ones"""
    s = [0, 1, 2, 255, 256, 257]
    for w in (1, 15, 16, 31):
        s += [(1 << (8 * w)) % r, ((1 << (8 * w)) - 1) % r]
    s += [r - 1, r - 2, (r - 1) // 2, (r >> 248) << 248]
    rng = np.random.default_rng(2024)
    s += [int.from_bytes(rng.bytes(32), "little") % r for _ in range(16)]
    return s


def mul_on_device(ctx, fb, cs, scalars_int):
    import torch
    d = ctx.upload(cs.scalar.encode_many(scalars_int))
    out = torch.empty((len(scalars_int), 8), dtype=torch.int64, device=d.device)
    with ctx.torch_stream():
        out.fill_(-1)
    fb.mul_device(d.data_ptr(), len(scalars_int), out.data_ptr())
    return ctx.download_tensor(out)


@pytest.fixture(scope="module")
def mul_expected(co, F):
    """curve name -> (P = [t] G, the edge scalars, [s] P for each of them by the oracle's best_multiexp): computed once, read by every test"""
    cache = {}

    def get(name):
        if name not in cache:
            cs = F.CURVES[name]
            t = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA998877665544332211 % cs.scalar.p
            P = co.fixed_base_mul(cs.id, cs.scalar.encode_many([t]))[0]
            s = edge_scalars(cs.scalar.p)
            want = np.stack([co.to_affine(cs.id, co.best_multiexp(cs.id, cs.scalar.encode_many([x]), P.reshape(1, 8), 1)) for x in s])
            want.setflags(write=False)
            cache[name] = (P, s, want)
        return cache[name]

    return get


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def test_fixed_base_abi_is_refused_without_device(pkg):
    lib = pkg.load_library()
    assert lib.dehalo_fixed_base_create(None, 2, None, None) == -1
    assert lib.dehalo_fixed_base_release(None, None) == -1
    assert lib.dehalo_fixed_base_mul_device(None, None, None, 0, None, None) == -1
    assert lib.dehalo_fixed_base_blind_device(None, None, None, None, 0, None) == -1
    assert lib.dehalo_params_fixed_base(None) is None


# ------------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", CURVES)
def test_mul_matches_best_multiexp(ctx, co, F, mul_expected, curve_name):
    cs = F.CURVES[curve_name]
    P, s, want = mul_expected(curve_name)
    assert (s[-17] >> 248) and not s[-17] & ((1 << 248) - 1)      # the top-byte-only scalar is what it says
    fb = ctx.fixed_base(cs.id, P)
    try:
        for count in COUNTS:
            idx = [i % len(s) for i in range(count)]
            got = mul_on_device(ctx, fb, cs, [s[i] for i in idx])
            assert np.array_equal(got, want[idx]), "count %d" % count
        assert not want[0].any() and want[1].tobytes() == P.tobytes()      # [0] P = the identity = (0, 0); [1] P = P
    finally:
        fb.release()


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", CURVES)
def test_mul_generator_and_identity_bases(ctx, co, F, curve_name):
    cs = F.CURVES[curve_name]
    s = edge_scalars(cs.scalar.p)
    G = co.fixed_base_mul(cs.id, cs.scalar.encode_many([1]))[0]
    fb = ctx.fixed_base(cs.id, G)
    try:
        assert np.array_equal(mul_on_device(ctx, fb, cs, s), co.fixed_base_mul(cs.id, cs.scalar.encode_many(s)))
    finally:
        fb.release()
    fb = ctx.fixed_base(cs.id, np.zeros(8, dtype=np.uint64))
    try:
        assert not mul_on_device(ctx, fb, cs, s).any()
        # ... and the blinding form leaves every point as it is
        jac = np.stack([co.best_multiexp(cs.id, cs.scalar.encode_many([x]), G.reshape(1, 8), 1) for x in (0, 1, 5)])
        got = _blind_through(ctx, cs, jac, [7, cs.scalar.p - 1, 0], lambda d, b, m: fb.blind_device(d, b, m))
        assert np.array_equal(got, np.stack([co.to_affine(cs.id, j) for j in jac]))
    finally:
        fb.release()


def _blind_through(ctx, cs, jac, blinds_int, launch):
    """jac + [blinds] W by `launch(d_jacobian, d_blinds, count)`, then dehalo_to_affine_device: (count, 8)"""
    import torch
    m = jac.shape[0]
    d = ctx.upload(np.ascontiguousarray(jac).reshape(m, 12))
    b = ctx.upload(cs.scalar.encode_many([x % cs.scalar.p for x in blinds_int]))
    aff = torch.empty((m, 8), dtype=torch.int64, device=d.device)
    launch(d.data_ptr(), b.data_ptr(), m)
    ctx.to_affine_device(cs.id, d.data_ptr(), m, aff.data_ptr())
    return ctx.download_tensor(aff)


def _blind_cases(co, cs, count, seed):
    """`count` MSM-like points C_i = [a_i] Q + [c_i] W with generic z and random blinds b_i -> (Jacobian points, blinds, W, C_i + [b_i] W by the oracle)"""
    r = cs.scalar.p
    QW = co.synth_bases(cs.id, 2)
    rng = np.random.default_rng(seed)
    rnd = lambda: int.from_bytes(rng.bytes(32), "little") % r
    rows = [(rnd(), rnd(), rnd()) for _ in range(count)]
    return _blind_rows(co, cs, QW, rows)


def _blind_rows(co, cs, QW, rows):
    r = cs.scalar.p
    jac = np.stack([co.best_multiexp(cs.id, cs.scalar.encode_many([a, c]), QW, 1) for a, c, _ in rows])
    want = np.stack([co.to_affine(cs.id, co.best_multiexp(cs.id, cs.scalar.encode_many([a, (c + b) % r]), QW, 1)) for a, c, b in rows])
    return jac, [b for _, _, b in rows], QW[1], want


def _check_blind(ctx, co, cs, fb, jac, blinds, w, want):
    got = _blind_through(ctx, cs, jac, blinds, lambda d, b, m: fb.blind_device(d, b, m))
    assert np.array_equal(got, want)
    if cs.name != "bn254":      # the kernel the table replaces: same points in, equal affine points out (it refuses BN254)
        dw = ctx.upload(np.asarray(w, dtype=np.uint64).reshape(1, 8))
        old = _blind_through(ctx, cs, jac, blinds, lambda d, b, m: ctx.blind_commitments_device(cs.id, d, b, m, dw.data_ptr()))
        assert np.array_equal(got, old)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", CURVES)
def test_blind_matches_the_kernel_it_replaces(ctx, co, F, curve_name):
    cs = F.CURVES[curve_name]
    w = co.synth_bases(cs.id, 2)[1]
    fb = ctx.fixed_base(cs.id, w)
    try:
        for count in (1, 8, 65):
            _check_blind(ctx, co, cs, fb, *_blind_cases(co, cs, count, 90 + count))
    finally:
        fb.release()


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", CURVES)
def test_blind_exceptional_cases(ctx, co, F, curve_name):
    """the final + C: C the identity, blind 0, both, C = [b] W (a doubling, b over many windows), C = -[b] W (the identity comes out), and C = W with
    b = r - 1, 1, 2 as test_blind_commitments_cancel_and_double has them"""
    cs = F.CURVES[curve_name]
    r = cs.scalar.p
    QW = co.synth_bases(cs.id, 2)
    b = 0x0102030405060708090A0B0C0D0E0F101112131415161718191A1B1C1D1E1F % r
    rows = [(0, 0, b), (5, 9, 0), (0, 0, 0), (0, b, b), (0, r - b, b), (0, 1, r - 1), (0, 1, 1), (0, 1, 2)]
    fb = ctx.fixed_base(cs.id, QW[1])
    try:
        got = _check_blind(ctx, co, cs, fb, *_blind_rows(co, cs, QW, rows))
        assert got[0].any() and got[1].any() and got[3].any() and got[6].any() and got[7].any()
        assert not got[2].any() and not got[4].any() and not got[5].any()
    finally:
        fb.release()


@pytest.mark.gpu
def test_params_ipa_owns_the_table_of_w(ctx, co, F, ipa_chain, native_ipa):
    cs = F.VESTA
    c, d = ipa_chain(6, False), native_ipa(6, False)
    b = [0x123456789ABCDEF0FEDCBA9876543210 % cs.scalar.p, cs.scalar.p - 1, 0]
    got = mul_on_device(ctx, d["params"].fixed_base, cs, b)
    w = np.asarray(c["w"], dtype=np.uint64).reshape(1, 8)
    want = np.stack([co.to_affine(cs.id, co.best_multiexp(cs.id, cs.scalar.encode_many([x]), w, 1)) for x in b])
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_k6_proof_through_the_table_is_accepted(po, co, F, ipa_chain, native_ipa):
    from dehalo2_amd import native, prover

    c, d = ipa_chain(6, False), native_ipa(6, False)
    P = native.Prover(d["params"], d["pk"])
    proof = P.create_proof(c["adv"], [[]], prover.SeededRng(7)).finalize()
    assert accepts(po, c, proof)
    P.release()


@pytest.mark.gpu
def test_fixed_base_argument_checks(ctx, pkg, co, F):
    import ctypes as C
    import torch
    lib = pkg.load_library()
    v = F.VESTA
    w = np.ascontiguousarray(co.synth_bases(v.id, 1)[0])
    h = C.c_void_p()
    assert lib.dehalo_fixed_base_create(ctx.handle, 7, w.ctypes.data, C.byref(h)) == -1 and b"unknown curve" in lib.dehalo_last_error(ctx.handle)
    assert lib.dehalo_fixed_base_create(ctx.handle, v.id, None, C.byref(h)) == -1              # null point
    assert lib.dehalo_fixed_base_create(ctx.handle, v.id, w.ctypes.data, None) == -1           # null out
    assert lib.dehalo_fixed_base_release(ctx.handle, None) == -1
    fb = ctx.fixed_base(v.id, w)
    d = torch.zeros((8, 12), dtype=torch.int64, device="cuda")
    s = torch.zeros((8, 4), dtype=torch.int64, device="cuda")
    o = torch.zeros((8, 8), dtype=torch.int64, device="cuda")
    assert lib.dehalo_fixed_base_mul_device(ctx.handle, None, s.data_ptr(), 8, o.data_ptr(), None) == -1              # null table
    assert lib.dehalo_fixed_base_mul_device(ctx.handle, fb.handle, None, 8, o.data_ptr(), None) == -1                 # null scalars
    assert lib.dehalo_fixed_base_mul_device(ctx.handle, fb.handle, s.data_ptr(), 8, None, None) == -1                 # null output
    assert lib.dehalo_fixed_base_mul_device(ctx.handle, fb.handle, s.data_ptr(), 1 << 29, o.data_ptr(), None) == -1   # size
    assert lib.dehalo_fixed_base_mul_device(ctx.handle, fb.handle, None, 0, None, None) == 0                          # nothing to do
    assert lib.dehalo_fixed_base_blind_device(ctx.handle, None, d.data_ptr(), s.data_ptr(), 8, None) == -1            # null table
    assert lib.dehalo_fixed_base_blind_device(ctx.handle, fb.handle, None, s.data_ptr(), 8, None) == -1               # null points
    assert lib.dehalo_fixed_base_blind_device(ctx.handle, fb.handle, d.data_ptr(), None, 8, None) == -1               # null blinds
    assert lib.dehalo_fixed_base_blind_device(ctx.handle, fb.handle, d.data_ptr(), s.data_ptr(), 1 << 29, None) == -1  # size
    assert lib.dehalo_fixed_base_blind_device(ctx.handle, fb.handle, None, None, 0, None) == 0                        # nothing to do
    fb.release()
    # a release followed by a second create on the same context
    fb = ctx.fixed_base(v.id, w)
    got = mul_on_device(ctx, fb, v, [1, 0])
    assert got[0].tobytes() == w.tobytes() and not got[1].any()
    fb.release()
