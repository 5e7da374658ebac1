"""g_to_lagrange on the device (dehalo_g_to_lagrange_device, csrc/gfft.cuh): the group FFT out[i] = [n^-1] sum_j [omega^(-i j)] g[j].

Every comparison is exact equality of affine points (the output is the canonical affine point, whatever the order of evaluation):
a trapdoor SRS, whose g_lagrange is known from the toxic waste; an unstructured g with known discrete logarithms, against the scalar-field
transform of the logarithms; the exceptional group-law paths a transform meets (identities, a = +-[t] b in mid-transform); a g with no known
logarithms at k = 17, against best_multiexp over g for single outputs and through the commitment identity <v, g_lagrange> = <lagrange_to_coeff(v), g>;
and the argument checks."""
import numpy as np
import pytest

S_TOXIC = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F


@pytest.fixture(scope="module")
def F(pkg):
    return pkg.fields


def _dom(cs, k):
    """omega_inv, n_inv of the 2^k domain over the curve's scalar field (canonical ints)"""
    f = cs.scalar
    omega = pow(f.root_of_unity, 1 << (f.two_adicity - k), f.p)
    return pow(omega, -1, f.p), pow(1 << k, -1, f.p)


def _gfft(ctx, cs, g, k, in_place):
    import torch
    d = ctx.upload(g)
    if in_place:
        ctx.g_to_lagrange(cs.id, d.data_ptr(), k)
        return ctx.download_tensor(d)
    out = torch.full((g.shape[0], 8), -1, dtype=torch.int64, device=d.device)
    ctx.g_to_lagrange(cs.id, d.data_ptr(), k, out.data_ptr())
    assert np.array_equal(ctx.download_tensor(d), g)          # the input is left alone
    return ctx.download_tensor(out)


def _both(ctx, cs, g, k, want):
    for in_place in (False, True):
        got = _gfft(ctx, cs, g, k, in_place)
        assert np.array_equal(got, want), ("in place" if in_place else "out of place", k)


def _logs_case(co, cs, r, k):
    """g = [r_j] G and its transform through the scalar field: [lagrange_to_coeff(r)_i] G"""
    f = cs.scalar
    omega_inv, n_inv = _dom(cs, k)
    rm = f.encode_many(r)
    g = co.fixed_base_mul(cs.id, rm, 8)
    want = co.fixed_base_mul(cs.id, co.lagrange_to_coeff(f.id, rm, k, f.encode(omega_inv), f.encode(n_inv), 8), 8)
    return g, want


# ------------------------------------------------------------------------------------------------------------------------------ 1. trapdoor SRS
@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", ["vesta", "pallas", "bn254"])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 6, 10, 14])
def test_trapdoor_srs(ctx, po, co, F, oracles, curve_name, k):
    import plonk_oracle as PO
    cs = F.CURVES[curve_name]
    srs = PO.setup_srs(getattr(po, curve_name.upper()), k, S_TOXIC, 8)
    _both(ctx, cs, srs["g"], k, srs["g_lagrange"])


# ------------------------------------------------------------------------------------------------------------------------------ 2. unstructured g, known logs
@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", ["vesta", "pallas"])
@pytest.mark.parametrize("k", [4, 9, 13])
def test_unstructured_g_with_known_logs(ctx, co, F, curve_name, k):
    cs = F.CURVES[curve_name]
    p, n = cs.scalar.p, 1 << k
    rng = np.random.default_rng(1000 + k)
    r = [int.from_bytes(rng.bytes(32), "little") % p for _ in range(n)]
    for i in range(0, n, 5):          # some zeros (identity points) ...
        r[i] = 0
    for i in range(3, n, 7):          # ... and some repeated values (equal points: doublings and cancellations inside butterflies)
        r[i] = r[1]
    g, want = _logs_case(co, cs, r, k)
    _both(ctx, cs, g, k, want)


# ------------------------------------------------------------------------------------------------------------------------------ 3. exceptional paths
@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", ["vesta", "pallas"])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_exceptional_paths(ctx, co, F, curve_name, k):
    cs = F.CURVES[curve_name]
    f = cs.scalar
    p, n = f.p, 1 << k
    omega_inv, _ = _dom(cs, k)
    omega = pow(omega_inv, -1, p)
    G = co.fixed_base_mul(cs.id, f.encode_many([1]))[0]
    ident = np.zeros((n, 8), dtype=np.uint64)
    # all identities
    _both(ctx, cs, ident, k, ident)
    # a constant g: [c] G at index 0, the identity elsewhere (every later butterfly sees a = [t] b or an identity)
    c = 0xC0FFEE1234567
    g, want = _logs_case(co, cs, [c] * n, k)
    assert np.array_equal(want[0], co.fixed_base_mul(cs.id, f.encode_many([c]))[0]) and not want[1:].any()
    _both(ctx, cs, g, k, want)
    # r_j = omega^(j t): G at index t only
    for t in sorted({0, 1, n // 2, n - 1}):
        g, want = _logs_case(co, cs, [pow(omega, j * t, p) for j in range(n)], k)
        e = ident.copy()
        e[t] = G
        assert np.array_equal(want, e)
        _both(ctx, cs, g, k, want)
    # upper half = lower half, upper half = -lower half
    rng = np.random.default_rng(77 + k)
    lo = [int.from_bytes(rng.bytes(32), "little") % p for _ in range(n // 2)]
    for r in (lo + lo, lo + [(-v) % p for v in lo]):
        g, want = _logs_case(co, cs, r, k)
        _both(ctx, cs, g, k, want)


# ------------------------------------------------------------------------------------------------------------------------------ 4. no discrete logs, at scale
@pytest.mark.gpu
def test_no_discrete_logs_at_scale(ctx, pkg, co, F):
    import torch
    from dehalo2_amd import native
    cs, k = F.VESTA, 17
    f = cs.scalar
    p, n = f.p, 1 << k
    omega_inv, n_inv = _dom(cs, k)
    g = co.synth_bases(cs.id, n)
    gl = _gfft(ctx, cs, g, k, False)
    # single outputs against best_multiexp over g with the scalars n^-1 omega^(-i j)
    for i in (0, 1, n // 2, n - 1):
        sc = co.powers(f.id, f.encode(pow(omega_inv, i, p)), f.encode(n_inv), n)
        want = co.to_affine(cs.id, co.best_multiexp(cs.id, sc, g, 8))
        assert np.array_equal(gl[i], want), i
    # <v, g_lagrange> = <lagrange_to_coeff(v), g> for a random vector, through the library's commitments
    rng = np.random.default_rng(17)
    v = f.encode_many([int.from_bytes(rng.bytes(32), "little") % p for _ in range(n)])
    coeffs = co.lagrange_to_coeff(f.id, v, k, f.encode(omega_inv), f.encode(n_inv), 8)
    uw = co.fixed_base_mul(cs.id, f.encode_many([3, 5]))
    prm = native.ParamsIPA.create(ctx, cs, k, g, gl, uw[0], uw[1])
    try:
        lib = pkg.load_library()
        out = torch.zeros((2, 8), dtype=torch.int64, device="cuda")
        d_v, d_c = ctx.upload(v), ctx.upload(coeffs)
        assert lib.dehalo_params_commit_device(ctx.handle, prm.handle, d_v.data_ptr(), 1, 1, out[0].data_ptr(), None) == 0
        assert lib.dehalo_params_commit_device(ctx.handle, prm.handle, d_c.data_ptr(), 1, 0, out[1].data_ptr(), None) == 0
        got = ctx.download_tensor(out)
        assert got[0].any() and np.array_equal(got[0], got[1])
    finally:
        prm.release()


# ------------------------------------------------------------------------------------------------------------------------------ 5. argument checks
@pytest.mark.gpu
def test_argument_checks(ctx, pkg, F):
    import torch
    lib = pkg.load_library()
    d = torch.zeros((32, 8), dtype=torch.int64, device="cuda")
    g2l = lib.dehalo_g_to_lagrange_device
    assert g2l(ctx.handle, F.VESTA.id, d.data_ptr(), 3, d.data_ptr() + 64, None) == -1                    # partial overlap
    assert g2l(ctx.handle, F.VESTA.id, d.data_ptr() + 64 * 4, 3, d.data_ptr(), None) == -1
    assert g2l(ctx.handle, F.VESTA.id, d.data_ptr(), 29, d.data_ptr(), None) == -1                        # k out of range
    assert g2l(ctx.handle, F.VESTA.id, None, 3, d.data_ptr(), None) == -1
    # an unknown curve: the code the other device calls return for one
    other = lib.dehalo_to_affine_device(ctx.handle, 7, d.data_ptr(), 1, d.data_ptr(), None)
    assert other != 0 and g2l(ctx.handle, 7, d.data_ptr(), 3, d.data_ptr(), None) == other
    # disjoint halves of one allocation are fine
    assert g2l(ctx.handle, F.VESTA.id, d.data_ptr(), 3, d.data_ptr() + 64 * 8, None) == 0
    ctx.synchronize()
