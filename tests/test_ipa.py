"""IPACommitmentScheme over Vesta / Pallas: ParamsIPA from its parts, the generator collapse kernel and the opening argument
(dehalo_params_ipa_create, dehalo_generator_collapse_device, dehalo_ipa_open).

CPU: the Python restatement of the opening (oracle/ipa.py) accepts its own reference proofs and rejects every altered byte.
GPU: the collapse against the C restatement of best_multiexp, element by element (edge cases included); device openings accepted by the
verifier, byte-identical to the reference prover under the same seeded scalar stream, and rejected once tampered with."""
import ctypes as C

import numpy as np
import pytest



@pytest.fixture(scope="module")
def F(pkg):
    return pkg.fields


@pytest.fixture(scope="module")
def IV(oracles):
    import ipa      # (the oracle's modules are on the path once the oracles fixture has loaded them)
    return ipa


def reference_opening(curve, g, u, w, poly, blind, x3, draw):
    """a stand-alone opening: ipa.open_reference on a fresh transcript"""
    import ipa
    import plonk_oracle
    return ipa.open_reference(plonk_oracle.Transcript(curve), curve, g, u, w, poly, blind, x3, draw)


def opening_accepted(curve, g, u, w, P, x3, v, proof):
    """a stand-alone opening's bytes, read through a fresh transcript"""
    import ipa
    import verifier
    return ipa.verify_opening(verifier.ReadTranscript(curve, proof), curve, g, u, w, P, x3, v)


def _srs(co, F, curve_spec, k, seed=7):
    """g: 2^k synthetic points; u, w: fixed-base multiples of two seeded scalars (a trapdoor SRS is fine for correctness)."""
    g = co.synth_bases(curve_spec.id, 1 << k)
    uw = co.fixed_base_mul(curve_spec.id, co.fill_scalars(curve_spec.scalar.id, "uniform", 2, seed))
    return g, uw[0], uw[1]


def _poly(F, curve_spec, n, seed):
    rng = np.random.default_rng(seed)
    p = curve_spec.scalar.p
    return [int.from_bytes(rng.bytes(32), "little") % p for _ in range(n)]


# ------------------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("k", [4, 5])
def test_reference_opening_verifies_and_tampering_is_rejected(IV, pkg, po, co, F, k):
    from dehalo2_amd.prover import SeededRng
    cs = F.VESTA
    curve = po.VESTA
    g, u, w = _srs(co, F, cs, k)
    poly = _poly(F, cs, 1 << k, 10 + k)
    blind, x3 = 12345 + k, 0xABCDEF + k
    proof = reference_opening(curve, g, u, w, poly, blind, x3, SeededRng(3).scalars)
    P = IV.commit_reference(curve, g, w, poly, blind)
    v = po.eval_polynomial(curve.scalar, poly, x3)
    assert len(proof) == 32 + 64 * k + 64
    assert opening_accepted(curve, g, u, w, P, x3, v, proof)
    assert not opening_accepted(curve, g, u, w, P, x3, (v + 1) % curve.scalar.p, proof)
    assert not opening_accepted(curve, g, u, w, P, (x3 + 1), v, proof)
    assert not opening_accepted(curve, g, u, w, P, x3, v, proof[:-1])
    assert not opening_accepted(curve, g, u, w, P, x3, v, proof + b"\0")
    for i in range(len(proof)):
        bad = bytearray(proof)
        bad[i] ^= 1 << (i % 8)
        assert not opening_accepted(curve, g, u, w, P, x3, v, bytes(bad)), i


def test_compute_b_is_the_folded_powers(IV, po):
    p = po.VESTA.scalar.p
    x, us = 987654321, [3, 5, 7, 11]
    b = [pow(x, i, p) for i in range(16)]
    for u in us:
        h = len(b) // 2
        b = [(b[i] + u * b[i + h]) % p for i in range(h)]
    assert b[0] == IV.compute_b(x, us, p)


def test_ipa_abi_is_refused_without_device_or_for_bn254(pkg):
    lib = pkg.load_library()
    assert lib.dehalo_params_scheme(None) == -1
    assert lib.dehalo_ipa_open(None, None, None, None, None, None, None) == -1
    assert lib.dehalo_generator_collapse_device(None, 2, None, 0, None, None, None) == -1


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _collapse_expected(co, curve_spec, pts, u_int):
    half = pts.shape[0] // 2
    p = curve_spec.scalar.p
    sc = curve_spec.scalar.encode_many([1, u_int % p])
    out = np.zeros((half, 8), dtype=np.uint64)
    for i in range(half):
        out[i] = co.to_affine(curve_spec.id, co.best_multiexp(curve_spec.id, sc, np.stack([pts[i], pts[half + i]]), 1))
    return out


def _collapse(ctx, curve_spec, pts, u_int, in_place=False):
    import torch
    d = ctx.upload(pts)
    out = d if in_place else torch.full((pts.shape[0] // 2, 8), -1, dtype=torch.int64, device=d.device)
    ctx.generator_collapse_device(curve_spec.id, d.data_ptr(), pts.shape[0], curve_spec.scalar.encode(u_int % curve_spec.scalar.p), out.data_ptr(), 0)
    return ctx.download_tensor(out)[: pts.shape[0] // 2]


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", ["vesta", "pallas"])
@pytest.mark.parametrize("log_len", [1, 2, 6, 11, 16])
def test_collapse_matches_best_multiexp(IV, ctx, co, F, curve_name, log_len):
    cs = F.CURVES[curve_name]
    n = 1 << log_len
    pts = co.synth_bases(cs.id, n + 7)[7:]                 # (an offset: G_hi is not G_lo's neighbour in the synthetic sequence)
    u = _poly(F, cs, 1, 100 + log_len)[0]
    got = _collapse(ctx, cs, pts, u)
    want = _collapse_expected(co, cs, pts, u)
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", ["vesta", "pallas"])
def test_collapse_edge_cases(IV, ctx, co, F, curve_name):
    cs = F.CURVES[curve_name]
    p = cs.scalar.p
    base = co.synth_bases(cs.id, 64)
    neg = base.copy()
    neg[:, 4:] = cs.base.encode_many([(-cs.base.decode(r[4:])) % cs.base.p for r in base])
    ident = np.zeros_like(base)
    cases = [
        (np.concatenate([base[:32], base[32:]]), [0, 1, p - 1, 2, (p - 1) // 2]),     # u in {0, 1, -1, ...}
        (np.concatenate([base[:32], base[:32]]), [1, 2, p - 1]),                       # G_lo = G_hi: u = 1 doubles, u = -1 cancels
        (np.concatenate([neg[:32], base[:32]]), [1, 3]),                               # G_lo = -G_hi: u = 1 gives the identity
        (np.concatenate([ident[:32], base[:32]]), [5, 1]),                             # identities in either half
        (np.concatenate([base[:32], ident[:32]]), [5, 0]),
        (ident, [7]),
    ]
    for pts, us in cases:
        for u in us:
            want = _collapse_expected(co, cs, pts, u)
            assert np.array_equal(_collapse(ctx, cs, pts, u), want), u
            assert np.array_equal(_collapse(ctx, cs, pts, u, in_place=True), want), u


@pytest.mark.gpu
def test_collapse_argument_checks(IV, ctx, pkg, F):
    import torch
    lib = pkg.load_library()
    d = torch.zeros((8, 8), dtype=torch.int64, device="cuda")
    u = F.VESTA.scalar.encode(3)
    assert lib.dehalo_generator_collapse_device(ctx.handle, F.VESTA.id, d.data_ptr(), 3, u.ctypes.data, d.data_ptr(), None) == -1       # odd
    assert lib.dehalo_generator_collapse_device(ctx.handle, F.BN254.id, d.data_ptr(), 8, u.ctypes.data, d.data_ptr(), None) == -5       # not Pasta
    assert lib.dehalo_generator_collapse_device(ctx.handle, F.VESTA.id, d.data_ptr(), 8, u.ctypes.data, d.data_ptr() + 64, None) == -1  # overlap


def _params(pkg, ctx, co, F, cs, k):
    g, u, w = _srs(co, F, cs, k)
    from dehalo2_amd import native
    return native.ParamsIPA.create(ctx, cs, k, g, g, w, u), g, u, w


@pytest.mark.gpu
def test_params_ipa(IV, pkg, ctx, co, F):
    lib = pkg.load_library()
    prm, g, u, w = _params(pkg, ctx, co, F, F.VESTA, 6)
    assert lib.dehalo_params_scheme(prm.handle) == 1
    assert lib.dehalo_params_size(prm.handle) == 0
    h = C.c_void_p()
    assert lib.dehalo_params_ipa_create(ctx.handle, F.BN254.id, 6, g.ctypes.data, g.ctypes.data, w.ctypes.data, u.ctypes.data, C.byref(h)) == -5
    prm.release()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 10, 14])
def test_ipa_open_is_accepted_and_tampering_rejected(IV, pkg, ctx, po, co, F, k):
    from dehalo2_amd.prover import SeededRng
    cs, curve = F.VESTA, po.VESTA
    prm, g, u, w = _params(pkg, ctx, co, F, cs, k)
    poly = _poly(F, cs, 1 << k, k)
    blind, x3 = 777 + k, 0x1234567 + k
    d_poly = ctx.upload(cs.scalar.encode_many(poly))
    proof = prm.open(d_poly.data_ptr(), blind, x3, rng=SeededRng(11)).finalize()
    assert len(proof) == 32 + 64 * k + 64
    P = IV.commit_reference(curve, g, w, poly, blind)
    v = po.eval_polynomial(curve.scalar, poly, x3)
    assert opening_accepted(curve, g, u, w, P, x3, v, proof)
    # the same seed gives the same bytes; another seed other bytes, also accepted
    assert prm.open(d_poly.data_ptr(), blind, x3, rng=SeededRng(11)).finalize() == proof
    other = prm.open(d_poly.data_ptr(), blind, x3, rng=SeededRng(12)).finalize()
    assert other != proof and opening_accepted(curve, g, u, w, P, x3, v, other)
    # an altered S, L_j, R_j, c or f is rejected, as is a wrong claim
    for off in [0, 32, 32 + 32 * (k - 1), 32 + 64 * k - 32, len(proof) - 64, len(proof) - 32]:
        bad = bytearray(proof)
        bad[off + 3] ^= 0x10
        assert not opening_accepted(curve, g, u, w, P, x3, v, bytes(bad)), off
    assert not opening_accepted(curve, g, u, w, P, x3, (v + 1) % curve.scalar.p, proof)
    assert not opening_accepted(curve, g, u, w, P, x3, v, proof[:-32])
    prm.release()


@pytest.mark.gpu
def test_ipa_open_matches_the_reference_prover(IV, pkg, ctx, po, co, F):
    """Byte for byte against ipa.open_reference under the same PCG64 stream: draw order and transcript order pinned between the two."""
    from dehalo2_amd.prover import SeededRng
    cs, curve = F.VESTA, po.VESTA
    k = 5
    prm, g, u, w = _params(pkg, ctx, co, F, cs, k)
    poly = _poly(F, cs, 1 << k, 5)
    blind, x3 = 4242, 0x55AA55
    d_poly = ctx.upload(cs.scalar.encode_many(poly))
    rng = SeededRng(21)
    got = prm.open(d_poly.data_ptr(), blind, x3, rng=rng).finalize()
    after = rng.scalars(1)
    ref_rng = SeededRng(21)
    want = reference_opening(curve, g, u, w, poly, blind, x3, ref_rng.scalars)
    assert got == want
    assert np.array_equal(after, ref_rng.scalars(1))      # the caller's generator moved past exactly the opening's draws
    prm.release()


@pytest.mark.gpu
def test_ipa_open_with_os_entropy(IV, pkg, ctx, po, co, F):
    """The default generator: s_poly from the device ChaCha20 stream, the blinds from the host's -- accepted, and fresh every call."""
    cs, curve = F.VESTA, po.VESTA
    k = 9
    prm, g, u, w = _params(pkg, ctx, co, F, cs, k)
    poly = _poly(F, cs, 1 << k, 9)
    blind, x3 = 99, 0xC0FFEE
    d_poly = ctx.upload(cs.scalar.encode_many(poly))
    a = prm.open(d_poly.data_ptr(), blind, x3).finalize()
    b = prm.open(d_poly.data_ptr(), blind, x3).finalize()
    P = IV.commit_reference(curve, g, w, poly, blind)
    v = po.eval_polynomial(curve.scalar, poly, x3)
    assert a != b
    assert opening_accepted(curve, g, u, w, P, x3, v, a)
    assert opening_accepted(curve, g, u, w, P, x3, v, b)
    prm.release()
