"""dehalo_ipa_s_device: the IPA verifier's scalars over g -- GuardIPA::compute_s of every proof of a batch, summed under the inits -- against
oracle/ipa.py compute_s in Python integers, bit for bit, on both Pasta scalar fields.

The kernel splits an index as hi 2^h + lo with h = ceil(k / 2) and reads one table per half: k = 1 has a high table of one entry (the init alone), k = 2 and 3
the smallest even and odd splits, k = 8 exactly one workgroup of outputs and tables of 16 entries, k = 9 two workgroups and unequal tables (32 and 16), k = 11
tables of 64 and 32 entries -- a low table as long as a wave, so a wave meets one high entry -- over eight workgroups.  count = 33 crosses the running sum's
reduction every 8 terms four times and leaves one term over; count = 5 stays below it."""
import numpy as np
import pytest

KS = [1, 2, 3, 8, 9, 11]
COUNTS = [1, 2, 5, 33]
CURVES = ["vesta", "pallas"]


@pytest.fixture(scope="module")
def IV(oracles):
    import ipa
    return ipa


def expected(IV, p, rows, inits):
    """sum_i compute_s(rows[i], inits[i]) in Python integers"""
    out = [0] * (1 << len(rows[0]))
    for us, init in zip(rows, inits):
        out = [(a + b) % p for a, b in zip(out, IV.compute_s(us, init, p))]
    return out


def run(IV, ctx, po, F, curve_name, rows, inits):
    """-> the kernel's output as (2^k, 4) u64"""
    import torch
    cs, f = F.CURVES[curve_name], getattr(po, curve_name.upper()).scalar
    k = len(rows[0])
    d_ch = ctx.upload(IV.enc(f, [u for us in rows for u in us]))
    d_in = ctx.upload(IV.enc(f, inits))
    out = torch.full((1 << k, 4), -1, dtype=torch.int64, device=d_ch.device)
    ctx.ipa_s_device(cs.id, d_ch.data_ptr(), d_in.data_ptr(), len(rows), k, out.data_ptr())
    return ctx.download_tensor(out).view(np.uint64)


def uniform(p, rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % p for _ in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", CURVES)
@pytest.mark.parametrize("k", KS)
def test_matches_compute_s_on_uniform_challenges(IV, ctx, po, F_, curve_name, k):
    f = getattr(po, curve_name.upper()).scalar
    rng = np.random.default_rng(1000 + k)
    for count in COUNTS:
        rows = [uniform(f.p, rng, k) for _ in range(count)]
        inits = uniform(f.p, rng, count)
        got = run(IV, ctx, po, F_, curve_name, rows, inits)
        want = IV.enc(f, expected(IV, f.p, rows, inits))
        assert np.array_equal(got, want), (k, count)      # canonical Montgomery words: the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", CURVES)
@pytest.mark.parametrize("k", [3, 9])
def test_structured_rows(IV, ctx, po, F_, curve_name, k):
    """all ones, all p - 1, one challenge zero (first, middle, last), an init of zero, an init of p - 1: each alone, where nothing masks a wrong zero, and together"""
    f = getattr(po, curve_name.upper()).scalar
    p = f.p
    rng = np.random.default_rng(77 + k)
    u = uniform(p, rng, k)
    cases = [([1] * k, 1), ([1] * k, u[0]), ([p - 1] * k, u[1]), ([p - 1] * k, p - 1)]
    for z in (0, k // 2, k - 1):
        cases.append(([0 if j == z else u[j] for j in range(k)], u[2]))
    cases += [(u, 0), ([0] * k, u[0]), (u, p - 1)]
    for us, init in cases:
        got = run(IV, ctx, po, F_, curve_name, [us], [init])
        assert np.array_equal(got, IV.enc(f, expected(IV, p, [us], [init]))), (us, init)
    rows, inits = [c[0] for c in cases], [c[1] for c in cases]
    got = run(IV, ctx, po, F_, curve_name, rows, inits)
    assert np.array_equal(got, IV.enc(f, expected(IV, p, rows, inits)))


@pytest.mark.gpu
def test_words_not_below_the_modulus_stand_for_their_residue(IV, ctx, po, F_):
    """a challenge or an init stored as value + p (still below 2^256 on the Pasta fields) gives the output of the value itself"""
    import torch
    f, cs, k = po.VESTA.scalar, F_.VESTA, 3
    rng = np.random.default_rng(5)
    us, init = uniform(f.p, rng, k), uniform(f.p, rng, 1)
    lift = lambda xs: np.frombuffer(b"".join((x * f.R % f.p + f.p).to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()
    d_ch, d_in = ctx.upload(lift(us)), ctx.upload(lift(init))
    out = torch.full((1 << k, 4), -1, dtype=torch.int64, device=d_ch.device)
    ctx.ipa_s_device(cs.id, d_ch.data_ptr(), d_in.data_ptr(), 1, k, out.data_ptr())
    assert np.array_equal(ctx.download_tensor(out).view(np.uint64), IV.enc(f, expected(IV, f.p, [us], init)))


@pytest.mark.gpu
def test_argument_checks(ctx, pkg, F_):
    import torch
    lib = pkg.load_library()
    d = torch.zeros((64, 4), dtype=torch.int64, device="cuda")
    call = lambda curve, count, k, ch=d.data_ptr(), ini=d.data_ptr(), out=d.data_ptr(): lib.dehalo_ipa_s_device(ctx.handle, curve, ch, ini, count, k, out, None)
    assert call(F_.BN254.id, 1, 3) == -5          # DEHALO_ERR_UNSUPPORTED: not a Pasta curve
    assert call(F_.VESTA.id, 1, 0) == -1          # DEHALO_ERR_INVALID
    assert call(F_.VESTA.id, 1, 29) == -1
    assert call(F_.VESTA.id, 0, 3) == -1
    assert call(F_.VESTA.id, 1 << 24, 3) == -1
    assert call(99, 1, 3) == -1
    assert call(F_.VESTA.id, 1, 3, ch=None) == -1
    assert call(F_.VESTA.id, 1, 3, ini=None) == -1
    assert call(F_.VESTA.id, 1, 3, out=None) == -1
    assert call(F_.PALLAS.id, 1, 3) == 0


def test_refused_without_a_context(pkg):
    assert pkg.load_library().dehalo_ipa_s_device(None, 2, None, None, 1, 3, None, None) == -1


@pytest.fixture(scope="module")
def F_(pkg):
    return pkg.fields
