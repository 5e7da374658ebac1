"""The field-vector kernels on structured values: zeros, ones, p - 1, deltas, single frequencies, roots of unity as points, and inversion operands chosen by the
integer the divstep loop starts from (tests/structured_inputs.py).  Uniform operands, which every other parity test draws, never make a kernel store a value
congruent to zero, never put an exact zero through a whole butterfly chain, never land a power ladder on one.

CPU (no mark): every closed form of structured_inputs equals the C restatement on the same input, at the GPU tests' sizes and over bn254_fr, pasta_fp and
pasta_fq -- the reference is pinned before a kernel is judged by it.
GPU: bit-exact against the closed form where there is one, against Python-integer recurrences or the C restatement otherwise; device outputs are written over
buffers of all-ones words."""
import numpy as np
import pytest

import structured_inputs as SI

NTT_LOGS = [1, 2, 3, 10, 11, 12, 13, 17]      # 10 / 11: one pass, even and odd radix (11 stages: the longest lazy chain); 12 / 13: two passes (12 on the half tile); 17: three
EVAL_NS = [1, 8, 2048, 2049, 4097]
KATE_NS = [2, 9, 2048, 2049, 4097]
PRODUCT_NS = [1023, 1025, 5000]
INVERT_NS = [1023, 1024, 1025]
SCALE_N = 4101
POISON = -1


def _poisoned(shape):
    import torch
    return torch.full(shape, POISON, dtype=torch.int64, device="cuda")


def _np(t):
    return t.cpu().numpy().view(np.uint64)


# ---------------------------------------------------------------- the cases, shared by the CPU and the GPU tests
def ntt_cases(po, co, fname, log_n):
    """yields (label, input, omega, expected, has_closed_form) for the forward and the inverse root; the inputs without a closed form take the C restatement's output"""
    F = SI.field(po, fname)
    n = 1 << log_n
    for direction, w in (("fwd", F.omega(log_n)), ("inv", F.inv(F.omega(log_n)))):
        omega = F.enc1(w)
        for name, a in SI.vectors(F, n, w).items():
            a = F.enc(a)
            closed = SI.ntt_closed_form(F, name, n, w)
            yield (direction, name), a, omega, (F.enc(closed) if closed is not None else co.best_fft(F.fid, a, omega, log_n, 4)), closed is not None


_EVAL, _KATE = {}, {}


def eval_cases(po, fname, n):
    """-> (vectors as encoded arrays by name, [(vector name, point name, point, expected value, closed form or None)]); expected = Horner in Python integers"""
    if (fname, n) not in _EVAL:
        F = SI.field(po, fname)
        vecs = SI.vectors(F, n)
        cases = [(vn, zn, z, SI.horner(a, z, F.p), SI.eval_closed_form(F, vn, n, zn)) for vn, a in vecs.items() for zn, z in SI.points(F, n).items()]
        _EVAL[(fname, n)] = ({vn: F.enc(a) for vn, a in vecs.items()}, cases)
    return _EVAL[(fname, n)]


def kate_cases(po, fname, n):
    """-> [(polynomial name, point name, point, coefficients (encoded), expected quotient (ints), closed form or None)]; expected = the Python recurrence"""
    if (fname, n) not in _KATE:
        F = SI.field(po, fname)
        out = []
        for zn, z in SI.points(F, n).items():
            for pn, a in SI.kate_polys(po, F, n, z).items():
                out.append((pn, zn, z, F.enc(a), SI.kate_recurrence(a, z, F.p), SI.kate_closed_form(po, F, pn, n, z)))
        _KATE[(fname, n)] = out
    return _KATE[(fname, n)]


def invert_vectors(po, fname):
    """-> [(values, inverses)] as ints: both operand lists at each length, zeros interleaved"""
    F = SI.field(po, fname)
    out = []
    for lst in SI.inversion_operands(F):
        for n in INVERT_NS:
            v = SI.padded_with_zeros(lst, n)
            assert set(lst) <= set(v)
            out.append((v, [F.inv(x) if x else 0 for x in v]))
    return out


def lincomb_cases(po, fname, n):
    """-> [(label, distinct columns (ints), column index per term, coefficients, sub0 or None, expected (ints))]"""
    F = SI.field(po, fname)
    p, c = F.p, SI.constant_c(F)
    A = SI.uniform_ints(po, F, n, 9100)
    B = SI.vectors(F, n)["sparse"]
    pm1 = [p - 1] * n
    cases = [("cancel2", [A], [0, 0], [c, p - c], None, [0] * n),
             ("pm1x40", [pm1], [0] * 40, [p - 1] * 40, None, [40] * n),
             ("sub0", [A, B], [0, 1, 0], [c, 5, p - 2], (c * A[0] + 5 * B[0] + (p - 2) * A[0]) % p, None)]
    for count in (41, 97):       # more columns than one launch takes: the later launches accumulate into the output
        cases.append(("pm1x%d" % count, [pm1], [0] * count, [p - 1] * count, None, [count] * n))
        cases.append(("cancel%d" % count, [A, B], [0, 1] * (count // 2) + [0], [c, 3, p - c, p - 3] * (count // 4) + [7], None, [7 * a % p for a in A]))
    out = []
    for label, cols, idx, coefs, sub0, closed in cases:
        want = SI.lincomb_ints([cols[i] for i in idx], coefs, sub0, p)
        assert closed is None or want == closed, label
        if label == "sub0":
            assert want[0] == 0 and any(want[1:])
        out.append((label, cols, idx, coefs, sub0, want))
    return out


def scale_cases(po, fname):
    """-> (vector (ints), [(pattern, device factor)])"""
    F = SI.field(po, fname)
    p, c = F.p, SI.constant_c(F)
    a = SI.uniform_ints(po, F, SCALE_N, 9200)
    a[::7] = [0] * len(a[::7])
    a[3::11] = [p - 1] * len(a[3::11])
    a[5::13] = [1] * len(a[5::13])
    mixed = [0, 1, p - 1, c, 1, p - 1, 0, p - c]
    pats = [[0] * per for per in (1, 2, 4, 8)] + [[1] * per for per in (1, 2, 4, 8)] + [[p - 1] * per for per in (1, 2, 4, 8)] + [mixed[:per] for per in (1, 2, 4, 8)]
    return a, [(pat, fac) for pat in pats for fac in (0, 1, p - 1)]


# ---------------------------------------------------------------- CPU: the closed forms against the C restatement
@pytest.mark.parametrize("fname", SI.FIELDS3)
@pytest.mark.parametrize("log_n", NTT_LOGS)
def test_ntt_closed_forms_equal_the_c_oracle(po, co, fname, log_n):
    F = SI.field(po, fname)
    closed_seen = 0
    for label, a, omega, want, closed in ntt_cases(po, co, fname, log_n):
        if closed:
            closed_seen += 1
            assert np.array_equal(co.best_fft(F.fid, a, omega, log_n, 4), want), label
    assert closed_seen >= 2 * (5 + 2 * len(SI.delta_positions(1 << log_n)))
    if log_n <= 3:               # and the definition itself, in Python integers
        w = F.omega(log_n)
        for name, a in SI.vectors(F, 1 << log_n, w).items():
            closed = SI.ntt_closed_form(F, name, 1 << log_n, w)
            assert closed is None or closed == po.dft_naive(F.of, a, w), name


@pytest.mark.parametrize("fname", SI.FIELDS3)
@pytest.mark.parametrize("n", EVAL_NS)
def test_eval_closed_forms_equal_the_c_oracle(po, co, fname, n):
    F = SI.field(po, fname)
    vecs, cases = eval_cases(po, fname, n)
    closed_seen = 0
    for vn, zn, z, want, closed in cases:
        if closed is not None:
            closed_seen += 1
            assert closed == want, (vn, zn)
        assert np.array_equal(co.eval_polynomial(F.fid, vecs[vn], F.enc1(z), 2), F.enc1(want)), (vn, zn)
    assert closed_seen >= len(vecs)      # at least p(0) = c_0 for every vector


@pytest.mark.parametrize("fname", SI.FIELDS3)
@pytest.mark.parametrize("n", KATE_NS)
def test_kate_closed_forms_equal_the_c_oracle(po, co, fname, n):
    F = SI.field(po, fname)
    closed_seen = set()
    for pn, zn, z, a, want, closed in kate_cases(po, fname, n):
        if closed is not None:
            closed_seen.add((pn, zn))
            assert closed == want, (pn, zn)
        assert np.array_equal(co.kate_division(F.fid, a, F.enc1(z)), F.enc(want)), (pn, zn)
        if pn == "multiple":     # (X - z) b: nothing remains
            assert SI.horner(F.dec(a), z, F.p) == 0
    assert {("one", "1"), ("one", "-1"), ("one", "0"), ("monomial", "w8"), ("multiple", "half")} <= closed_seen
    if n >= 4:
        ones_at_minus_one = [c for pn, zn, z, a, want, c in kate_cases(po, fname, n) if (pn, zn) == ("one", "-1")][0]
        assert ones_at_minus_one[-3:] == [1, 0, 1]


@pytest.mark.parametrize("fname", SI.FIELDS3)
def test_product_and_inversion_closed_forms_equal_the_c_oracle(po, co, fname):
    F = SI.field(po, fname)
    p = F.p
    xs, vs = SI.inversion_operands(F)
    assert len(vs) > 500 and [x * pow(2, SI.INTERNAL_SHIFT, p) % p for x in xs] == vs
    last = vs[-1]
    assert last < p and last + (1 << 240) >= p and all((last >> (30 * i)) & 0x3FFFFFFF == 0x3FFFFFFF for i in range(8))
    for v, inv in invert_vectors(po, fname):
        assert all(x * y % p == (1 if x else 0) for x, y in zip(v, inv))
        assert np.array_equal(co.batch_invert(F.fid, F.enc(v)), F.enc(inv))
    for n in PRODUCT_NS:
        cases, zero_at = SI.grand_product_cases(po, F, n)
        for name, (num, den, closed) in cases.items():
            want = SI.grand_product_ints(num, den, p)
            assert closed is None or closed == want, (n, name)
            if name == "zero_in_num":
                assert all(want[:zero_at + 1]) and not any(want[zero_at + 1:])
            assert np.array_equal(co.grand_product(F.fid, F.enc(num), F.enc(den)), F.enc(want)), (n, name)


@pytest.mark.parametrize("fname", SI.FIELDS3)
def test_lincomb_and_scale_closed_forms_equal_the_c_oracle(po, co, fname):
    F = SI.field(po, fname)
    for label, cols, idx, coefs, sub0, want in lincomb_cases(po, fname, SCALE_N):
        enc = [F.enc(col) for col in cols]
        got = co.lincomb(F.fid, [enc[i] for i in idx], F.enc(coefs), F.enc1(sub0) if sub0 is not None else None)
        assert np.array_equal(got, F.enc(want)), label
    a, cases = scale_cases(po, fname)
    for pat, fac in cases:
        want = SI.scale_ints(SI.scale_ints(a, pat, F.p), [fac], F.p)
        got = co.scale_periodic(F.fid, co.scale_periodic(F.fid, F.enc(a), F.enc(pat)), F.enc([fac]))
        assert np.array_equal(got, F.enc(want)), (pat[:2], len(pat), fac)


# ---------------------------------------------------------------- GPU: NTT
@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS3)
@pytest.mark.parametrize("log_n", NTT_LOGS)
def test_ntt_structured_inputs(pkg, po, co, ctx, fname, log_n):
    """every store of a single-frequency transform but one is congruent to zero, and exact zeros are what climbs to the top of the butterflies' lazy range"""
    spec = pkg.fields.FIELDS[fname]
    for label, a, omega, want, _ in ntt_cases(po, co, fname, log_n):
        assert np.array_equal(pkg.best_fft(ctx, spec, a, omega, log_n), want), label


@pytest.mark.gpu
def test_ntt_structured_inputs_full_twiddle_table(pkg, po, co, fname="bn254_fr"):
    """the same on a context that keeps all N powers of omega (the default one reads the half table and negates)"""
    spec = pkg.fields.FIELDS[fname]
    full = pkg.Context(0)
    full.set_tuning("ntt_full_table_log", 24)
    for log_n in (11, 13):
        for label, a, omega, want, _ in ntt_cases(po, co, fname, log_n):
            assert np.array_equal(pkg.best_fft(full, spec, a, omega, log_n), want), (log_n, label)
    full.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
@pytest.mark.parametrize("j,k", [(5, 10), (3, 11), (5, 12)])
def test_domain_wrappers_structured_inputs(pkg, po, ctx, fname, j, k):
    """constant, X and zero through lagrange_to_coeff / coeff_to_extended / extended_to_coeff (the zero-padded input, the zeta factors before and after), and the
    constant and zero polynomials through the internal-form pair"""
    import torch
    ev = pkg.evaluation
    F, spec = SI.field(po, fname), pkg.fields.FIELDS[fname]
    p, c = F.p, SI.constant_c(F)
    d = pkg.EvaluationDomain(ctx, spec, j, k)
    n, ext_n, keep = d.n, 1 << d.extended_k, d.n * (j - 1)
    const_poly, x_poly, zero = [c] + [0] * (n - 1), [0, 1] + [0] * (n - 2), [0] * n
    assert np.array_equal(d.lagrange_to_coeff(F.enc([c] * n)), F.enc(const_poly))
    assert np.array_equal(d.lagrange_to_coeff(F.enc(zero)), F.enc(zero))
    coset, v = [], d.g_coset
    for _ in range(ext_n):
        coset.append(v)
        v = v * d.extended_omega % p
    for poly, ext in ((const_poly, [c] * ext_n), (x_poly, coset), (zero, [0] * ext_n)):
        got = d.coeff_to_extended(F.enc(poly))
        assert np.array_equal(got, F.enc(ext))
        assert np.array_equal(d.extended_to_coeff(got), F.enc(poly + [0] * (keep - n)))
    e = F.enc1
    for poly, value in ((const_poly, c), (zero, 0)):
        dc = ctx.upload(F.enc(poly))
        dext = _poisoned((ext_n, 4))
        torch.cuda.synchronize()
        ctx.coset_ntt_form_device(spec.id, dc.data_ptr(), k, dext.data_ptr(), d.extended_k, e(d.extended_omega), e(d.g_coset), 1, ev.FORM_OUT_INTERNAL)
        ctx.synchronize()
        internal = np.array(po.limbs64(value * pow(2, SI.INTERNAL_SHIFT, p) % p), dtype=np.uint64)      # x * 2^261 mod p, canonical
        assert np.array_equal(_np(dext), np.tile(internal, (ext_n, 1)))
        ctx.coset_intt_form_device(spec.id, dext.data_ptr(), d.extended_k, e(d.extended_omega_inv), e(d.extended_ifft_divisor), e(d.g_coset), 1, ev.FORM_IN_INTERNAL)
        ctx.synchronize()
        got = _np(dext)
        assert np.array_equal(got[:n], F.enc(poly)) and not got[n:].any()


# ---------------------------------------------------------------- GPU: eval_polynomial
@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
@pytest.mark.parametrize("n", EVAL_NS)
def test_eval_polynomial_structured(pkg, po, ctx, fname, n):
    """every vector family at 0, 1, -1, 2, 1/2 and at roots of unity of order 8, 2048 and n: x^8 and x^2048 equal to one, sums of whole periods equal to zero"""
    F = SI.field(po, fname)
    vecs, cases = eval_cases(po, fname, n)
    for vn, zn, z, want, _ in cases:
        assert np.array_equal(ctx.eval_polynomial(F.fid, vecs[vn], F.enc1(z)), F.enc1(want)), (vn, zn)


@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
@pytest.mark.parametrize("n", EVAL_NS)
def test_eval_polynomial_multi_structured(pkg, po, ctx, fname, n):
    """five polynomials x four points a call, all pairs and under a `wanted` mask, over a poisoned output"""
    import torch
    F = SI.field(po, fname)
    vecs, cases = eval_cases(po, fname, n)
    want = {(vn, zn): w for vn, zn, z, w, _ in cases}
    pts = SI.points(F, n)
    names = list(vecs)
    dev = {vn: ctx.upload(a) for vn, a in vecs.items()}
    masks = [0b1011, 0b0000, 0b0100, 0b1111, 0b0001]
    for g, zgroup in enumerate((["0", "1", "-1", "2"], ["half", "w8", "w2048", "wn"], ["wn_inv", "w8", "-1", "0"])):
        penc = F.enc([pts[zn] for zn in zgroup])
        for first in range(0, len(names), 5):
            group = (names + names)[first:first + 5]
            for wanted in (None, masks[g:] + masks[:g]):
                out = _poisoned((4, 5, 4))
                torch.cuda.synchronize()
                ctx.eval_polynomial_multi_device(F.fid, [dev[vn].data_ptr() for vn in group], n, penc, out.data_ptr(), wanted=wanted)
                ctx.synchronize()
                got = _np(out)
                for i, zn in enumerate(zgroup):
                    for b, vn in enumerate(group):
                        w = want[(vn, zn)] if wanted is None or (wanted[b] >> i) & 1 else 0
                        assert np.array_equal(got[i, b], F.enc1(w)), (vn, zn, wanted)


# ---------------------------------------------------------------- GPU: kate_division, vanishing quotient
@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
@pytest.mark.parametrize("n", KATE_NS)
def test_kate_division_structured(pkg, po, ctx, fname, n):
    """the host entry point and the batched device one (the six polynomials of a point in one launch, poisoned outputs): quotients that are all zero, all one,
    alternating 1, 0, a shift, powers of a root of unity, and the exact b of (X - z) b"""
    import torch
    F = SI.field(po, fname)
    cases = kate_cases(po, fname, n)
    for zn in SI.points(F, n):
        group = [c for c in cases if c[1] == zn]
        z = F.enc1(group[0][2])
        for pn, _, _, a, want, _ in group:
            assert np.array_equal(ctx.kate_division(F.fid, a, z), F.enc(want)), (pn, zn)
        da = ctx.upload(np.stack([c[3] for c in group]))
        dq = _poisoned((len(group), n, 4))
        torch.cuda.synchronize()
        ctx.kate_division_batch_device(F.fid, [da[i].data_ptr() for i in range(len(group))], n, np.tile(z, (len(group), 1)), [dq[i].data_ptr() for i in range(len(group))])
        ctx.synchronize()
        got = _np(dq)
        for i, (pn, _, _, a, want, _) in enumerate(group):
            assert np.array_equal(got[i, :n - 1], F.enc(want)), (pn, zn)


def _vq_point_sets(po, F, n):
    """name -> points (ints), those of at most n points"""
    p = F.p
    wn = F.omega(SI.log2_ceil(n))
    x = SI.uniform_ints(po, F, 1, 9300)[0]
    w2048 = F.omega(11)
    sets = {"zero": [0], "pm_one": [1, p - 1], "x_wx": [x, wn * x % p, F.inv(wn) * x % p], "w8": [pow(F.omega(3), i, p) for i in range(1, 8)],
            "w2048": [pow(w2048, i, p) for i in range(5, 37)]}
    return {k: v for k, v in sets.items() if len(v) <= n and len(set(v)) == len(v)}


def _run_vq(ctx, F, polys, n, sets):
    import torch
    d = ctx.upload(np.stack(polys))
    out = _poisoned((len(polys), n, 4))
    torch.cuda.synchronize()
    ctx.vanishing_quotient_batch_device(F.fid, [d[i].data_ptr() for i in range(len(polys))], n, [F.enc(s) for s in sets], [out[i].data_ptr() for i in range(len(polys))])
    ctx.synchronize()
    return _np(out)


@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
@pytest.mark.parametrize("n", KATE_NS)
def test_vanishing_quotient_structured(pkg, po, co, ctx, fname, n):
    """the six polynomials by {0}, {1, -1}, {x, w x, x / w} and 32 consecutive powers of w_2048, against the chain of co.kate_division (and of Python-integer
    divisions at n <= 64); the top m outputs exactly zero over a poisoned buffer"""
    import shplonk_oracle as SO
    F = SI.field(po, fname)
    for sname, pts in _vq_point_sets(po, F, n).items():
        m = len(pts)
        polys = SI.kate_polys(po, F, n, pts[0])
        got = _run_vq(ctx, F, [F.enc(a) for a in polys.values()], n, [pts] * len(polys))
        for b, (pn, a) in enumerate(polys.items()):
            q = F.enc(a)
            for z in pts:
                q = co.kate_division(F.fid, q, F.enc1(z)) if q.shape[0] > 1 else np.zeros((0, 4), dtype=np.uint64)
            assert q.shape[0] == n - m
            if n <= 64:
                assert np.array_equal(q, F.enc(SO.chained_quotient(a, pts, F.p))), (sname, pn)
            assert np.array_equal(got[b, :n - m], q), (sname, pn)
            assert not got[b, n - m:].any(), (sname, pn)


@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
def test_vanishing_quotient_of_all_ones_by_the_eighth_roots(pkg, po, co, ctx, fname):
    """(X^4096 - 1) / (X - 1) by the seven 8th roots of unity other than 1: sum_k X^(8 k), every other coefficient and the remainder exactly zero"""
    F = SI.field(po, fname)
    n = 4096
    pts = [pow(F.omega(3), i, F.p) for i in range(1, 8)]
    want = [1 if i % 8 == 0 else 0 for i in range(n - 7)]
    q = F.enc([1] * n)
    for z in pts:
        q = co.kate_division(F.fid, q, F.enc1(z))
    assert np.array_equal(q, F.enc(want))
    got = _run_vq(ctx, F, [F.enc([1] * n), F.enc([F.p - 1] * n)], n, [pts, pts[::-1]])
    assert np.array_equal(got[0, :n - 7], F.enc(want)) and not got[0, n - 7:].any()
    assert np.array_equal(got[1, :n - 7], F.enc([F.p - w if w else 0 for w in want])) and not got[1, n - 7:].any()


# ---------------------------------------------------------------- GPU: lincomb, scale
@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
def test_lincomb_structured(pkg, po, ctx, fname):
    """sums that cancel to zero in one launch and across accumulating launches (41 and 97 columns), 40 / 41 / 97 products (p-1)(p-1), and sub0 equal to the sum"""
    import torch
    F = SI.field(po, fname)
    n = SCALE_N
    for label, cols, idx, coefs, sub0, want in lincomb_cases(po, fname, n):
        d = [ctx.upload(F.enc(col)) for col in cols]
        out = _poisoned((n, 4))
        torch.cuda.synchronize()
        ctx.lincomb_device(F.fid, [d[i].data_ptr() for i in idx], F.enc(coefs), n, out.data_ptr(), F.enc1(sub0) if sub0 is not None else None)
        ctx.synchronize()
        assert np.array_equal(_np(out), F.enc(want)), label


@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
def test_scale_structured(pkg, po, ctx, fname):
    """patterns of zeros, ones, p - 1 and a mix at periods 1, 2, 4, 8, then the device factor 0, 1, p - 1, on a vector that holds 0, 1 and p - 1 itself"""
    import torch
    F = SI.field(po, fname)
    a, cases = scale_cases(po, fname)
    enc_a = F.enc(a)
    for pat, fac in cases:
        d = ctx.upload(enc_a)
        dfac = ctx.upload(F.enc([fac]))
        torch.cuda.synchronize()
        ctx.scale_device(F.fid, d.data_ptr(), SCALE_N, F.enc(pat), 0)
        ctx.synchronize()
        want = SI.scale_ints(a, pat, F.p)
        assert np.array_equal(_np(d), F.enc(want)), (pat[:2], len(pat))
        ctx.scale_device(F.fid, d.data_ptr(), SCALE_N, None, dfac.data_ptr())
        ctx.synchronize()
        assert np.array_equal(_np(d), F.enc(SI.scale_ints(want, [fac], F.p))), (pat[:2], len(pat), fac)


# ---------------------------------------------------------------- GPU: inversion, products
@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
def test_batch_invert_structured(pkg, po, ctx, fname):
    """both operand lists at 1023 / 1024 / 1025 elements with zeros interleaved, through the host and the device entry point and through field_op "inv".
    The batch inversion runs f29_inv_safegcd once a call, on the product of the call's non-zero elements; the last part therefore gives every x of the first list
    a call of its own, between two zeros, so that the divstep loop starts from exactly each chosen integer."""
    import torch
    F = SI.field(po, fname)
    for v, inv in invert_vectors(po, fname):
        enc_v, enc_inv = F.enc(v), F.enc(inv)
        assert np.array_equal(ctx.batch_invert(F.fid, enc_v), enc_inv), len(v)
        d = ctx.upload(enc_v)
        torch.cuda.synchronize()
        ctx.batch_invert_device(F.fid, d.data_ptr(), len(v))
        ctx.synchronize()
        assert np.array_equal(_np(d), enc_inv), len(v)
    xs, vs = SI.inversion_operands(F)
    for lst in (xs, vs):
        assert np.array_equal(ctx.field_op(F.fid, "inv", F.enc(lst)), F.enc([F.inv(x) for x in lst]))
    rows = [y for x in xs for y in (0, x, 0)]
    d = ctx.upload(F.enc(rows))
    torch.cuda.synchronize()
    for i in range(len(xs)):
        ctx.batch_invert_device(F.fid, d.data_ptr() + 96 * i, 3)
    ctx.synchronize()
    got = _np(d).reshape(len(xs), 3, 4)
    want = F.enc([y for x in xs for y in (0, F.inv(x), 0)]).reshape(len(xs), 3, 4)
    bad = [hex(vs[i]) for i in range(len(xs)) if not np.array_equal(got[i], want[i])]
    assert not bad, "wrong inverses for the divstep starting integers %r" % bad[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
@pytest.mark.parametrize("n", PRODUCT_NS)
def test_grand_product_structured(pkg, po, ctx, fname, n):
    """running products that stay one, alternate between 1 and p - 1, and are exactly zero behind a zero numerator; prefix_product_device out of place over a
    poisoned buffer and in place"""
    import torch
    F = SI.field(po, fname)
    p = F.p
    cases, zero_at = SI.grand_product_cases(po, F, n)
    for name, (num, den, _) in cases.items():
        want = SI.grand_product_ints(num, den, p)
        assert np.array_equal(ctx.grand_product(F.fid, F.enc(num), F.enc(den)), F.enc(want)), name
        if name in ("ones", "pm1", "zero_in_num"):
            want = F.enc(SI.grand_product_ints(num, [1] * n, p))
            d = ctx.upload(F.enc(num))
            out = _poisoned((n, 4))
            torch.cuda.synchronize()
            ctx.prefix_product_device(F.fid, d.data_ptr(), n, out.data_ptr())
            ctx.prefix_product_device(F.fid, d.data_ptr(), n, d.data_ptr())
            ctx.synchronize()
            assert np.array_equal(_np(out), want) and np.array_equal(_np(d), want), name


# ---------------------------------------------------------------- GPU: field_op
@pytest.mark.gpu
@pytest.mark.parametrize("fname", ["bn254_fr", "bn254_fq", "pasta_fp", "pasta_fq"])
def test_field_mul_lands_on_one_minus_one_and_zero(pkg, po, ctx, fname):
    """256 pairs each of (x, 1/x), (x, -1/x), (0, x) and (p-1, p-1), through the 8 x 32-bit and the 9 x 29-bit multiplier"""
    F = SI.field(po, fname)
    p = F.p
    xs = SI.uniform_ints(po, F, 256, 9400)
    a = F.enc(xs + xs + [0] * 256 + [p - 1] * 256)
    b = F.enc([F.inv(x) for x in xs] + [p - F.inv(x) for x in xs] + xs + [p - 1] * 256)
    want = F.enc([1] * 256 + [p - 1] * 256 + [0] * 256 + [1] * 256)
    for op in ("mul", "mul29"):
        assert np.array_equal(ctx.field_op(F.fid, op, a, b), want), op
        assert np.array_equal(ctx.field_op(F.fid, op, b, a), want), op
