"""What the C ABI does with 256-bit words that are not below the modulus, and with points given more than 64 bytes apart (include/dehalo.h "Non-canonical
words").  Every other test feeds the library what halo2curves produces -- words below p, scalars below r, points 64 bytes apart -- and a C or
Rust caller can hand over anything else.

The contract: a word w read from caller memory stands for w mod p (rule 1); what the library computes and writes is below p (rule 2); the entry points that only
move elements copy the words (rule 3); coordinates are field elements, the identity is the 64 zero bytes (rule 4); bases registered with a stride above 64
bytes are the first 64 bytes of each slot (rule 5).

CPU (no mark): tests/noncanonical_inputs.py itself -- which multiples of p fit which field, residues kept, no family empty -- and that the truth of the GPU
rows, the oracle on the input canonicalised in Python integers, is what it should be on the planted zeros.
GPU: one row per entry point of the issue's table (dehalo.h names the entry points that read caller words through the same kernels and have no row of their
own).  REDUCED rows: on every family of lifted input the row takes, the output equals, word for word, the oracle's on the canonicalised input, and every output
word is below p.  The rows that own a kernel (field ops, best_fft, eval_polynomial, lincomb and scale, batch inversion) take every family; the rows that reach
the same kernels through another entry point (the batched NTT forms, the domain wrappers, the divisions, the products, the MSMs' scalars) keep all_max, mix, the
four special words and of the single lifts those at the first and the last index and at one or two block edges.  COPY rows (upload, download): the output words
are the input words.  Device outputs are written over buffers of all-ones words."""
import ctypes as C

import numpy as np
import pytest

import noncanonical_inputs as NI
import structured_inputs as SI
from test_structured_values import EVAL_NS, KATE_NS, NTT_LOGS, PRODUCT_NS

INVERT_NS = [1, 1023, 1025, 4097]             # one element, a partial block, a second block, a second level of block totals
MSM_NS = [1, 65, 1000]
CURVES = ["bn254", "pallas", "vesta"]
POISON = -1


def _poisoned(shape):
    """all-ones words, in place before anything is queued on the context's stream (which nothing orders with torch's)"""
    import torch
    t = torch.full(shape, POISON, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t


def _np(t):
    return t.cpu().numpy().view(np.uint64)


def reduced(got, want, p, label):
    """the REDUCED verdict: word for word the truth on the canonicalised input, and every word below p"""
    got = np.ascontiguousarray(got, dtype=np.uint64).reshape(-1, 4)
    want = np.ascontiguousarray(want, dtype=np.uint64).reshape(-1, 4)
    assert got.shape == want.shape, label
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError("%r: %d of %d words differ from the truth on the canonicalised input, first at %d: got %s (%s p), want %s" % (
            label, len(bad), len(got), bad[0], hex(NI.to_ints(got[bad[0]])[0]), "below" if NI.all_below(got[bad[0]], p) else "NOT below", hex(NI.to_ints(want[bad[0]])[0])))
    assert NI.all_below(got, p), label


def fam(po, fname, n, seed, singles=True):
    """the families of n uniform elements of the field: [(name, stored, canonical)]"""
    F = po.FIELDS[fname]
    return NI.families(NI.uniform_words(po, F, n, seed), F.p, seed=seed, singles=singles)


# ================================================================================================================ CPU
@pytest.mark.parametrize("fname", NI.ALL_FIELDS)
def test_which_multiples_of_p_fit(po, fname):
    """j = 1 fits every canonical word of all four fields, j <= 4 every BN254 word, j = 2 every Pasta word -- and no more than that"""
    p = po.FIELDS[fname].p
    every = NI.FAMILY_LIFTS[fname]
    assert every == ((1, 2, 3, 4) if fname.startswith("bn254") else (1, 2)) and 1 in every
    edge = NI.to_words([0, 1, p - 1, NI.W % p])
    for j in every:
        out = NI.to_ints(NI.lift(edge, j, p))
        assert out == [v + j * p for v in NI.to_ints(edge)] and all(p <= v < NI.W for v in out)
    assert NI.max_lift(p - 1, p) == every[-1] and NI.max_lift(0, p) == every[-1] + 1      # one more fits the small words only
    with pytest.raises(AssertionError, match="does not fit"):
        NI.lift(edge, every[-1] + 1, p)
    with pytest.raises(OverflowError):
        NI.to_words([NI.W])
    assert NI.to_ints(NI.lift(edge, [0, 1, 0, every[-1]], p)) == [0, 1 + p, p - 1, NI.W % p + every[-1] * p]


@pytest.mark.parametrize("fname", NI.ALL_FIELDS)
@pytest.mark.parametrize("n", [1, 2, 65, 1025, 4097])
def test_families_keep_residues_and_none_is_empty(po, fname, n):
    p = po.FIELDS[fname].p
    base = NI.uniform_words(po, po.FIELDS[fname], n, 40 + n)
    fams = NI.families(base, p)
    names = [name for name, _, _ in fams]
    assert names[:2] == ["all_max", "mix"] and names[-4:] == list(NI.special_words(p))
    assert ["one@%d" % i for i in NI.positions(n)] == names[2:-4] and "one@0" in names and "one@%d" % (n - 1) in names
    if n == 4097:
        assert {"one@%d" % i for i in (255, 256, 1023, 1024, 2047, 2048)} <= set(names)
    for name, stored, canonical in fams:
        si, ci = NI.to_ints(stored), NI.to_ints(canonical)
        assert len(si) == n and all(0 <= v < NI.W for v in si) and all(v < p for v in ci), name
        assert [v % p for v in si] == ci and np.array_equal(NI.canon(stored, p), canonical), name
        lifted = [i for i, v in enumerate(si) if v >= p]
        assert lifted, "family %s is empty" % name
        if name == "all_max":
            assert len(lifted) == n and all(v + p >= NI.W for v in si)
        if name.startswith("one@"):
            assert lifted == [int(name[4:])] and si[lifted[0]] + p >= NI.W
        if name in NI.special_words(p):
            assert lifted == NI.positions(n) and {si[i] for i in lifted} == {NI.special_words(p)[name][0]}
            assert np.array_equal(np.delete(canonical, lifted, axis=0), np.delete(base, lifted, axis=0))
        else:
            assert np.array_equal(canonical, base), name
    if n >= 1025:
        mix = NI.to_ints(fams[1][1])
        js, top = {(v - c) // p for v, c in zip(mix, NI.to_ints(base))}, NI.FAMILY_LIFTS[fname][-1]
        assert {0, 1} < js <= {0, 1, top, top + 1}            # (top + 1 fits a word below 2^256 mod p: nearly every Pasta word, two in seven of BN254's)
    sp = NI.special_words(p)
    assert sp["zero_as_p"] == (p, 0) and sp["zero_as_top_multiple"][0] % p == 0 and sp["zero_as_top_multiple"][0] + p >= NI.W
    assert sp["one_as_R_plus_p"][1] == NI.W % p and sp["all_ones_word"][0] == NI.W - 1


@pytest.mark.parametrize("fname", SI.FIELDS3)
def test_the_truth_is_the_oracle_on_the_canonicalised_input(po, co, fname):
    """the planted zeros come out of the canonicalisation as zeros and the oracle leaves them zero, the elements around them inverted"""
    F = SI.field(po, fname)
    for name, stored, canonical in fam(po, fname, 1025, 7):
        inv = co.batch_invert(F.fid, canonical)
        ci = NI.to_ints(canonical)
        assert F.dec(inv) == [F.inv(x) if x else 0 for x in F.dec(canonical)], name
        assert all((v == 0) == (NI.to_ints(inv[i:i + 1])[0] == 0) for i, v in enumerate(ci)), name
        if name.startswith("zero_as"):
            assert [i for i, v in enumerate(ci) if v == 0] == NI.positions(1025)


# ================================================================================================================ GPU: field ops
@pytest.mark.gpu
@pytest.mark.parametrize("fname", NI.ALL_FIELDS)
def test_field_ops(pkg, po, co, ctx, fname):
    """REDUCED: add, sub, mul, mul29 with one and with both operands lifted; inv, to_mont, from_mont; the operand of inv stored as p gives 0"""
    F = SI.field(po, fname)
    p, n = F.p, 1100
    b_canon = NI.uniform_words(po, F.of, n, 52)
    b_all = [("canonical", b_canon), ("all_max", NI.families(b_canon, p, singles=False)[0][1]), ("mix", NI.families(b_canon, p, seed=9, singles=False)[1][1])]
    for name, sa, ca in fam(po, fname, n, 51):
        for op in ("add", "sub", "mul", "mul29"):
            want = co.field_op(F.fid, op if op != "mul29" else "mul", ca, b_canon)
            for bname, sb in b_all:
                reduced(ctx.field_op(F.fid, op, sa, sb), want, p, (op, name, bname))
            if op != "sub":
                reduced(ctx.field_op(F.fid, op, b_all[1][1], sa), want, p, (op, "swapped", name))
        reduced(ctx.field_op(F.fid, "inv", sa), F.enc([F.inv(x) if x else 0 for x in F.dec(ca)]), p, ("inv", name))
        reduced(ctx.field_op(F.fid, "to_mont", sa), co.field_op(F.fid, "to_mont", ca), p, ("to_mont", name))
        reduced(ctx.field_op(F.fid, "from_mont", sa), co.field_op(F.fid, "from_mont", ca), p, ("from_mont", name))
    just_p = NI.to_words([p, 2 * p, 3 * p, 0])
    assert not ctx.field_op(F.fid, "inv", just_p).any()
    # the device form, out of place over a poisoned buffer
    name, sa, ca = fam(po, fname, n, 51)[1]
    da, db, out = ctx.upload(sa), ctx.upload(b_all[1][1]), _poisoned((n, 4))
    ctx.field_op_device(F.fid, "mul", da.data_ptr(), db.data_ptr(), out.data_ptr(), n)
    ctx.synchronize()
    reduced(_np(out), co.field_op(F.fid, "mul", ca, b_canon), p, "mul, device")


# ================================================================================================================ GPU: NTT and domain
@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS3)
@pytest.mark.parametrize("log_n", [0] + NTT_LOGS)
def test_ntt(pkg, po, co, ctx, fname, log_n):
    """REDUCED: best_fft forward and inverse on every family, with the root canonical and lifted.  A transform of one element is no copy: it stores the
    canonical word like every other size (the pass's output multiplication runs)."""
    F = SI.field(po, fname)
    p, n = F.p, 1 << log_n
    fams = fam(po, fname, n, 60 + log_n)
    truth = {}
    for direction, w in (("fwd", F.omega(log_n)), ("inv", F.inv(F.omega(log_n)))):
        omega = F.enc1(w)
        omegas = [("canonical", omega), ("lifted 1", NI.lift_word(omega, p, 1)), ("lifted max", NI.lift_word(omega, p))]
        for name, stored, canonical in fams:
            key = (direction, canonical.tobytes())
            if key not in truth:
                truth[key] = co.best_fft(F.fid, canonical, omega, log_n, 4) if log_n else canonical
            for oname, om in (omegas if name in ("all_max", "mix") else omegas[:1]):
                reduced(ctx.ntt(F.fid, stored, log_n, om), truth[key], p, (direction, name, oname))


@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
@pytest.mark.parametrize("k", [3, 11, 13])
def test_ntt_batched_device_entry_points(pkg, po, co, ctx, fname, k):
    """REDUCED: ntt_device, intt_scaled_device and lagrange_to_coeff_device, one family per polynomial of the batch, root and divisor lifted"""
    F = SI.field(po, fname)
    p, n = F.p, 1 << k
    fams = [f for f in fam(po, fname, n, 80 + k) if not f[0].startswith("one@") or f[0] in ("one@0", "one@%d" % (n - 1))]
    stored, canonical = np.stack([f[1] for f in fams]), [f[2] for f in fams]
    w, wi, ni = F.enc1(F.omega(k)), F.enc1(F.inv(F.omega(k))), F.enc1(F.inv(n))
    lw, lwi, lni = NI.lift_word(w, p), NI.lift_word(wi, p), NI.lift_word(ni, p)
    d = ctx.upload(stored)
    ctx.ntt_device(F.fid, d.data_ptr(), k, lw, len(fams))
    ctx.synchronize()
    got = _np(d)
    for b, f in enumerate(fams):
        reduced(got[b], co.best_fft(F.fid, canonical[b], w, k, 2), p, ("ntt_device", f[0]))
    d = ctx.upload(stored)
    out = _poisoned((len(fams), n, 4))
    ctx.lagrange_to_coeff_device(F.fid, d.data_ptr(), out.data_ptr(), k, lwi, lni, len(fams))
    ctx.intt_scaled_device(F.fid, d.data_ptr(), k, lwi, lni, len(fams))
    ctx.synchronize()
    got, got_out = _np(d), _np(out)
    for b, f in enumerate(fams):
        want = co.lagrange_to_coeff(F.fid, canonical[b], k, wi, ni, 2)
        reduced(got[b], want, p, ("intt_scaled_device", f[0]))
        reduced(got_out[b], want, p, ("lagrange_to_coeff_device", f[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
@pytest.mark.parametrize("j,k", [(5, 10), (3, 11), (5, 12)])
def test_domain_wrappers(pkg, po, co, ctx, fname, j, k):
    """REDUCED: lagrange_to_coeff, coeff_to_extended and extended_to_coeff (host entry points and the batched device ones) on lifted data with lifted roots,
    divisors and zeta"""
    F, spec = SI.field(po, fname), pkg.fields.FIELDS[fname]
    p = F.p
    d = pkg.EvaluationDomain(ctx, spec, j, k)
    n, ek, ext_n = d.n, d.extended_k, 1 << d.extended_k
    e = F.enc1
    lift1 = lambda v: NI.lift_word(e(v), p)
    keep = lambda f: not f[0].startswith("one@") or f[0] in ("one@0", "one@%d" % (n - 1), "one@1023", "one@1024")
    for name, stored, canonical in filter(keep, fam(po, fname, n, 90 + k)):
        reduced(ctx.intt_scaled(F.fid, stored, k, lift1(d.omega_inv), lift1(d.ifft_divisor)), co.lagrange_to_coeff(F.fid, canonical, k, e(d.omega_inv), e(d.ifft_divisor), 4), p,
                ("lagrange_to_coeff", name))
        want_ext = co.coeff_to_extended(F.fid, canonical, k, ek, e(d.extended_omega), e(d.g_coset), 4)
        reduced(ctx.coset_ntt(F.fid, stored, k, ek, lift1(d.extended_omega), lift1(d.g_coset)), want_ext, p, ("coeff_to_extended", name))
        dc, dext = ctx.upload(np.stack([stored, canonical])), _poisoned((2, ext_n, 4))
        ctx.coset_ntt_device(F.fid, dc.data_ptr(), k, dext.data_ptr(), ek, lift1(d.extended_omega), e(d.g_coset), 2)
        ctx.synchronize()
        got = _np(dext)
        reduced(got[0], want_ext, p, ("coset_ntt_device", name))
        reduced(got[1], want_ext, p, ("coset_ntt_device, canonical beside lifted", name))
    ext_keep = lambda f: not f[0].startswith("one@") or f[0] in ("one@0", "one@%d" % (ext_n - 1), "one@2047", "one@2048")
    for name, stored, canonical in filter(ext_keep, fam(po, fname, ext_n, 95 + k)):
        want = co.extended_to_coeff(F.fid, canonical, ek, e(d.extended_omega_inv), e(d.extended_ifft_divisor), e(d.g_coset), 4)
        reduced(ctx.coset_intt(F.fid, stored, ek, lift1(d.extended_omega_inv), lift1(d.extended_ifft_divisor), lift1(d.g_coset)), want, p, ("extended_to_coeff", name))
        dv = ctx.upload(stored)
        ctx.coset_intt_device(F.fid, dv.data_ptr(), ek, e(d.extended_omega_inv), lift1(d.extended_ifft_divisor), lift1(d.g_coset), 1)
        ctx.synchronize()
        reduced(_np(dv), want, p, ("coset_intt_device", name))


# ================================================================================================================ GPU: evaluation and division
def _points(po, F, n):
    """the points a lifted polynomial is evaluated / divided at: (name, stored word, canonical word)"""
    p = F.p
    z = SI.uniform_ints(po, F, 1, 3000 + n)[0]
    out = [("z", F.enc1(z), F.enc1(z)), ("z lifted", NI.lift_word(F.enc1(z), p), F.enc1(z))]
    for name, (stored, stands_for) in NI.special_words(p).items():
        out.append((name, NI.to_words([stored])[0], NI.to_words([stands_for])[0]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
@pytest.mark.parametrize("n", EVAL_NS)
def test_eval_polynomial(pkg, po, co, ctx, fname, n):
    """REDUCED: eval_polynomial with lifted coefficients and a lifted point; eval_polynomial_device over a batch; the multi-point and any-points forms"""
    F = SI.field(po, fname)
    p = F.p
    pts = _points(po, F, n)
    fams = fam(po, fname, n, 100 + n)
    truth = {}

    def want(canonical, zc):
        key = (canonical.tobytes(), zc.tobytes())
        if key not in truth:
            truth[key] = co.eval_polynomial(F.fid, canonical, zc, 2)
        return truth[key]

    for name, stored, canonical in fams:
        for zn, zs, zc in (pts if name in ("all_max", "mix", "all_ones_word") else pts[1:2]):
            reduced(ctx.eval_polynomial(F.fid, stored, zs), want(canonical, zc), p, (name, zn))
    # the batch of one call: every family a polynomial; and the multi forms: five polynomials, four points
    stack = ctx.upload(np.stack([f[1] for f in fams]))
    out = _poisoned((len(fams), 4))
    ctx.eval_polynomial_device(F.fid, stack.data_ptr(), n, n, len(fams), pts[1][1], out.data_ptr())
    ctx.synchronize()
    got = _np(out)
    for b, f in enumerate(fams):
        reduced(got[b], want(f[2], pts[1][2]), p, ("eval_polynomial_device", f[0]))
    group = [0, 1, len(fams) - 4, len(fams) - 2, len(fams) - 1]
    four = [pts[1], pts[2], pts[4], pts[5]]
    for launch in ("multi", "points"):
        out = _poisoned((4, 5, 4))
        fn = ctx.eval_polynomial_multi_device if launch == "multi" else ctx.eval_polynomial_points_device
        fn(F.fid, [stack[b].data_ptr() for b in group], n, np.stack([q[1] for q in four]), out.data_ptr())
        ctx.synchronize()
        got = _np(out)
        for i, q in enumerate(four):
            for c, b in enumerate(group):
                reduced(got[i, c], want(fams[b][2], q[2]), p, (launch, fams[b][0], q[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
@pytest.mark.parametrize("n", KATE_NS)
def test_kate_division_and_vanishing_quotient(pkg, po, co, ctx, fname, n):
    """REDUCED: kate_division (host, and the batched device form over a poisoned buffer) with lifted coefficients and a lifted point; the vanishing quotient
    by {z, z', z''} given lifted, against the chain of divisions on the canonical input"""
    F = SI.field(po, fname)
    p = F.p
    pts = _points(po, F, n)
    fams = [f for f in fam(po, fname, n, 200 + n) if not f[0].startswith("one@") or f[0] in ("one@0", "one@%d" % (n - 1), "one@2047", "one@2048")]
    for name, stored, canonical in fams:
        for zn, zs, zc in (pts if name in ("all_max", "mix") else pts[1:2]):
            reduced(ctx.kate_division(F.fid, stored, zs), co.kate_division(F.fid, canonical, zc), p, (name, zn))
    group = fams[:8]
    da = ctx.upload(np.stack([f[1] for f in group]))
    dq = _poisoned((len(group), n, 4))
    ctx.kate_division_batch_device(F.fid, [da[i].data_ptr() for i in range(len(group))], n, np.tile(pts[1][1], (len(group), 1)), [dq[i].data_ptr() for i in range(len(group))])
    ctx.synchronize()
    got = _np(dq)
    for i, f in enumerate(group):
        reduced(got[i, :n - 1], co.kate_division(F.fid, f[2], pts[1][2]), p, ("kate_division_batch_device", f[0]))
    zs = SI.uniform_ints(po, F, 3, 3100 + n)
    if n > len(zs):
        lifted_set = np.stack([NI.lift_word(F.enc1(z), p) for z in zs])
        dq = _poisoned((len(group), n, 4))
        ctx.vanishing_quotient_batch_device(F.fid, [da[i].data_ptr() for i in range(len(group))], n, [lifted_set] * len(group), [dq[i].data_ptr() for i in range(len(group))])
        ctx.synchronize()
        got = _np(dq)
        for i, f in enumerate(group):
            q = f[2]
            for z in zs:
                q = co.kate_division(F.fid, q, F.enc1(z))
            reduced(got[i, :n - len(zs)], q, p, ("vanishing_quotient", f[0]))
            assert not got[i, n - len(zs):].any(), f[0]


# ================================================================================================================ GPU: linear kernels
@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
def test_lincomb_and_scale(pkg, po, co, ctx, fname):
    """REDUCED: lincomb with lifted columns, lifted coefficients and a lifted constant to subtract (one launch and two); scale by a lifted pattern and by a
    lifted device factor"""
    F = SI.field(po, fname)
    p, n = F.p, 4101
    fams = fam(po, fname, n, 300)
    other = NI.uniform_words(po, F.of, n, 301)
    for count in (3, 41):
        coefs = NI.uniform_words(po, F.of, count, 302 + count)
        coef_fams = NI.families(coefs, p, edges=(), singles=False)
        for name, stored, canonical in fams:
            cols_c = [canonical if i % 2 == 0 else other for i in range(count)]
            d0, d1 = ctx.upload(stored), ctx.upload(other)
            for cname, cs, cc in ([coef_fams[0], coef_fams[1], coef_fams[2]] if name in ("all_max", "mix") else coef_fams[:1]):
                for sname, sub_s, sub_c in ([("none", None, None)] + [(q[0], q[1], q[2]) for q in _points(po, F, n)[1:]] if name == "all_max" else [("z lifted",) + _points(po, F, n)[1][1:]]):
                    want = co.lincomb(F.fid, cols_c, cc, sub_c)
                    out = _poisoned((n, 4))
                    ctx.lincomb_device(F.fid, [(d0 if i % 2 == 0 else d1).data_ptr() for i in range(count)], cs, n, out.data_ptr(), sub_s)
                    ctx.synchronize()
                    reduced(_np(out), want, p, ("lincomb", count, name, cname, sname))
    pat = NI.uniform_words(po, F.of, 8, 310)
    fac = NI.uniform_words(po, F.of, 1, 311)
    for name, stored, canonical in fams:
        for period in (1, 8):
            want = co.scale_periodic(F.fid, canonical, pat[:period])
            d = ctx.upload(stored)
            ctx.scale_device(F.fid, d.data_ptr(), n, NI.lift(pat[:period], 1, p), 0)
            ctx.synchronize()
            reduced(_np(d), want, p, ("scale, pattern", name, period))
        dfac = ctx.upload(NI.lift(fac, 1, p))
        ctx.scale_device(F.fid, d.data_ptr(), n, None, dfac.data_ptr())
        ctx.synchronize()
        reduced(_np(d), co.scale_periodic(F.fid, want, fac), p, ("scale, device factor", name))
    # a factor that is zero mod p, stored as p
    d, dfac = ctx.upload(fams[0][1]), ctx.upload(NI.to_words([p]))
    ctx.scale_device(F.fid, d.data_ptr(), n, None, dfac.data_ptr())
    ctx.synchronize()
    assert not _np(d).any()


# ================================================================================================================ GPU: inversion and products
@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
@pytest.mark.parametrize("n", INVERT_NS)
def test_batch_invert(pkg, po, co, ctx, fname, n):
    """REDUCED: zeros stored as multiples of p at index 0, the last index and both sides of every block edge (all together, and one at a time): those positions
    give 0 and every other element is still inverted -- one live multiple of p would make the call's only inversion, and with it every output, zero"""
    F = SI.field(po, fname)
    p = F.p
    fams = fam(po, fname, n, 400 + n)
    base = fams[0][2]
    for j in sorted({1, NI.max_lift(0, p)}):                  # one zero at a time, as p and as the largest multiple of p
        for i in NI.positions(n):
            s, c = base.copy(), base.copy()
            s[i], c[i] = NI.to_words([j * p])[0], 0
            fams.append(("zero %d p @%d" % (j, i), s, c))
    for name, stored, canonical in fams:
        want = co.batch_invert(F.fid, canonical)
        reduced(ctx.batch_invert(F.fid, stored), want, p, ("host", name))
        d = ctx.upload(stored)
        ctx.batch_invert_device(F.fid, d.data_ptr(), n)
        ctx.synchronize()
        reduced(_np(d), want, p, ("device", name))


@pytest.mark.gpu
@pytest.mark.parametrize("fname", SI.FIELDS2)
@pytest.mark.parametrize("n", PRODUCT_NS)
def test_grand_and_prefix_products(pkg, po, co, ctx, fname, n):
    """REDUCED: grand_product (host, device, batch) with lifted numerators and denominators, denominators that are zero mod p included (their inverse is 0, as
    upstream's batch_invert leaves it); prefix_product_device"""
    F = SI.field(po, fname)
    p = F.p
    num = NI.uniform_words(po, F.of, n, 500 + n)
    num_l = NI.families(num, p, singles=False)[1][1]
    fams = [f for f in fam(po, fname, n, 501 + n) if not f[0].startswith("one@") or f[0] in ("one@0", "one@%d" % (n - 1), "one@1023", "one@1024")]
    for name, den_s, den_c in fams:
        want = co.grand_product(F.fid, num, den_c)
        reduced(ctx.grand_product(F.fid, num_l, den_s), want, p, ("grand_product", name))
        dn, dd, z = ctx.upload(num_l), ctx.upload(den_s), _poisoned((n, 4))
        ctx.grand_product_device(F.fid, dn.data_ptr(), dd.data_ptr(), n, z.data_ptr())
        ctx.synchronize()
        reduced(_np(z), want, p, ("grand_product_device", name))
    # the batch: every family a column
    dn = ctx.upload(np.stack([num_l] * len(fams)))
    dd = ctx.upload(np.stack([f[1] for f in fams]))
    z = _poisoned((len(fams), n, 4))
    ctx.grand_product_batch_device(F.fid, dn.data_ptr(), dd.data_ptr(), n, len(fams), n, z.data_ptr())
    ctx.synchronize()
    got = _np(z)
    for b, f in enumerate(fams):
        reduced(got[b], co.grand_product(F.fid, num, f[2]), p, ("grand_product_batch_device", f[0]))
    ones = F.enc([1] * n)
    for name, stored, canonical in fams:
        d, out = ctx.upload(stored), _poisoned((n, 4))
        ctx.prefix_product_device(F.fid, d.data_ptr(), n, out.data_ptr())
        ctx.prefix_product_device(F.fid, d.data_ptr(), n, d.data_ptr())
        ctx.synchronize()
        want = co.grand_product(F.fid, canonical, ones)
        reduced(_np(out), want, p, ("prefix_product_device", name))
        reduced(_np(d), want, p, ("prefix_product_device, in place", name))


# ================================================================================================================ GPU: the lookup argument, the copies
@pytest.mark.gpu
@pytest.mark.parametrize("fname", NI.ALL_FIELDS)
@pytest.mark.parametrize("n", [1, 513, 2049, 4100])
def test_permute_expression_pair(pkg, po, co, ctx, fname, n):
    """REDUCED: x and x + p are the same key, and the permuted columns are written from the sorted canonical keys -- they are those of the canonical input,
    word for word below p, not the caller's words moved (host entry point, device entry point over poisoned buffers, the pointer-table form)"""
    import lookup_inputs as LI
    F = SI.field(po, fname)
    p = F.p
    inputs, table, _ = LI.general_case(po, F, "uniform", n)
    ci, ct = F.enc(inputs), F.enc(table)
    want_i, want_t = co.permute_expression_pair(F.fid, ci, ct, n)
    for (name, si, _), (_, st, _) in zip(NI.families(ci, p, seed=3, singles=False)[:2], NI.families(ct, p, seed=4, singles=False)[:2]):
        for label, a, t in (("both", si, st), ("inputs", si, ct), ("table", ci, st)):
            gi, gt = ctx.permute_expression_pair(F.fid, a, t, n)
            reduced(gi, want_i, p, (name, label, "inputs"))
            reduced(gt, want_t, p, (name, label, "table"))
        da, dt, oi, ot = ctx.upload(si), ctx.upload(st), _poisoned((n, 4)), _poisoned((n, 4))
        ctx.permute_expression_pair_device(F.fid, da.data_ptr(), dt.data_ptr(), n, oi.data_ptr(), ot.data_ptr())
        ctx.synchronize()
        reduced(_np(oi), want_i, p, (name, "device", "inputs"))
        reduced(_np(ot), want_t, p, (name, "device", "table"))
        oi, ot = _poisoned((2, n, 4)), _poisoned((2, n, 4))
        ctx.permute_expression_pair_ptrs_device(F.fid, [da.data_ptr(), da.data_ptr()], [dt.data_ptr(), dt.data_ptr()], n, [oi[0].data_ptr(), oi[1].data_ptr()],
                                                [ot[0].data_ptr(), ot[1].data_ptr()])
        ctx.synchronize()
        for y in range(2):
            reduced(_np(oi)[y], want_i, p, (name, "ptrs", y, "inputs"))
            reduced(_np(ot)[y], want_t, p, (name, "ptrs", y, "table"))
    # an input that is in the table only mod p is in the table; one that is not, is not
    if n > 1:
        miss = next(v for v in range(1, 1000) if v not in set(table))
        bad = ci.copy()
        bad[n // 2] = NI.lift_word(F.enc1(miss), p)
        with pytest.raises(pkg.DehaloError) as e:
            ctx.permute_expression_pair(F.fid, bad, NI.families(ct, p, seed=4, singles=False)[0][1], n)
        assert e.value.code == -6


@pytest.mark.gpu
def test_upload_and_download_copy_words(pkg, po, ctx):
    """COPY: upload and download move bytes"""
    for fname in NI.ALL_FIELDS:
        for name, stored, _ in fam(po, fname, 1025, 600, singles=False):
            d = ctx.upload(stored)
            assert np.array_equal(ctx.download(d.data_ptr(), 1025), stored) and np.array_equal(ctx.download_tensor(d), stored), (fname, name)


# ================================================================================================================ GPU: scalars lifted by r
def _scalar_families(po, cs, n, seed):
    fams = NI.families(NI.uniform_words(po, po.FIELDS[cs.scalar.name], n, seed), cs.scalar.p, edges=(64, 256, 512), seed=seed)
    return [f for f in fams if not f[0].startswith("one@") or f[0] in ("one@0", "one@%d" % (n - 1), "one@63", "one@64", "one@256")]


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", MSM_NS)
def test_msm_with_scalars_lifted_by_r(pkg, po, co, ctx, curve, n):
    """REDUCED (the point is that of the canonical scalars): dehalo_msm, msm_batch, msm_device, msm_device_affine over window tables and over a single row,
    and best_multiexp"""
    cs = pkg.fields.CURVES[curve]
    bases = co.synth_bases(cs.id, n)
    fams = _scalar_families(po, cs, n, 700 + n)
    truth = {}
    for name, stored, canonical in fams:
        key = canonical.tobytes()
        if key not in truth:
            truth[key] = co.to_affine(cs.id, co.best_multiexp(cs.id, canonical, bases, 1))
    want = [truth[f[2].tobytes()] for f in fams]
    for precompute in (True, False):
        reg = ctx.register_bases(cs.id, bases, 0, precompute)
        try:
            for (name, stored, _), w in zip(fams, want):
                assert np.array_equal(ctx.to_affine(cs.id, ctx.msm(reg, stored))[0], w.reshape(8)), ("msm", precompute, name)
            got = ctx.to_affine(cs.id, ctx.msm_batch(reg, [f[1] for f in fams]))
            assert np.array_equal(got, np.stack(want).reshape(-1, 8)), ("msm_batch", precompute)
            d = ctx.upload(np.stack([f[1] for f in fams]))
            jac, jac2, aff = _poisoned((len(fams), 12)), _poisoned((len(fams), 12)), _poisoned((len(fams), 8))
            ctx.msm_device(reg, d.data_ptr(), n, len(fams), jac.data_ptr())
            ctx.msm_device_affine(reg, d.data_ptr(), n, len(fams), jac2.data_ptr(), aff.data_ptr())
            ctx.synchronize()
            assert np.array_equal(ctx.to_affine(cs.id, _np(jac)), np.stack(want).reshape(-1, 8)), ("msm_device", precompute)
            assert np.array_equal(_np(aff), np.stack(want).reshape(-1, 8)), ("msm_device_affine", precompute)
            assert np.array_equal(ctx.to_affine(cs.id, _np(jac2)), np.stack(want).reshape(-1, 8)), ("msm_device_affine, jacobian", precompute)
        finally:
            reg.release()
    for (name, stored, _), w in zip(fams, want):
        assert np.array_equal(ctx.to_affine(cs.id, ctx.best_multiexp(cs.id, stored, bases))[0], w.reshape(8)), ("best_multiexp", name)


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_fixed_base_and_blinds_with_scalars_lifted_by_r(pkg, po, co, ctx, curve):
    """REDUCED: fixed_base_mul and fixed_base_blind on all three curves; blind_commitments and the generator_collapse challenge on the Pasta curves"""
    import torch
    cs = pkg.fields.CURVES[curve]
    r = cs.scalar.p
    qw = co.synth_bases(cs.id, 2)
    w = qw[1]
    fb = ctx.fixed_base(cs.id, w)
    mul_truth, blind_truth = {}, {}      # per canonical scalar vector: most families of a size share one
    try:
        for n in MSM_NS:
            # C_i = [a_i] Q, to be blinded to C_i + [b_i] W
            a = NI.uniform_words(po, po.FIELDS[cs.scalar.name], n, 810 + n)
            jac = np.stack([co.best_multiexp(cs.id, a[i:i + 1], qw[:1], 1) for i in range(n)]).reshape(n, 12)
            for name, stored, canonical in _scalar_families(po, cs, n, 800 + n):
                key = (n, canonical.tobytes())
                if key not in mul_truth:
                    mul_truth[key] = np.stack([co.to_affine(cs.id, co.best_multiexp(cs.id, canonical[i:i + 1], w.reshape(1, 8), 1)) for i in range(n)]).reshape(n, 8)
                    blind_truth[key] = np.stack([co.to_affine(cs.id, co.best_multiexp(cs.id, np.stack([a[i], canonical[i]]), qw, 1)) for i in range(n)]).reshape(n, 8)
                d, out = ctx.upload(stored), _poisoned((n, 8))
                fb.mul_device(d.data_ptr(), n, out.data_ptr())
                assert np.array_equal(ctx.download_tensor(out), mul_truth[key]), ("fixed_base_mul", n, name)
                launches = [("fixed_base_blind", lambda dj, db: fb.blind_device(dj, db, n))]
                if curve != "bn254":
                    dw = ctx.upload(w.reshape(1, 8))
                    launches.append(("blind_commitments", lambda dj, db: ctx.blind_commitments_device(cs.id, dj, db, n, dw.data_ptr())))
                for lname, launch in launches:
                    dj, db, aff = ctx.upload(jac), ctx.upload(stored), torch.empty((n, 8), dtype=torch.int64, device="cuda")
                    launch(dj.data_ptr(), db.data_ptr())
                    ctx.to_affine_device(cs.id, dj.data_ptr(), n, aff.data_ptr())
                    assert np.array_equal(ctx.download_tensor(aff), blind_truth[key]), (lname, n, name)
    finally:
        fb.release()
    if curve == "bn254":
        return
    g = co.synth_bases(cs.id, 128)
    u = NI.uniform_words(po, po.FIELDS[cs.scalar.name], 1, 820)
    want = np.stack([co.to_affine(cs.id, co.best_multiexp(cs.id, np.stack([cs.scalar.encode(1), u[0]]), np.stack([g[i], g[64 + i]]), 1)) for i in range(64)]).reshape(64, 8)
    for j in range(1, NI.max_lift(NI.to_ints(u)[0], r) + 1):
        d, out = ctx.upload(g), _poisoned((64, 8))
        ctx.generator_collapse_device(cs.id, d.data_ptr(), 128, NI.lift(u, j, r)[0], out.data_ptr())
        assert np.array_equal(ctx.download_tensor(out), want), ("generator_collapse", j)
    d, out = ctx.upload(g), _poisoned((64, 8))
    ctx.generator_collapse_device(cs.id, d.data_ptr(), 128, NI.to_words([r])[0], out.data_ptr())      # the challenge 0 stored as r: g[i] itself
    assert np.array_equal(ctx.download_tensor(out), g[:64])


# ================================================================================================================ GPU: coordinates lifted by p
def _coordinate_families(po, cs, bases, seed):
    """[(name, stored points, the canonical points)]: the residue-keeping families over the 2 n coordinates (a zero stored as p is no coordinate of a point)"""
    n = bases.shape[0]
    fams = NI.families(np.ascontiguousarray(bases).reshape(2 * n, 4), cs.base.p, edges=(128, 256), seed=seed)
    return [(name, s.reshape(n, 8), bases) for name, s, c in fams if name in ("all_max", "mix", "one@0", "one@%d" % (2 * n - 1), "one@127", "one@128")]


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", MSM_NS)
def test_coordinates_lifted_by_p(pkg, po, co, ctx, curve, n):
    """REDUCED: bases_register (host and device, tables and a single row), best_multiexp and fixed_base_create over points whose coordinates are lifted give
    the results over the canonical points; points_check reports status 1 on them; points_compress writes the canonical encoding"""
    lib = pkg.load_library()
    cs = pkg.fields.CURVES[curve]
    bases = co.synth_bases(cs.id, n)
    scalars = co.fill_scalars(cs.scalar.id, "uniform", n, 900 + n)
    want = co.to_affine(cs.id, co.best_multiexp(cs.id, scalars, bases, 1)).reshape(8)
    dcanon, enc_canon = ctx.upload(bases), _poisoned((n, 4))
    ctx.points_compress(cs.id, dcanon.data_ptr(), n, enc_canon.data_ptr())
    assert ctx.points_check(cs.id, dcanon.data_ptr(), n) == 0
    for name, stored, _ in _coordinate_families(po, cs, bases, 901 + n):
        for precompute in (True, False):
            reg = ctx.register_bases(cs.id, stored, 0, precompute)
            try:
                assert np.array_equal(ctx.to_affine(cs.id, ctx.msm(reg, scalars))[0], want), ("register, host", precompute, name)
            finally:
                reg.release()
            d, h = ctx.upload(stored), C.c_void_p()
            ctx._check(lib.dehalo_bases_register_device(ctx.handle, cs.id, C.c_void_p(d.data_ptr()), n, 0, int(precompute), C.byref(h)))
            reg = pkg.Bases(ctx, h, cs.id, n)
            try:
                assert np.array_equal(ctx.to_affine(cs.id, ctx.msm(reg, scalars))[0], want), ("register, device", precompute, name)
            finally:
                reg.release()
        assert np.array_equal(ctx.to_affine(cs.id, ctx.best_multiexp(cs.id, scalars, stored))[0], want), ("best_multiexp", name)
        d, enc = ctx.upload(stored), _poisoned((n, 4))
        assert ctx.points_check(cs.id, d.data_ptr(), n) == 1, name
        ctx.points_compress(cs.id, d.data_ptr(), n, enc.data_ptr())
        ctx.synchronize()
        assert np.array_equal(_np(enc), _np(enc_canon)), ("points_compress", name)
    # fixed_base_create of a point with lifted coordinates: the table of the canonical point
    s = NI.uniform_words(po, po.FIELDS[cs.scalar.name], 9, 950)
    pt = bases[n - 1]
    want_fb = np.stack([co.to_affine(cs.id, co.best_multiexp(cs.id, s[i:i + 1], pt.reshape(1, 8), 1)) for i in range(9)]).reshape(9, 8)
    for name, stored, _ in NI.families(pt.reshape(2, 4), cs.base.p, edges=(), singles=True)[:4]:
        fb = ctx.fixed_base(cs.id, stored.reshape(8))
        try:
            ds, out = ctx.upload(s), _poisoned((9, 8))
            fb.mul_device(ds.data_ptr(), 9, out.data_ptr())
            assert np.array_equal(ctx.download_tensor(out), want_fb), ("fixed_base_create", name)
        finally:
            fb.release()


# ================================================================================================================ GPU: bases given more than 64 bytes apart
@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", MSM_NS)
def test_strided_bases(pkg, po, co, ctx, curve, n):
    """rule 5: dehalo_bases_register with stride_bytes 72 and 96 -- the first 64 bytes of a slot are the point, the rest (here 0xA5 bytes, where a caller
    might keep a flag) is not read; identities at index 0 and n - 1 are (0, 0).  The MSM's point equals the stride-64 registration's bit for bit, and the C
    oracle's."""
    lib = pkg.load_library()
    cs = pkg.fields.CURVES[curve]
    bases = co.synth_bases(cs.id, n).copy()
    bases[0] = 0
    bases[n - 1] = 0
    scalars = co.fill_scalars(cs.scalar.id, "uniform", n, 1000 + n)
    want = co.to_affine(cs.id, co.best_multiexp(cs.id, scalars, bases, 1)).reshape(8)
    assert want.any() == (n > 2)
    for precompute in (1, 0):
        ref = ctx.register_bases(cs.id, bases, 0, bool(precompute))
        try:
            plain = ctx.msm(ref, scalars)
        finally:
            ref.release()
        assert np.array_equal(ctx.to_affine(cs.id, plain)[0], want), precompute
        for stride in (72, 96):
            slots = np.full((n, stride), 0xA5, dtype=np.uint8)
            slots[:, :64] = bases.view(np.uint8).reshape(n, 64)
            h = C.c_void_p()
            ctx._check(lib.dehalo_bases_register(ctx.handle, cs.id, slots.ctypes.data_as(C.POINTER(C.c_uint64)), n, stride, 0, precompute, C.byref(h)))
            reg = pkg.Bases(ctx, h, cs.id, n)
            try:
                got = ctx.msm(reg, scalars)
            finally:
                reg.release()
            # (an MSM may return any Jacobian representative of its point, dehalo.h: the comparison is of the affine words, bit for bit)
            assert np.array_equal(ctx.to_affine(cs.id, got)[0], ctx.to_affine(cs.id, plain)[0]) and np.array_equal(ctx.to_affine(cs.id, got)[0], want), (precompute, stride)
            assert (slots[:, 64:] == 0xA5).all()


# ================================================================================================================ GPU: the quotient kernels
QUOTIENT_FIELDS = ["bn254_fr", "pasta_fp"]
QUOTIENT_LOG = 8              # 256 rows: two blocks of the quotient kernels' 128 threads


class _Lifted:
    """uploads canonical integers as lifted words (every element by the largest multiple that fits, or the 0 / 1 / largest mix), a new draw per column"""

    def __init__(self, ctx, F, mode):
        self.ctx, self.F, self.pick, self.draws = ctx, F, {"all_max": 0, "mix": 1}[mode], 0

    def words(self, ints):
        self.draws += 1
        return NI.families(self.F.enc(list(ints)), self.F.p, seed=1000 + self.draws, singles=False)[self.pick][1]

    def up(self, ints):
        return self.ctx.upload(self.words(ints))

    def word(self, v):
        return NI.lift_word(self.F.enc1(v % self.F.p), self.F.p)


def _down(ctx, t):
    ctx.synchronize()
    return ctx.download_tensor(t)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["all_max", "mix"])
@pytest.mark.parametrize("fname", QUOTIENT_FIELDS)
def test_graph_evaluate(pkg, po, ctx, fname, mode):
    """REDUCED: graph_evaluate (one program a call, and the batch) over lifted fixed, advice and instance columns, lifted challenges, beta, gamma, theta and y and
    a lifted previous column: programs of 0, 1 and 7 constants, 1 and 12 LDS slots, and one that spills to HBM"""
    import quotient_inputs as QI
    from test_quotient_structured import BATCH_LOG, _Dev, _graph_ref, batch_env
    assert BATCH_LOG == QUOTIENT_LOG
    dev = _Dev(pkg, ctx, po, fname)
    F, rows = dev.F, 1 << QUOTIENT_LOG
    p = F.p
    env = batch_env(po, fname)
    progs = [(("batch", i), QI.batch_program(po, F, i)) for i in range(4)] + [(("batch", 3, "spill"), QI.batch_program(po, F, 3, spill=True))]
    L = _Lifted(ctx, F, mode)
    cols = {k: [L.up(c) for c in env[k]] for k in ("fixed", "advice", "instance")}
    ptrs = {k: [t.data_ptr() for t in v] for k, v in cols.items()}
    ch = np.stack([L.word(c) for c in env["challenges"]])
    sc = [L.word(env[k]) for k in ("beta", "gamma", "theta", "y")]
    cgs = [dev.compile(g) for _, g in progs]
    try:
        outs = dev.poisoned(rows, len(progs))
        ctx.graph_evaluate_batch_device([cg.handle.value for cg in cgs], ptrs["fixed"], ptrs["advice"], ptrs["instance"], ch, *sc, QUOTIENT_LOG, 2, [t.data_ptr() for t in outs])
        for (key, g), out in zip(progs, outs):
            reduced(_down(ctx, out), F.enc(_graph_ref(po, F, key, g, env, rows, 2)), p, ("batch",) + key)
        for (key, g), cg in zip(progs, cgs):
            out, = dev.poisoned(rows)
            ctx.graph_evaluate_device(cg.handle, ptrs["fixed"], ptrs["advice"], ptrs["instance"], ch, *sc, QUOTIENT_LOG, 2, 0, out.data_ptr())
            reduced(_down(ctx, out), F.enc(_graph_ref(po, F, key, g, env, rows, 2)), p, ("alone",) + key)
        # a program that adds PREVIOUS, the previous column lifted, out of place and in place
        g = QI.handwritten_programs(po, rows)["reads_previous"]
        henv = QI.uniform_env(po, F, rows, 1, 2, 1, 1, 0x3200)
        previous = QI.uniform(po, F, rows, 0x3201)
        want = F.enc(po.graph_evaluate(F.of, g, henv, rows, 2, previous))
        hcols = {k: [L.up(c) for c in henv[k]] for k in ("fixed", "advice", "instance")}
        cg = dev.compile(g)
        cgs.append(cg)
        prev, (out,) = L.up(previous), dev.poisoned(rows)
        args = ([t.data_ptr() for t in hcols["fixed"]], [t.data_ptr() for t in hcols["advice"]], [t.data_ptr() for t in hcols["instance"]],
                np.stack([L.word(c) for c in henv["challenges"]]), *[L.word(henv[k]) for k in ("beta", "gamma", "theta", "y")], QUOTIENT_LOG, 2)
        ctx.graph_evaluate_device(cg.handle, *args, prev.data_ptr(), out.data_ptr())
        reduced(_down(ctx, out), want, p, "previous, out of place")
        ctx.graph_evaluate_device(cg.handle, *args, prev.data_ptr(), prev.data_ptr())
        reduced(_down(ctx, prev), want, p, "previous, in place")
    finally:
        for cg in cgs:
            cg.release()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["all_max", "mix"])
@pytest.mark.parametrize("fname", QUOTIENT_FIELDS)
def test_permutation_lookup_and_shuffle_h(pkg, po, ctx, fname, mode):
    """REDUCED: the permutation, lookup (one and eight a launch) and shuffle terms of h over lifted columns, Lagrange columns, running values and challenges"""
    import quotient_inputs as QI
    from test_shuffle import _shuffle_families, _shuffle_reference
    F = SI.field(po, fname)
    p, rows, spec = F.p, 1 << QUOTIENT_LOG, pkg.fields.FIELDS[fname]
    L = _Lifted(ctx, F, mode)
    # permutation: seven columns in four sets, uniform and drawn from the edge values (zeros among them: lifted, they are multiples of p)
    shape, sc = (7, 2, 4), QI.perm_scalars(po, F, QUOTIENT_LOG)
    inputs = [("uniform", QI.perm_uniform(po, F, rows, shape, 0x4000 + QUOTIENT_LOG))] + [(n, QI.perm_families(po, F, QUOTIENT_LOG, shape, sc)[n][0]) for n in ("edge_columns", "satisfied")]
    for name, d in inputs:
        for rs, lr in ((1, -6), (4, -1)):
            want = F.enc(QI.perm_reference(po, F, d, shape, lr, sc, rs))
            keep = {k: [L.up(c) for c in d[k]] for k in ("z", "cols", "sigma")}
            lag = [L.up(d[k]) for k in ("l0", "l_last", "l_active")]
            values = L.up(d["values"])
            ctx.permutation_h_device(spec.id, [t.data_ptr() for t in keep["z"]], [t.data_ptr() for t in keep["cols"]], [t.data_ptr() for t in keep["sigma"]], shape[1], lr,
                                     lag[0].data_ptr(), lag[1].data_ptr(), lag[2].data_ptr(), L.word(sc["beta"]), L.word(sc["gamma"]), L.word(sc["y"]), L.word(sc["delta"]),
                                     L.word(sc["beta"] * sc["zeta"]), L.word(sc["omega"]), QUOTIENT_LOG, rs, values.data_ptr())
            reduced(_down(ctx, values), want, p, ("permutation_h", name, rs, lr))
    # lookups
    lsc = QI.lookup_scalars(po, F)
    fams, lags = QI.lookup_families(po, F, QUOTIENT_LOG, lsc), QI.lookup_lagrange(po, F, QUOTIENT_LOG)
    lw = [L.word(lsc[k]) for k in ("beta", "gamma", "y")]
    for ln in ("uniform", "edges"):
        lag = lags[ln]
        dl = [L.up(c) for c in lag[:3]]
        df = [{k: L.up(h[k]) for k in ("z", "a", "s", "tv")} for _, h, _ in fams]
        chained = lag[3]
        for (name, h, _), t in zip(fams, df):
            values = L.up(lag[3])
            ctx.lookup_h_device(spec.id, t["z"].data_ptr(), t["a"].data_ptr(), t["s"].data_ptr(), t["tv"].data_ptr(), dl[0].data_ptr(), dl[1].data_ptr(), dl[2].data_ptr(),
                                *lw, QUOTIENT_LOG, 4, values.data_ptr())
            reduced(_down(ctx, values), F.enc(QI.lookup_reference(po, F, lag[3], h, lag, lsc, 4)), p, ("lookup_h", name, ln))
            chained = QI.lookup_reference(po, F, chained, h, lag, lsc, 1)
        values = L.up(lag[3])
        ctx.lookup_h_batch_device(spec.id, [(t["z"].data_ptr(), t["a"].data_ptr(), t["s"].data_ptr(), t["tv"].data_ptr()) for t in df], dl[0].data_ptr(), dl[1].data_ptr(),
                                  dl[2].data_ptr(), *lw, QUOTIENT_LOG, 1, values.data_ptr())
        reduced(_down(ctx, values), F.enc(chained), p, ("lookup_h_batch", ln))
        # shuffles, eight a launch
        sfams = _shuffle_families(po, F, QUOTIENT_LOG)[:8]
        y = QI.uniform(po, F, 1, 0x5F1)[0]
        ds = [tuple(L.up(c) for c in f) for f in sfams]
        for rs in (1, 4):
            values = L.up(lag[3])
            ctx.shuffle_h_batch_device(spec.id, [tuple(t.data_ptr() for t in f) for f in ds], dl[0].data_ptr(), dl[1].data_ptr(), dl[2].data_ptr(), L.word(y), QUOTIENT_LOG, rs,
                                       values.data_ptr())
            reduced(_down(ctx, values), F.enc(_shuffle_reference(p, lag[3], sfams, lag[:3], y, rs)), p, ("shuffle_h", ln, rs))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["all_max", "mix"])
@pytest.mark.parametrize("fname", QUOTIENT_FIELDS)
def test_product_terms_and_their_products(pkg, po, ctx, fname, mode):
    """REDUCED: product_terms over lifted columns, permutations, powers of omega and challenges, at rows where a numerator's or a denominator's factor is zero
    mod p; and the grand products of those very terms (grand_product_batch), whose denominators that are zero invert to zero"""
    import quotient_inputs as QI
    from dehalo2_amd.keygen import delta_of
    F, spec = SI.field(po, fname), pkg.fields.FIELDS[fname]
    p = F.p
    L = _Lifted(ctx, F, mode)
    for n in (129, 1000):
        d = QI.product_inputs(po, F, n, "both", delta_of(spec))
        want_num, want_den = QI.product_reference(F, d, n)
        assert any(0 in w for w in want_num) and any(0 in w for w in want_den)
        ncols, chunk, nl = QI.PRODUCT_MODES["both"]
        sets = (ncols + chunk - 1) // chunk
        dc, ds, dom = [L.up(c) for c in d["cols"]], [L.up(c) for c in d["sigma"]], L.up(d["omega_powers"])
        dlk = [[L.up(c) for c in four] for four in d["lookups"]]
        num, den = _poisoned((sets + nl, n, 4)), _poisoned((sets + nl, n, 4))
        factors = L.words([d["beta"] * pow(d["delta"], chunk * s, p) % p for s in range(sets)])
        ctx.product_terms_device(spec.id, [t.data_ptr() for t in dc], [t.data_ptr() for t in ds], chunk, dom.data_ptr(), L.word(d["beta"]), L.word(d["gamma"]), L.word(d["delta"]),
                                 factors, [tuple(t.data_ptr() for t in four) for four in dlk], n, num.data_ptr(), den.data_ptr(), n)
        got_n, got_d = _down(ctx, num), _down(ctx, den)
        for q in range(sets + nl):
            reduced(got_n[q], F.enc(want_num[q]), p, ("product_terms, numerator", n, q))
            reduced(got_d[q], F.enc(want_den[q]), p, ("product_terms, denominator", n, q))
        z = _poisoned((sets + nl, n, 4))
        ctx.grand_product_batch_device(spec.id, num.data_ptr(), den.data_ptr(), n, sets + nl, n, z.data_ptr())
        got_z = _down(ctx, z)
        for q in range(sets + nl):
            acc, want = 1, []
            for a, b in zip(want_num[q], want_den[q]):
                want.append(acc)
                acc = acc * a % p * (pow(b, -1, p) if b else 0) % p
            reduced(got_z[q], F.enc(want), p, ("grand product of the terms", n, q))


# ================================================================================================================ GPU: the witness check, a whole proof
def _lift_columns(cols, p, pick):
    """(columns, n, 4) words -> the same lifted, family `pick` (0: every element by the largest multiple, 1: the mix)"""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    return NI.families(cols.reshape(-1, 4), p, seed=77, singles=False)[pick][1].reshape(cols.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["mont", "device", "canonical"])
def test_check_witness(pkg, co, ctx, form):
    """rule 1 for the witness check in the three forms it takes advice in (host Montgomery, device Montgomery, host plain integers): lifted advice reports what
    the canonical advice reports -- nothing on a satisfied circuit (the copied cell and its copy lifted by different multiples; lookup inputs and table keys
    lifted), the same two gate rows on a broken one, the same lookup rows on a value that is not in the table"""
    import test_check_witness as CW
    from dehalo2_amd import native
    p = pkg.fields.BN254_FR.p
    fid = pkg.fields.BN254_FR.id
    params = native.ParamsKZG.setup(ctx, pkg.fields.BN254, 6, CW.S_SETUP)
    try:
        cases = []
        cs, fixed, advice, asm = CW.build_circuit(pkg, "R7", 6)
        cases.append(("R7", cs, fixed, advice, asm, ()))
        bad = advice.copy()
        bad[1, CW.Q_LO + 9] = (5, 0, 0, 0)
        cases.append(("R7 broken", cs, fixed, bad, asm, ()))
        cs0, fixed0, advice0, asm0 = CW.case_zero_as_p(pkg, p, 0)
        cases.append(("zero residual", cs0, fixed0, advice0, asm0, ()))
        cs5, fixed5, advice5, asm5 = CW.build_circuit(pkg, "R5", 6)
        bad = advice5.copy()
        bad[1, 40, 0] += np.uint64(1)
        cases.append(("R5 copy broken", cs5, fixed5, bad, asm5, ()))
        for name, kw in CW.LOOKUP_CASES.items():
            cases.append(("lookup " + name,) + CW.lookup_circuit(pkg, 6, **kw(6)) + ((),))
        seen = set()
        for name, cs, fixed, advice, asm, sels in cases:
            fails, counters = CW.enumerate_failures(cs, 6, p, fixed, advice, asm.mapping)
            seen.add(bool(fails))
            pk = native.ProvingKey.keygen(ctx, params, cs, fixed, asm, sels)
            try:
                adv = advice if form == "canonical" else np.stack([co.field_op(fid, "to_mont", advice[i]) for i in range(advice.shape[0])])
                for pick in (0, 1):
                    lifted = _lift_columns(adv, p, pick)
                    assert np.array_equal(NI.canon(lifted.reshape(-1, 4), p), adv.reshape(-1, 4)) and not np.array_equal(lifted, adv)
                    given = ctx.upload(lifted) if form == "device" else lifted
                    rep = pk.check_witness(given, [[]] * cs.num_instance, assembly=asm, canonical=form == "canonical", cap=64)
                    CW.same_report(rep, fails, counters)
            finally:
                pk.release()
        assert seen == {True, False}
    finally:
        params.release()


@pytest.fixture(scope="module")
def r7_chain(pkg, po, co):
    """tests/proof_chains.py's KZG chain of test_rotations' R7 circuit at k = 6, with the restatement's proof over the canonical witness"""
    import proof_chains as PC
    from test_rotations import build_circuit
    cs, fixed, advice, asm = build_circuit(pkg, "R7", 6)
    c = dict(PC.kzg_chain(po, co, cs.description(), 6, fixed, asm.mapping, advice), cs=cs, fixed=fixed, asm=asm)
    c["want"] = PC.prove(po, c, [])[0]
    return c


@pytest.mark.gpu
def test_a_whole_proof_over_a_lifted_witness(pkg, po, ctx, r7_chain):
    """one k = 6 proof whose advice columns are lifted: byte for byte the proof over the canonical witness (the circuit has no instance column)"""
    import pairing as pr
    from dehalo2_amd import native, prover
    c = r7_chain
    p = pkg.fields.BN254_FR.p
    params = native.ParamsKZG.create(ctx, pkg.fields.BN254, 6, c["srs"]["g"], c["srs"]["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(c["s_g2"]))
    pk = native.ProvingKey.keygen(ctx, params, c["cs"], c["fixed"], c["asm"], ())
    pk.transcript_repr = c["rep"]
    P = native.Prover(params, pk)
    try:
        assert P.create_proof(c["adv"], [], prover.SeededRng(7)).finalize() == c["want"]
        for pick in (0, 1):
            lifted = _lift_columns(c["adv"], p, pick)
            assert not NI.all_below(lifted.reshape(-1, 4), p)
            proof = P.create_proof(lifted, [], prover.SeededRng(7)).finalize()
            diff = [i // 32 for i in range(0, len(c["want"]), 32) if proof[i:i + 32] != c["want"][i:i + 32]]
            assert len(proof) == len(c["want"]) and not diff, "proof items differ from the proof over the canonical witness: %r" % diff[:8]
    finally:
        P.release(); pk.release(); params.release()


# ================================================================================================================ GPU: instance columns
# The instance values are the one place where HOST code reads a caller's word: the KZG prover hashes every value into the transcript (common_scalar), the
# IPA prover commits to the column; both also copy the words to the device for the quotient.
def _instance_families(f, inst):
    """[(name, stored instance words)] standing for the canonical ints `inst`: every value lifted by the largest multiple that fits, the 0 / 1 / largest mix,
    one value lifted by one p"""
    words = f.encode_many(inst)
    fams = NI.families(words, f.p, edges=(), seed=5, singles=False)[:2]
    one = words.copy()
    one[len(inst) - 1] = NI.lift(words[-1:], 1, f.p)[0]
    out = [(name, s) for name, s, _ in fams] + [("last by p", one)]
    for name, s in out:
        assert np.array_equal(NI.canon(s, f.p), words) and not np.array_equal(s, words), name
    return out


@pytest.fixture(scope="module")
def instance_chains(pkg, po, co):
    """scheme -> (chain, cs, fixed, assembly, instance values, the restatement's proofs over the canonical witness: of `inst` and of `inst` with a zero
    appended) for tests/test_ipa_proof.py's one-instance-column circuit at k = 6"""
    import proof_chains as PC
    from test_ipa_proof import _instance_circuit
    cs, desc, inst, fixed, advice, asm = _instance_circuit(pkg, po, 6)
    out = {}
    for scheme, make in (("kzg", PC.kzg_chain), ("ipa", PC.ipa_chain)):
        c = make(po, co, desc, 6, fixed, asm.mapping, advice)
        out[scheme] = (c, cs, fixed, asm, inst, PC.prove(po, c, [inst])[0], PC.prove(po, c, [inst + [0]])[0])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["kzg", "ipa"])
def test_a_whole_proof_over_lifted_advice_and_instances(pkg, po, ctx, instance_chains, scheme):
    """a k = 6 proof of a circuit with an instance column, advice AND instance values lifted: byte for byte the proof over the canonical witness and the
    canonical instances -- under KZG (the instance values are hashed as scalars) and under IPA (the instance column is committed); an instance value 0
    appended as the word p is the value 0 appended"""
    import pairing as pr
    from dehalo2_amd import native, prover
    c, cs, fixed, asm, inst, want, want_zero = instance_chains[scheme]
    if scheme == "kzg":
        curve = pkg.fields.BN254
        params = native.ParamsKZG.create(ctx, curve, 6, c["srs"]["g"], c["srs"]["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(c["s_g2"]))
    else:
        curve = pkg.fields.VESTA
        params = native.ParamsIPA.create(ctx, curve, 6, c["srs"]["g"], c["srs"]["g_lagrange"], c["w"], c["u"])
    f = curve.scalar
    pk = native.ProvingKey.keygen(ctx, params, cs, fixed, asm, ())
    pk.transcript_repr = c["rep"]
    P = native.Prover(params, pk)

    def same(proof, expected, label):
        diff = [i // 32 for i in range(0, len(expected), 32) if proof[i:i + 32] != expected[i:i + 32]]
        assert len(proof) == len(expected) and not diff, "%r: proof items differ from the proof over the canonical witness and instances: %r" % (label, diff[:8])

    try:
        same(P.create_proof(c["adv"], [inst], prover.SeededRng(7)).finalize(), want, "canonical")
        same(P.create_proof(c["adv"], [f.encode_many(inst)], prover.SeededRng(7)).finalize(), want, "canonical, given as words")
        for name, words in _instance_families(f, inst):
            for pick in (0, 1):
                same(P.create_proof(_lift_columns(c["adv"], f.p, pick), [words], prover.SeededRng(7)).finalize(), want, (name, pick))
            same(P.create_proof(c["adv"], [words], prover.SeededRng(7)).finalize(), want, (name, "advice canonical"))
            with_zero = np.concatenate([words, NI.to_words([f.p])])
            same(P.create_proof(c["adv"], [with_zero], prover.SeededRng(7)).finalize(), want_zero, (name, "0 appended as p"))
        assert want_zero != want or scheme == "ipa"
    finally:
        P.release(); pk.release(); params.release()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["mont", "device", "canonical"])
def test_check_witness_with_lifted_instances(pkg, po, co, ctx, form):
    """the witness check of the same circuit (gate q (a - instance) = 0 on four rows), advice and instance values lifted: nothing to report for the right
    instances, gate 0 at row 2 for a wrong third value -- what the canonical words report"""
    import test_check_witness as CW
    from dehalo2_amd import native
    from test_ipa_proof import _instance_circuit
    f = pkg.fields.BN254_FR
    cs, desc, inst, fixed, advice, asm = _instance_circuit(pkg, po, 6)
    usable = 64 - (cs.blinding_factors() + 1)
    counters = {"rows": usable, "lookup_inputs": 0, "cells_in_cycles": 0}
    params = native.ParamsKZG.setup(ctx, pkg.fields.BN254, 6, CW.S_SETUP)
    pk = native.ProvingKey.keygen(ctx, params, cs, fixed, asm, ())
    try:
        adv = advice if form == "canonical" else np.stack([co.field_op(f.id, "to_mont", advice[i]) for i in range(advice.shape[0])])
        for values, fails in ((inst, []), (inst[:2] + [inst[2] + 1] + inst[3:], [(CW.GATE, 0, 2)])):
            CW.same_report(pk.check_witness(adv, [values], assembly=asm, canonical=form == "canonical", cap=64), fails, counters)
            for name, words in _instance_families(f, values):
                for pick in (0, 1):
                    lifted = _lift_columns(adv, f.p, pick)
                    given = ctx.upload(lifted) if form == "device" else lifted
                    CW.same_report(pk.check_witness(given, [words], assembly=asm, canonical=form == "canonical", cap=64), fails, counters)
    finally:
        pk.release(); params.release()
