"""Exceptional group-law paths of the MSM at scale: bases that are equal, opposite, identities, window multiples of each other
or small multiples of one point, under scalars that make bucket sums, partial sums, tree nodes and window sums collide.

The kernels add with incomplete XYZZ formulas and resolve identity operands, P + P and P + (-P) after the fact (ec29.cuh); the generic
points of co.synth_bases never reach those branches.  Every result here is compared, bit for bit after to_affine, with TWO references:

  closed form   every base is a known multiple k_i of the generator G, so MSM(s, P) = [sum s_i k_i mod r] G -- one double-and-add
                in Python integers (po.ec_mul): no Pippenger, no buckets, no Montgomery form;
  C oracle      co.best_multiexp, the C restatement of upstream, on the very same arrays.

The CPU tests (no gpu mark) pin the two references against each other over every base and scalar family on all three curves, and pin
the k_i against the arrays (co.fixed_base_mul(k_i) == bases); the GPU tests then hold the library to both.  -P is made by negating y
in Montgomery form, [m]P by the oracle -- never by the library under test."""
import numpy as np
import pytest

from conftest import enc_points

CURVES = ["bn254", "pallas", "vesta"]
KSTEP = 0x9E3779B97F4A7C15          # co.synth_bases: P_i = (1 + i * KSTEP) G   (oracle/pyoracle.py synth_bases)
ID_RUN = 1500                       # a contiguous run of identities longer than a sort block (msm_sort_block <= 1024 threads)

BASE_FAMILIES = ["generic", "same", "dup_adj", "pairs_adj", "pairs_shift1", "pairs_split", "generic+id7", "generic+id_ends", "generic+id_run",
                 "pairs_adj+id7", "pairs_adj+id_ends", "pairs_split+id_run", "small", "chain", "chain_alt"]
SCALAR_FAMILIES = ["uniform", "ladder", "ladder_even", "ladder_top", "ladder_one", "pair_equal_few", "pair_equal_uniform", "negdup", "chain_equal", "repeats"]
REPEAT_MULTS = [6000, 2500, 1200, 700, 300, 200, 90, 60, 33, 17, 9, 5, 3, 2, 1, 1] + [130] * 20 + [40] * 100 + [7] * 200      # 1 .. 6000 points per bucket (19121 points)


def _ints(limbs):
    """n x 4 u64 (plain little-endian limbs) -> Python integers"""
    b = np.ascontiguousarray(limbs, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def chain_run(c):
    """Run length of the window chain: the windows of a c-bit registration, shortened so that d * 2^(c (run - 1)) with d < 2^(c-1) stays below 2^252 < r."""
    return min((256 + c - 1) // c, (252 - (c - 1)) // c + 1) & ~1      # (even: a run of alternating signs cancels)


class Lab:
    """Builders of the degenerate inputs and of the two references.  Everything is seeded and deterministic."""

    def __init__(self, pkg, po, co):
        self.pkg, self.po, self.co = pkg, po, co
        self._gen, self._bases, self._refs = {}, {}, {}

    def spec(self, cname):
        return self.pkg.fields.CURVES[cname]

    # ---- bases: (n x 8 u64 affine Montgomery, [k_i]) ----
    def generic(self, cname, n):
        got = self._gen.get(cname)
        if got is None or got[0].shape[0] < n:
            spec = self.spec(cname)
            got = self._gen[cname] = (self.co.synth_bases(spec.id, n), [(1 + i * KSTEP) % spec.scalar.p for i in range(n)])
        return got[0][:n].copy(), got[1][:n]

    def neg(self, cname, pts):
        """-P: y -> p - y on the Montgomery limbs (the identity (0, 0) stays itself)"""
        spec = self.spec(cname)
        out = np.array(pts, dtype=np.uint64).reshape(-1, 8)
        out[:, 4:] = self.co.field_op(spec.base.id, "sub", np.zeros((out.shape[0], 4), np.uint64), np.ascontiguousarray(out[:, 4:]))
        return out

    def multiples(self, cname, ks):
        """[k] G from the oracle"""
        spec = self.spec(cname)
        return self.co.fixed_base_mul(spec.id, spec.scalar.encode_many(ks), 8)

    def bases(self, cname, fam, n, c=13):
        key = (cname, fam, n, c if fam.startswith("chain") else 0)
        if key not in self._bases:
            self._bases[key] = self._build_bases(cname, fam, n, c)
        return self._bases[key]

    def _build_bases(self, cname, fam, n, c):
        r = self.spec(cname).scalar.p
        fam, _, ident = fam.partition("+")
        h = n // 2
        if fam == "generic":
            pts, ks = self.generic(cname, n)
        elif fam == "same":                              # A: n copies of one point
            g, k = self.generic(cname, 3)
            pts, ks = np.tile(g[2], (n, 1)), [k[2]] * n
        elif fam == "dup_adj":                           # P_0, P_0, P_1, P_1, ...
            g, k = self.generic(cname, (n + 1) // 2)
            pts, ks = np.repeat(g, 2, axis=0)[:n], [k[i // 2] for i in range(n)]
        elif fam in ("pairs_adj", "pairs_shift1"):       # B: P_i, -P_i adjacent; shift1: one unpaired point in front, so pairs sit at odd offsets
            s = 1 if fam == "pairs_shift1" else 0
            g, k = self.generic(cname, n // 2 + 2)
            q, kq = g[s:], k[s:]
            pts = np.empty((2 * len(q), 8), np.uint64)
            pts[0::2], pts[1::2] = q, self.neg(cname, q)
            ks = [kq[i // 2] if i % 2 == 0 else r - kq[i // 2] for i in range(2 * len(q))]
            if s:
                pts, ks = np.concatenate([g[:1], pts]), [k[0]] + ks
            pts, ks = pts[:n].copy(), ks[:n]
        elif fam == "pairs_split":                       # B: P_i at i, -P_i at i + n/2 (another sort slice); an odd n leaves the last point unpaired
            g, k = self.generic(cname, n - h)
            pts = np.concatenate([g[:h], self.neg(cname, g[:h]), g[h:]])
            ks = k[:h] + [r - x for x in k[:h]] + k[h:]
        elif fam == "small":                             # E: {1..16} P up, then {1..16} (-P): bucket sums and running sums collide constantly
            g, k = self.generic(cname, 6)
            m = self.multiples(cname, [(j + 1) * k[5] % r for j in range(16)])
            cyc = np.concatenate([m, self.neg(cname, m)])
            kc = [(j + 1) * k[5] % r for j in range(16)] + [r - (j + 1) * k[5] % r for j in range(16)]
            pts, ks = np.tile(cyc, ((n + 31) // 32, 1))[:n].copy(), [kc[i % 32] for i in range(n)]
        elif fam in ("chain", "chain_alt"):              # D: P_j = [2^c] P_{j-1} in runs; chain_alt negates every second point of a run
            run = chain_run(c)
            _, k = self.generic(cname, (n + run - 1) // run)
            ks = [k[i // run] * pow(2, c * (i % run), r) % r for i in range(n)]
            pts = self.multiples(cname, ks)
            if fam == "chain_alt":
                odd = np.arange(n) % run % 2 == 1
                pts[odd] = self.neg(cname, pts[odd])
                ks = [r - x if o else x for x, o in zip(ks, odd)]
        else:
            raise KeyError(fam)
        if ident:                                        # C: identities (0, 0)
            mask = np.zeros(n, bool)
            if ident == "id7":
                mask[6::7] = True
            elif ident == "id_ends":
                mask[[0, n - 1]] = True
            elif ident == "id_run":
                lo = min(n // 5, max(0, n - ID_RUN))
                mask[lo:lo + ID_RUN] = True
            else:
                raise KeyError(ident)
            pts[mask] = 0
            ks = [0 if z else x for x, z in zip(ks, mask)]
        assert pts.shape == (n, 8) and len(ks) == n
        return np.ascontiguousarray(pts), ks

    @staticmethod
    def pair_id(bfam, n):
        """index of the pair a base belongs to, so that 'equal scalars on a pair' follows the layout of the base family"""
        fam = bfam.partition("+")[0]
        i = np.arange(n)
        if fam == "pairs_shift1":
            return (i + 1) // 2
        if fam == "pairs_split":
            return np.where(i < 2 * (n // 2), i % max(1, n // 2), i)
        return i // 2

    # ---- scalars: n x 4 u64 Montgomery ----
    def small_scalars(self, cname, vals):
        spec = self.spec(cname)
        vals = np.asarray(vals, dtype=np.int64)
        uniq = np.unique(vals)
        return spec.scalar.encode_many([int(v) for v in uniq])[np.searchsorted(uniq, vals)]

    def scalars(self, cname, sfam, bfam, n, c=13, seed=1):
        spec, co = self.spec(cname), self.co
        fid, nb, i = spec.scalar.id, 1 << (c - 1), np.arange(n)
        pid = self.pair_id(bfam, n)
        if sfam == "uniform":
            return co.fill_scalars(fid, "uniform", n, 9000 + seed)
        if sfam == "ladder":           # one non-zero digit, every bucket the same number of points
            return self.small_scalars(cname, i % nb + 1)
        if sfam == "ladder_even":      # every second bucket
            return self.small_scalars(cname, 2 * (i % (nb // 2)) + 2)
        if sfam == "ladder_top":       # the upper half of the buckets
            return self.small_scalars(cname, nb // 2 + 1 + i % (nb // 2))
        if sfam == "ladder_one":       # a single bucket
            return self.small_scalars(cname, np.full(n, nb // 3 + 1))
        if sfam == "pair_equal_few":   # equal scalars on a pair, five buckets in all: long chains of P, -P in one bucket
            return self.small_scalars(cname, 1 + pid % 5)
        if sfam == "pair_equal_uniform":
            return co.fill_scalars(fid, "uniform", int(pid.max()) + 1, 9100 + seed)[pid]
        if sfam == "negdup":           # s and r - s on the two members of a pair: the signed digits negate
            u = co.fill_scalars(fid, "uniform", int(pid.max()) + 1, 9200 + seed)[pid]
            odd = i % 2 == 1
            u[odd] = co.field_op(fid, "sub", np.zeros((int(odd.sum()), 4), np.uint64), np.ascontiguousarray(u[odd]))
            return u
        if sfam == "chain_equal":      # position t of a run gets d * 2^(c (run - 1 - t)): every member of a run contributes the SAME point [d 2^(c (run-1))] P_run
            run = chain_run(c)
            vals = [(1 + (j // run) % max(1, nb // 2 - 1)) << (c * (run - 1 - j % run)) for j in range(n)]
            return spec.scalar.encode_many(vals)
        if sfam == "repeats":          # 1 .. 6000 points per bucket, contiguous (pairs stay together), the rest of the column zero
            vals, pos = np.zeros(n, np.int64), 0
            for j, m in enumerate(REPEAT_MULTS):
                m = min(m, n - pos)
                vals[pos:pos + m] = 3 + j
                pos += m
            return self.small_scalars(cname, vals)
        raise KeyError(sfam)

    # ---- the two references, as affine rows (8 u64, identity = zeros) ----
    def closed_form(self, cname, ks, scalars):
        spec, po = self.spec(cname), self.po
        s = _ints(self.co.field_op(spec.scalar.id, "from_mont", scalars))
        assert len(s) == len(ks)
        total = sum(a * b for a, b in zip(s, ks)) % spec.scalar.p
        cv = po.CURVES[cname]
        return enc_points(spec.base, [po.ec_mul(cv, total, (cv.gx, cv.gy)) if total else None])[0]

    def oracle(self, cname, bases, scalars):
        spec = self.spec(cname)
        return self.co.to_affine(spec.id, self.co.best_multiexp(spec.id, scalars, bases, 16))

    def case(self, cname, bfam, sfam, n, c=13):
        """(bases, k_i, scalars, closed form, C oracle), cached: the references do not depend on how the library is configured"""
        key = (cname, bfam, sfam, n, c if (bfam.startswith("chain") or sfam.startswith(("ladder", "chain", "repeats"))) else 0)
        if key not in self._refs:
            bases, ks = self.bases(cname, bfam, n, c)
            sc = self.scalars(cname, sfam, bfam, n, c)
            self._refs[key] = (bases, ks, sc, self.closed_form(cname, ks, sc), self.oracle(cname, bases, sc))
        return self._refs[key]


@pytest.fixture(scope="module")
def lab(pkg, po, co):
    return Lab(pkg, po, co)


# ================================================================ CPU: reference against reference
@pytest.mark.parametrize("cname", CURVES)
def test_base_families_are_the_multiples_they_claim(lab, cname):
    """The arrays (built by tiling, by negating y, by zeroing) against [k_i] G from the oracle's fixed-base multiplication: the closed form rests on these k_i."""
    for n, c in ((2 * ID_RUN + 77, 13), (640, 4)):
        for bfam in BASE_FAMILIES:
            bases, ks = lab.bases(cname, bfam, n, c)
            assert np.array_equal(bases, lab.multiples(cname, ks)), (cname, bfam, n)
    b, ks = lab.bases(cname, "pairs_adj+id7", 70)
    r = lab.spec(cname).scalar.p
    assert ks[6] == 0 and not b[6].any() and (ks[0] + ks[1]) % r == 0 and np.array_equal(b[0, :4], b[1, :4]) and not np.array_equal(b[0, 4:], b[1, 4:])
    b, ks = lab.bases(cname, "chain", 40, 8)
    assert chain_run(8) == 30 and ks[1] == ks[0] * 256 % r and ks[30] == 1 + KSTEP
    assert [chain_run(c) for c in (4, 13, 16, 17)] == [62, 18, 14, 14]


@pytest.mark.parametrize("cname", CURVES)
def test_closed_form_equals_c_oracle_on_every_family(lab, cname):
    """Every base family under every scalar family (and three window widths for the families that depend on one): [sum s_i k_i] G in Python integers
    equals the C restatement of best_multiexp.  The GPU tests below never rest on an oracle that is itself wrong at these edges."""
    n, checked = 4096 + 37, 0
    for bfam in BASE_FAMILIES:
        for sfam in SCALAR_FAMILIES:
            for c in ((4, 8, 13) if (bfam.startswith("chain") or sfam.startswith(("ladder", "chain"))) else (13,)):
                _, _, _, closed, orc = lab.case(cname, bfam, sfam, n, c)
                assert np.array_equal(closed, orc), (cname, bfam, sfam, c)
                checked += 1
    assert checked >= len(BASE_FAMILIES) * len(SCALAR_FAMILIES)


@pytest.mark.parametrize("cname", CURVES)
def test_closed_form_equals_c_oracle_at_2_15(lab, cname):
    n = 1 << 15
    for bfam, sfam, c in (("generic", "uniform", 13), ("same", "ladder", 13), ("pairs_adj+id7", "uniform", 13), ("pairs_adj+id7", "pair_equal_uniform", 13),
                          ("pairs_adj", "ladder", 13), ("pairs_split+id_run", "pair_equal_few", 13), ("small", "repeats", 16), ("chain_alt", "chain_equal", 16)):
        _, _, _, closed, orc = lab.case(cname, bfam, sfam, n, c)
        assert np.array_equal(closed, orc), (cname, bfam, sfam)


def test_cancelling_cases_cancel(lab):
    """The cases the GPU tests use as 'whole column is the identity' really are, by the closed form (which never adds a point)."""
    for bfam, sfam in (("pairs_adj", "pair_equal_few"), ("pairs_adj", "pair_equal_uniform"), ("pairs_split", "pair_equal_few"), ("pairs_split", "pair_equal_uniform"),
                       ("same", "negdup"), ("dup_adj", "negdup"), ("pairs_adj", "ladder_one"), ("pairs_split", "ladder_one"), ("chain_alt", "chain_equal")):
        for n, c in ((1 << 11, 8), (1 << 14, 13)):
            assert not lab.case("pallas", bfam, sfam, n, c)[3].any(), (bfam, sfam, n)
    assert lab.case("pallas", "pairs_shift1", "pair_equal_few", 1 << 11)[3].any()      # the unpaired point in front survives


# ================================================================ GPU
class _Tuning:
    """Launch-geometry knobs for one block of a test; the defaults come back in a finally (ctx is session-scoped)."""
    DEFAULTS = {"msm_sort_block": 1024, "msm_acc_block": 128, "msm_acc_points": 48}

    def __init__(self, ctx, **knobs):
        self.ctx, self.knobs = ctx, knobs

    def __enter__(self):
        for k, v in self.knobs.items():
            self.ctx.set_tuning(k, v)

    def __exit__(self, *exc):
        for k in self.knobs:
            self.ctx.set_tuning(k, self.DEFAULTS[k])


def _check(got, case, what):
    closed, orc = case[3], case[4]
    assert np.array_equal(got, closed), ("closed form", what)
    assert np.array_equal(got, orc), ("C oracle", what)


# (base family, scalar family): chosen so that every resolver meets an identity made by a cancellation, P == Q and P == -Q --
#   accumulation (x29_add_mixed): same / dup / small under any column (P + P on the first addition of a chain), pairs under equal scalars (P + (-P), then the
#     identity accumulator takes the next point), negdup (the digits negate the SAME table entry);
#   merge and reduction tree (x29q_add_mem, x29q_double_mem): ladders over `same` (X + X at every node of every level), over pairs (X + (-X) at the leaves, identities
#     above), even / top-half / single-bucket ladders (A_t = X_hi copies of identities and of equal sums), small (multiples that collide here and there);
#   window sums (k_msm_final: x29_add_quad, x29_double_quad, x29_add behind them; single-row tables): chain / chain_alt under chain_equal -- every window's weighted
#     sum is the same point, or its negative.
# (An identity operand that is NOT all-zero limbs -- ZZ = p -- cannot be fed to x29_add, x29_add_quad or x29q_add_mem from here: every resolver answers a cancellation with
#  the all-zero record and the entry points test z = 0 exactly.  Only x29_add_mixed meets its identity branch, through the all-zero accumulator, which has no early exit.)
COMBOS = [("same", "uniform"), ("same", "negdup"), ("dup_adj", "negdup"), ("pairs_adj", "pair_equal_few"), ("pairs_shift1", "pair_equal_few"),
          ("pairs_split", "pair_equal_uniform"), ("pairs_adj+id7", "uniform"), ("pairs_adj+id7", "pair_equal_uniform"), ("pairs_split+id_run", "pair_equal_few"),
          ("generic+id_ends", "uniform"), ("generic+id_run", "ladder"), ("generic+id7", "ladder_top"), ("small", "uniform"), ("small", "pair_equal_few"), ("small", "ladder"),
          ("same", "ladder"), ("same", "ladder_top"), ("same", "ladder_even"), ("same", "ladder_one"), ("pairs_adj", "ladder"), ("pairs_adj+id_ends", "ladder_top"),
          ("pairs_split", "ladder_even"), ("pairs_adj+id7", "ladder_one"), ("chain", "chain_equal"), ("chain", "uniform"), ("chain_alt", "chain_equal"),
          ("chain_alt", "ladder")]

# curve, n, window bits (0: the library's choice), precomputed tables, knobs.  Every width of {0, 4, 8, 13, 16} with and without tables, 17 with; n = 2^11, 2^13, 2^14,
# 2^15, 2^16 and two sizes that are no power of two; each knob at both values.
GRID = [("bn254", 1 << 14, 0, True, {}), ("bn254", 1 << 14, 0, False, {"msm_acc_points": 4}), ("bn254", 1 << 11, 4, True, {"msm_sort_block": 512}),
        ("bn254", 1 << 14, 13, False, {"msm_acc_block": 768}), ("bn254", 1 << 11, 17, True, {}), ("bn254", 1 << 11, 16, False, {}),
        ("pallas", 1 << 15, 0, True, {"msm_acc_points": 4, "msm_acc_block": 768}), ("pallas", 1 << 13, 8, False, {"msm_sort_block": 512}), ("pallas", 1 << 13, 16, True, {}),
        ("pallas", 1 << 11, 4, False, {}), ("pallas", 1 << 11, 13, True, {"msm_acc_points": 4}),
        ("vesta", (1 << 14) + 37, 0, False, {}), ("vesta", (1 << 13) + 37, 8, True, {"msm_acc_block": 768}), ("vesta", (1 << 13) + 37, 17, True, {"msm_sort_block": 512}),
        ("vesta", 1 << 16, 13, True, {}), ("vesta", 1 << 11, 16, False, {"msm_sort_block": 512, "msm_acc_points": 4})]


@pytest.mark.gpu
@pytest.mark.parametrize("cname,n,c,precompute,knobs", GRID, ids=["%s-n%d-c%d-%s%s" % (g[0], g[1], g[2], "tables" if g[3] else "rows", "".join("-%s%d" % (k[4:], v) for k, v in g[4].items())) for g in GRID])
def test_msm_degenerate_grid(pkg, lab, ctx, cname, n, c, precompute, knobs):
    """Every combination of COMBOS at one point of GRID: each column alone (batch 1), all columns of a base family as one batch of six (repeated cyclically), and a prefix
    of the registration -- against both references."""
    spec = lab.spec(cname)
    cw = c
    if c == 0:      # the library's choice for this n: the chain and the ladders are built for it
        h = ctx.register_bases(spec.id, lab.generic(cname, n)[0], 0, precompute)
        cw = h.window_bits
        h.release()
    by_base = {}
    for bfam, sfam in COMBOS:
        by_base.setdefault(bfam, []).append(sfam)
    with _Tuning(ctx, **knobs):
        for bfam, sfams in by_base.items():
            cases = [lab.case(cname, bfam, sfam, n, cw) for sfam in sfams]
            h = ctx.register_bases(spec.id, cases[0][0], c, precompute)
            try:
                assert h.window_bits == cw and h.precomputed == precompute
                for sfam, case in zip(sfams, cases):
                    _check(ctx.to_affine(spec.id, ctx.msm(h, case[2]))[0], case, (bfam, sfam, "alone"))
                got = ctx.to_affine(spec.id, ctx.msm_batch(h, [cases[j % len(cases)][2] for j in range(6)]))
                for j in range(6):
                    _check(got[j], cases[j % len(cases)], (bfam, sfams[j % len(cases)], "batch of 6, column %d" % j))
            finally:
                h.release()
        # a prefix MSM over a longer registration: the pairs and identities of the first m bases under the first m scalars of two columns
        m = n - n // 3
        bases, ks = lab.bases(cname, "pairs_adj+id7", n, cw)
        h = ctx.register_bases(spec.id, bases, c, precompute)
        try:
            for sfam in ("pair_equal_uniform", "ladder"):
                sc = lab.scalars(cname, sfam, "pairs_adj+id7", n, cw)[:m]
                case = (None, None, None, lab.closed_form(cname, ks[:m], sc), lab.oracle(cname, bases[:m], sc))
                _check(ctx.to_affine(spec.id, ctx.msm(h, sc))[0], case, ("prefix", sfam))
        finally:
            h.release()


@pytest.mark.gpu
@pytest.mark.parametrize("bfam", ["same", "pairs_adj", "small", "dup_adj"])
def test_msm_repeats_reach_every_merge_class_with_degenerate_partial_sums(pkg, lab, ctx, bfam):
    """1 .. 6000 points in single buckets over bases that are equal, opposite or small multiples: the partial sums of one bucket are then equal (same: every full lane
    holds [L] P), identities made by cancellation (pairs_adj) or collide now and then (small).  msm_acc_points is fixed, so the number of partial sums of a bucket follows
    from its multiplicity; msm_last_shape must show that every class of the merge (2-8 records, 9-64, 65-512, more than 512) had buckets."""
    cname, n = "bn254", 1 << 15
    spec = lab.spec(cname)
    with _Tuning(ctx, msm_acc_points=48):
        h = ctx.register_bases(spec.id, lab.bases(cname, bfam, n)[0], 0, True)
        try:
            assert 3 + len(REPEAT_MULTS) <= 1 << (h.window_bits - 1)          # every value of the column is one non-zero digit: one bucket
            case = lab.case(cname, bfam, "repeats", n, h.window_bits)
            _check(ctx.to_affine(spec.id, ctx.msm(h, case[2]))[0], case, (bfam, "repeats"))
            sh = ctx.msm_last_shape()
            assert sh["merge_light"] and sh["merge_32"] and sh["merge_wave"] and sh["merge_block"], sh
            assert sh["pairs"] == sum(REPEAT_MULTS)
            others = [lab.case(cname, bfam, sfam, n, h.window_bits) for sfam in ("uniform", "negdup", "pair_equal_few", "ladder_one", "pair_equal_uniform")]
            cols = [case] + others
            got = ctx.to_affine(spec.id, ctx.msm_batch(h, [x[2] for x in cols]))
            for j, x in enumerate(cols):
                _check(got[j], x, (bfam, "batch of 6, column %d" % j))
            sh = ctx.msm_last_shape()
            assert sh["merge_light"] and sh["merge_32"] and sh["merge_wave"] and sh["merge_block"], sh
        finally:
            h.release()


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("precompute", [True, False])
def test_msm_total_cancellation_is_the_identity_everywhere(pkg, lab, ctx, cname, precompute):
    """Whole columns whose result is the identity: the Jacobian output has z = 0, the affine output is (0, 0) -- through msm, through msm_batch with the cancelling
    column between two ordinary ones, and through msm_device_affine."""
    import torch
    spec, n = lab.spec(cname), 1 << 13
    for bfam, zero_fams in (("pairs_adj", ("pair_equal_few", "pair_equal_uniform", "ladder_one")), ("pairs_split", ("pair_equal_few", "pair_equal_uniform")),
                            ("dup_adj", ("negdup",)), ("chain_alt", ("chain_equal",))):
        h = ctx.register_bases(spec.id, lab.bases(cname, bfam, n)[0], 13, precompute)
        try:
            ordinary = [lab.case(cname, bfam, "uniform", n, 13), lab.case(cname, bfam, "ladder_top", n, 13)]
            for sfam in zero_fams:
                zc = lab.case(cname, bfam, sfam, n, 13)
                assert not zc[3].any() and not zc[4].any()                       # both references: the identity
                jac = ctx.msm(h, zc[2]).reshape(3, 4)
                assert not jac[2].any(), (bfam, sfam, "z")
                assert not ctx.to_affine(spec.id, jac)[0].any()
                cols = [ordinary[0], zc, ordinary[1]]
                jb = ctx.msm_batch(h, [x[2] for x in cols])
                assert not jb[1].reshape(3, 4)[2].any(), (bfam, sfam, "batch z")
                for j, x in enumerate(cols):
                    _check(ctx.to_affine(spec.id, jb)[j], x, (bfam, sfam, "batch", j))
                with ctx.torch_stream():
                    d = ctx.upload(np.stack([x[2] for x in cols]))
                    dj = torch.full((3, 12), -1, dtype=torch.int64, device="cuda")
                    da = torch.full((3, 8), -1, dtype=torch.int64, device="cuda")
                    ctx.msm_device_affine(h, d.data_ptr(), n, 3, dj.data_ptr(), da.data_ptr(), 0)
                    ctx.synchronize()
                    ga, gj = da.cpu().numpy().view(np.uint64), dj.cpu().numpy().view(np.uint64)
                assert not ga[1].any() and not gj[1, 8:].any(), (bfam, sfam, "device affine")
                for j, x in enumerate(cols):
                    _check(ga[j], x, (bfam, sfam, "device affine", j))
                    _check(ctx.to_affine(spec.id, gj[j])[0], x, (bfam, sfam, "device jacobian", j))
        finally:
            h.release()


def _jacobians(spec, rng, pts, plain_z=False):
    """affine canonical points (None = identity) -> n x 12 u64 Jacobian, each with a z of its own (equal points need not be equal records); the identity: z = 0 under
    non-zero garbage x, y"""
    p, out = spec.base.p, np.zeros((len(pts), 12), np.uint64)
    for i, P in enumerate(pts):
        z = 1 if plain_z else int(rng.integers(2, 1 << 62)) * int(rng.integers(2, 1 << 62)) % p
        x, y = (int(rng.integers(1, 1 << 62)), int(rng.integers(1, 1 << 62))) if P is None else (P[0] * z * z % p, P[1] * z * z * z % p)
        out[i, :4], out[i, 4:8] = spec.base.encode(x), spec.base.encode(y)
        if P is not None:
            out[i, 8:] = spec.base.encode(z)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVES)
def test_point_sum_device_on_equal_opposite_and_identity_entries(pkg, po, lab, ctx, cname):
    """k_point_sum (x29_add on strided lane sums, then a shuffle tree): all entries equal, alternating P, -P, identities with z = 0 under garbage x, y, a sum that
    cancels entirely.  Reference: the closed form [sum k_i] G."""
    import torch
    spec, cv = lab.spec(cname), po.CURVES[cname]
    r, G = spec.scalar.p, (cv.gx, cv.gy)
    rng = np.random.default_rng(77)
    kP = (1 + 2 * KSTEP) % r
    P = po.ec_mul(cv, kP, G)
    N = po.ec_neg(cv, P)
    Q = po.ec_mul(cv, 5, G)
    lists = []
    for count in (1, 2, 3, 64, 1000):
        lists.append(("equal", [P] * count, count * kP))
        lists.append(("alternating", [P if i % 2 == 0 else N for i in range(count)], (count % 2) * kP))
        lists.append(("identities", [None if i % 3 != 1 else P for i in range(count)], len(range(1, count, 3)) * kP))
        lists.append(("cancels", [P, N] * (count // 2) + [None] * (count % 2), 0))
        lists.append(("equal then one other", [P] * (count - 1) + [Q], (count - 1) * kP + 5))
    lists.append(("65 = one lane holds two", [P] * 65, 65 * kP))
    lists.append(("2 P against -2 P", [P, P, po.ec_neg(cv, po.ec_mul(cv, 2 * kP, G))], 0))
    for plain_z in (False, True):
        for name, pts, k in lists:
            want = enc_points(spec.base, [po.ec_mul(cv, k % r, G) if k % r else None])[0]
            with ctx.torch_stream():
                d = ctx.upload(_jacobians(spec, rng, pts, plain_z))
                out = torch.full((1, 12), -1, dtype=torch.int64, device="cuda")
                ctx.point_sum_device(spec.id, d.data_ptr(), len(pts), out.data_ptr(), 0)
                ctx.synchronize()
                got = out.cpu().numpy().view(np.uint64)
            assert np.array_equal(ctx.to_affine(spec.id, got)[0], want), (cname, name, len(pts), plain_z)
            if not want.any():
                assert not got[0, 8:].any(), (cname, name, len(pts), "z")


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVES)
def test_to_affine_with_identities_at_every_position(pkg, po, co, lab, ctx, cname):
    """to_affine / to_affine_device on batches with z = 0 records under garbage x, y: at the first, the last and every position of a group of 64 (the kernel's
    block; a batched inversion must not let one zero spoil its group), every second record, and an all-identity batch."""
    import torch
    spec, cv = lab.spec(cname), po.CURVES[cname]
    rng = np.random.default_rng(5)
    n = 200
    pts = [po.ec_mul(cv, 3 + i, (cv.gx, cv.gy)) for i in range(n)]
    masks = [{0}, {n - 1}, {0, n - 1}, set(range(0, n, 2)), set(range(64, 128)), set(range(n))] + [{j, 64 + (j + 1) % 64, 191 - j % 8} for j in range(64)]
    for mask in masks:
        cur = [None if i in mask else P for i, P in enumerate(pts)]
        jac, want = _jacobians(spec, rng, cur), enc_points(spec.base, cur)
        assert np.array_equal(ctx.to_affine(spec.id, jac), want), (cname, sorted(mask)[:4])
        assert all(np.array_equal(co.to_affine(spec.id, jac[i]), want[i]) for i in (0, 63, 64, n - 1))
        with ctx.torch_stream():
            d = ctx.upload(jac)
            out = torch.full((n, 8), -1, dtype=torch.int64, device="cuda")
            ctx.to_affine_device(spec.id, d.data_ptr(), n, out.data_ptr(), 0)
            ctx.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint64), want), (cname, sorted(mask)[:4], "device")


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVES)
def test_unregistered_multiexp_and_params_commit_on_pairs_and_identities(pkg, lab, ctx, cname):
    """ctx.best_multiexp (the one-shot path: single-row tables made for the call) and Params.commit / commit_lagrange / commit_many on bases made of P, -P pairs and
    identities."""
    spec, k = lab.spec(cname), 12
    n = 1 << k
    fams = ("pairs_adj+id7", "pairs_split+id_run", "pairs_adj+id_ends")
    for bfam in fams:
        for sfam in ("uniform", "pair_equal_uniform", "pair_equal_few", "ladder"):
            case = lab.case(cname, bfam, sfam, n, 13)
            _check(ctx.to_affine(spec.id, ctx.best_multiexp(spec.id, case[2], case[0]))[0], case, ("best_multiexp", bfam, sfam))
            _check(ctx.to_affine(spec.id, pkg.best_multiexp(ctx, spec, case[2], case[0]))[0], case, ("pkg.best_multiexp", bfam, sfam))
    g, gl = lab.bases(cname, fams[0], n)[0], lab.bases(cname, fams[1], n)[0]
    params = pkg.Params(ctx, spec, k, g, g_lagrange=gl)
    try:
        sfams = ("uniform", "pair_equal_uniform", "pair_equal_few", "negdup", "ladder_one")
        on_g = [lab.case(cname, fams[0], sfam, n, params.g.window_bits) for sfam in sfams]
        on_gl = [lab.case(cname, fams[1], sfam, n, params.g_lagrange.window_bits) for sfam in sfams]
        for case_g, case_l, sfam in zip(on_g, on_gl, sfams):
            _check(ctx.to_affine(spec.id, params.commit(case_g[2]))[0], case_g, ("commit", sfam))
            _check(ctx.to_affine(spec.id, params.commit_lagrange(case_l[2]))[0], case_l, ("commit_lagrange", sfam))
        for cases, lagrange in ((on_g, False), (on_gl, True)):
            got = ctx.to_affine(spec.id, params.commit_many([x[2] for x in cases], lagrange=lagrange))
            for j, x in enumerate(cases):
                _check(got[j], x, ("commit_many", lagrange, sfams[j]))
    finally:
        params.release()
