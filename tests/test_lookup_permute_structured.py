"""The lookup-permutation kernels (csrc/lookup_permute.hip) on structured keys and at their launch edges (tests/lookup_inputs.py): keys that differ in one chosen
32-bit word with the words below it ordered the other way round, word and limb boundaries, both ends of the field, theta * tag + value; misses that differ from a
key in one bit, lie between two adjacent keys or just outside the table; all four fields; every size class of the distinct-rows path and its boundaries;
distinct rows whose keys coincide; the wave-uniform shortcut of the rank kernel; runs of equal keys across merge blocks and tiles; the status words across
launch groups of 16 lookups; and check_witness's membership test on the same sort.

CPU (no mark): oracle/pyoracle.py permute_expression_pair on Python integers -- the reference of every GPU test here -- equals the C restatement byte for byte,
satisfies the argument's own conditions, and refuses every crafted miss, for every family and field.
GPU: np.array_equal against that reference, no tolerance; device outputs are written over buffers of all-ones words."""
import numpy as np
import pytest

import lookup_inputs as LI
from test_check_witness import LOOKUP, device_report, enumerate_failures, kzg_params, limbs, same_report      # noqa: F401  (kzg_params: a fixture)

EDGE_NS = [1, 2, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 6145, 10241]
EDGE_FAMILIES = ["word_0", "word_3", "theta_tag"]
DISTINCT_DS = [1, 2, 63, 64, 65, 128, 129, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048]
DISTINCT_N = 4100
MISS_N = 4100                                   # rows 0, n - 1 and 4096 (the first row of the last, partial tile)
MISS_ROWS = [0, MISS_N - 1, 4096]
POISON = -1


# ---------------------------------------------------------------- the reference, computed once per case and left unchanged
_REF = {}


def want(po, F, name, inputs, table, n):
    """-> (A', S') of the Python reference, encoded; cached under `name`"""
    key = (F.name,) + tuple(name)
    if key not in _REF:
        res = LI.reference(po, F, inputs, table, n)
        assert res is not None, key
        a, s = F.enc(res[0]), F.enc(res[1])
        a.setflags(write=False)
        s.setflags(write=False)
        _REF[key] = (a, s)
    return _REF[key]


# ---------------------------------------------------------------- CPU: the generators and the reference
def test_word_families_are_decided_by_their_word_alone(po):
    for fname in LI.FIELDS4:
        F = LI.field(po, fname)
        for w in range(8):
            ks = sorted(LI.keys(po, F, "word_%d" % w, 300))
            ws = [LI.words(k) for k in ks]
            assert all(a[w + 1:] == b[w + 1:] and a[w] < b[w] for a, b in zip(ws, ws[1:]))
            assert all(a[x] > b[x] for a, b in zip(ws, ws[1:]) for x in range(w))                       # every lower word: the reverse order
            assert all(k[7] < LI.TOP_WORD_BOUND for k in ws)
            if w < 7:
                assert {0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF} <= {k[w] for k in ws}
        assert {0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 64) + 1, (1 << 224) - 1, F.p - 2, F.p - 1, (F.p - 1) // 2, (F.p + 1) // 2} <= set(LI.keys(po, F, "carry", 22))
        assert max(LI.keys(po, F, "small", 600)) < 1 << 16


def test_crafted_misses_cover_every_word_and_both_sides(po):
    F = LI.field(po, "bn254_fr")
    ks = LI.keys(po, F, "word_0", 300)
    labels = [name for name, _ in LI.crafted_misses(F, ks)]
    assert all(("word%d_bit0" % w) in labels for w in range(8)) and "max_plus_1" in labels and "min_minus_1" in labels and "p_minus_1" in labels
    between = [v for name, v in LI.crafted_misses(F, ks) if name.startswith("between")]
    assert between and all(v - 1 in ks and v + 1 in ks for v in between)                                # v and v + 2 are keys, v + 1 is not
    assert "min_minus_1" not in [name for name, _ in LI.crafted_misses(F, LI.keys(po, F, "carry", 22))]  # (zero is a key)


def test_plateaus_and_wave_shapes_are_what_they_say(po):
    F = LI.field(po, "bn254_fr")
    table, srt = LI.plateau_table(po, F)
    assert len(table) == 511 + 513 + 2047 + 2049 + 4097 + (LI.PLATEAU_KEYS - 5) and sorted(set(table)) == srt
    assert sorted(table.count(srt[r]) for r, _ in LI.PLATEAU_RUNS) == [511, 513, 2047, 2049, 4097]
    ks = LI.keys(po, F, "word_0", 100)
    for shape in LI.WAVE_SHAPES:
        v = LI.wave_inputs(ks, shape, 4137)
        groups = [v[i:i + 64] for i in range(0, 4137, 64)]
        odd = {"but_lane_0": 0, "but_lane_31": 31, "but_lane_63": 63}.get(shape)
        for g in groups[:-1]:
            if odd is None:
                assert len(set(g)) == (2 if shape == "alternating" else 1)
            else:
                assert len(set(g)) == 2 and len(set(g[:odd] + g[odd + 1:])) == 1
        assert len(groups[-1]) == 41


def _cpu_shapes(po, F, family):
    """one small shape each of the general and the distinct tables: (label, inputs, table, n, keys)"""
    inputs, table, ks = LI.general_case(po, F, family, 531)
    yield "general", inputs, table, 531, ks + [F.p - 1]
    inputs, table, _, _ = LI.distinct_case(po, F, family, 65, 300)
    yield "distinct", inputs, table, 300, sorted(set(table))


@pytest.mark.parametrize("fname", LI.FIELDS4)
@pytest.mark.parametrize("family", LI.FAMILIES)
def test_python_reference_agrees_with_c_and_holds_the_invariants(po, co, family, fname):
    F = LI.field(po, fname)
    for label, inputs, table, n, ks in _cpu_shapes(po, F, family):
        res = LI.reference(po, F, inputs, table, n)
        assert res is not None
        LI.check_invariants(inputs, table, n, res)
        ei, et = F.enc(inputs), F.enc(table)
        got = co.permute_expression_pair(F.fid, ei, et, n)
        assert got is not None
        assert got[0].tobytes() == F.enc(res[0]).tobytes() and got[1].tobytes() == F.enc(res[1]).tobytes(), (label, family, fname)
        assert F.dec(got[0]) == res[0]                                                                  # (and the encoding round-trips)
        misses = LI.crafted_misses(F, ks)
        assert len(misses) >= 10
        for i, (name, v) in enumerate(misses):
            row = (0, n - 1, n // 2)[i % 3]
            bad, ebad = list(inputs), ei.copy()
            bad[row], ebad[row] = v, F.enc1(v)
            assert LI.reference(po, F, bad, table, n) is None, (label, name)
            assert co.permute_expression_pair(F.fid, ebad, et, n) is None, (label, name)


# ---------------------------------------------------------------- GPU helpers
def _np(t):
    return t.cpu().numpy().view(np.uint64)


def _poisoned(n):
    import torch
    return torch.full((n, 4), POISON, dtype=torch.int64, device="cuda")


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def run_ptrs(ctx, F, n, inputs, tables, table_of, deferred=False):
    """lookups as pointer lists: inputs[y] (encoded) looks up tables[table_of[y]] -> (A' list, S' list, status or None)"""
    import torch
    d_in, d_tab = [ctx.upload(np.ascontiguousarray(a)) for a in inputs], [ctx.upload(np.ascontiguousarray(t)) for t in tables]
    oi, ot = [_poisoned(n) for _ in inputs], [_poisoned(n) for _ in inputs]
    status = torch.full((len(inputs),), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    args = (F.fid, _ptrs(d_in), [d_tab[t].data_ptr() for t in table_of], n, _ptrs(oi), _ptrs(ot))
    try:
        if deferred:
            ctx.permute_expression_pair_ptrs_deferred_device(*args, status.data_ptr(), 0)
        else:
            ctx.permute_expression_pair_ptrs_device(*args, 0)
    finally:
        ctx.synchronize()
    return [_np(o) for o in oi], [_np(o) for o in ot], status.cpu().numpy() if deferred else None


def run_distinct(ctx, F, n, lookups, tables, with_status=True):
    """lookups: [(inputs (encoded), table index)]; tables: [(table (encoded), rep rows, multiplicities)] -> (A' list, S' list, status or None).  Without the status
    array the call synchronises and raises on a miss."""
    import torch
    d_tab = [(ctx.upload(np.ascontiguousarray(t)), ctx.upload(np.ascontiguousarray(r, dtype=np.uint32)), ctx.upload(np.ascontiguousarray(m, dtype=np.uint32)), len(r))
             for t, r, m in tables]
    d_in = [ctx.upload(np.ascontiguousarray(a)) for a, _ in lookups]
    which = [t for _, t in lookups]
    oi, ot = [_poisoned(n) for _ in lookups], [_poisoned(n) for _ in lookups]
    status = torch.full((len(lookups),), 9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    try:
        ctx.permute_expression_pair_distinct_device(F.fid, _ptrs(d_in), [d_tab[t][0].data_ptr() for t in which], n, _ptrs(oi), _ptrs(ot),
                                                    [d_tab[t][1].data_ptr() for t in which], [d_tab[t][2].data_ptr() for t in which], [d_tab[t][3] for t in which],
                                                    status.data_ptr() if with_status else 0, 0)
    finally:
        ctx.synchronize()
    return [_np(o) for o in oi], [_np(o) for o in ot], status.cpu().numpy() if with_status else None


def same(got_i, got_t, ref, label):
    assert np.array_equal(got_i, ref[0]), ("A'",) + tuple(label)
    assert np.array_equal(got_t, ref[1]), ("S'",) + tuple(label)


def distinct_equals_reference(po, ctx, F, n, lookups, tables, label):
    """lookups: [(inputs as ints, table index)], tables: [(table as ints, rep, mult)]: the status form of the call, every lookup against the reference"""
    gi, gt, st = run_distinct(ctx, F, n, [(F.enc(a), t) for a, t in lookups], [(F.enc(t), r, m) for t, r, m in tables])
    assert not st.any(), (label, st)
    for y, (a, t) in enumerate(lookups):
        same(gi[y], gt[y], want(po, F, tuple(label) + (y,), a, tables[t][0], n), tuple(label) + (y,))


# ---------------------------------------------------------------- GPU: the general path
@pytest.mark.gpu
@pytest.mark.parametrize("fname", LI.FIELDS4)
@pytest.mark.parametrize("family", LI.FAMILIES)
def test_general_families_by_field(po, ctx, family, fname):
    """n = 4097: three tiles, so both merge passes have a short or an empty B run.  The host entry point, and the pointer-list one with two lookups of one table."""
    F, n = LI.field(po, fname), 4097
    inputs, table, _ = LI.general_case(po, F, family, n)
    other = LI.general_case(po, F, family, n, seed=2)[0]
    et = F.enc(table)
    ref = want(po, F, ("general", family, n, 0), inputs, table, n)
    pi, pt = ctx.permute_expression_pair(F.fid, F.enc(inputs), et, n)
    same(pi, pt, ref, (family, fname, "host"))
    gi, gt, _ = run_ptrs(ctx, F, n, [F.enc(inputs), F.enc(other)], [et], [0, 0])
    same(gi[0], gt[0], ref, (family, fname, "ptrs", 0))
    same(gi[1], gt[1], want(po, F, ("general", family, n, 1), other, table, n), (family, fname, "ptrs", 1))


@pytest.mark.gpu
@pytest.mark.parametrize("fname", LI.FIELDS2)
@pytest.mark.parametrize("family", EDGE_FAMILIES)
@pytest.mark.parametrize("n", EDGE_NS)
def test_general_launch_edges(po, ctx, n, family, fname):
    """around the 512-output merge block and the 2048-key tile, up to six tiles; p - 1 against the +infinity padding where there is any.  The strided batch entry
    point (two lookups, each with its own table) and the deferred pointer-list one."""
    import torch
    F = LI.field(po, fname)
    cases = [LI.general_case(po, F, family, n, seed=s) for s in (1, 2)]
    refs = [want(po, F, ("edge", family, n, y), c[0], c[1], n) for y, c in enumerate(cases)]
    if n % 2048:
        assert all(F.p - 1 in c[0] and F.p - 1 in c[1] for c in cases)
    stride = n + 3
    ins, tabs = np.zeros((2, stride, 4), dtype=np.uint64), np.zeros((2, stride, 4), dtype=np.uint64)
    for y, c in enumerate(cases):
        ins[y, :n], tabs[y, :n] = F.enc(c[0]), F.enc(c[1])
        ins[y, n:], tabs[y, n:] = F.enc1(F.p - 2), F.enc1(3)                                            # beyond the usable rows: ignored
    di, dt = ctx.upload(ins), ctx.upload(tabs)
    oi, ot = torch.full_like(di, POISON), torch.full_like(dt, POISON)
    ctx.permute_expression_pair_batch_device(F.fid, di.data_ptr(), dt.data_ptr(), n, 2, stride, oi.data_ptr(), ot.data_ptr(), 0)
    ctx.synchronize()
    gi, gt = _np(oi), _np(ot)
    for y in range(2):
        same(gi[y, :n], gt[y, :n], refs[y], (family, fname, n, "batch", y))
        assert (gi[y, n:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (gt[y, n:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()      # nothing written past the column
    gi, gt, st = run_ptrs(ctx, F, n, [ins[0, :n], ins[1, :n]], [tabs[0, :n], tabs[1, :n]], [0, 1], deferred=True)
    assert not st.any()
    for y in range(2):
        same(gi[y], gt[y], refs[y], (family, fname, n, "deferred", y))


@pytest.mark.gpu
@pytest.mark.parametrize("fname", LI.FIELDS2)
def test_general_plateaus_across_merge_blocks_and_tiles(po, ctx, fname):
    """runs of 511, 513, 2047, 2049 and 4097 equal keys, rows shuffled, five tiles (an odd count): both partition diagonals of a merge block fall inside a run that
    A and B share.  Four lookups of the one table."""
    F = LI.field(po, fname)
    table, srt = LI.plateau_table(po, F)
    n = len(table)
    assert 9000 < n < 11000 and (n + 2047) // 2048 == 5
    shapes = LI.plateau_inputs(srt, n)
    gi, gt, _ = run_ptrs(ctx, F, n, [F.enc(v) for v in shapes.values()], [F.enc(table)], [0] * len(shapes))
    for y, (name, v) in enumerate(shapes.items()):
        same(gi[y], gt[y], want(po, F, ("plateau", name), v, table, n), (fname, name))


@pytest.mark.gpu
@pytest.mark.parametrize("fname", LI.FIELDS2)
def test_general_input_tiles(po, ctx, fname):
    """n = 2049: one input in the second tile of the rank kernel"""
    F, n = LI.field(po, fname), 2049
    table, shapes = LI.input_tile_cases(po, F, n)
    et = F.enc(table)
    for name, v in shapes.items():
        pi, pt = ctx.permute_expression_pair(F.fid, F.enc(v), et, n)
        same(pi, pt, want(po, F, ("input tiles", name), v, table, n), (fname, name))


@pytest.mark.gpu
@pytest.mark.parametrize("fname", LI.FIELDS2)
@pytest.mark.parametrize("family", LI.FAMILIES)
def test_general_crafted_misses(pkg, po, ctx, family, fname):
    """every crafted miss, one at a time, at row 0, at row n - 1 and at the first row of the last partial tile: error -6, and the next call on the same context
    with the good inputs is right"""
    F, n = LI.field(po, fname), MISS_N
    inputs, table, ks = LI.general_case(po, F, family, n)
    ei, et = F.enc(inputs), F.enc(table)
    ref = want(po, F, ("general", family, n, 0), inputs, table, n)
    misses = LI.crafted_misses(F, ks + [F.p - 1])
    assert len(misses) >= 10
    for name, v in misses:
        for row in MISS_ROWS:
            bad = ei.copy()
            bad[row] = F.enc1(v)
            with pytest.raises(pkg.DehaloError) as e:
                ctx.permute_expression_pair(F.fid, bad, et, n)
            assert e.value.code == -6, (family, fname, name, row)
        pi, pt = ctx.permute_expression_pair(F.fid, ei, et, n)
        same(pi, pt, ref, (family, fname, "after", name))


@pytest.mark.gpu
def test_status_words_across_launch_groups(pkg, po, ctx):
    """18 lookups of one table are two launch groups (16 + 2): a miss each in lookups 0, 15, 16 and 17 sets exactly those status words, the other fourteen lookups
    are right; the synchronous call names a failing lookup by its index in the call"""
    F, n, B = LI.field(po, "bn254_fr"), 4097, 18
    _, table, ks = LI.general_case(po, F, "word_3", n)
    misses = LI.crafted_misses(F, ks + [F.p - 1])
    ins = [LI.general_case(po, F, "word_3", n, seed=10 + y)[0] for y in range(B)]
    enc = [F.enc(v) for v in ins]
    bad_at = {0: 0, 15: n - 1, 16: 4096, 17: 2048}
    for j, (y, row) in enumerate(bad_at.items()):
        enc[y] = enc[y].copy()
        enc[y][row] = F.enc1(misses[3 * j][1])
    gi, gt, st = run_ptrs(ctx, F, n, enc, [F.enc(table)], [0] * B, deferred=True)
    assert [y for y in range(B) if st[y]] == sorted(bad_at), st
    for y in range(B):
        if y not in bad_at:
            same(gi[y], gt[y], want(po, F, ("groups", y), ins[y], table, n), ("groups", y))
    with pytest.raises(pkg.DehaloError) as e:
        run_ptrs(ctx, F, n, enc, [F.enc(table)], [0] * B)
    assert e.value.code == -6 and "lookup 0 " in str(e.value)
    enc[0], enc[15] = F.enc(ins[0]), F.enc(ins[15])                                                     # the first group is clean now: the second group's own misses
    with pytest.raises(pkg.DehaloError) as e:
        run_ptrs(ctx, F, n, enc, [F.enc(table)], [0] * B)
    assert e.value.code == -6 and "lookup 16 " in str(e.value), str(e.value)


# ---------------------------------------------------------------- GPU: the distinct-rows path
@pytest.mark.gpu
@pytest.mark.parametrize("family", ["word_0", "theta_tag"])
@pytest.mark.parametrize("d", DISTINCT_DS + [2049])
def test_distinct_size_classes(po, ctx, d, family):
    """dlen 64 .. 2048 and both sides of every boundary (up to 512: the counting sort; above: the tile sort; 2048: the rank kernel's LDS opt-in); 2049 distinct
    rows take the general path"""
    F, n = LI.field(po, "bn254_fr"), max(d, DISTINCT_N)
    inputs, table, rep, mult = LI.distinct_case(po, F, family, d, n)
    distinct_equals_reference(po, ctx, F, n, [(inputs, 0)], [(table, rep, mult)], ("size", family, d))


@pytest.mark.gpu
@pytest.mark.parametrize("fname", LI.FIELDS4)
@pytest.mark.parametrize("d", [65, 513, 2048])
def test_distinct_by_field(po, ctx, d, fname):
    F, n = LI.field(po, fname), DISTINCT_N
    for family in ("word_0", "theta_tag"):
        inputs, table, rep, mult = LI.distinct_case(po, F, family, d, n)
        distinct_equals_reference(po, ctx, F, n, [(inputs, 0)], [(table, rep, mult)], ("size", family, d))


@pytest.mark.gpu
@pytest.mark.parametrize("family", LI.FAMILIES)
@pytest.mark.parametrize("d", [300, 1500])
def test_distinct_families(po, ctx, d, family):
    """300: dlen 512 and the counting sort, on keys equal in seven of eight words; 1500: the tile sort and the LDS opt-in"""
    F, n = LI.field(po, "bn254_fr"), DISTINCT_N
    inputs, table, rep, mult = LI.distinct_case(po, F, family, d, n)
    distinct_equals_reference(po, ctx, F, n, [(inputs, 0)], [(table, rep, mult)], ("family", family, d))


@pytest.mark.gpu
@pytest.mark.parametrize("counts", [(3, 1024), (2048, 5)])
def test_distinct_two_tables_of_very_different_counts(po, ctx, counts):
    """the small table is searched with the big one's dlen: its few keys sit in front of a tile of +infinity padding"""
    F, n = LI.field(po, "bn254_fr"), DISTINCT_N
    tabs, ins = [], []
    for t, (d, family) in enumerate(zip(counts, ("theta_tag", "word_0"))):
        inputs, table, rep, mult = LI.distinct_case(po, F, family, d, n, seed=3 + t)
        tabs.append((table, rep, mult))
        ins.append(inputs)
    which = [0, 1, 0, 0, 1]
    lookups = [(ins[t] if y < 2 else [ins[t][(i * (y + 2)) % n] for i in range(n)], t) for y, t in enumerate(which)]
    distinct_equals_reference(po, ctx, F, n, lookups, tabs, ("two tables",) + counts)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [300, 1500])
@pytest.mark.parametrize("shape", ["all_one", "one_heavy_all_looked_up", "heavy_never_looked_up"])
def test_distinct_multiplicities(po, ctx, shape, d):
    """all_one: n = d, every row its own key.  one_heavy_all_looked_up: one key holds n - d + 1 rows and every key is looked up, so the single-copy keys leave no
    leftover.  heavy_never_looked_up: the leftovers are the heavy key's copies and nothing of it is a first occurrence."""
    F = LI.field(po, "bn254_fr")
    ks = LI.keys(po, F, "word_0", d)
    n = d if shape == "all_one" else DISTINCT_N
    heavy = d // 2
    entries = [(k, n - d + 1 if (i == heavy and shape != "all_one") else 1) for i, k in enumerate(ks)]
    table, rep, mult = LI.distinct_table(entries, 11)
    if shape == "heavy_never_looked_up":
        pool = ks[:heavy] + ks[heavy + 1:]
        inputs = [pool[i] for i in LI.draw(n, len(pool), 12)]
        assert ks[heavy] not in inputs
    else:
        inputs = ks + [ks[i] for i in LI.draw(n - d, d, 13)]
    sparse = [ks[(d - 1) if i % 5 else 0] for i in range(n)]                                             # a second lookup of the same table: two keys only
    distinct_equals_reference(po, ctx, F, n, [(inputs, 0), (sparse, 0)], [(table, rep, mult)], ("mult", shape, d))


COINCIDING = {"two_adjacent": [(10, 11)], "two_100_apart": [(20, 120)], "run_of_40": [(50, 50 + j) for j in range(1, 40)]}


@pytest.mark.gpu
@pytest.mark.parametrize("d", [300, 1500])
@pytest.mark.parametrize("shape", list(COINCIDING) + ["all_equal"])
def test_distinct_rows_whose_keys_coincide(po, ctx, shape, d):
    """separate entries (own representative row, own multiplicity) that hold the SAME value: their multiplicities add up.  The reference sees the table only."""
    F, n = LI.field(po, "bn254_fr"), DISTINCT_N
    if shape == "all_equal":
        d = 70 if d == 300 else 1100
    ks = LI.keys(po, F, "word_0", d)
    if shape == "all_equal":
        ks = [ks[0]] * d
    else:
        for src, dst in COINCIDING[shape]:
            ks[dst] = ks[src]
    mults = LI.spread_multiplicities(d, n, 21)
    mults[0], mults[10] = mults[10], mults[0]                                                            # the heavy entry is one of the coinciding ones in "two_adjacent"
    flat = [k for k, m in zip(ks, mults) for _ in range(m)]
    order = np.random.default_rng(22).permutation(n).tolist()
    table = [flat[i] for i in order]
    first = np.cumsum([0] + mults[:-1])
    where = np.empty(n, dtype=np.int64)
    where[order] = np.arange(n)
    rep = np.array([where[s] for s in first], dtype=np.uint32)                                           # the entries stay in the order given: "adjacent" means adjacent
    assert all(table[int(r)] == k for r, k in zip(rep, ks)) and sum(mults) == n
    uniq = sorted(set(ks))
    looked_up = [ks[i] for i in LI.draw(n, d, 23)]
    looked_up[0], looked_up[n - 1] = ks[COINCIDING.get(shape, [(0, 0)])[0][0]], ks[COINCIDING.get(shape, [(0, 0)])[0][0]]
    lookups = [(looked_up, 0)]
    if len(uniq) > 1:
        dup = ks[COINCIDING[shape][0][0]]
        pool = [k for k in uniq if k != dup]
        lookups.append(([pool[i] for i in LI.draw(n, len(pool), 24)], 0))                                # the coinciding key is never looked up: all its copies are leftovers
    distinct_equals_reference(po, ctx, F, n, lookups, [(table, rep, np.array(mults, dtype=np.uint32))], ("coincide", shape, d))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [100, 1500])
@pytest.mark.parametrize("shape", LI.WAVE_SHAPES)
def test_distinct_wave_shapes(po, ctx, shape, d):
    """the rank kernel counts a wave whose 64 inputs are one value with one atomic: waves that are uniform, uniform but for lane 0 / 31 / 63, alternating, and
    the last wave cut by n with its live lanes all equal"""
    F = LI.field(po, "bn254_fr")
    n = DISTINCT_N + 37 if shape == "last_wave_cut" else DISTINCT_N
    ks = LI.keys(po, F, "word_0", d)
    table, rep, mult = LI.distinct_table(list(zip(ks, LI.spread_multiplicities(d, n, 31))), 32)
    distinct_equals_reference(po, ctx, F, n, [(LI.wave_inputs(ks, shape, n), 0)], [(table, rep, mult)], ("wave", shape, d))


@pytest.mark.gpu
@pytest.mark.parametrize("family", LI.WORD_FAMILIES + ["carry"])
def test_distinct_crafted_misses(pkg, po, ctx, family):
    """synchronous form: error -6; status form: the flag of that lookup only, and the lookups beside it are right"""
    F, n, d = LI.field(po, "bn254_fr"), DISTINCT_N, 300
    inputs, table, rep, mult = LI.distinct_case(po, F, family, d, n)
    ei, tab = F.enc(inputs), (F.enc(table), rep, mult)
    ref = want(po, F, ("family", family, d, 0), inputs, table, n)
    misses = LI.crafted_misses(F, sorted(set(table)))
    assert len(misses) >= 10
    for j, (name, v) in enumerate(misses):
        bad = ei.copy()
        bad[MISS_ROWS[j % 3]] = F.enc1(v)
        with pytest.raises(pkg.DehaloError) as e:
            run_distinct(ctx, F, n, [(bad, 0)], [tab], with_status=False)
        assert e.value.code == -6, (family, name)
        gi, gt, st = run_distinct(ctx, F, n, [(ei, 0), (bad, 0), (ei, 0)], [tab])
        assert st[0] == 0 and st[1] != 0 and st[2] == 0, (family, name, st)
        same(gi[0], gt[0], ref, (family, name, 0))
        same(gi[2], gt[2], ref, (family, name, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 512, 2048])
def test_distinct_misses_beside_a_full_tile(po, ctx, d):
    """d = dlen: no +infinity padding behind the largest key among the keys searched.  A miss above the maximum, one below the minimum, one between"""
    F, n = LI.field(po, "bn254_fr"), DISTINCT_N
    inputs, table, rep, mult = LI.distinct_case(po, F, "word_1", d, n)
    ei, tab = F.enc(inputs), (F.enc(table), rep, mult)
    picked = [v for name, v in LI.crafted_misses(F, sorted(set(table))) if name in ("max_plus_1", "min_minus_1", "p_minus_1") or name.startswith("between")]
    assert len(picked) >= 4
    for j, v in enumerate(picked):
        bad = ei.copy()
        bad[MISS_ROWS[j % 3]] = F.enc1(v)
        _, _, st = run_distinct(ctx, F, n, [(bad, 0), (ei, 0)], [tab])
        assert st[0] != 0 and st[1] == 0, (d, j, st)


# ---------------------------------------------------------------- GPU: check_witness's membership test (lookup_sort_tables, chk_cmp)
@pytest.mark.gpu
@pytest.mark.parametrize("w", [0, 3, 7])
def test_check_witness_membership_on_word_keys(pkg, po, co, ctx, kzg_params, w):
    """one lookup of one expression (a in t), so the compressed value is the cell itself.  k = 12: the 4090 usable table rows are two tiles and a merge.  The witness
    is satisfied except for three rows that hold a value one bit away from a key"""
    from dehalo2_amd import plonk as P
    F, k = LI.field(po, "bn254_fr"), 12
    n = 1 << k
    cs = P.ConstraintSystem(num_advice=1, num_fixed=1, num_instance=0)
    cs.enable_equality(P.ADVICE, 0)
    cs.lookup([(cs.query_advice(0), cs.query_fixed(0))])
    usable = n - (cs.blinding_factors() + 1)
    ks = LI.keys(po, F, "word_%d" % w, 500)
    misses = [v for name, v in LI.crafted_misses(F, ks) if name.startswith("word")]
    assert len(misses) == 16
    pick = [misses[2 * w], misses[2 * w + 1], misses[(2 * w + 2) % 16]]                                 # two bits of word w, one bit of the next word
    assert all(min(bin(v ^ key).count("1") for key in ks) == 1 for v in pick)
    table = [ks[r % len(ks)] for r in range(usable)] + [0] * (n - usable)                               # (zero is no key: the unusable rows are no part of the table)
    assert 0 not in ks
    a = [ks[i] for i in LI.draw(usable, len(ks), 41)] + [0] * (n - usable)
    rows = [0, 2053, usable - 1]
    for row, v in zip(rows, pick):
        a[row] = v
    fixed, advice = limbs(table, n)[None], limbs(a, n)[None]
    fails, counters = enumerate_failures(cs, k, F.p, fixed, advice, None)
    assert fails == [(LOOKUP, 0, r) for r in rows]
    same_report(device_report(pkg, co, ctx, kzg_params(k), cs, fixed, advice, P.Assembly(1, n), mapping=None), fails, counters)
    good = list(a)
    for row in rows:
        good[row] = ks[3]
    advice = limbs(good, n)[None]
    fails, counters = enumerate_failures(cs, k, F.p, fixed, advice, None)
    assert not fails
    same_report(device_report(pkg, co, ctx, kzg_params(k), cs, fixed, advice, P.Assembly(1, n), mapping=None), fails, counters)
