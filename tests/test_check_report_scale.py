"""dehalo_check_witness at the scale of the workload: reports of millions of failures, every edge of the count / scan / emit pipeline, all four regions of the
bitmap, shuffles over a merged sort, a checking program with spilled slots, the grouping loops of check_body, and a domain below one wave.

tests/test_check_witness.py holds the checker to an enumerator over circuits of 2^5 .. 2^8 rows with a handful of failures.  Here the circuits come from
tests/check_inputs.py, whose failure sets are boolean arrays written straight from the inputs (GRID, MIXED, the grouping keys) or a collections.Counter over
the rows (shuffles); the spilled-slot key's expected report is the enumerator's.
CPU: every closed form equals the enumerator at k = 6 and 8; the Counter reference equals a brute-force count; the GRID edge placements land in the words they
are named after; the spill key's checking program needs more slots than the LDS holds.
GPU: the device's totals, `written` and stored failures against the closed form at k = 16 (GRID: 272 bitmap rows, 1088 tiles, two chunks of the scan), k = 12
(MIXED, shuffles), k = 8 (spill), k = 6 (17 tables, 9 shuffles) and k = 4 (a quarter wave)."""
import collections
import functools
import time

import numpy as np
import pytest

import check_inputs as CI
from check_inputs import COPY, GATE, LOOKUP, SHUFFLE
from test_check_witness import enumerate_failures, kzg_params, same_report      # noqa: F401  (kzg_params: a fixture)

GRID_K, GRID_S, GRID_A = 16, 16, 17      # 272 bitmap rows x 1024 words = 1088 tiles: bitmap rows 256 .. 271 are the scan's second chunk
CAP_MAX = 1 << 18
MIXED_K = 12
MIXED_SHAPES = {"GLPH": (3, 2, 3, 1), "G-PH": (3, 0, 3, 1), "GLP-": (3, 2, 3, 0)}


def field_p(pkg):
    return pkg.fields.BN254_FR.p


def enumerated(pkg, cs, k, fixed, adv, mapping):
    """the enumerator's failures over small-integer columns, as tuples"""
    fails, _ = enumerate_failures(cs, k, field_p(pkg), CI.columns(fixed), CI.columns(adv), mapping)
    return fails


# ============================================================================================================================== CPU: the references agree
@pytest.mark.parametrize("k,S,A", [(6, 16, 17), (8, 3, 4)])
def test_grid_closed_form_is_the_enumerators(pkg, oracles, k, S, A):
    n = 1 << k
    usable = n - CI.BLINDING_ROWS
    cs, s = CI.grid_cs(pkg, S, A), CI.grid_fixed(k, S)
    assert s[:, usable:].all() and (s.sum(axis=0) == 1).sum() >= n // 4      # all ones on the unusable rows and the bands, one-hot elsewhere
    for w in (CI.grid_unusable(A, n, usable), CI.grid_random(k, A, 0.3, 5), CI.grid_random(k, A, 1.0, 6)):
        want = CI.report_of(CI.grid_bitmap(s, w, usable), (S * A, 0, 0, 0))
        assert CI.as_tuples(want["failures"]) == enumerated(pkg, cs, k, s, w, None)
        assert want["totals"] == (len(want["failures"]), 0, 0, 0)
    assert not len(CI.report_of(CI.grid_bitmap(s, CI.grid_unusable(A, n, usable), usable), (S * A, 0, 0, 0))["failures"])
    assert len(want["failures"]) == int((s[:, :usable] != 0).sum()) * A      # every w non-zero: every non-zero s on a usable row fails under every w_j


@functools.lru_cache(maxsize=None)
def grid_edge_cases():
    """-> (s, {name: (w, expected report)}): every placement of check_inputs.grid_edges alone, and all of them together.  Asserts, without a device, that the
    expected lists hold a failure in the words the placements are named after."""
    k, S, A = GRID_K, GRID_S, GRID_A
    n = 1 << k
    usable, words = n - CI.BLINDING_ROWS, n // 64
    s = CI.grid_fixed(k, S)
    edges = CI.grid_edges(k, S, A)
    word = lambda g, r: g * words + r // 64
    t = {name: target for name, (_, target) in edges.items()}
    # the words: first and last of the bitmap, bits 0 and 63, both sides of a tile edge inside one bitmap row, both sides of the scan's chunk edge
    assert word(*t["first word, bit 0"]) == 0 and t["first word, bit 0"][1] % 64 == 0
    assert t["bit 63"][1] % 64 == 63
    assert word(*t["last word of the bitmap"]) == S * A * words - 1 and t["last word of the bitmap"] == (S * A - 1, usable - 1)
    a, b = t["last word of a tile"], t["first word of the next tile"]
    assert a[0] == b[0] and word(*a) + 1 == word(*b) and word(*b) % CI.TILE_WORDS == 0 and (a[1], b[1]) == (16383, 16384)
    a, b = t["last row before the second chunk"], t["first word of the second chunk"]
    assert CI.tile_of(words, *a) == CI.CHUNK_TILES - 1 and CI.tile_of(words, *b) == CI.CHUNK_TILES and a == (255, usable - 1) and b[0] == 256 and b[1] < 64
    assert usable == 65530 and s[:, usable:].all() and (s.sum(axis=0) == 1).sum() > 3 * n // 4      # one-hot on most rows
    out, every = {}, []
    for name, (cells, target) in edges.items():
        w = CI.grid_witness(A, n, usable, cells)
        want = CI.report_of(CI.grid_bitmap(s, w, usable), (S * A, 0, 0, 0))
        assert (GATE,) + target in CI.as_tuples(want["failures"]), name
        out[name] = (w, want)
        every += cells
    w = CI.grid_witness(A, n, usable, every)
    want = CI.report_of(CI.grid_bitmap(s, w, usable), (S * A, 0, 0, 0))
    got = set(CI.as_tuples(want["failures"]))
    assert all((GATE,) + target in got for target in t.values())
    out["all placements"] = (w, want)
    return s, out


def test_grid_edge_placements_fail_in_the_words_they_name():
    s, cases = grid_edge_cases()
    assert len(cases) == 8 and all(0 < len(want["failures"]) < 200 for _, want in cases.values())


def mixed_case(pkg, k, shape):
    G, L, P_, H = shape
    cs, fixed, asm = CI.mixed_cs(pkg, G, L, P_, H), CI.mixed_fixed(k), CI.mixed_assembly(pkg, k, P_)
    good = CI.mixed_satisfied(k, G, L, P_, H)
    breaks = CI.mixed_breaks(k, G, L, P_, H)
    witnesses = {"satisfied": good}
    for name, cells in breaks.items():
        witnesses[name] = CI.with_cells(good, cells)
    witnesses["all together"] = CI.with_cells(good, [c for cells in breaks.values() for c in cells])
    return cs, fixed, asm, witnesses


def mixed_want(k, shape, fixed, adv, mapping):
    G, L, P_, H = shape
    return CI.report_of(CI.mixed_bitmap(k, G, L, P_, H, fixed, adv, mapping), (G, L, P_ if mapping is not None else 0, H))


@pytest.mark.parametrize("k", [6, 8])
@pytest.mark.parametrize("name", list(MIXED_SHAPES))
def test_mixed_closed_form_is_the_enumerators(pkg, oracles, k, name):
    """gates, lookups and copies from the enumerator, shuffles from the brute-force count, appended in region order"""
    shape = MIXED_SHAPES[name]
    G, L, P_, H = shape
    n = 1 << k
    usable = n - CI.BLINDING_ROWS
    cs, fixed, asm, witnesses = mixed_case(pkg, k, shape)
    kinds = set()
    for mapping in (asm.mapping, None):
        for wname, adv in witnesses.items():
            want = mixed_want(k, shape, fixed, adv, mapping)
            fails = enumerated(pkg, cs, k, fixed, adv, mapping)
            for h in range(H):
                x, y = adv[G + L + P_ + 2 * h, :usable].tolist(), adv[G + L + P_ + 2 * h + 1, :usable].tolist()
                fails += [(SHUFFLE, h, int(r)) for r in np.nonzero(CI.brute_shuffle_failures(x, y))[0]]
            assert CI.as_tuples(want["failures"]) == fails, (wname, mapping is None)
            assert (not fails) == (wname == "satisfied" or (mapping is None and wname.startswith("copies")))
            if wname == "all together" and mapping is not None:
                kinds = {f[0] for f in fails}
                rows = {(f[0], f[2]) for f in fails}
                assert all((kind, r) in rows for kind in kinds for r in (0, usable - 1))      # the first and the last usable row of every region
    assert kinds == {kind for kind, cnt in zip((GATE, LOOKUP, COPY, SHUFFLE), shape) if cnt}


def test_counter_shuffle_reference_is_the_brute_force_one():
    rng = np.random.default_rng(3)
    for u in (10, 58, 250):
        x = rng.integers(0, max(2, u // 4), size=u).tolist()
        for changes in (0, 1, 3):
            y = [x[i] for i in rng.permutation(u)]
            for c in range(changes):
                y[int(rng.integers(u))] = (u // 8 if c % 2 else 10 ** 6 + c)      # a value the inputs hold, a value they do not
            assert np.array_equal(CI.counter_shuffle_failures(x, y), CI.brute_shuffle_failures(x, y))
            assert CI.counter_shuffle_failures(x, y).any() == (sorted(x) != sorted(y))
    # tuples
    x = [(i % 3, i % 2) for i in range(30)]
    y = list(reversed(x))
    y[0] = (y[0][1], y[0][0] + 5)
    assert np.array_equal(CI.counter_shuffle_failures(x, y), CI.brute_shuffle_failures(x, y)) and CI.counter_shuffle_failures(x, y).any()


def test_merged_shuffle_variants_fail_where_the_counter_says(pkg):
    p = field_p(pkg)
    usable = (1 << 12) - CI.BLINDING_ROWS
    x, names = CI.merged_shuffle_inputs(p, usable)
    assert sorted(set(collections.Counter(x).values())) == [1, 2, 64, 2049]
    sides = CI.merged_shuffle_sides(p, x, names)
    fails = {name: CI.counter_shuffle_failures(x, y) for name, y in sides.items()}
    assert [int(f.sum()) for f in fails.values()] == [0, 1, 1, 2049 + 64]
    assert x[int(np.nonzero(fails["below every input"])[0][0])] == names["smallest"] and x[int(np.nonzero(fails["above every input"])[0][0])] == names["largest"]
    assert min(sides["below every input"]) < min(x) and max(sides["above every input"]) > max(x) and max(sides["above every input"]) < p


def spill_case(pkg, k=8, q_rows=200):
    p = field_p(pkg)
    cs = CI.spill_cs(pkg, p)
    fixed, good = CI.spill_witness(p, k, q_rows)
    bad = good.copy()
    for col, row in ((0, 3), (CI.SPILL_T, 77), (CI.SPILL_T, q_rows - 1)):      # t_0 on row 3, t_19 on rows 77 and 199
        bad[col, row, 0] ^= np.uint64(1)
    return cs, fixed, good, bad


def test_spill_key_needs_more_slots_than_the_lds_holds(pkg, oracles):
    """The library's graph entry points do not report a program's slot counts, so the allocator is walked by hand: check_inputs.check_program_slots restates
    gate_check_graph's sharing and compile_graph's copy propagation and liveness scan.  All twenty products are live when gate 0 ends: 20 + the running sum."""
    p = field_p(pkg)
    cs, fixed, good, bad = spill_case(pkg)
    slots, calcs, written, read = CI.check_program_slots(cs, p)
    assert slots > CI.LDS_SLOTS and slots >= CI.SPILL_T + 1
    assert any(sl is not None and sl >= CI.LDS_SLOTS for sl in written)            # k_graph_check's EVS_SLOT_HBM store
    assert any(sl >= CI.LDS_SLOTS for rd in read for sl in rd)                     # ... and its load
    assert calcs == CI.SPILL_T + (CI.SPILL_T - 1) + 1 + 2 * CI.SPILL_T + (CI.SPILL_T + 1)      # products, sums, q *, (sub, q *) per gate, roots
    # the walk on a program that does not spill: R5's gate q (a(2) - a(1) - a) (test_rotations) is two differences, a product and the root
    from test_rotations import build_circuit
    assert CI.check_program_slots(build_circuit(pkg, "R5", 6)[0], p)[:2] == (1, 4)
    fails, _ = enumerate_failures(cs, 8, p, fixed, good, None)
    assert not fails
    fails, _ = enumerate_failures(cs, 8, p, fixed, bad, None)
    assert fails == [(GATE, 0, 3), (GATE, 0, 77), (GATE, 0, 199), (GATE, 1, 77), (GATE, 1, 199), (GATE, 20, 3)]


def tables_case(pkg, k=6, T=17):
    n = 1 << k
    cs = CI.tables_cs(pkg, T)
    fixed, good = CI.tables_values(k, T)
    bad = CI.with_cells(good, [(0, 9, 100 * 16 + 3), (15, n - CI.BLINDING_ROWS - 1, 100 * 16 + 1), (16, 0, 2)])      # each a value of ANOTHER group's table
    return cs, fixed, good, bad


def shuffles_case(pkg, k=6, H=9):
    cs = CI.shuffles_cs(pkg, H)
    good = CI.shuffles_values(k, H)
    bad = CI.with_cells(good, [(2 * 0 + 1, 4, 500), (2 * 7 + 1, 0, 7500), (2 * 8 + 1, (1 << k) - CI.BLINDING_ROWS - 1, 1000 * 7 + 1)])
    return cs, good, bad


def test_grouping_closed_forms_are_the_enumerators(pkg, oracles):
    k, n = 6, 64
    usable = n - CI.BLINDING_ROWS
    cs, fixed, good, bad = tables_case(pkg)
    assert len({cs.lookups[l][1][0] for l in range(17)}) == 17
    for adv, rows in ((good, []), (bad, [(LOOKUP, 0, 9), (LOOKUP, 15, usable - 1), (LOOKUP, 16, 0)])):
        want = CI.report_of(CI.tables_bitmap(fixed, adv, usable), (0, 17, 0, 0))
        assert CI.as_tuples(want["failures"]) == rows == enumerated(pkg, cs, k, fixed, adv, None)
    cs, good, bad = shuffles_case(pkg)
    assert len(cs.shuffles) == 9 and not CI.shuffles_bitmap(good, usable).any()
    b = CI.shuffles_bitmap(bad, usable)
    assert sorted(set(np.nonzero(b)[0].tolist())) == [0, 7, 8]
    for h in range(9):
        assert np.array_equal(b[h, :usable], CI.brute_shuffle_failures(bad[2 * h, :usable].tolist(), bad[2 * h + 1, :usable].tolist()))
    # the quarter wave: MIXED at k = 4, closed form against the enumerator and the brute-force count
    shape = (1, 1, 1, 1)
    cs, fixed, asm, witnesses = mixed_case(pkg, 4, shape)
    for adv in witnesses.values():
        fails = enumerated(pkg, cs, 4, fixed, adv, asm.mapping)
        fails += [(SHUFFLE, 0, int(r)) for r in np.nonzero(CI.brute_shuffle_failures(adv[3, :10].tolist(), adv[4, :10].tolist()))[0]]
        assert CI.as_tuples(mixed_want(4, shape, fixed, adv, asm.mapping)["failures"]) == fails


# ============================================================================================================================== GPU
def keygen(pkg, ctx, params, cs, fixed, asm):
    from dehalo2_amd import native
    return native.ProvingKey.keygen(ctx, params, cs, CI.columns(fixed) if np.asarray(fixed).ndim == 2 else fixed, asm, ())


@pytest.fixture(scope="module")
def grid_key(pkg, ctx, kzg_params):
    """one key for every GRID case (the s_i are part of it); the keygen is timed and printed"""
    from dehalo2_amd import plonk as P
    k, S, A = GRID_K, GRID_S, GRID_A
    s, cases = grid_edge_cases()
    cs = CI.grid_cs(pkg, S, A)
    params = kzg_params(k)
    ctx.synchronize()
    t0 = time.perf_counter()
    pk = keygen(pkg, ctx, params, cs, s, P.Assembly(0, 1 << k))
    ctx.synchronize()
    print("\nGRID keygen at k = %d, S = %d, A = %d: %.2f s" % (k, S, A, time.perf_counter() - t0))
    yield dict(pk=pk, s=s, n=1 << k, usable=(1 << k) - CI.BLINDING_ROWS, regions=(S * A, 0, 0, 0))
    pk.release()


def grid_run(pkg, ctx, key, w, cap, want=None):
    want = want or CI.report_of(CI.grid_bitmap(key["s"], w, key["usable"]), key["regions"])
    got = CI.raw_report(pkg, ctx, key["pk"], CI.columns(w), None, cap)
    CI.same(got, want, cap)
    assert (got["rows"], got["lookup_inputs"], got["shuffle_inputs"], got["cells_in_cycles"]) == (key["usable"], 0, 0, 0)
    return want


@pytest.mark.gpu
def test_grid_zero_witness_reports_nothing(pkg, ctx, grid_key):
    w = CI.grid_unusable(GRID_A, grid_key["n"], grid_key["usable"])
    assert w[:, grid_key["usable"]:].all() and grid_key["s"][:, grid_key["usable"]:].all()      # the unusable rows would fail under every gate
    want = grid_run(pkg, ctx, grid_key, w, 64)
    assert len(want["failures"]) == 0


@pytest.mark.gpu
def test_grid_edges(pkg, ctx, grid_key):
    """a failure in the first and the last word of the bitmap, on bits 0 and 63, on both sides of a tile edge inside a bitmap row and of the scan's chunk edge
    (tiles 1023 | 1024): every placement on its own, then all together"""
    _, cases = grid_edge_cases()
    for name, (w, want) in cases.items():
        assert len(want["failures"]) < 1000
        grid_run(pkg, ctx, grid_key, w, 1000, want)


@pytest.mark.gpu
def test_grid_dense_band(pkg, ctx, grid_key):
    """every w_j non-zero on the band: 272 x 10000 failures, full words, tiles whose four waves all hold set bits; the emission of 2^18 crosses 100 tiles"""
    n, usable = grid_key["n"], grid_key["usable"]
    lo, hi = CI.grid_ones(GRID_K)[1]
    w = CI.grid_unusable(GRID_A, n, usable)
    w[:, lo:hi] = 1 + np.arange(hi - lo)[None, :] % 5
    want = CI.report_of(CI.grid_bitmap(grid_key["s"], w, usable), grid_key["regions"])
    assert len(want["failures"]) == GRID_S * GRID_A * (hi - lo) == 2720000
    for cap in (0, 100, CAP_MAX):
        grid_run(pkg, ctx, grid_key, w, cap, want)


@pytest.mark.gpu
def test_grid_medium_density(pkg, ctx, grid_key):
    """about 200 000 failures in all 1088 tiles, all stored: the position of every tile's first failure is its prefix, over both chunks of the scan"""
    n, usable, words = grid_key["n"], grid_key["usable"], grid_key["n"] // 64
    w = CI.grid_random(GRID_K, GRID_A, 0.055, 11)
    want = CI.report_of(CI.grid_bitmap(grid_key["s"], w, usable), grid_key["regions"])
    f = want["failures"]
    tiles = (f["index"].astype(np.int64) * words + f["row"] // 64) // CI.TILE_WORDS
    assert 150000 < len(f) <= CAP_MAX and len(np.unique(tiles)) == GRID_S * GRID_A * words // CI.TILE_WORDS == 1088
    grid_run(pkg, ctx, grid_key, w, CAP_MAX, want)


@pytest.mark.gpu
def test_grid_cap_cuts(pkg, ctx, grid_key):
    """written = min(cap, total), the stored list is the prefix, the totals do not move; one cap ends after two of a word's set bits"""
    n, usable = grid_key["n"], grid_key["usable"]
    w = CI.grid_random(GRID_K, GRID_A, 0.001, 12)
    w[3, 20000:20008] = 1                                    # eight neighbours in the band: a word with eight set bits in every bitmap row i * A + 3
    want = CI.report_of(CI.grid_bitmap(grid_key["s"], w, usable), grid_key["regions"])
    f = want["failures"]
    total = len(f)
    assert 2000 < total < 10000
    word = f["index"].astype(np.int64) * (n // 64) + f["row"] // 64
    inside = next(i for i in range(1, total - 2) if word[i] == word[i + 1] == word[i + 2] and word[i - 1] != word[i]) + 2
    assert word[inside - 1] == word[inside]                  # the cap's last stored failure and the first one left out share a word
    for cap in (1, 63, 64, 65, inside, total - 1, total, total + 1):
        grid_run(pkg, ctx, grid_key, w, cap, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MIXED_SHAPES))
def test_mixed_regions(pkg, ctx, kzg_params, name):
    """k = 12, 64 words per bitmap row.  GLPH: the lookups start at word 192 and the copies at word 320, inside a tile; the shuffles at word 512, the first of
    tile 2.  Without the mapping P = 0 and the shuffles move to word 320.  G-PH: no lookups, bounds[0] == bounds[1].  GLP-: the copies are the last region
    and end in the bitmap's last word (without the mapping: the lookups do), bounds[2] == bounds[3] is read from the last word."""
    k, shape = MIXED_K, MIXED_SHAPES[name]
    G, L, P_, H = shape
    n = 1 << k
    usable, words = n - CI.BLINDING_ROWS, n // 64
    if name == "GLPH":
        assert (G * words, (G + L) * words, (G + L + P_) * words) == (192, 320, 512) and 192 % CI.TILE_WORDS and 320 % CI.TILE_WORDS and 512 % CI.TILE_WORDS == 0
    cs, fixed, asm, witnesses = mixed_case(pkg, k, shape)
    pk = keygen(pkg, ctx, kzg_params(k), cs, fixed, asm)
    try:
        for mapping in (asm.mapping, None):
            for wname, adv in witnesses.items():
                want = mixed_want(k, shape, fixed, adv, mapping)
                total = len(want["failures"])
                assert (total == 0) == (wname == "satisfied" or (mapping is None and wname.startswith("copies"))) and total < 4096
                got = CI.raw_report(pkg, ctx, pk, CI.columns(adv), mapping, 4096)
                CI.same(got, want, 4096)
                assert (got["rows"], got["lookup_inputs"], got["shuffle_inputs"]) == (usable, L * usable, H * usable)
                if wname == "all together":
                    kinds = got["failures"]["kind"].astype(np.int64)
                    present = [kind for kind, cnt in zip((GATE, LOOKUP, COPY, SHUFFLE), (G, L, P_ if mapping is not None else 0, H)) if cnt]
                    assert sorted(set(kinds.tolist())) == present and (np.diff(kinds) >= 0).all()
                    assert all(t > 0 for t, kind in zip(got["totals"], (GATE, LOOKUP, COPY, SHUFFLE)) if kind in present)
                    last_kind, last_index = present[-1], {GATE: G, LOOKUP: L, COPY: P_, SHUFFLE: H}[present[-1]] - 1
                    assert (last_kind, last_index, usable - 1) in CI.as_tuples(want["failures"])      # a failure in the bitmap's last word
                    for cap in (0, 1):
                        CI.same(CI.raw_report(pkg, ctx, pk, CI.columns(adv), mapping, cap), want, cap)
    finally:
        pk.release()


@pytest.mark.gpu
def test_shuffle_over_a_merged_sort(pkg, ctx, kzg_params):
    """k = 12: both sorted sides are two sort tiles and a merge; the 2049-run of equal values crosses the tile edge of the sorted list.  A side value below and
    one above every input; one copy of the 2049-run turned into a copy of the 64-run: all 2113 rows of both runs fail (nine blocks of k_check_shuffle)"""
    from dehalo2_amd import plonk as P
    k, p = 12, field_p(pkg)
    n = 1 << k
    usable = n - CI.BLINDING_ROWS
    cs = CI.shuffles_cs(pkg, 1)
    x, names = CI.merged_shuffle_inputs(p, usable)
    pk = keygen(pkg, ctx, kzg_params(k), cs, np.zeros((1, n), dtype=np.int64), P.Assembly(0, n))
    try:
        totals = []
        for name, y in CI.merged_shuffle_sides(p, x, names).items():
            b = np.zeros((1, n), dtype=bool)
            b[0, :usable] = CI.counter_shuffle_failures(x, y)
            want = CI.report_of(b, (0, 0, 0, 1))
            totals.append(len(want["failures"]))
            got = CI.raw_report(pkg, ctx, pk, CI.int_columns([x + [3] * (n - usable), y + [4] * (n - usable)], n), None, 4096)
            CI.same(got, want, 4096)
            assert got["shuffle_inputs"] == usable
        assert totals == [0, 1, 1, 2113]
    finally:
        pk.release()


@pytest.mark.gpu
def test_spilled_slots_in_the_checking_program(pkg, co, ctx, kzg_params):
    """k_graph_check's EVS_SLOT_HBM stores and loads: the key of test_spill_key_needs_more_slots_than_the_lds_holds (the slot count comes from walking the
    allocator by hand there: the library's graph entry points do not report it), values over the whole field, expected from the enumerator"""
    from dehalo2_amd import native, plonk as P
    k, p = 8, field_p(pkg)
    cs, fixed, good, bad = spill_case(pkg)
    assert CI.check_program_slots(cs, p)[0] > CI.LDS_SLOTS
    pk = native.ProvingKey.keygen(ctx, kzg_params(k), cs, fixed, P.Assembly(0, 1 << k), ())
    try:
        for adv in (good, bad):
            fails, counters = enumerate_failures(cs, k, p, fixed, adv, None)
            assert len(fails) == (0 if adv is good else 6)
            same_report(pk.check_witness(adv, [], assembly=None, canonical=True), fails, counters)
    finally:
        pk.release()


@pytest.mark.gpu
def test_seventeen_tables(pkg, ctx, kzg_params):
    """check_body sorts sixteen tables a call: table 16 is a second call, whose output takes the place of the first's.  The broken inputs of lookups 0 and 15
    hold a value of table 16, that of lookup 16 a value of table 0: a search in the other group's sorted table would find them"""
    from dehalo2_amd import plonk as P
    k, n = 6, 64
    cs, fixed, good, bad = tables_case(pkg)
    pk = keygen(pkg, ctx, kzg_params(k), cs, fixed, P.Assembly(0, n))
    try:
        for adv in (good, bad):
            fails, counters = enumerate_failures(cs, k, field_p(pkg), CI.columns(fixed), CI.columns(adv), None)
            assert fails == ([] if adv is good else [(LOOKUP, 0, 9), (LOOKUP, 15, 57), (LOOKUP, 16, 0)])
            same_report(pk.check_witness(CI.columns(adv), [], assembly=None, canonical=True), fails, counters)
    finally:
        pk.release()


@pytest.mark.gpu
def test_nine_shuffles(pkg, ctx, kzg_params):
    """check_body sorts eight shuffles' sides a call: shuffle 8 is a second call"""
    from dehalo2_amd import plonk as P
    k, n = 6, 64
    usable = n - CI.BLINDING_ROWS
    cs, good, bad = shuffles_case(pkg)
    pk = keygen(pkg, ctx, kzg_params(k), cs, np.zeros((1, n), dtype=np.int64), P.Assembly(0, n))
    try:
        for adv in (good, bad):
            want = CI.report_of(CI.shuffles_bitmap(adv, usable), (0, 0, 0, 9))
            assert sorted(set(want["failures"]["index"].tolist())) == ([] if adv is good else [0, 7, 8])
            got = CI.raw_report(pkg, ctx, pk, CI.columns(adv), None, 256)
            CI.same(got, want, 256)
            assert got["shuffle_inputs"] == 9 * usable
    finally:
        pk.release()


@pytest.mark.gpu
def test_a_quarter_wave(pkg, ctx, kzg_params):
    """k = 4: 16 rows, 10 usable -- every checking kernel runs a quarter of one wave.  One gate, one lookup, one permutation column, one shuffle; a failure
    on the last usable row of every region, alone and together"""
    k, shape = 4, (1, 1, 1, 1)
    cs, fixed, asm, witnesses = mixed_case(pkg, k, shape)
    pk = keygen(pkg, ctx, kzg_params(k), cs, fixed, asm)
    try:
        for wname, adv in witnesses.items():
            want = mixed_want(k, shape, fixed, adv, asm.mapping)
            if wname.endswith("last"):
                assert 9 in want["failures"]["row"].tolist()
            got = CI.raw_report(pkg, ctx, pk, CI.columns(adv), asm.mapping, 64)
            CI.same(got, want, 64)
            assert got["rows"] == 10
        assert sorted(set(got["failures"]["kind"].tolist())) == [GATE, LOOKUP, COPY, SHUFFLE]
    finally:
        pk.release()
