"""Circuit families for dehalo_check_witness (csrc/check.hip, csrc/check.cuh) whose failure set is written down in closed form, and the call through the C ABI.

The checker's report is one bitmap in (kind, index, row) order: a bitmap row of ceil(n / 64) words per gate polynomial, lookup, permutation column and shuffle,
counted and emitted in tiles of 256 words and scanned in chunks of 1024 tiles.  The families here are built so that the bitmap is a boolean numpy array computed
straight from the inputs -- no expression is evaluated --, which makes reports of millions of failures cheap to state:

    GRID    S fixed columns s_i, A advice columns w_j, one gate s_i * w_j per pair: gate i * A + j fails at row r iff s_i[r] != 0 and w_j[r] != 0 and r < usable
    MIXED   G gates q * g_m, L lookups b_l in t, P permutation columns, H shuffles x_h ~ y_h: all four regions of the bitmap in one key
    SPILL   twenty products live across twenty-one gates: a checking program whose slots do not fit the LDS budget (expected from the enumerator, not closed)

A plain helper, imported like tests/lookup_inputs.py.  All values are canonical integers.

    cs, s = grid_cs(pkg, S, A), grid_fixed(k, S)      want = report_of(grid_bitmap(s, w, usable), (S * A, 0, 0, 0))
    got = raw_report(pkg, ctx, pk, columns(w), None, cap)       same(got, want, cap)
"""
import collections
import ctypes as C

import numpy as np

GATE, LOOKUP, COPY, SHUFFLE = 0, 1, 2, 3
FAILURE = np.dtype([("kind", "<u4"), ("index", "<u4"), ("row", "<u4"), ("reserved", "<u4")])      # dehalo_check_failure
TILE_WORDS, CHUNK_TILES = 256, 1024                                                                # CK_THREADS of check.hip; k_check_scan's trip
BLINDING_ROWS = 6                                                                                  # every column here is queried once: blinding_factors() + 1


# ---- the report ---------------------------------------------------------------------------------------------------------------------------------------------
def columns(values):
    """(columns, n) small non-negative integers -> (columns, n, 4) u64 canonical"""
    v = np.asarray(values, dtype=np.uint64)
    out = np.zeros(v.shape + (4,), dtype=np.uint64)
    out[..., 0] = v
    return out


def report_of(bitmap, regions):
    """bitmap: bool (R, n), the bitmap rows in the checker's order; regions = (G, L, P, H) with G + L + P + H == R.
    -> dict(failures: FAILURE array in (kind, index, row) order, totals: (gate, lookup, copy, shuffle))"""
    bitmap = np.asarray(bitmap, dtype=bool)
    assert bitmap.ndim == 2 and bitmap.shape[0] == sum(regions)
    at = np.argwhere(bitmap)                                                                       # row-major: (bitmap row, row) ascending
    starts = np.cumsum((0,) + tuple(regions))
    kind = np.searchsorted(starts[1:], at[:, 0], side="right")
    out = np.zeros(at.shape[0], dtype=FAILURE)
    out["kind"], out["index"], out["row"] = kind, at[:, 0] - starts[kind], at[:, 1]
    totals = tuple(int(np.count_nonzero(kind == x)) for x in (GATE, LOOKUP, COPY, SHUFFLE))
    return dict(failures=out, totals=totals)


def as_tuples(failures):
    return [(int(f["kind"]), int(f["index"]), int(f["row"])) for f in failures]


def from_tuples(fails, regions=None):
    """the enumerator's [(kind, index, row)] -> report_of's dict"""
    out = np.zeros(len(fails), dtype=FAILURE)
    for i, (kind, index, row) in enumerate(fails):
        out[i] = (kind, index, row, 0)
    return dict(failures=out, totals=tuple(sum(1 for f in fails if f[0] == x) for x in (GATE, LOOKUP, COPY, SHUFFLE)))


def raw_report(pkg, ctx, pk, advice, mapping, cap):
    """dehalo_check_witness itself over canonical host advice; the failure array is a numpy structured array the library writes into (no Python list).
    The array is one entry longer than `cap` and filled with ones: what the library leaves untouched is seen to be untouched."""
    from dehalo2_amd import native
    from dehalo2_amd._lib import CCheckFailure, CCheckReport
    adv = np.ascontiguousarray(advice, dtype=np.uint64)
    m = None if mapping is None else np.ascontiguousarray(getattr(mapping, "mapping", mapping), dtype=np.uint64).reshape(-1)
    buf = np.zeros(cap + 1, dtype=FAILURE)
    buf.view(np.uint32)[:] = 0xFFFFFFFF
    ptrs, lens = (C.c_void_p * 1)(), (C.c_size_t * 1)()
    rep = CCheckReport()
    rc = pkg.load_library().dehalo_check_witness(ctx.handle, pk.handle, adv.ctypes.data, ptrs, lens, 0, None if m is None else m.ctypes.data, native.PROOF_ADVICE_CANONICAL,
                                                 C.cast(buf.ctypes.data, C.POINTER(CCheckFailure)) if cap else None, cap, C.byref(rep))
    assert rc == 0, rc
    written = int(rep.written)
    assert written <= cap and (buf[written:].view(np.uint32) == 0xFFFFFFFF).all()
    return dict(failures=buf[:written], written=written, totals=(int(rep.gate_failures), int(rep.lookup_failures), int(rep.copy_failures), int(rep.shuffle_failures)),
                rows=int(rep.rows), lookup_inputs=int(rep.lookup_inputs), shuffle_inputs=int(rep.shuffle_inputs), cells_in_cycles=int(rep.cells_in_cycles))


def same(got, want, cap):
    """the device's report is the expected one: the totals whatever the cap, written = min(cap, total), the stored failures the first `written` in order"""
    total = len(want["failures"])
    assert got["totals"] == want["totals"], (got["totals"], want["totals"])
    assert got["written"] == min(cap, total), (got["written"], cap, total)
    g, w = got["failures"], want["failures"][:got["written"]]
    if not np.array_equal(g, w):
        bad = next(i for i in range(len(w)) if g[i] != w[i])
        raise AssertionError("failure %d of %d: got %r, want %r" % (bad, len(w), g[bad], w[bad]))


def tile_of(words, bitmap_row, row):
    """the tile of the count / emit kernels that holds the bit (bitmap_row, row)"""
    return (bitmap_row * words + row // 64) // TILE_WORDS


# ---- GRID ---------------------------------------------------------------------------------------------------------------------------------------------------
def grid_cs(pkg, S, A):
    from dehalo2_amd import plonk as P
    cs = P.ConstraintSystem(num_advice=A, num_fixed=S, num_instance=0)
    s, w = [cs.query_fixed(i) for i in range(S)], [cs.query_advice(j) for j in range(A)]
    for i in range(S):
        cs.create_gate([P.mul(s[i], w[j]) for j in range(A)])
    assert all(cs.gates[i * A + j] == ("product", ("fixed", i, 0), ("advice", j, 0)) for i in range(S) for j in range(A))      # gate i * A + j is s_i * w_j
    assert cs.blinding_factors() + 1 == BLINDING_ROWS and cs.degree() == 3
    return cs


def grid_ones(k):
    """the row intervals on which EVERY s_i is 1: sixteen rows around the first tile edge inside a bitmap row (row 16384; n / 4 below k = 16), a band
    (rows 20000 .. 29999 at k = 16), and the last rows from a multiple of 16 on -- the last ten usable rows and the six unusable ones"""
    n = 1 << k
    edge = min(16384, n // 4)
    band = (20000, 30000) if k == 16 else (5 * n // 16, 15 * n // 32)
    return [(edge - 8, edge + 8), band, (n - 16, n)]


def grid_fixed(k, S):
    """s[i, r] = 1 iff r % S == i, or r lies in one of grid_ones(k)'s intervals"""
    n = 1 << k
    r = np.arange(n)
    s = (r[None, :] % S == np.arange(S)[:, None]).astype(np.int64)
    for lo, hi in grid_ones(k):
        s[:, lo:hi] = 1
    return s


def grid_bitmap(s, w, usable):
    """gate (i, j) fails at row r iff s_i[r] != 0 and w_j[r] != 0 and r < usable -> bool (S * A, n), bitmap row i * A + j"""
    S, n = s.shape
    A = w.shape[0]
    b = (s[:, None, :] != 0) & (w[None, :, :] != 0)
    b[:, :, usable:] = False
    return b.reshape(S * A, n)


def grid_unusable(A, n, usable):
    """w: zero on the usable rows, non-zero on the others (where every s_i is 1 too): the base of every GRID witness"""
    w = np.zeros((A, n), dtype=np.int64)
    w[:, usable:] = 7 + np.arange(A)[:, None]
    return w


def grid_edges(k, S, A):
    """-> {name: ([(advice column, row)], (bitmap row, row) that must then fail)}: cells to make non-zero, one placement per edge of the report pipeline"""
    n = 1 << k
    usable, words = n - BLINDING_ROWS, n // 64
    last = usable - 1
    tile_rows = TILE_WORDS * 64
    assert words % TILE_WORDS == 0 and last >= n - 16 and last % 64 not in (0, 63)
    hi = CHUNK_TILES * TILE_WORDS // words                   # the first bitmap row of the scan's second chunk
    assert 0 < hi < S * A and (CHUNK_TILES * TILE_WORDS) % words == 0
    edge = grid_ones(k)[0][0] + 8
    assert edge % tile_rows == 0 and 0 < edge < n
    top = (S - 1) * A + A - 1
    low = next(r for r in range(64) if r % S == hi // A)
    return {
        "first word, bit 0": ([(0, 0)], (0, 0)),
        "bit 63": ([(2, 63)], ((63 % S) * A + 2, 63)),
        "last word of the bitmap": ([(A - 1, last)], (top, last)),
        "last word of a tile": ([(3, edge - 1)], (1 * A + 3, edge - 1)),
        "first word of the next tile": ([(3, edge)], (1 * A + 3, edge)),
        "last row before the second chunk": ([((hi - 1) % A, last)], (hi - 1, last)),
        "first word of the second chunk": ([(hi % A, low)], (hi, low)),
    }


def grid_witness(A, n, usable, cells, value=1):
    w = grid_unusable(A, n, usable)
    for j, r in cells:
        w[j, r] = value
    return w


def grid_random(k, A, density, seed):
    """w non-zero with probability `density` on every row (values 1 .. 999), the unusable rows non-zero"""
    n = 1 << k
    rng = np.random.default_rng(seed)
    w = np.where(rng.random((A, n)) < density, rng.integers(1, 1000, size=(A, n)), 0).astype(np.int64)
    w[:, n - BLINDING_ROWS:] = 7
    return w


# ---- MIXED --------------------------------------------------------------------------------------------------------------------------------------------------
TABLE = 8      # the lookups' table holds 0 .. TABLE - 1


def mixed_cs(pkg, G, L, P_, H):
    """advice: g_0 .. g_(G-1) | b_0 .. b_(L-1) | c_0 .. c_(P-1) | x_0, y_0, .. ; fixed: q (all ones), t (r % TABLE).
    gate m: q g_m; lookup l: b_l in t; permutation columns c_*; shuffle h: x_h ~ y_h"""
    from dehalo2_amd import plonk as P
    cs = P.ConstraintSystem(num_advice=G + L + P_ + 2 * H, num_fixed=2, num_instance=0)
    q, t = cs.query_fixed(0), cs.query_fixed(1)
    cs.create_gate([P.mul(q, cs.query_advice(m)) for m in range(G)])
    for l in range(L):
        cs.lookup([(cs.query_advice(G + l), t)])
    for c in range(P_):
        cs.enable_equality(P.ADVICE, G + L + c)
    for h in range(H):
        cs.shuffle([(cs.query_advice(G + L + P_ + 2 * h), cs.query_advice(G + L + P_ + 2 * h + 1))])
    assert cs.blinding_factors() + 1 == BLINDING_ROWS
    return cs


def mixed_fixed(k):
    n = 1 << k
    return np.stack([np.ones(n, dtype=np.int64), np.arange(n) % TABLE])


def mixed_assembly(pkg, k, P_):
    """copies on the first and the last usable row, inside a column, between columns, and one into an unusable row"""
    from dehalo2_amd import plonk as P
    n = 1 << k
    last = n - BLINDING_ROWS - 1
    asm = P.Assembly(P_, n)
    if P_:
        asm.copy(0, 0, P_ - 1, last)             # first column's first row = last column's last usable row
        asm.copy(0, 1, 0, 2)
        asm.copy(P_ - 1, 0, P_ - 1, n - 1)       # ... and an unusable row
        if P_ > 1:
            asm.copy(1, 3, 0, last)
            asm.copy(1, 4, P_ - 1, 5)
    return asm


def mixed_satisfied(k, G, L, P_, H, seed=1):
    """(num_advice, n) integers that satisfy everything: g = 0; b in the table; c constant 5 (every copy holds); y a permutation of x over the usable rows.
    The unusable rows hold values that would fail everywhere."""
    n = 1 << k
    usable = n - BLINDING_ROWS
    rng = np.random.default_rng(seed)
    adv = np.zeros((G + L + P_ + 2 * H, n), dtype=np.int64)
    for l in range(L):
        adv[G + l, :usable] = rng.integers(0, TABLE, size=usable)
    adv[G + L:G + L + P_, :] = 5
    for h in range(H):
        x = rng.integers(0, max(2, usable // 3), size=usable) + 1000
        adv[G + L + P_ + 2 * h, :usable] = x
        adv[G + L + P_ + 2 * h + 1, :usable] = x[rng.permutation(usable)]
    adv[:G + L, usable:] = 999
    adv[G + L + P_:, usable:] = 777 + np.arange(n - usable)
    adv[G + L + P_ + 1::2, usable:] += 100
    return adv


def counter_shuffle_failures(x, y):
    """a usable row fails when its input occurs a different number of times among the usable inputs and on the usable shuffle side -> bool per row.
    x, y: the usable rows' tuples (or values), as lists"""
    cx, cy = collections.Counter(x), collections.Counter(y)
    return np.array([cx[v] != cy[v] for v in x], dtype=bool)


def brute_shuffle_failures(x, y):
    """the same, by counting: O(u^2)"""
    return np.array([sum(1 for a in x if a == v) != sum(1 for b in y if b == v) for v in x], dtype=bool)


def mixed_bitmap(k, G, L, P_, H, fixed, adv, mapping):
    """the closed form: bool (G + L + P + H, n).  mapping None: the copies are not checked and have no bitmap rows"""
    n = 1 << k
    usable = n - BLINDING_ROWS
    q, t = fixed
    rows = []
    for m in range(G):
        rows.append((q != 0) & (adv[m] != 0))
    for l in range(L):
        rows.append(~np.isin(adv[G + l], t[:usable]))
    for b in rows:
        b[usable:] = False
    if mapping is not None:
        m = np.asarray(mapping, dtype=np.int64).reshape(-1)
        flat = adv[G + L:G + L + P_].reshape(-1)
        rows += list((flat != flat[m]).reshape(P_, n))                # (every cell of a cycle, the unusable rows' among them)
    for h in range(H):
        x, y = adv[G + L + P_ + 2 * h, :usable].tolist(), adv[G + L + P_ + 2 * h + 1, :usable].tolist()
        b = np.zeros(n, dtype=bool)
        b[:usable] = counter_shuffle_failures(x, y)
        rows.append(b)
    return np.stack(rows) if rows else np.zeros((0, n), dtype=bool)


def mixed_breaks(k, G, L, P_, H):
    """-> {name: [(advice column, row, value)]}: one broken cell on the first and on the last usable row of every region that exists"""
    last = (1 << k) - BLINDING_ROWS - 1
    out = {}
    if G:
        out["gates first"], out["gates last"] = [(0, 0, 3)], [(G - 1, last, 3)]
    if L:
        out["lookups first"], out["lookups last"] = [(G, 0, TABLE)], [(G + L - 1, last, 500)]
    if P_:
        out["copies first"], out["copies last"] = [(G + L, 0, 6)], [(G + L + P_ - 1, last, 9)]
    if H:
        out["shuffles first"], out["shuffles last"] = [(G + L + P_, 0, 11)], [(G + L + P_ + 2 * H - 2, last, 12)]
    return out


def with_cells(adv, cells):
    out = adv.copy()
    for col, row, v in cells:
        out[col, row] = v
    return out


# ---- shuffles over a merged sort ------------------------------------------------------------------------------------------------------------------------------
def merged_shuffle_inputs(p, usable, seed=9):
    """-> (x: the usable rows' inputs as ints in a seeded order, names): singles, ten pairs, one run of 64 and one of 2049.  The smallest input is 5, the largest
    p - 2; the 2049-run's value lies above 1000 singles, the pairs and the 64-run, so in the sorted list it covers the indices 1084 .. 3132 and crosses the
    sort's tile edge at 2048"""
    assert usable >= 2049 + 64 + 20 + 1100
    singles = usable - 2049 - 64 - 20
    low = [5 + 3 * i for i in range(1000)]                                     # 5 .. 3002
    big, run64 = 1 << 200, (1 << 130) + 1
    pairs = [(1 << 64) + i for i in range(10)]
    high = [(1 << 250) + 7 * i for i in range(singles - 1001)] + [p - 2]
    vals = low + [big] * 2049 + [run64] * 64 + [v for v in pairs for _ in (0, 1)] + high
    assert len(vals) == usable and len(set(low + high)) == singles and max(vals) == p - 2 and min(vals) == 5
    srt = sorted(vals)
    assert srt.index(big) == 1084 and srt[1084 + 2048] == big and srt[2047] == srt[2048] == big
    order = np.random.default_rng(seed).permutation(usable).tolist()
    return [vals[i] for i in order], dict(big=big, run64=run64, smallest=5, largest=p - 2)


def merged_shuffle_sides(p, x, names, seed=10):
    """-> {variant: the usable rows' shuffle side}"""
    usable = len(x)
    perm = [x[i] for i in np.random.default_rng(seed).permutation(usable).tolist()]

    def replaced(old, new):
        y = list(perm)
        y[y.index(old)] = new
        return y
    return {"permutation": perm, "below every input": replaced(names["smallest"], 2), "above every input": replaced(names["largest"], p - 1),
            "2049-run loses one to the 64-run": replaced(names["big"], names["run64"])}


def int_columns(cols, n):
    """[[int]] (each at most n long, any size below 2^256) -> (columns, n, 4) u64"""
    from test_check_witness import limbs
    return np.stack([limbs(col, n) for col in cols])


# ---- SPILL --------------------------------------------------------------------------------------------------------------------------------------------------
SPILL_T = 20
LDS_SLOTS = 13      # EVH_MAX_LDS_SLOTS of csrc/evalh_types.hpp


def spill_constants(p, seed=21):
    """c_1 .. c_20 over the whole field with c_1 + .. + c_20 = 0 (gate 0 is the sum of all t_j, gate m fixes t_(20 - m) = c_m)"""
    import random
    rnd = random.Random(seed)
    c = [rnd.randrange(1, p) for _ in range(SPILL_T - 1)]
    c.append(-sum(c) % p)
    assert c[-1] != 0
    return [None] + c


def spill_cs(pkg, p):
    """21 advice w_j, one fixed q; t_j = w_j w_(j+1); gate 0: q (((t_0 + t_1) + t_2) + .. + t_19); gate m = 1 .. 20: q (t_(20 - m) - c_m)"""
    from dehalo2_amd import plonk as P
    cs = P.ConstraintSystem(num_advice=SPILL_T + 1, num_fixed=1, num_instance=0)
    q = cs.query_fixed(0)
    w = [cs.query_advice(j) for j in range(SPILL_T + 1)]
    t = [P.mul(w[j], w[j + 1]) for j in range(SPILL_T)]
    c = spill_constants(p)
    cs.create_gate([P.mul(q, P.sum_(*t))] + [P.mul(q, P.sum_(t[SPILL_T - m], ("neg", ("const", c[m])))) for m in range(1, SPILL_T + 1)])
    assert cs.blinding_factors() + 1 == BLINDING_ROWS
    return cs


def spill_witness(p, k, q_rows, seed=22):
    """-> (fixed (1, n, 4), advice (21, n, 4)) satisfied: on every row w_0 is drawn over the field and w_(j+1) = c_(20 - j) / w_j, so t_j = c_(20 - j)"""
    import random
    rnd = random.Random(seed)
    n = 1 << k
    c = spill_constants(p)
    cols = [[0] * n for _ in range(SPILL_T + 1)]
    for r in range(n):
        cols[0][r] = rnd.randrange(1, p)
        for j in range(SPILL_T):
            cols[j + 1][r] = c[SPILL_T - j] * pow(cols[j][r], -1, p) % p if r < q_rows else rnd.randrange(p)
    return int_columns([[1] * q_rows], n), int_columns(cols, n)


def check_program_slots(cs, p):
    """The slots of the key's checking program, by walking the library's two steps by hand on the constraint system's expression tuples:
    plonk_host.hpp gate_check_graph (GraphBuilder::add_expression with its shared subexpressions, one root Store per gate polynomial) and capi.hip
    compile_graph (copy propagation of the column Stores, then the liveness scan: a slot is reused once its value was read for the last time, the lowest
    free slot first).  -> (slots in all, calculations after copy propagation, [slot written by every calculation], [slots read by every calculation]).
    Handles the nodes the families here use: const, fixed, advice, neg, sum, product."""
    consts, calcs, n_int = [0, 1, 2], [], [0]
    ZERO, ONE, TWO = ("c", 0), ("c", 1), ("c", 2)

    def const(v):
        v %= p
        if v not in consts:
            consts.append(v)
        return ("c", consts.index(v))

    def calc(op, a, b=ZERO):
        for c in calcs:
            if c[:3] == (op, a, b) and not c[4]:
                return ("i", c[3])
        calcs.append((op, a, b, n_int[0], False))
        n_int[0] += 1
        return ("i", n_int[0] - 1)

    def expr(e):
        kind = e[0]
        if kind == "const":
            return const(e[1])
        if kind in ("fixed", "advice"):
            return calc("store", ("col",) + tuple(e))
        if kind == "neg":
            if e[1][0] == "const":
                return const(-e[1][1])
            a = expr(e[1])
            return a if a == ZERO else calc("neg", a)
        if kind == "sum":
            if e[2][0] == "neg":
                a, b = expr(e[1]), expr(e[2][1])
                return calc("neg", b) if a == ZERO else (a if b == ZERO else calc("sub", a, b))
            a, b = expr(e[1]), expr(e[2])
            return b if a == ZERO else (a if b == ZERO else calc("add", *sorted((a, b))))
        if kind == "product":
            a, b = expr(e[1]), expr(e[2])
            if ZERO in (a, b):
                return ZERO
            if ONE in (a, b):
                return b if a == ONE else a
            if TWO in (a, b):
                return calc("double", b if a == TWO else a)
            return calc("square", a) if a == b else calc("mul", *sorted((a, b)))
        raise ValueError(kind)

    for g in cs.gates:
        r = expr(g)
        calcs.append(("store", r, ZERO, n_int[0], True))      # the root: a calculation of its own, never shared
        n_int[0] += 1
    # copy propagation: a Store of a column (or constant) that is no root and not the last calculation is dropped, its readers read the source
    alias, kept = {}, []
    for i, (op, a, b, target, root) in enumerate(calcs):
        a, b = alias.get(a, a), alias.get(b, b)
        if op == "store" and not root and a[0] != "i" and i + 1 != len(calcs):
            alias[("i", target)] = a
            continue
        kept.append((op, a, b, target, root))
    binary = ("add", "sub", "mul")
    reads = [[s[1] for s in ((a, b) if op in binary else (a,)) if s[0] == "i"] for op, a, b, _, _ in kept]
    last_use = {}
    for i, rs in enumerate(reads):
        for v in rs:
            last_use[v] = i
    last_use[kept[-1][3]] = len(kept)
    dying = collections.defaultdict(list)
    for v, at in last_use.items():
        dying[at].append(v)
    slot_of, free, nxt, written, read = {}, [], 0, [], []
    for i, (op, a, b, target, root) in enumerate(kept):
        read.append([slot_of[v] for v in reads[i]])
        for v in dying[i]:
            if v in slot_of and v != target:
                free.append(slot_of.pop(v))
        if target not in slot_of:
            if free:
                slot_of[target] = min(free)
                free.remove(slot_of[target])
            else:
                slot_of[target] = nxt
                nxt += 1
        sl = slot_of[target]
        written.append(None if root else sl)                  # (k_graph_check ballots a root's value and stores it nowhere)
        if last_use.get(target, -1) <= i and i + 1 != len(kept):
            free.append(sl)
            del slot_of[target]
    return nxt, len(kept), written, read


# ---- grouping loops -----------------------------------------------------------------------------------------------------------------------------------------
def tables_cs(pkg, T):
    """T single-expression lookups a_l in t_l over T distinct fixed table columns (check_body sorts the tables sixteen a call)"""
    from dehalo2_amd import plonk as P
    cs = P.ConstraintSystem(num_advice=T, num_fixed=T, num_instance=0)
    for l in range(T):
        cs.lookup([(cs.query_advice(l), cs.query_fixed(l))])
    assert cs.blinding_factors() + 1 == BLINDING_ROWS
    return cs


def tables_values(k, T):
    """table l holds 100 l + (0 .. 9) over the usable rows (and 100 l + 50, no entry, on the unusable ones); input l walks its table.  No table holds a value of
    another: a search in the wrong sorted table misses on every row.  -> (fixed, advice) as (T, n) integers"""
    n = 1 << k
    usable = n - BLINDING_ROWS
    r = np.arange(n)
    fixed = 100 * np.arange(T)[:, None] + (r[None, :] % 10)
    fixed[:, usable:] = 100 * np.arange(T)[:, None] + 50
    adv = 100 * np.arange(T)[:, None] + ((3 * r[None, :] + np.arange(T)[:, None]) % 10)
    return fixed.astype(np.int64), adv.astype(np.int64)


def tables_bitmap(fixed, adv, usable):
    T, n = adv.shape
    b = np.stack([~np.isin(adv[l], fixed[l, :usable]) for l in range(T)])
    b[:, usable:] = False
    return b


def shuffles_cs(pkg, H):
    """H shuffles x_h ~ y_h (check_body sorts eight shuffles' sides a call)"""
    from dehalo2_amd import plonk as P
    cs = P.ConstraintSystem(num_advice=2 * H, num_fixed=1, num_instance=0)
    for h in range(H):
        cs.shuffle([(cs.query_advice(2 * h), cs.query_advice(2 * h + 1))])
    assert cs.blinding_factors() + 1 == BLINDING_ROWS
    return cs


def shuffles_values(k, H):
    """x_h = 1000 h + (r % 7) over the usable rows, y_h = x_h reversed; zero on the unusable rows -> (2 H, n) integers"""
    n = 1 << k
    usable = n - BLINDING_ROWS
    adv = np.zeros((2 * H, n), dtype=np.int64)
    for h in range(H):
        x = 1000 * h + (np.arange(usable) * (h + 2)) % 7
        adv[2 * h, :usable], adv[2 * h + 1, :usable] = x, x[::-1]
    return adv


def shuffles_bitmap(adv, usable):
    H, n = adv.shape[0] // 2, adv.shape[1]
    b = np.zeros((H, n), dtype=bool)
    for h in range(H):
        b[h, :usable] = counter_shuffle_failures(adv[2 * h, :usable].tolist(), adv[2 * h + 1, :usable].tolist())
    return b
