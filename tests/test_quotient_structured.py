"""The quotient-numerator kernels (csrc/evalh.cuh: k_graph_eval, k_graph_eval_batch, k_perm_h, k_lookup_h, k_lookup_h_batch, k_product_terms) on structured
values and at their launch edges (tests/quotient_inputs.py).  The parity tests run them on uniform columns at one geometry each; uniform values never make two
operands equal, zero or p - 1 -- the normal case on a real proof -- and one full workgroup never reaches a partial block, a second block's spill index, a
rotation across a block boundary, the batch's second staging region or the slow staging path.

CPU (no mark): oracle/pyoracle.py equals the C restatement on every input family and on a subset of the geometries, and the closed forms (a satisfied argument
folds only zeros: values * y^terms; the empty program; the single operations) hold in plain integers -- the reference is pinned before a kernel is judged by it.
GPU: exact equality of canonical integers with pyoracle (k_product_terms: with Python integers), outputs written over a non-zero pattern.

The edge set E (45 values): 0, 1, 2, p-1, p-2, (p-1)/2, (p+1)/2; x with x * 2^261 mod p in {1, p-1, 2^(29j) - 1, 2^(29j): j = 1..8} and their negatives; x with
x * 2^256 mod p in {1, p-1}; two uniform values."""
import numpy as np
import pytest

import quotient_inputs as QI
import structured_inputs as SI

POISON = 0x5A5A5A5A5A5A5A5A
GEOMETRY_FIELDS = ["bn254_fr", "pasta_fp"]
GRAPH_LOGS = [0, 3, 6, 7, 8, 10]
GRAPH_ROT_SCALES = [1, 4, 8]
LIVE = [1, 10, 11, 13, 14, 20]      # 10: the last size within 48 KiB of LDS, 11: the first that needs the attribute; 13: the last all-LDS size, 14: the first HBM slot
_REF = {}


def _ref(key, fn):
    """a reference is computed once and shared by the CPU and the GPU tests"""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _graph_ref(po, F, key, g, env, rows, rot_scale, previous=None):
    return _ref(("graph", F.name) + key, lambda: po.graph_evaluate(F.of, g, env, rows, rot_scale, previous))


def _co_graph(co, F, g, env, log_rows, rot_scale, previous=None):
    e1 = lambda v: F.enc1(v or 0)
    return co.graph_evaluate(F.fid, F.enc(g["constants"]), g["rotations"], g["calcs"], g["num_intermediates"], [F.enc(c) for c in env["fixed"]],
                             [F.enc(c) for c in env["advice"]], [F.enc(c) for c in env["instance"]], F.enc(env["challenges"]), e1(env["beta"]), e1(env["gamma"]),
                             e1(env["theta"]), e1(env["y"]), log_rows, rot_scale, F.enc(previous) if previous is not None else None, 2)


# ---------------------------------------------------------------- the cases, shared by the CPU and the GPU tests
def pair_case(po, fname):
    """-> (env, log_rows, {name: graph}, the spill / PREVIOUS program, its previous column = -A)"""
    F = SI.field(po, fname)
    A, B, log_rows = _ref(("pairs", fname), lambda: QI.pair_columns(po, F))
    env = {"fixed": [], "advice": [A, B], "instance": [], "challenges": [], "beta": 0, "gamma": 0, "theta": 0, "y": 0}
    return env, log_rows, QI.op_programs(po), QI.spill_previous_program(po), [(-a) % F.p for a in A]


def pair_closed_forms(F, A, B):
    """what the single operations make of (A, B), in plain integers"""
    p = F.p
    zero = [0] * len(A)
    out = {"add": [(a + b) % p for a, b in zip(A, B)], "sub": [(a - b) % p for a, b in zip(A, B)], "mul": [a * b % p for a, b in zip(A, B)],
           "square": [a * a % p for a in A], "double": [2 * a % p for a in A], "negate": [(-a) % p for a in A], "store": list(A),
           "horner": [(((a * b + a) * b + b) * b * b + 1) % p for a, b in zip(A, B)], "neg_of_sub_self": zero, "neg_plus_self": zero,
           "zero_minus_b": [(-b) % p for b in B], "b_minus_zero": list(B)}
    for name in ("zero_mul", "zero_mul_self", "zero_square", "zero_double", "zero_negate", "zero_add_self", "zero_store", "zero_horner"):
        out[name] = zero
    return out


def rotation_group(po, fname, log_rows):
    F, rows = SI.field(po, fname), 1 << log_rows
    env = _ref(("env", fname, "rot", log_rows), lambda: QI.uniform_env(po, F, rows, 2, 2, 1, 1, 0x3000 + log_rows))
    g = QI.rotation_program(po, rows)
    return env, [(("rot", log_rows, rs), g, rs, None) for rs in GRAPH_ROT_SCALES]


def live_group(po, fname, log_rows, sizes=LIVE):
    F, rows = SI.field(po, fname), 1 << log_rows
    env = _ref(("env", fname, "live", log_rows), lambda: QI.uniform_env(po, F, rows, 1, 1, 1, 0, 0x3100 + log_rows))
    cases = [(("live", log_rows, L), QI.live_program(po, rows, L), 4, None) for L in sizes]
    if 14 in sizes:
        cases.append((("live", log_rows, "14 in place"), QI.live_program(po, rows, 14, True), 4, None))
    return env, cases


HAND_LOG = 8


def handwritten_group(po, fname):
    F, rows = SI.field(po, fname), 1 << HAND_LOG
    env = _ref(("env", fname, "hand"), lambda: QI.uniform_env(po, F, rows, 1, 2, 1, 1, 0x3200))
    previous = _ref(("prev", fname, "hand"), lambda: QI.uniform(po, F, rows, 0x3201))
    cases = [(("hand", name), g, 2, None) for name, g in QI.handwritten_programs(po, rows).items()]
    cases.append((("hand", "reads_previous", "given"), QI.handwritten_programs(po, rows)["reads_previous"], 2, previous))
    return env, cases


STAGING = [(2, 2, 1, 12), (2, 2, 1, 13), (20, 20, 0, 2), (20, 20, 1, 2)]      # 12 / 13 challenges and 40 / 41 columns: the last one-launch staging, the first slow one
STAGING_LOG = 8


def staging_group(po, fname, shape):
    F = SI.field(po, fname)
    nf, na, ni, nchal = shape
    env = _ref(("env", fname, "stage", shape), lambda: QI.uniform_env(po, F, 1 << STAGING_LOG, nf, na, ni, nchal, 0x3300 + nf + nchal + ni))
    return env, [(("stage", shape), QI.staging_program(po, nf, na, ni, nchal), 2, None)]


BATCH_LOG = 8


def batch_env(po, fname, nchal=2):
    F = SI.field(po, fname)
    return _ref(("env", fname, "batch", nchal), lambda: QI.uniform_env(po, F, 1 << BATCH_LOG, *QI.BATCH_ENV, nchal, 0x3400 + nchal))


def batch_calls(po, fname):
    """-> [(label, env, [(key, graph)])]: the counts on the pool of 17 programs; one call with a spilling program among the others and one with 13 challenges
    (both take the per-program fallback)"""
    F = SI.field(po, fname)
    pool = [(("batch", i), QI.batch_program(po, F, i)) for i in range(17)]
    calls = [("count %d" % c, batch_env(po, fname), pool[:c]) for c in QI.BATCH_COUNTS]
    calls.append(("spill", batch_env(po, fname), pool[:3] + [(("batch", 3, "spill"), QI.batch_program(po, F, 3, spill=True))] + pool[4:6]))
    calls.append(("13 challenges", batch_env(po, fname, 13), [(("batch", i, 13), QI.batch_program(po, F, i, nchal=13)) for i in range(3)]))
    return calls


def perm_sweep(ext_k):
    """-> [(shape, rot_scale, last_rotation)]: every shape with the (rot_scale, last_rotation) pairs in turn, and every pair on (7, 2, 4)"""
    rows = 1 << ext_k
    pairs = [(rs, lr) for rs in QI.perm_rot_scales(ext_k) for lr in QI.perm_last_rotations(rows)]
    out = [(shape, *pairs[(i + ext_k) % len(pairs)]) for i, shape in enumerate(QI.PERM_SHAPES)]
    return out + [((7, 2, 4), rs, lr) for rs, lr in pairs]


def perm_ref(po, F, key, d, shape, last_rotation, sc, rot_scale):
    return _ref(("perm", F.name) + key, lambda: QI.perm_reference(po, F, d, shape, last_rotation, sc, rot_scale))


PERM_FAMILY_KS = [1, 7, 8]
PERM_FAMILY_SHAPES = [(7, 2, 4), (3, 3, 2)]


def perm_family_cases(po, fname, ext_k):
    """-> [(key, inputs, closed form or None, shape, rot_scale, last_rotation, scalars)]"""
    F = SI.field(po, fname)
    sc = QI.perm_scalars(po, F, ext_k)
    out = []
    for si, shape in enumerate(PERM_FAMILY_SHAPES):
        fams = _ref(("permfam", fname, ext_k, shape), lambda: QI.perm_families(po, F, ext_k, shape, sc))
        for fi, (name, (d, closed)) in enumerate(fams.items()):
            rs = QI.perm_rot_scales(ext_k)[(fi + si) % len(QI.perm_rot_scales(ext_k))]
            out.append(((ext_k, shape, name), d, closed, shape, rs, -6 if (fi + si) % 2 else -1, sc))
    return out


def lookup_cases(po, fname, log_rows):
    """-> (families, Lagrange columns by name, scalars, [(family index, Lagrange name, rot_scale)])"""
    F = SI.field(po, fname)
    sc = QI.lookup_scalars(po, F)
    fams = _ref(("lookupfam", fname, log_rows), lambda: QI.lookup_families(po, F, log_rows, sc))
    lag = _ref(("lookuplag", fname, log_rows), lambda: QI.lookup_lagrange(po, F, log_rows))
    singles = [(fi, ln, rs) for rs in QI.LOOKUP_ROT_SCALES for ln in ("uniform", "indicator") for fi in range(len(fams))]
    singles += [(fi, ln, rs) for rs in QI.LOOKUP_ROT_SCALES for ln in ("zero", "edges") for fi in (4, 5)]
    return fams, lag, sc, singles


def lookup_ref(po, F, key, values, h, lag, sc, rot_scale):
    return _ref(("lookup", F.name) + key, lambda: QI.lookup_reference(po, F, values, h, lag, sc, rot_scale))


def lookup_batches(fams):
    """-> [(family indices, Lagrange name, rot_scale)]: counts 1 to 8, and the same lookup in all eight slots"""
    out = [(list(range(c)), ("indicator", "uniform")[c % 2], QI.LOOKUP_ROT_SCALES[(c // 2) % 2]) for c in range(1, 9)]
    return out + [([4] * 8, "edges", 4), ([5] * 8, "indicator", 1)]


# ---------------------------------------------------------------- CPU: the reference is pinned
@pytest.mark.parametrize("fname", QI.ALL_FIELDS)
def test_edge_set_and_pair_programs_equal_the_c_oracle(po, co, fname):
    F = SI.field(po, fname)
    p = F.p
    E = QI.edge_values(po, F)
    shift = lambda x: x * pow(2, SI.INTERNAL_SHIFT, p) % p
    internal = {shift(x) for x in E}
    assert {1, p - 1} | {(1 << (29 * j)) - 1 for j in range(1, 9)} | {1 << (29 * j) for j in range(1, 9)} <= internal
    assert {p - (1 << 29), p - (1 << 232) + 1} <= internal and {1, p - 1} <= {x * pow(2, 256, p) % p for x in E}
    env, log_rows, programs, spill, previous = pair_case(po, fname)
    A, B = env["advice"]
    assert {(a, b) for a, b in zip(A, B)} >= {(a, b) for a in E for b in E} and len(A) == 1 << log_rows
    closed = pair_closed_forms(F, A, B)
    assert set(closed) == set(programs) and len(programs) > 16       # more than two groups of eight in one batched call
    for name, g in programs.items():
        want = _graph_ref(po, F, ("pair", name), g, env, len(A), 1)
        assert want == closed[name], name
        assert np.array_equal(_co_graph(co, F, g, env, log_rows, 1), F.enc(want)), name
    want = _graph_ref(po, F, ("pair", "spill"), spill, env, len(A), 1, previous)
    assert np.array_equal(_co_graph(co, F, spill, env, log_rows, 1, previous), F.enc(want))


@pytest.mark.parametrize("fname", GEOMETRY_FIELDS)
def test_graph_geometry_reference_equals_the_c_oracle(po, co, fname):
    """a subset of the geometries: rotations at 1, 8 and 128 rows (the tables wrap several times), the live-intermediate programs at both ends, every hand-written
    program (the empty one evaluates to zero), the slow-staging shapes and the batch's programs"""
    F = SI.field(po, fname)
    groups = [(rotation_group(po, fname, lr), lr) for lr in (0, 3, 7)] + [(live_group(po, fname, 8, [1, 14, 20]), 8), (handwritten_group(po, fname), HAND_LOG)]
    groups += [(staging_group(po, fname, shape), STAGING_LOG) for shape in STAGING[1::2]]
    for (env, cases), log_rows in groups:
        for key, g, rot_scale, previous in cases:
            want = _graph_ref(po, F, key, g, env, 1 << log_rows, rot_scale, previous)
            assert np.array_equal(_co_graph(co, F, g, env, log_rows, rot_scale, previous), F.enc(want)), key
            if key == ("hand", "empty"):
                assert want == [0] * (1 << log_rows)
    for label, env, progs in batch_calls(po, fname)[-3:]:
        for key, g in progs:
            want = _graph_ref(po, F, key, g, env, 1 << BATCH_LOG, 2)
            assert np.array_equal(_co_graph(co, F, g, env, BATCH_LOG, 2), F.enc(want)), key


def _co_perm(co, F, d, shape, last_rotation, sc, ext_k, rot_scale):
    e1 = F.enc1
    return co.permutation_h(F.fid, F.enc(d["values"]), [F.enc(c) for c in d["z"]], [F.enc(c) for c in d["cols"]], [F.enc(c) for c in d["sigma"]], shape[1],
                            last_rotation, F.enc(d["l0"]), F.enc(d["l_last"]), F.enc(d["l_active"]), e1(sc["beta"]), e1(sc["gamma"]), e1(sc["y"]), e1(sc["delta"]),
                            e1(sc["beta"] * sc["zeta"] % F.p), e1(sc["omega"]), ext_k, rot_scale, 2)


@pytest.mark.parametrize("fname", QI.ALL_FIELDS)
def test_permutation_families_equal_the_c_oracle(po, co, fname):
    """every structured family (bn254_fq, of two-adicity 1: at two rows only) and the shape sweep at 2, 4 and 64 rows; (0, 1, 0) leaves the values alone and the
    empty last set of (3, 3, 2) contributes z(wX) - z(X)"""
    F = SI.field(po, fname)
    closed_seen = set()
    for ext_k in (PERM_FAMILY_KS if fname != "bn254_fq" else [1]):
        for key, d, closed, shape, rs, lr, sc in perm_family_cases(po, fname, ext_k):
            want = perm_ref(po, F, key, d, shape, lr, sc, rs)
            if closed is not None:
                closed_seen.add(key[2])
                assert want == closed, key
            assert np.array_equal(_co_perm(co, F, d, shape, lr, sc, ext_k, rs), F.enc(want)), key
    assert {"l_zero", "satisfied", "satisfied_values_zero"} <= closed_seen
    for ext_k in ([1, 2, 6] if fname != "bn254_fq" else [1]):
        sc = QI.perm_scalars(po, F, ext_k)
        for shape, rs, lr in perm_sweep(ext_k):
            d = QI.perm_uniform(po, F, 1 << ext_k, shape, 0x4000 + ext_k)
            want = perm_ref(po, F, ("sweep", ext_k, shape, rs, lr), d, shape, lr, sc, rs)
            assert np.array_equal(_co_perm(co, F, d, shape, lr, sc, ext_k, rs), F.enc(want)), (ext_k, shape, rs, lr)
            if shape == (0, 1, 0):
                assert want == d["values"]
    # the empty last set, in plain integers: one more set whose product is z(wX) - z(X)
    p, ext_k, rs, lr = F.p, 1, 1, -1
    sc = QI.perm_scalars(po, F, ext_k)
    d = QI.perm_uniform(po, F, 2, (3, 3, 2), 0x4000 + ext_k)
    one_set = dict(d, z=d["z"][:1])
    y = sc["y"]
    with_one = QI.perm_reference(po, F, one_set, (3, 3, 1), lr, sc, rs)
    # terms of two sets: l0 (1 - z0), l_last (z1^2 - z1), l0 (z1 - z0(w^last X)), set 0, set 1; of one set: l0 (1 - z0), l_last (z0^2 - z0), set 0
    z0, z1 = d["z"]
    want = []
    for i in range(2):
        set0 = (with_one[i] - (d["values"][i] * y * y + (1 - z0[i]) * d["l0"][i] * y + (z0[i] * z0[i] - z0[i]) * d["l_last"][i]) * y) % p
        v = d["values"][i]
        v = (v * y + (1 - z0[i]) * d["l0"][i]) % p
        v = (v * y + (z1[i] * z1[i] - z1[i]) * d["l_last"][i]) % p
        v = (v * y + (z1[i] - z0[(i + lr * rs) % 2]) * d["l0"][i]) % p
        v = (v * y + set0) % p
        v = (v * y + (z1[(i + rs) % 2] - z1[i]) * d["l_active"][i]) % p
        want.append(v)
    assert QI.perm_reference(po, F, d, (3, 3, 2), lr, sc, rs) == want


@pytest.mark.parametrize("fname", QI.ALL_FIELDS)
def test_lookup_families_equal_the_c_oracle(po, co, fname):
    """every family under every choice of Lagrange columns at 1, 2, 64 and 128 rows; a satisfied lookup folds five zeros: values * y^5"""
    F = SI.field(po, fname)
    e1 = F.enc1
    for log_rows in (0, 1, 6, 7):
        fams, lag, sc, singles = lookup_cases(po, fname, log_rows)
        for fi, ln, rs in singles:
            name, h, satisfied = fams[fi]
            values = lag[ln][3]
            want = lookup_ref(po, F, (log_rows, fi, ln, rs), values, h, lag[ln], sc, rs)
            if satisfied or ln == "zero":
                assert want == [v * pow(sc["y"], 5, F.p) % F.p for v in values], (log_rows, name, ln)
            got = co.lookup_h(F.fid, F.enc(values), F.enc(h["z"]), F.enc(h["a"]), F.enc(h["s"]), F.enc(h["tv"]), F.enc(lag[ln][0]), F.enc(lag[ln][1]), F.enc(lag[ln][2]),
                              e1(sc["beta"]), e1(sc["gamma"]), e1(sc["y"]), log_rows, rs, 2)
            assert np.array_equal(got, F.enc(want)), (log_rows, name, ln, rs)


# ---------------------------------------------------------------- GPU
class _Dev:
    """uploads canonical integers in the form under test and reads results back as memory-form arrays"""

    def __init__(self, pkg, ctx, po, fname, internal=False):
        ev = pkg.evaluation
        self.pkg, self.ctx, self.F, self.spec, self.internal = pkg, ctx, SI.field(po, fname), pkg.fields.FIELDS[fname], internal
        self.flags = (ev.COLUMNS_INTERNAL | ev.VALUES_INTERNAL) if internal else 0

    def up(self, vals):
        t = self.ctx.upload(self.F.enc(vals))
        if self.internal:
            self.ctx.convert_form_device(self.spec.id, t.data_ptr(), t.data_ptr(), len(vals), True)
        return t

    def poisoned(self, rows, count=1):
        import torch
        outs = [torch.full((rows, 4), POISON, dtype=torch.int64, device="cuda") for _ in range(count)]
        torch.cuda.synchronize()           # the context's stream is not torch's
        return outs

    def down(self, t):
        """t (rows x 4, in the form under test) -> memory-form array; converts t in place"""
        if self.internal:
            self.ctx.convert_form_device(self.spec.id, t.data_ptr(), t.data_ptr(), t.shape[0], False)
        self.ctx.synchronize()
        return self.ctx.download_tensor(t)

    def check(self, t, want, label):
        got = self.down(t)
        exp = self.F.enc(want)
        if not np.array_equal(got, exp):
            bad = np.nonzero((got != exp).any(axis=1))[0]
            i = int(bad[0])
            if (got[i] == np.uint64(POISON)).all() and not self.internal:
                word = "the poison"
            elif int.from_bytes(got[i].tobytes(), "little") >= self.F.p:
                word = "a non-canonical word 0x%x" % int.from_bytes(got[i].tobytes(), "little")
            else:
                word = hex(self.F.dec(got[i:i + 1])[0])
            raise AssertionError("%s: %d of %d rows differ, first row %d: got %s, want %s" % (label, len(bad), len(want), i, word, hex(want[i])))

    def env_ptrs(self, env):
        cols = {k: [self.up(c) for c in env[k]] for k in ("fixed", "advice", "instance")}
        return cols, {k: [t.data_ptr() for t in v] for k, v in cols.items()}

    def compile(self, g):
        ev = self.pkg.evaluation
        return ev.GraphEvaluator(constants=list(g["constants"]), rotations=list(g["rotations"]), calculations=list(g["calcs"]),
                                 num_intermediates=g["num_intermediates"]).compile(self.ctx, self.spec)

    def evaluate(self, cg, ptrs, env, log_rows, rot_scale, d_previous, d_out):
        nz = lambda v: v if v else None        # (a null beta .. y reads as zero)
        cg.evaluate_device(ptrs["fixed"], ptrs["advice"], ptrs["instance"], env["challenges"], nz(env["beta"]), nz(env["gamma"]), nz(env["theta"]), nz(env["y"]),
                           log_rows, rot_scale, d_previous, d_out, 0, self.flags)

    def evaluate_batch(self, cgs, ptrs, env, log_rows, rot_scale, d_outs):
        enc = lambda v: self.spec.encode(v) if v else None
        ch = self.spec.encode_many(list(env["challenges"])) if env["challenges"] else None
        self.ctx.graph_evaluate_batch_device([cg.handle.value for cg in cgs], ptrs["fixed"], ptrs["advice"], ptrs["instance"], ch, enc(env["beta"]), enc(env["gamma"]),
                                             enc(env["theta"]), enc(env["y"]), log_rows, rot_scale, [t.data_ptr() for t in d_outs], 0, self.flags)


def _run_graph_group(dev, po, env, log_rows, cases):
    """each program of `cases` alone through evaluate_device, over one upload of the environment, into a poisoned output"""
    keep, ptrs = dev.env_ptrs(env)
    for key, g, rot_scale, previous in cases:
        want = _graph_ref(po, dev.F, key, g, env, 1 << log_rows, rot_scale, previous)
        cg = dev.compile(g)
        prev = dev.up(previous) if previous is not None else None
        out, = dev.poisoned(1 << log_rows)
        dev.evaluate(cg, ptrs, env, log_rows, rot_scale, prev.data_ptr() if prev is not None else 0, out.data_ptr())
        dev.check(out, want, key)
        if prev is not None:      # in place: previous == out
            dev.evaluate(cg, ptrs, env, log_rows, rot_scale, prev.data_ptr(), prev.data_ptr())
            dev.check(prev, want, key + ("in place",))
        cg.release()
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize("internal", [False, True], ids=["standard", "internal"])
@pytest.mark.parametrize("fname", QI.ALL_FIELDS)
def test_graph_operations_on_every_pair_of_edge_values(pkg, po, ctx, fname, internal):
    """every operation on every ordered pair of E (2048 rows, 16 blocks): all the non-spilling programs in ONE batched call (20 programs: three staging
    regions), then one by one; then -(A - A) and -A through an HBM slot, added to PREVIOUS = the NEGATE program's own device output"""
    dev = _Dev(pkg, ctx, po, fname, internal)
    env, log_rows, programs, spill, previous = pair_case(po, fname)
    rows = 1 << log_rows
    keep, ptrs = dev.env_ptrs(env)
    names = list(programs)
    cgs = [dev.compile(programs[n]) for n in names]
    outs = dev.poisoned(rows, len(names))
    dev.evaluate_batch(cgs, ptrs, env, log_rows, 1, outs)
    for n, out in zip(names, outs):
        dev.check(out, _graph_ref(po, dev.F, ("pair", n), programs[n], env, rows, 1), ("batched", n))
    negated = None
    for n, cg in zip(names, cgs):
        out, = dev.poisoned(rows)
        dev.evaluate(cg, ptrs, env, log_rows, 1, 0, out.data_ptr())
        if n == "negate":          # kept in the form under test, before check() converts `out`
            import torch
            ctx.synchronize()
            negated = out.clone()
            torch.cuda.synchronize()
        dev.check(out, _graph_ref(po, dev.F, ("pair", n), programs[n], env, rows, 1), ("alone", n))
        cg.release()
    want = _graph_ref(po, dev.F, ("pair", "spill"), spill, env, rows, 1, previous)
    cg = dev.compile(spill)
    out, = dev.poisoned(rows)
    dev.evaluate(cg, ptrs, env, log_rows, 1, negated.data_ptr(), out.data_ptr())
    dev.check(out, want, "spill")
    dev.evaluate(cg, ptrs, env, log_rows, 1, negated.data_ptr(), negated.data_ptr())
    dev.check(negated, want, "spill in place")
    cg.release()
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows", GRAPH_LOGS)
@pytest.mark.parametrize("fname", GEOMETRY_FIELDS)
def test_graph_rows_and_rotations(pkg, po, ctx, fname, log_rows):
    """1 row to 8 blocks (a partial block below 128 rows), rot_scale 1, 4 and 8, every column kind at 0, +-1, 2, -3, 5 and two rotations of several wraps"""
    env, cases = rotation_group(po, fname, log_rows)
    _run_graph_group(_Dev(pkg, ctx, po, fname), po, env, log_rows, cases)


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows", [8, 10])
@pytest.mark.parametrize("fname", GEOMETRY_FIELDS)
def test_graph_live_intermediates(pkg, po, ctx, fname, log_rows):
    """exactly L intermediates alive to the end: the 48 KiB LDS boundary (10 / 11), the LDS -> HBM boundary (13 / 14), seven HBM slots (20) in several blocks
    (spill index slot * rows + row), and a result read from HBM"""
    env, cases = live_group(po, fname, log_rows)
    _run_graph_group(_Dev(pkg, ctx, po, fname), po, env, log_rows, cases)


@pytest.mark.gpu
@pytest.mark.parametrize("fname", GEOMETRY_FIELDS)
def test_graph_handwritten_programs(pkg, po, ctx, fname):
    """what the host compiler treats specially: a target written twice, t = t + x and t = t * t, a dead value, Stores that are propagated, kept (last; of an
    intermediate; target written again), the empty program (all zero over the poison), PREVIOUS without a previous column and with one"""
    env, cases = handwritten_group(po, fname)
    _run_graph_group(_Dev(pkg, ctx, po, fname), po, env, HAND_LOG, cases)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", STAGING, ids=lambda s: "%df_%da_%di_%dch" % s)
@pytest.mark.parametrize("fname", GEOMETRY_FIELDS)
def test_graph_staging_paths(pkg, po, ctx, fname, shape):
    env, cases = staging_group(po, fname, shape)
    _run_graph_group(_Dev(pkg, ctx, po, fname), po, env, STAGING_LOG, cases)


@pytest.mark.gpu
@pytest.mark.parametrize("fname", GEOMETRY_FIELDS)
def test_graph_batch_entry_point(pkg, po, ctx, fname):
    """dehalo_graph_evaluate_batch_device with 1, 2, 8, 9 and 17 programs of 0, 1 and 7 constants and 1 and 12 LDS slots (12: the batch kernel's LDS
    attribute), with a spilling program among them and with 13 challenges: program i's output equals the reference of program i alone"""
    dev = _Dev(pkg, ctx, po, fname)
    for label, env, progs in batch_calls(po, fname):
        keep, ptrs = dev.env_ptrs(env)
        cgs = [dev.compile(g) for _, g in progs]
        outs = dev.poisoned(1 << BATCH_LOG, len(progs))
        dev.evaluate_batch(cgs, ptrs, env, BATCH_LOG, 2, outs)
        for (key, g), out in zip(progs, outs):
            dev.check(out, _graph_ref(po, dev.F, key, g, env, 1 << BATCH_LOG, 2), (label,) + key)
        for cg in cgs:
            cg.release()
        del keep


def _perm_device(dev, d, ptrs, shape, last_rotation, sc, ext_k, rot_scale, values):
    ncols, chunk, nsets = shape
    dev.pkg.evaluation.permutation_h_device(dev.ctx, dev.spec, ptrs["z"][:nsets], ptrs["cols"][:ncols], ptrs["sigma"][:ncols], chunk, last_rotation, ptrs["l0"],
                                            ptrs["l_last"], ptrs["l_active"], sc["beta"], sc["gamma"], sc["y"], sc["delta"], sc["zeta"], sc["omega"], ext_k, rot_scale,
                                            values.data_ptr(), 0, dev.flags)


def _perm_upload(dev, d):
    keep = {k: [dev.up(c) for c in d[k]] for k in ("z", "cols", "sigma")}
    keep.update({k: dev.up(d[k]) for k in ("l0", "l_last", "l_active")})
    return keep, {k: ([t.data_ptr() for t in v] if isinstance(v, list) else v.data_ptr()) for k, v in keep.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("ext_k", QI.PERM_EXT_KS)
@pytest.mark.parametrize("fname", ["bn254_fr", "pasta_fq"])
def test_permutation_h_shapes(pkg, po, ctx, fname, ext_k):
    """2 rows (half = 1) to 8 blocks; no set at all (values untouched), no column, an empty last set, one column per set; rot_scale 1, 2, 4; last rotations -1, -6
    and one beyond the rows"""
    dev = _Dev(pkg, ctx, po, fname)
    F, rows = dev.F, 1 << ext_k
    sc = QI.perm_scalars(po, F, ext_k)
    keep, ptrs = _perm_upload(dev, QI.perm_uniform(po, F, rows, QI.PERM_MAX, 0x4000 + ext_k))
    for shape, rs, lr in perm_sweep(ext_k):
        d = QI.perm_uniform(po, F, rows, shape, 0x4000 + ext_k)
        want = perm_ref(po, F, ("sweep", ext_k, shape, rs, lr), d, shape, lr, sc, rs)
        values = dev.up(d["values"])
        _perm_device(dev, d, ptrs, shape, lr, sc, ext_k, rs, values)
        dev.check(values, want, (shape, rs, lr))
        if shape == (0, 1, 0):
            assert want == d["values"]
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize("internal", [False, True], ids=["standard", "internal"])
@pytest.mark.parametrize("ext_k", PERM_FAMILY_KS)
@pytest.mark.parametrize("fname", QI.ALL_FIELDS)
def test_permutation_h_structured_columns(pkg, po, ctx, fname, ext_k, internal):
    """z = 1, z = 0, z boolean; indicator and all-zero Lagrange columns; left factor 0, right factor 0; the identity permutation (left - right = 0 on every row);
    columns drawn from E; the satisfied argument.  bn254_fq (two-adicity 1) runs at two rows."""
    if fname == "bn254_fq" and ext_k > 1:
        dev = _Dev(pkg, ctx, po, fname, internal)
        F, rows = dev.F, 1 << ext_k
        d = QI.perm_uniform(po, F, rows, (3, 3, 1), 0x4100)
        sc = dict(QI.perm_scalars(po, F, 1), omega=F.p - 1)
        keep, ptrs = _perm_upload(dev, d)
        values = dev.up(d["values"])
        with pytest.raises(pkg.DehaloError):
            _perm_device(dev, d, ptrs, (3, 3, 1), -1, sc, ext_k, 1, values)
        dev.check(values, d["values"], "values after the refused call")
        return
    dev = _Dev(pkg, ctx, po, fname, internal)
    for key, d, closed, shape, rs, lr, sc in perm_family_cases(po, fname, ext_k):
        want = perm_ref(po, dev.F, key, d, shape, lr, sc, rs)
        keep, ptrs = _perm_upload(dev, d)
        values = dev.up(d["values"])
        _perm_device(dev, d, ptrs, shape, lr, sc, ext_k, rs, values)
        dev.check(values, want, key)


def _lookup_upload(dev, fams, lag):
    df = [{k: dev.up(h[k]) for k in ("z", "a", "s", "tv")} for _, h, _ in fams]
    dl = {ln: [dev.up(c) for c in cols[:3]] for ln, cols in lag.items()}
    return df, dl


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows", QI.LOOKUP_LOGS)
@pytest.mark.parametrize("fname", ["bn254_fr", "pasta_fp", "bn254_fq"])
def test_lookup_h_structured(pkg, po, ctx, fname, log_rows):
    """k_lookup_h at 1 row to 8 blocks, rot_scale 1 and 4: a' == s', a' constant, z = 1, (a' + beta)(s' + gamma) = table value with z constant, columns from E, the
    satisfied lookup, all zero -- under uniform, indicator, all-zero and E-valued Lagrange columns; 8 blocks also in the internal form"""
    for internal in ([False, True] if log_rows == 8 else [False]):
        dev = _Dev(pkg, ctx, po, fname, internal)
        fams, lag, sc, singles = lookup_cases(po, fname, log_rows)
        df, dl = _lookup_upload(dev, fams, lag)
        for fi, ln, rs in singles:
            want = lookup_ref(po, dev.F, (log_rows, fi, ln, rs), lag[ln][3], fams[fi][1], lag[ln], sc, rs)
            values = dev.up(lag[ln][3])
            t, l = df[fi], dl[ln]
            pkg.evaluation.lookup_h_device(ctx, dev.spec, t["z"].data_ptr(), t["a"].data_ptr(), t["s"].data_ptr(), t["tv"].data_ptr(), l[0].data_ptr(), l[1].data_ptr(),
                                           l[2].data_ptr(), sc["beta"], sc["gamma"], sc["y"], log_rows, rs, values.data_ptr(), 0, dev.flags)
            dev.check(values, want, (fams[fi][0], ln, rs, internal))


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows", QI.LOOKUP_LOGS)
@pytest.mark.parametrize("fname", ["bn254_fr", "pasta_fp"])
def test_lookup_h_batch_structured(pkg, po, ctx, fname, log_rows):
    """k_lookup_h_batch with 1 to 8 of the structured lookups, and with the SAME lookup's pointers in all eight slots: lookup_h applied lookup after lookup"""
    dev = _Dev(pkg, ctx, po, fname)
    fams, lag, sc, _ = lookup_cases(po, fname, log_rows)
    df, dl = _lookup_upload(dev, fams, lag)
    for idx, ln, rs in lookup_batches(fams):
        want = lag[ln][3]
        for fi in idx:
            want = QI.lookup_reference(po, dev.F, want, fams[fi][1], lag[ln], sc, rs)
        values = dev.up(lag[ln][3])
        tuples = [(df[fi]["z"].data_ptr(), df[fi]["a"].data_ptr(), df[fi]["s"].data_ptr(), df[fi]["tv"].data_ptr()) for fi in idx]
        l = dl[ln]
        pkg.evaluation.lookup_h_batch_device(ctx, dev.spec, tuples, l[0].data_ptr(), l[1].data_ptr(), l[2].data_ptr(), sc["beta"], sc["gamma"], sc["y"], log_rows, rs,
                                             values.data_ptr(), 0, dev.flags)
        dev.check(values, want, (idx, ln, rs))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(QI.PRODUCT_MODES))
@pytest.mark.parametrize("fname", QI.ALL_FIELDS)
def test_product_terms_structured(pkg, po, ctx, fname, mode):
    """k_product_terms at 1, 127, 128, 129 and 1000 rows: columns drawn from E, rows where a numerator's or a denominator's factor is exactly zero; permutation
    sets only, lookups only, both; a stride beyond n whose gap keeps its pattern"""
    import torch
    from dehalo2_amd.keygen import delta_of
    dev = _Dev(pkg, ctx, po, fname)
    F, spec = dev.F, dev.spec
    p = F.p
    for n in QI.PRODUCT_NS:
        d = QI.product_inputs(po, F, n, mode, delta_of(spec))
        want_num, want_den = QI.product_reference(F, d, n)
        assert any(0 in w for w in want_num) and any(0 in w for w in want_den) or n == 1
        ncols, chunk, nl = QI.PRODUCT_MODES[mode]
        sets, stride = (ncols + chunk - 1) // chunk, n + 5
        dc, ds, dom = [dev.up(c) for c in d["cols"]], [dev.up(c) for c in d["sigma"]], dev.up(d["omega_powers"])
        dlk = [[dev.up(c) for c in four] for four in d["lookups"]]
        num = torch.full((sets + nl, stride, 4), POISON, dtype=torch.int64, device="cuda")
        den = torch.full((sets + nl, stride, 4), POISON, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.product_terms_device(spec.id, [t.data_ptr() for t in dc], [t.data_ptr() for t in ds], chunk, dom.data_ptr(), F.enc1(d["beta"]), F.enc1(d["gamma"]),
                                 F.enc1(d["delta"]), F.enc([d["beta"] * pow(d["delta"], chunk * s, p) % p for s in range(sets)]) if sets else np.zeros((1, 4), dtype=np.uint64),
                                 [tuple(t.data_ptr() for t in four) for four in dlk], n, num.data_ptr(), den.data_ptr(), stride)
        ctx.synchronize()
        got_n, got_d = ctx.download_tensor(num), ctx.download_tensor(den)
        for q in range(sets + nl):
            assert np.array_equal(got_n[q, :n], F.enc(want_num[q])), (n, q, "numerator")
            assert np.array_equal(got_d[q, :n], F.enc(want_den[q])), (n, q, "denominator")
        assert (got_n[:, n:] == np.uint64(POISON)).all() and (got_d[:, n:] == np.uint64(POISON)).all(), (n, "the gap between the columns was written")
