"""Structured inputs and hand-built programs for the quotient-numerator kernels (csrc/evalh.cuh), in canonical Python integers.

Uniform columns never make two operands equal, zero or p - 1, which is where the lazily reduced helpers (evh_add / evh_sub / evh_neg, the conditional
subtractions of 2p and 4p, the two stores) have their edges -- and where real proofs live: a satisfied permutation has left == right, a lookup a' == s' on most
rows, z = 1 at row 0, mostly-zero Lagrange columns.  This module builds those operands, programs at every launch geometry and compiler shape of interest, and the
permutation / lookup / grand-product inputs; tests/test_quotient_structured.py pins oracle/pyoracle.py on them against the C restatement (no GPU) and then judges
the kernels by it.  A plain helper beside tests/structured_inputs.py, whose StructuredField F it takes.

A graph is pyoracle's dict {constants, rotations, calcs, num_intermediates}; a calculation (op, a, b, parts, target); a source (kind, index, rotation index).
"""
import structured_inputs as SI

ALL_FIELDS = ["bn254_fr", "bn254_fq", "pasta_fp", "pasta_fq"]
LDS_SLOTS = 13               # EVH_MAX_LDS_SLOTS: intermediates beyond them live in HBM
ZERO = (0, 0, 0)             # SRC_CONSTANT 0: the unused operand of a unary calculation


_UNIFORM = {}


def uniform(po, F, n, seed):
    """n uniform values of the stream `seed`, drawn once (callers copy before they write)"""
    key = (F.name, n, seed)
    if key not in _UNIFORM:
        _UNIFORM[key] = SI.uniform_ints(po, F, n, seed) if n else []
    return list(_UNIFORM[key])


# ---- 1. the edge-value set ----------------------------------------------------------------------------------------------------------------------------------
def edge_values(po, F):
    """45 canonical integers: small and large constants; values whose device-internal form x * 2^261 mod p is 1, p - 1, 2^(29 j) - 1 or 2^(29 j), j = 1..8
    (the limb boundaries of the 9 x 29-bit representation), and their negatives; values whose memory form x * 2^256 mod p is 1 or p - 1; two uniform values.
    45^2 = 2025 ordered pairs fit 2048 rows."""
    p = F.p
    vs = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    back = pow(1 << SI.INTERNAL_SHIFT, -1, p)
    internal = [1, p - 1] + [(1 << (29 * j)) - 1 for j in range(1, 9)] + [1 << (29 * j) for j in range(1, 9)]
    assert all(0 < v < p for v in internal)
    xs = [v * back % p for v in internal]
    vs += xs + [p - x for x in xs]
    back256 = pow(1 << 256, -1, p)
    vs += [back256, (p - 1) * back256 % p]
    vs += uniform(po, F, 2, 0xED6E)
    seen, out = set(), []
    for v in vs:
        assert 0 <= v < p
        if v not in seen:
            seen.add(v)
            out.append(v)
    assert len(out) == 45, len(out)
    return out


def cyclic(E, n, offset=0, step=1):
    """n values drawn cyclically from E"""
    return [E[(offset + step * i) % len(E)] for i in range(n)]


def pair_columns(po, F):
    """-> (A, B, log_rows): A[i] = E[i // |E|], B[i] = E[i % |E|] over every ordered pair, padded with uniform values to 2048 rows"""
    E = edge_values(po, F)
    m = len(E) * len(E)
    pad = uniform(po, F, 2 * (2048 - m), 0xAB01)
    A = [E[i // len(E)] for i in range(m)] + pad[::2]
    B = [E[i % len(E)] for i in range(m)] + pad[1::2]
    assert len(A) == len(B) == 2048
    return A, B, 11


# ---- 2. one tiny program per operation ----------------------------------------------------------------------------------------------------------------------
def _graph(constants, rotations, calcs, num_intermediates=None):
    if num_intermediates is None:
        num_intermediates = 1 + max([c[4] for c in calcs], default=-1)
    return {"constants": list(constants), "rotations": list(rotations), "calcs": list(calcs), "num_intermediates": num_intermediates}


def op_programs(po):
    """name -> graph over advice columns A (0) and B (1).  None spills or reads PREVIOUS, so all of them go into one batched call.  `zero_*`: NEGATE(A - A) is
    the negation of an exact zero, the one value the device holds as 2p; each of these programs puts it through one more operation."""
    A, B = (po.SRC_ADVICE, 0, 0), (po.SRC_ADVICE, 1, 0)
    I = lambda i: (po.SRC_INTERMEDIATE, i, 0)
    C = lambda i: (po.SRC_CONSTANT, i, 0)
    G = lambda *calcs: _graph([0, 1, 2], [0], calcs)
    out = {
        "add": G((po.CALC_ADD, A, B, (), 0)),
        "sub": G((po.CALC_SUB, A, B, (), 0)),
        "mul": G((po.CALC_MUL, A, B, (), 0)),
        "square": G((po.CALC_SQUARE, A, ZERO, (), 0)),
        "double": G((po.CALC_DOUBLE, A, ZERO, (), 0)),
        "negate": G((po.CALC_NEGATE, A, ZERO, (), 0)),
        "store": G((po.CALC_STORE, A, ZERO, (), 0)),
        "horner": G((po.CALC_HORNER, A, B, (A, B, C(0), C(1)), 0)),
        "neg_of_sub_self": G((po.CALC_SUB, A, A, (), 0), (po.CALC_NEGATE, I(0), ZERO, (), 1)),
        "neg_plus_self": G((po.CALC_NEGATE, A, ZERO, (), 0), (po.CALC_ADD, I(0), A, (), 1)),
    }
    z2p = [(po.CALC_SUB, A, A, (), 0), (po.CALC_NEGATE, I(0), ZERO, (), 1)]          # intermediate 1 = -(0)
    for name, last in (("zero_mul", (po.CALC_MUL, I(1), B, (), 2)), ("zero_mul_self", (po.CALC_MUL, I(1), I(1), (), 2)),
                       ("zero_square", (po.CALC_SQUARE, I(1), ZERO, (), 2)), ("zero_double", (po.CALC_DOUBLE, I(1), ZERO, (), 2)),
                       ("zero_negate", (po.CALC_NEGATE, I(1), ZERO, (), 2)), ("zero_add_self", (po.CALC_ADD, I(1), I(1), (), 2)),
                       ("zero_minus_b", (po.CALC_SUB, I(1), B, (), 2)), ("b_minus_zero", (po.CALC_SUB, B, I(1), (), 2)),
                       ("zero_store", (po.CALC_STORE, I(1), ZERO, (), 2)), ("zero_horner", (po.CALC_HORNER, I(1), I(1), (I(1), B, I(1)), 2))):
        out[name] = G(*z2p, last)
    return out


def spill_previous_program(po):
    """13 live products fill the LDS slots, so -(A - A) and then -A land in the first HBM slot (stored canonically, read back), are added to PREVIOUS and folded
    with everything else; run with previous = -A (a NEGATE program's own device output) the sum -A + previous is 2 (-A)."""
    A, B = (po.SRC_ADVICE, 0, 0), (po.SRC_ADVICE, 1, 0)
    I = lambda i: (po.SRC_INTERMEDIATE, i, 0)
    calcs = [(po.CALC_MUL, A if i % 2 else B, B, (), i) for i in range(LDS_SLOTS)]
    n = LDS_SLOTS
    calcs += [(po.CALC_SUB, A, A, (), n), (po.CALC_NEGATE, I(n), ZERO, (), n + 1),           # 2p, into HBM slot 0 (the SUB's, free again)
              (po.CALC_ADD, I(n + 1), (po.SRC_PREVIOUS, 0, 0), (), n + 2),                    # 0 + previous
              (po.CALC_NEGATE, A, ZERO, (), n + 3), (po.CALC_ADD, I(n + 3), (po.SRC_PREVIOUS, 0, 0), (), n + 4),
              (po.CALC_HORNER, I(n + 2), B, tuple(I(i) for i in range(LDS_SLOTS)) + (I(n + 4), I(n + 1)), n + 5)]
    return _graph([0, 1, 2], [0], calcs)


# ---- 3. geometry and compiler shapes ------------------------------------------------------------------------------------------------------------------------
def rotation_table(rows):
    """0, +-1, 2, -3, 5 and two entries that wrap several times at every rot_scale"""
    return [0, 1, -1, 2, -3, 5, 2 * rows + 3, -(3 * rows + 1)]


def uniform_env(po, F, rows, nf, na, ni, nchal, seed):
    u = uniform(po, F, rows * (nf + na + ni) + nchal + 4, seed)
    col = lambda j: u[j * rows:(j + 1) * rows]
    tail = u[rows * (nf + na + ni):]
    return {"fixed": [col(j) for j in range(nf)], "advice": [col(nf + j) for j in range(na)], "instance": [col(nf + na + j) for j in range(ni)],
            "challenges": tail[4:], "beta": tail[0], "gamma": tail[1], "theta": tail[2], "y": tail[3]}


def rotation_program(po, rows):
    """every column of a (2 fixed, 2 advice, 1 instance) environment at every rotation of the table, folded by one Horner in the challenge, after a product and
    a difference of rotated cells"""
    rots = rotation_table(rows)
    cols = [(po.SRC_FIXED, 0), (po.SRC_FIXED, 1), (po.SRC_ADVICE, 0), (po.SRC_ADVICE, 1), (po.SRC_INSTANCE, 0)]
    parts = tuple((k, i, r) for r in range(len(rots)) for k, i in cols)
    calcs = [(po.CALC_MUL, (po.SRC_ADVICE, 0, 1), (po.SRC_FIXED, 1, 6), (), 0),
             (po.CALC_SUB, (po.SRC_INSTANCE, 0, 7), (po.SRC_INTERMEDIATE, 0, 0), (), 1),
             (po.CALC_HORNER, (po.SRC_INTERMEDIATE, 1, 0), (po.SRC_CHALLENGE, 0, 0), parts, 2)]
    return _graph([0, 1, 2], rots, calcs)


def live_program(po, rows, L, result_in_place=False):
    """exactly L intermediates alive to the end (products of rotated cells: slots 0 .. L-1, the ones from 13 on in HBM), closed by one Horner over all of them.
    The Horner's operands die at it, so its own target takes slot 0; result_in_place makes it write the LAST intermediate again instead, which keeps that
    intermediate's slot (for L = 14 the first HBM slot: the program's result is then read from HBM)."""
    rots = rotation_table(rows)
    nr = len(rots)
    kinds = [po.SRC_FIXED, po.SRC_ADVICE, po.SRC_INSTANCE]
    calcs = [(po.CALC_MUL, (kinds[i % 3], 0, i % nr), (kinds[(i + 1) % 3], 0, (3 * i + 1) % nr), (), i) for i in range(L)]
    parts = tuple((po.SRC_INTERMEDIATE, i, 0) for i in range(L))
    if result_in_place:
        calcs.append((po.CALC_HORNER, (po.SRC_INTERMEDIATE, L - 1, 0), (po.SRC_Y, 0, 0), parts, L - 1))
        return _graph([0, 1, 2], rots, calcs, L)
    calcs.append((po.CALC_HORNER, (po.SRC_CONSTANT, 2, 0), (po.SRC_Y, 0, 0), parts, L))
    return _graph([0, 1, 2], rots, calcs, L + 1)


def handwritten_programs(po, rows):
    """name -> graph over (1 fixed, 2 advice, 1 instance, 1 challenge): the shapes the host compiler treats specially (copy propagation of Store, liveness,
    slot reuse), which a generator that gives every calculation a fresh target never emits"""
    rots = rotation_table(rows)
    F0, A0, A1, N0 = (po.SRC_FIXED, 0, 0), (po.SRC_ADVICE, 0, 0), (po.SRC_ADVICE, 1, 0), (po.SRC_INSTANCE, 0, 0)
    I = lambda i: (po.SRC_INTERMEDIATE, i, 0)
    G = lambda calcs, n=None: _graph([0, 1, 2], rots, calcs, n)
    return {
        "target_written_twice": G([(po.CALC_MUL, A0, A1, (), 0), (po.CALC_ADD, I(0), F0, (), 1), (po.CALC_SUB, N0, A1, (), 0), (po.CALC_MUL, I(0), I(1), (), 2)]),
        "accumulate_in_place": G([(po.CALC_STORE, A0, ZERO, (), 0), (po.CALC_ADD, I(0), A1, (), 0), (po.CALC_MUL, I(0), I(0), (), 0), (po.CALC_ADD, I(0), F0, (), 0),
                                  (po.CALC_DOUBLE, I(0), ZERO, (), 1)]),
        "dead_value": G([(po.CALC_MUL, A0, A1, (), 0), (po.CALC_MUL, F0, N0, (), 1), (po.CALC_ADD, I(0), N0, (), 2), (po.CALC_SQUARE, A1, ZERO, (), 3),
                         (po.CALC_SUB, I(2), F0, (), 4)]),
        "store_propagated": G([(po.CALC_STORE, (po.SRC_ADVICE, 1, 4), ZERO, (), 0), (po.CALC_STORE, (po.SRC_FIXED, 0, 2), ZERO, (), 1), (po.CALC_MUL, A0, N0, (), 2),
                               (po.CALC_HORNER, I(2), (po.SRC_CHALLENGE, 0, 0), (I(0), I(1), I(0), I(2)), 3)]),
        "store_last": G([(po.CALC_MUL, A0, A1, (), 0), (po.CALC_STORE, (po.SRC_INSTANCE, 0, 3), ZERO, (), 1)]),
        "store_last_only": G([(po.CALC_STORE, (po.SRC_ADVICE, 0, 5), ZERO, (), 0)]),
        "store_of_intermediate": G([(po.CALC_MUL, A0, F0, (), 0), (po.CALC_STORE, I(0), ZERO, (), 1), (po.CALC_NEGATE, I(0), ZERO, (), 0), (po.CALC_ADD, I(0), I(1), (), 2),
                                    (po.CALC_ADD, I(2), I(1), (), 3)]),
        "store_target_rewritten": G([(po.CALC_STORE, A0, ZERO, (), 0), (po.CALC_MUL, I(0), A1, (), 1), (po.CALC_STORE, F0, ZERO, (), 0), (po.CALC_ADD, I(0), I(1), (), 2)]),
        "empty": G([], 0),
        "reads_previous": G([(po.CALC_HORNER, (po.SRC_PREVIOUS, 0, 0), (po.SRC_Y, 0, 0), (A0, (po.SRC_PREVIOUS, 0, 0)), 0)]),
    }


def staging_program(po, nf, na, ni, nchal):
    """reads the last challenge and the last column of every kind (and the first of each)"""
    parts = [(po.SRC_FIXED, nf - 1, 1), (po.SRC_ADVICE, na - 1, 2), (po.SRC_FIXED, 0, 0), (po.SRC_ADVICE, 0, 0), (po.SRC_CHALLENGE, 0, 0)]
    if ni:
        parts.append((po.SRC_INSTANCE, ni - 1, 1))
    parts += [(po.SRC_BETA, 0, 0), (po.SRC_GAMMA, 0, 0), (po.SRC_THETA, 0, 0), (po.SRC_CONSTANT, 2, 0)]
    return _graph([0, 1, 2], [0, 1, -1], [(po.CALC_HORNER, (po.SRC_Y, 0, 0), (po.SRC_CHALLENGE, nchal - 1, 0), tuple(parts), 0)])


BATCH_COUNTS = [1, 2, 8, 9, 17]
BATCH_ENV = (2, 2, 1)        # fixed, advice, instance


def batch_program(po, F, index, nchal=2, spill=False):
    """program `index` of a batch: 0, 7 or 1 constants and 1 or 12 LDS slots in turn (programs 0 and 1 already differ in both), every constant, the last
    challenge and an index-dependent choice of cells read; spill: 14 live intermediates, the last in HBM"""
    nconst = (0, 7, 1)[index % 3]
    live = 14 if spill else (1, 12)[(index // 2 + index) % 2]
    consts = uniform(po, F, nconst, 0xC0 + index)
    cells = [(po.SRC_FIXED, 0), (po.SRC_FIXED, 1), (po.SRC_ADVICE, 0), (po.SRC_ADVICE, 1), (po.SRC_INSTANCE, 0)]
    cell = lambda j: cells[(index + j) % 5] + ((index + 2 * j) % 3,)
    calcs = [(po.CALC_MUL, cell(2 * i), cell(2 * i + 1), (), i) for i in range(live)]
    parts = tuple((po.SRC_INTERMEDIATE, i, 0) for i in range(live)) + tuple((po.SRC_CONSTANT, i, 0) for i in range(nconst)) + ((po.SRC_BETA, 0, 0),)
    calcs.append((po.CALC_HORNER, cell(99), (po.SRC_CHALLENGE, nchal - 1, 0), parts, live))
    return _graph(consts, [0, 1, -2], calcs)


# ---- 4. permutation terms -----------------------------------------------------------------------------------------------------------------------------------
PERM_SHAPES = [(0, 1, 0), (0, 1, 1), (1, 1, 1), (3, 3, 1), (4, 3, 2), (7, 2, 4), (6, 1, 6), (3, 3, 2)]      # (ncols, chunk_len, nsets); the last: an empty last set
PERM_EXT_KS = [1, 2, 6, 7, 8, 10]


def perm_rot_scales(ext_k):
    return [r for r in (1, 2, 4) if r <= (1 << ext_k)]


def perm_last_rotations(rows):
    return [-1, -6, -(rows + 3)]


def perm_scalars(po, F, ext_k, seed=0x5CA1):
    beta, gamma, y, delta = uniform(po, F, 4, seed)
    return {"beta": beta, "gamma": gamma, "y": y, "delta": delta, "zeta": po.zeta(F.of), "omega": F.omega(ext_k)}


PERM_MAX = (7, 1, 6)         # the most columns and the most sets of PERM_SHAPES


def perm_uniform(po, F, rows, shape, seed):
    """uniform inputs of `shape`: the leading sets and columns of one pool per (rows, seed), so that every shape of a sweep reads the same uploaded columns"""
    ncols, _, nsets = shape
    mc, ms = PERM_MAX[0], PERM_MAX[2]
    u = uniform(po, F, rows * (ms + 2 * mc + 4), seed)
    col = lambda j: u[j * rows:(j + 1) * rows]
    return {"z": [col(j) for j in range(nsets)], "cols": [col(ms + j) for j in range(ncols)], "sigma": [col(ms + mc + j) for j in range(ncols)],
            "l0": col(ms + 2 * mc), "l_last": col(ms + 2 * mc + 1), "l_active": col(ms + 2 * mc + 2), "values": col(ms + 2 * mc + 3)}


def indicators(rows, last_rotation=-6):
    """l0 / l_last / l_active as 0/1 columns: l0 at row 0, l_last at the last usable row, l_active on the rows before it"""
    u = rows + last_rotation if rows + last_rotation >= 1 else rows - 1
    l0 = [1 if i == 0 else 0 for i in range(rows)]
    l_last = [1 if i == u else 0 for i in range(rows)]
    l_active = [1 if i < u else 0 for i in range(rows)]
    return l0, l_last, l_active


def perm_families(po, F, ext_k, shape, sc):
    """name -> (inputs, closed form or None).  The closed forms: a satisfied argument folds nothing but zeros, so values only pick up one factor y per term
    (2 + (nsets - 1) + nsets of them)."""
    p = F.p
    rows = 1 << ext_k
    ncols, chunk, nsets = shape
    E = edge_values(po, F)
    base = lambda seed: perm_uniform(po, F, rows, shape, 0x4200 + ext_k)      # one pool: the families differ in what they override
    beta, gamma, delta, zeta, w = sc["beta"], sc["gamma"], sc["delta"], sc["zeta"], sc["omega"]
    wp = [pow(w, i, p) for i in range(rows)]
    ident = [[pow(delta, j, p) * zeta % p * wp[i] % p for i in range(rows)] for j in range(ncols)]          # sigma_j = delta^j zeta omega^row
    terms = 2 + max(0, nsets - 1) + nsets
    out = {}

    def put(name, seed, closed=None, **over):
        d = base(seed)
        d.update(over)
        out[name] = (d, closed)

    put("z_one", 1, z=[[1] * rows for _ in range(nsets)])
    put("z_zero", 2, z=[[0] * rows for _ in range(nsets)])
    put("z_parity", 3, z=[[(i + s) % 2 for i in range(rows)] for s in range(nsets)])
    l0, l_last, l_active = indicators(rows)
    put("l_indicator", 4, l0=l0, l_last=l_last, l_active=l_active, values=[0] * rows)
    d = base(5)
    put("l_zero", 5, closed=[v * pow(sc["y"], terms if nsets else 0, p) % p for v in d["values"]], l0=[0] * rows, l_last=[0] * rows, l_active=[0] * rows)
    d = base(6)      # left factor 0 on every fourth row, right factor 0 on the others
    cols = [[(-(beta * d["sigma"][j][i] + gamma)) % p if i % 4 == 0 else (-(pow(delta, j, p) * beta % p * zeta % p * wp[i] + gamma)) % p for i in range(rows)]
            for j in range(ncols)]
    put("factor_zero", 6, cols=cols)
    c = SI.constant_c(F)
    put("identity_z_const", 7, sigma=ident, z=[[c] * rows for _ in range(nsets)])
    put("edge_columns", 8, z=[cyclic(E, rows, 3 * s, 1) for s in range(nsets)], cols=[cyclic(E, rows, 5 * j + 1, 2) for j in range(ncols)],
        sigma=[cyclic(E, rows, 7 * j + 2, 4) for j in range(ncols)], l0=cyclic(E, rows, 11, 1), l_last=cyclic(E, rows, 13, 7), l_active=cyclic(E, rows, 17, 8),
        values=cyclic(E, rows, 19, 11))
    d = base(9)
    put("satisfied", 9, closed=[v * pow(sc["y"], terms if nsets else 0, p) % p for v in d["values"]], sigma=ident, z=[[1] * rows for _ in range(nsets)],
        l0=l0, l_last=l_last, l_active=l_active)
    put("satisfied_values_zero", 10, closed=[0] * rows, sigma=ident, z=[[1] * rows for _ in range(nsets)], l0=l0, l_last=l_last, l_active=l_active, values=[0] * rows)
    return out


def perm_reference(po, F, d, shape, last_rotation, sc, rot_scale):
    return po.permutation_h(F.of, d["values"], d["z"], d["cols"], d["sigma"], shape[1], last_rotation, d["l0"], d["l_last"], d["l_active"], sc["beta"], sc["gamma"],
                            sc["y"], sc["delta"], sc["zeta"], sc["omega"], rot_scale)


# ---- 5. lookup terms ----------------------------------------------------------------------------------------------------------------------------------------
LOOKUP_LOGS = [0, 1, 6, 7, 8, 10]
LOOKUP_ROT_SCALES = [1, 4]


def lookup_scalars(po, F, seed=0x100C):
    beta, gamma, y = uniform(po, F, 3, seed)
    return {"beta": beta, "gamma": gamma, "y": y}


def lookup_families(po, F, log_rows, sc):
    """-> [(name, {z, a, s, tv}, satisfied)] -- eight of them, one per slot of a full batch; satisfied: every one of the five terms is zero under the indicator
    (or any) Lagrange columns"""
    p, rows = F.p, 1 << log_rows
    E = edge_values(po, F)
    beta, gamma = sc["beta"], sc["gamma"]
    u = uniform(po, F, 4 * rows * 8, 0x7AB1 + log_rows)
    col = lambda j: u[j * rows:(j + 1) * rows]
    c = SI.constant_c(F)
    fams = []
    fams.append(("a_eq_s", {"z": col(0), "a": col(1), "s": col(1), "tv": col(2)}, False))
    fams.append(("a_const", {"z": col(3), "a": [c] * rows, "s": col(4), "tv": col(5)}, False))
    fams.append(("z_one", {"z": [1] * rows, "a": col(6), "s": col(7), "tv": col(8)}, False))
    a, s = col(9), col(10)
    fams.append(("product_holds", {"z": [c] * rows, "a": a, "s": s, "tv": [(x + beta) * (t + gamma) % p for x, t in zip(a, s)]}, False))
    fams.append(("edge_columns", {"z": cyclic(E, rows, 1, 1), "a": cyclic(E, rows, 2, 2), "s": cyclic(E, rows, 2, 4), "tv": cyclic(E, rows, 7, 7)}, False))
    a = col(11)
    fams.append(("satisfied", {"z": [1] * rows, "a": a, "s": a, "tv": [(x + beta) * (x + gamma) % p for x in a]}, True))
    fams.append(("zeros", {"z": [0] * rows, "a": [0] * rows, "s": [0] * rows, "tv": [0] * rows}, False))
    a = cyclic(E, rows, 5, 1)
    fams.append(("satisfied_edges", {"z": [1] * rows, "a": a, "s": a, "tv": [(x + beta) * (x + gamma) % p for x in a]}, True))
    return fams


def lookup_lagrange(po, F, log_rows):
    """name -> (l0, l_last, l_active, values)"""
    rows = 1 << log_rows
    E = edge_values(po, F)
    u = uniform(po, F, 4 * rows, 0x1A6 + log_rows)
    col = lambda j: u[j * rows:(j + 1) * rows]
    return {"uniform": (col(0), col(1), col(2), col(3)), "indicator": indicators(rows) + (col(3),), "zero": ([0] * rows, [0] * rows, [0] * rows, col(3)),
            "edges": (cyclic(E, rows, 0, 1), cyclic(E, rows, 9, 2), cyclic(E, rows, 4, 4), cyclic(E, rows, 6, 8))}


def lookup_reference(po, F, values, h, lag, sc, rot_scale):
    return po.lookup_h(F.of, values, h["z"], h["a"], h["s"], h["tv"], lag[0], lag[1], lag[2], sc["beta"], sc["gamma"], sc["y"], rot_scale)


# ---- 6. the grand products' per-row factors -----------------------------------------------------------------------------------------------------------------
PRODUCT_NS = [1, 127, 128, 129, 1000]
PRODUCT_MODES = {"sets": (7, 3, 0), "lookups": (0, 3, 2), "both": (5, 2, 3)}      # (ncols, chunk_len, nlookups): ncols never a multiple of chunk_len


def product_inputs(po, F, n, mode, delta):
    """columns drawn from E, and rows where a factor is exactly zero: row i of column i % ncols makes the denominator's factor zero when i % 3 == 0 and the
    numerator's when i % 3 == 1; the lookups' rows hit a' = -beta, s' = -gamma, A = -beta, S = -gamma in turn"""
    p = F.p
    ncols, chunk, nl = PRODUCT_MODES[mode]
    E = edge_values(po, F)
    beta, gamma = uniform(po, F, 2, 0x9A0D)
    omega = F.omega(min(10, F.of.S))     # (the kernel reads the column of powers: any element serves a field of small two-adicity)
    om = [pow(omega, i, p) for i in range(n)]
    cols = [cyclic(E, n, 3 * j, j + 1) for j in range(ncols)]
    sig = [cyclic(E, n, 5 * j + 1, 2 * j + 1) for j in range(ncols)]
    for i in range(n):
        if ncols and i % 3 < 2:
            j = i % ncols
            cols[j][i] = (-(beta * sig[j][i] + gamma)) % p if i % 3 == 0 else (-(pow(delta, j, p) * beta % p * om[i] + gamma)) % p
    lk = [[cyclic(E, n, 7 * l + t, t + 1) for t in range(4)] for l in range(nl)]
    for l in range(nl):
        for i in range(l, n, 5):
            lk[l][i % 4][i] = (-(beta if i % 2 == 0 else gamma)) % p      # A / a' against beta, S / s' against gamma
    return {"cols": cols, "sigma": sig, "lookups": lk, "omega_powers": om, "beta": beta, "gamma": gamma, "delta": delta, "chunk": chunk}


def product_reference(F, d, n):
    """-> (numerators, denominators): one list of n per permutation set, then one per lookup"""
    p, beta, gamma, delta, chunk = F.p, d["beta"], d["gamma"], d["delta"], d["chunk"]
    ncols = len(d["cols"])
    num, den = [], []
    for s in range((ncols + chunk - 1) // chunk):
        wn, wd = [], []
        for i in range(n):
            a = b = 1
            for j in range(s * chunk, min(ncols, (s + 1) * chunk)):
                b = b * (d["cols"][j][i] + beta * d["sigma"][j][i] + gamma) % p
                a = a * (d["cols"][j][i] + pow(delta, j, p) * beta % p * d["omega_powers"][i] + gamma) % p
            wn.append(a)
            wd.append(b)
        num.append(wn)
        den.append(wd)
    for A, S, a_, s_ in d["lookups"]:
        num.append([(A[i] + beta) * (S[i] + gamma) % p for i in range(n)])
        den.append([(a_[i] + beta) * (s_[i] + gamma) % p for i in range(n)])
    return num, den
