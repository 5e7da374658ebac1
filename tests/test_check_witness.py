"""dehalo_check_witness -- MockProver::verify over a proving key, on the device.

The expected failures come from an enumerator written here over oracle/rowcheck.py's `_evaluate` (upstream dev.rs MockProver::verify: every gate polynomial on
every usable row, every lookup input tuple against the usable rows' table tuples -- EXACT tuple membership --, every permutation cell against the cell the
mapping sends it to), all failures in (kind, index, row) order.  The device compares lookup tuples through a theta compression; its list must be the same.
CPU: the enumerator agrees with rowcheck.verify on every case; null arguments.  GPU: satisfied circuits over both scalar fields, zero represented as p,
single broken cells, the usable boundary and the wrap, counts / order / cap, lookups of one and two expressions across more than one sort tile, the library's own
mod_pow and pose_enc witnesses, copy constraints, and agreement with the verifier."""
import ctypes as C

import numpy as np
import pytest

from test_rotations import Q_HI, Q_LO, S_TOXIC, build_circuit, kzg_accepts, kzg_chain      # noqa: F401  (kzg_chain: a fixture)

GATE, LOOKUP, COPY = 0, 1, 2


def limbs(values, n):
    out = np.zeros((n, 4), dtype=np.uint64)
    for i, v in enumerate(values):
        for j in range(4):
            out[i, j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


def enumerate_failures(cs, k, p, fixed, advice, mapping):
    """-> (failures [(kind, index, row)] sorted, counters).  advice / fixed canonical (columns, n, 4) u64; mapping None = copies unchecked."""
    import rowcheck
    n = 1 << k
    usable = n - (cs.blinding_factors() + 1)
    cols = {"fixed": [rowcheck.ints(fixed[i]) for i in range(cs.num_fixed)], "advice": [rowcheck.ints(advice[i]) for i in range(cs.num_advice)],
            "instance": [[0] * n for _ in range(cs.num_instance)]}
    fails = []
    for g, gate in enumerate(cs.gates):
        fails += [(GATE, g, r) for r in range(usable) if rowcheck._evaluate(gate, cols, r, n, p)]
    for li, (inputs, table) in enumerate(cs.lookups):
        rows = set(tuple(rowcheck._evaluate(t, cols, r, n, p) for t in table) for r in range(usable))
        fails += [(LOOKUP, li, r) for r in range(usable) if tuple(rowcheck._evaluate(e, cols, r, n, p) for e in inputs) not in rows]
    cells = 0
    if mapping is not None:
        m = np.asarray(mapping, dtype=np.int64).reshape(-1)
        flat = [v for kind, idx in cs.permutation_columns for v in cols[kind][idx]]
        for cell in np.nonzero(m != np.arange(m.size))[0].tolist():
            cells += 1
            if flat[cell] != flat[int(m[cell])]:
                fails.append((COPY, cell // n, cell % n))
    assert fails == sorted(fails)
    return fails, {"rows": usable, "lookup_inputs": usable * len(cs.lookups), "cells_in_cycles": cells}


def agrees_with_rowcheck(cs, k, p, fixed, advice, mapping):
    """rowcheck.verify (which assumes five blinding factors) returns the enumerator's counters for a satisfied witness and names its first failure otherwise"""
    import rowcheck
    assert cs.blinding_factors() == rowcheck.BLINDING_FACTORS == 5
    fails, counters = enumerate_failures(cs, k, p, fixed, advice, mapping)
    if not fails:
        assert rowcheck.verify(cs.description(), k, p, fixed, advice, mapping) == counters
        return fails
    with pytest.raises(AssertionError) as e:
        rowcheck.verify(cs.description(), k, p, fixed, advice, mapping)
    kind, index, row = fails[0]
    want = {GATE: "gate %d is not satisfied at row %d" % (index, row), LOOKUP: "lookup %d: the input of row %d is not in the table" % (index, row),
            COPY: "copy constraint between different values at cell %d" % (index * (1 << k) + row)}[kind]
    assert want in str(e.value)
    return fails


# ---------------------------------------------------------------------------------------------------------------------------- the cases
def case_zero_as_p(pkg, p, third=0):
    """R5 with the Fibonacci run p - 1, 1, 0, 1, 1, ...: the residual of the first row is -p as an integer.  `third`: the run's third value"""
    cs, fixed, advice, asm = build_circuit(pkg, "R5", 6)
    a = [0] * 64
    a[Q_LO], a[Q_LO + 1] = p - 1, 1
    for r in range(Q_LO, Q_HI):
        a[r + 2] = (a[r + 1] + a[r]) % p
    assert a[Q_LO + 2] == 0
    a[Q_LO + 2] = third
    advice = advice.copy()
    advice[0] = limbs(a, 64)
    advice[1, 40] = advice[0, Q_LO]
    return cs, fixed, advice, asm


def case_rlast_low(pkg, change=None):
    """Rlast with the selector on rows 0..27: rows 0..bf read b in the top unusable rows"""
    cs, fixed, advice, asm = build_circuit(pkg, "Rlast", 6)
    bf, n = cs.blinding_factors(), 64
    fixed = fixed.copy()
    fixed[0, :, 0] = 0
    fixed[0, 0:28, 0] = 1
    a = [0] * n
    a[0], a[1] = 1, 2
    for r in range(0, 28):
        a[r + 2] = a[r + 1] + a[r]
    b = [0] * n
    for r in range(0, 40):
        b[r] = 3 + r % (bf + 1)
    for r in range(n - (bf + 1), n):
        b[r] = b[(r + bf + 1) % n]
    b[40] = a[Q_LO]
    if change is not None:
        b[change] += 1
    advice = np.stack([limbs(a, n), limbs(b, n)])
    return cs, fixed, advice, asm


def case_many(pkg, p):
    """k = 8, R5 with the selector on rows 2..200 and every third a value off by one"""
    cs, fixed, advice, asm = build_circuit(pkg, "R5", 8)
    n = 256
    fixed = fixed.copy()
    fixed[0, :, 0] = 0
    fixed[0, 2:201, 0] = 1
    a = [0] * n
    a[2], a[3] = 1, 2
    for r in range(2, 201):
        a[r + 2] = (a[r + 1] + a[r]) % p
    for r in range(2, 203, 3):
        a[r] = (a[r] + 1) % p
    b = [0] * n
    b[40] = a[Q_LO]      # the copy constraint holds: gate failures only
    advice = np.stack([limbs(a, n), limbs(b, n)])
    return cs, fixed, advice, asm


def lookup_circuit(pkg, k, a_values=None, table_extra=None):
    """One advice a, fixed q (selector), t0 (tags), t1 (values).  Lookup A: q a in t1.  Lookup B: (q, q a) in (t0, t1) -- the tag of every selected row is 1.
    Table: row 0 (0, 0), rows 1..16 (1, 0..15), rows 17..20 (2, 100..103).  The selector is on for rows 0 .. 3 n / 4."""
    from dehalo2_amd import plonk as P
    n = 1 << k
    cs = P.ConstraintSystem(num_advice=1, num_fixed=3, num_instance=0)
    cs.enable_equality(P.ADVICE, 0)
    q, a = cs.query_fixed(0), cs.query_advice(0)
    t0, t1 = cs.query_fixed(1), cs.query_fixed(2)
    cs.lookup([(P.mul(q, a), t1)])
    cs.lookup([(q, t0), (P.mul(q, a), t1)])
    sel = 3 * n // 4
    fixed = np.zeros((3, n, 4), dtype=np.uint64)
    fixed[0, :sel, 0] = 1
    fixed[1, 1:17, 0], fixed[2, 1:17, 0] = 1, np.arange(16)
    fixed[1, 17:21, 0], fixed[2, 17:21, 0] = 2, 100 + np.arange(4)
    for row, (tag, value) in (table_extra or {}).items():
        fixed[1, row, 0], fixed[2, row, 0] = tag, value
    advice = np.zeros((1, n, 4), dtype=np.uint64)
    advice[0, :sel, 0] = np.arange(sel) % 16
    for row, v in (a_values or {}).items():
        advice[0, row, 0] = v
    return cs, fixed, advice, P.Assembly(1, n)


def mod_pow_circuit(pkg, broken):
    """the library's own mod_pow witness at k = 14 (1024-bit modulus: the smallest circuit with the RangeChip's two-column lookups)"""
    import random
    from dehalo2_amd import native, plonk
    rnd = random.Random(1024)
    n16, x16 = rnd.getrandbits(1024) | (1 << 1023) | 1, rnd.getrandbits(1000)
    nat = native.synthesize(native.CIRCUIT_MOD_POW, 14, n_big=n16, e=0b11, x=x16, exp_bits=2, bits_len=1024, keygen=True)
    cs = plonk.maingate_cs(True)
    asm = plonk.Assembly(6, 1 << 14)
    asm.mapping = nat["mapping"].astype(np.int64)
    advice = nat["advice"]
    if broken:
        row = int(np.nonzero(nat["selectors"][0])[0][0])      # a composition row: one limb no longer fits its eight bits
        advice = advice.copy()
        advice[0, row] = (1 << 8, 0, 0, 0)
    return cs, nat["fixed"], advice, asm, nat["selectors"]


@pytest.fixture(scope="module")
def mod_pow_broken(pkg):
    cs, fixed, advice, asm, sels = mod_pow_circuit(pkg, True)
    fails, counters = enumerate_failures(cs, 14, pkg.fields.BN254_FR.p, fixed, advice, asm.mapping)
    return dict(cs=cs, fixed=fixed, advice=advice, asm=asm, sels=sels, fails=fails, counters=counters)


def small_cases(pkg, p):
    """name -> (cs, k, fixed, advice, assembly): every small case of the GPU tests"""
    out = {}
    for name in ("R5", "R7", "R9all"):
        out[name] = build_circuit(pkg, name, 6)
    out["zero as p"] = case_zero_as_p(pkg, p)
    out["zero as p, third value 1"] = case_zero_as_p(pkg, p, 1)
    cs, fixed, advice, asm = build_circuit(pkg, "R7", 6)
    bad = advice.copy()
    bad[1, Q_LO + 9] = (5, 0, 0, 0)
    out["R7 one b value"] = (cs, fixed, bad, asm)
    out["Rlast low rows"] = case_rlast_low(pkg)
    out["Rlast low rows, b[60] changed"] = case_rlast_low(pkg, 60)
    cs, fixed, advice, asm = build_circuit(pkg, "R5", 6)
    bad = advice.copy()
    bad[1, 40, 0] += np.uint64(1)
    out["R5 copy"] = (cs, fixed, bad, asm)
    for name, kw in LOOKUP_CASES.items():
        out["lookup " + name] = lookup_circuit(pkg, 6, **kw(6))
    return {name: (c[0], int(c[1].shape[1]).bit_length() - 1, c[1], c[2], c[3]) for name, c in out.items()}


LOOKUP_CASES = {
    "satisfied": lambda k: {},
    "a = 16": lambda k: dict(a_values={(1 << k) // 2 + 5: 16}),
    "wrong tag": lambda k: dict(a_values={(1 << k) // 2 + 5: 101}),
    "table entry on an unusable row": lambda k: dict(a_values={(1 << k) // 2 + 5: 50}, table_extra={(1 << k) - 1: (1, 50)}),
}


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_enumerator_agrees_with_rowcheck_on_the_small_cases(pkg, oracles):
    p = pkg.fields.BN254_FR.p
    seen = {}
    for name, (cs, k, fixed, advice, asm) in small_cases(pkg, p).items():
        if name == "R9all":      # a is read at four rotations: six blinding factors, which rowcheck.verify does not know -- the enumerator alone
            assert cs.blinding_factors() == 6
            seen[name], counters = enumerate_failures(cs, k, p, fixed, advice, asm.mapping)
            assert counters["rows"] == 64 - 7
            continue
        seen[name] = agrees_with_rowcheck(cs, k, p, fixed, advice, asm.mapping)
    assert not seen["R5"] and not seen["R7"] and not seen["R9all"] and not seen["zero as p"] and not seen["Rlast low rows"] and not seen["lookup satisfied"]
    assert seen["zero as p, third value 1"] == [(GATE, 0, Q_LO), (GATE, 0, Q_LO + 1), (GATE, 0, Q_LO + 2)]
    assert seen["R7 one b value"] == [(GATE, 1, Q_LO + 4), (GATE, 1, Q_LO + 12)]      # the rows that read b[Q_LO + 9] at rotations +5 and -3
    assert seen["Rlast low rows, b[60] changed"] == [(GATE, 1, 2)]                    # row 2 reads b at 2 - 6 = 60 (mod 64)
    assert seen["R5 copy"] == [(COPY, 0, Q_LO), (COPY, 1, 40)]
    half = 32 + 5
    assert seen["lookup a = 16"] == [(LOOKUP, 0, half), (LOOKUP, 1, half)]
    assert seen["lookup wrong tag"] == [(LOOKUP, 1, half)]
    assert seen["lookup table entry on an unusable row"] == [(LOOKUP, 0, half), (LOOKUP, 1, half)]


def test_enumerator_agrees_with_rowcheck_on_the_larger_cases(pkg, oracles, mod_pow_broken):
    p = pkg.fields.BN254_FR.p
    cs, fixed, advice, asm = case_many(pkg, p)
    fails = agrees_with_rowcheck(cs, 8, p, fixed, advice, asm.mapping)
    assert len(fails) > 64 and len(fails) % 64 and len({r // 64 for _, _, r in fails}) >= 3 and {kind for kind, _, _ in fails} == {GATE}
    cs, fixed, advice, asm = lookup_circuit(pkg, 12, **LOOKUP_CASES["a = 16"](12))
    assert agrees_with_rowcheck(cs, 12, p, fixed, advice, asm.mapping) == [(LOOKUP, 0, 2053), (LOOKUP, 1, 2053)]
    m = mod_pow_broken
    assert {kind for kind, _, _ in m["fails"]} == {GATE, LOOKUP} and len(m["fails"]) == 2, m["fails"]
    import rowcheck
    with pytest.raises(AssertionError) as e:
        rowcheck.verify(m["cs"].description(), 14, p, m["fixed"], m["advice"], m["asm"].mapping)
    assert "gate %d is not satisfied at row %d" % m["fails"][0][1:] in str(e.value)


def test_null_arguments_are_rejected_without_a_device(pkg):
    from dehalo2_amd._lib import CCheckReport
    lib = pkg.load_library()
    rep = CCheckReport()
    assert lib.dehalo_check_witness(None, None, None, None, None, 0, None, 0, None, 0, C.byref(rep)) == -1
    assert lib.dehalo_check_witness(None, None, None, None, None, 0, None, 0, None, 0, None) == -1


# ---------------------------------------------------------------------------------------------------------------------------- GPU
S_SETUP = 0x5EED5EED5EED5EED


@pytest.fixture(scope="module")
def kzg_params(pkg, ctx):
    from dehalo2_amd import native
    cache = {}

    def get(k):
        if k not in cache:
            cache[k] = native.ParamsKZG.setup(ctx, pkg.fields.BN254, k, S_SETUP)
        return cache[k]

    yield get
    for prm in cache.values():
        prm.release()


def device_report(pkg, co, ctx, params, cs, fixed, advice, asm, selectors=(), mapping="asm", cap=64, form="mont"):
    """keygen + check_witness.  form: "mont" (host, Montgomery), "canonical" (host, plain integers), "device" (Montgomery, a device tensor)"""
    from dehalo2_amd import native
    pk = native.ProvingKey.keygen(ctx, params, cs, fixed, asm, selectors)
    try:
        fid = params.curve.scalar.id
        adv = advice if form == "canonical" else np.stack([co.field_op(fid, "to_mont", advice[i]) for i in range(advice.shape[0])])
        if form == "device":
            adv = ctx.upload(np.ascontiguousarray(adv))
        return pk.check_witness(adv, [[]] * cs.num_instance, assembly=asm if isinstance(mapping, str) else mapping, canonical=form == "canonical", cap=cap)
    finally:
        pk.release()


def same_report(rep, fails, counters, cap=64):
    assert rep.failures == fails[:cap], (rep.failures, fails[:cap])
    assert rep.written == min(cap, len(fails))
    assert (rep.gate_failures, rep.lookup_failures, rep.copy_failures) == tuple(sum(1 for f in fails if f[0] == kind) for kind in (GATE, LOOKUP, COPY))
    assert (rep.rows, rep.lookup_inputs, rep.cells_in_cycles) == (counters["rows"], counters["lookup_inputs"], counters["cells_in_cycles"])
    assert rep.ok == (not fails)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["R5", "R7", "R9all"])
def test_satisfied_circuits_report_nothing(pkg, co, ctx, kzg_params, name):
    p = pkg.fields.BN254_FR.p
    cs, fixed, advice, asm = build_circuit(pkg, name, 6)
    fails, counters = enumerate_failures(cs, 6, p, fixed, advice, asm.mapping)
    assert not fails and counters["cells_in_cycles"] == 2
    same_report(device_report(pkg, co, ctx, kzg_params(6), cs, fixed, advice, asm), fails, counters)


@pytest.mark.gpu
def test_satisfied_and_broken_over_vesta(pkg, po, co, ctx):
    """the other scalar field (pasta::Fp), a key made under ParamsIPA"""
    import plonk_oracle as PO
    from dehalo2_amd import native
    spec, p = pkg.fields.VESTA, pkg.fields.VESTA.scalar.p
    srs = PO.setup_srs(po.VESTA, 6, S_TOXIC, 8)
    uw = co.fixed_base_mul(spec.id, co.fill_scalars(spec.scalar.id, "uniform", 2, 7))
    params = native.ParamsIPA.create(ctx, spec, 6, srs["g"], srs["g_lagrange"], uw[1], uw[0])
    cs, fixed, advice, asm = build_circuit(pkg, "R7", 6)
    fails, counters = enumerate_failures(cs, 6, p, fixed, advice, asm.mapping)
    assert not fails
    same_report(device_report(pkg, co, ctx, params, cs, fixed, advice, asm), fails, counters)
    bad = advice.copy()
    bad[1, Q_LO + 9] = limbs([p - 1], 1)[0]
    fails, counters = enumerate_failures(cs, 6, p, fixed, bad, asm.mapping)
    assert fails == [(GATE, 1, Q_LO + 4), (GATE, 1, Q_LO + 12)]
    same_report(device_report(pkg, co, ctx, params, cs, fixed, bad, asm), fails, counters)
    params.release()


@pytest.mark.gpu
def test_the_librarys_own_witnesses_pass(pkg, co, ctx, kzg_params):
    """mod_pow at k = 14 (five two-column range lookups over one table) and pose_enc at K = 11 (no lookups, six permutation columns)"""
    from dehalo2_amd import native, plonk
    cs, fixed, advice, asm, sels = mod_pow_circuit(pkg, False)
    n = 1 << 14
    rep = device_report(pkg, co, ctx, kzg_params(14), cs, fixed, advice, asm, sels, form="canonical")
    cells = int(np.count_nonzero(np.asarray(asm.mapping).reshape(-1) != np.arange(6 * n)))
    assert rep.ok and rep.failures == [] and (rep.rows, rep.lookup_inputs, rep.cells_in_cycles) == (n - 6, 5 * (n - 6), cells) and cells > 0
    nat = native.synthesize(native.CIRCUIT_POSE_ENC, 11, key=[5, 6], message=[0, 0], keygen=True)
    cs = plonk.maingate_cs(False)
    asm = plonk.Assembly(6, 1 << 11)
    asm.mapping = nat["mapping"].astype(np.int64)
    rep = device_report(pkg, co, ctx, kzg_params(11), cs, nat["fixed"], nat["advice"], asm, form="canonical")
    cells = int(np.count_nonzero(asm.mapping.reshape(-1) != np.arange(6 << 11)))
    assert rep.ok and (rep.rows, rep.lookup_inputs, rep.cells_in_cycles) == ((1 << 11) - 6, 0, cells)


@pytest.mark.gpu
def test_zero_written_as_p(pkg, co, ctx, kzg_params):
    """a slot value is < 2p: a residual of -p must count as zero, and a residual of 1 - p must not"""
    p = pkg.fields.BN254_FR.p
    for third, want in ((0, []), (1, [(GATE, 0, Q_LO), (GATE, 0, Q_LO + 1), (GATE, 0, Q_LO + 2)])):
        cs, fixed, advice, asm = case_zero_as_p(pkg, p, third)
        fails, counters = enumerate_failures(cs, 6, p, fixed, advice, asm.mapping)
        assert fails == want
        same_report(device_report(pkg, co, ctx, kzg_params(6), cs, fixed, advice, asm), fails, counters)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["mont", "device", "canonical"])
def test_one_broken_gate_value(pkg, co, ctx, kzg_params, form):
    p = pkg.fields.BN254_FR.p
    cs, fixed, advice, asm = build_circuit(pkg, "R7", 6)
    bad = advice.copy()
    bad[1, Q_LO + 9] = (5, 0, 0, 0)
    fails, counters = enumerate_failures(cs, 6, p, fixed, bad, asm.mapping)
    assert fails == [(GATE, 1, Q_LO + 4), (GATE, 1, Q_LO + 12)]
    same_report(device_report(pkg, co, ctx, kzg_params(6), cs, fixed, bad, asm, form=form), fails, counters)


@pytest.mark.gpu
def test_the_usable_boundary_and_the_wrap(pkg, co, ctx, kzg_params):
    p = pkg.fields.BN254_FR.p
    n = 64
    # R5: b is queried at rotation 0 only, so b on the first unusable row is read by no usable row; R7: a is read at 0, 1, 2, so a[61] is read by rows 59..61
    for name, col, row in (("R5", 1, 58), ("R7", 0, 61)):
        cs, fixed, advice, asm = build_circuit(pkg, name, 6)
        usable = n - (cs.blinding_factors() + 1)
        assert usable == 58 and all((row - rot) % n >= usable for c, rot in cs.advice_queries if c == col)
        bad = advice.copy()
        bad[col, row] = (7, 0, 0, 0)
        fails, counters = enumerate_failures(cs, 6, p, fixed, bad, asm.mapping)
        assert not fails
        same_report(device_report(pkg, co, ctx, kzg_params(6), cs, fixed, bad, asm), fails, counters)
    for change, want in ((None, []), (60, [(GATE, 1, 2)]), (63, [(GATE, 1, 5)])):
        cs, fixed, advice, asm = case_rlast_low(pkg, change)
        fails, counters = enumerate_failures(cs, 6, p, fixed, advice, asm.mapping)
        assert fails == want
        same_report(device_report(pkg, co, ctx, kzg_params(6), cs, fixed, advice, asm), fails, counters)


@pytest.mark.gpu
def test_counts_order_and_cap(pkg, co, ctx, kzg_params):
    from dehalo2_amd import native
    from dehalo2_amd._lib import CCheckReport
    p = pkg.fields.BN254_FR.p
    cs, fixed, advice, asm = case_many(pkg, p)
    fails, counters = enumerate_failures(cs, 8, p, fixed, advice, asm.mapping)
    assert len(fails) > 64 and len(fails) % 64
    for cap in (1000, 10):
        same_report(device_report(pkg, co, ctx, kzg_params(8), cs, fixed, advice, asm, cap=cap), fails, counters, cap)
    # cap = 0 with failures = NULL, through the C ABI itself
    pk = native.ProvingKey.keygen(ctx, kzg_params(8), cs, fixed, asm, ())
    mapping = np.ascontiguousarray(asm.mapping, dtype=np.uint64)
    ptrs, lens = (C.c_void_p * 1)(), (C.c_size_t * 1)()
    rep = CCheckReport()
    rc = pkg.load_library().dehalo_check_witness(ctx.handle, pk.handle, np.ascontiguousarray(advice).ctypes.data, ptrs, lens, 0, mapping.ctypes.data, native.PROOF_ADVICE_CANONICAL,
                                                 None, 0, C.byref(rep))
    assert rc == 0 and (rep.gate_failures, rep.lookup_failures, rep.copy_failures, rep.written) == (len(fails), 0, 0, 0)
    pk.release()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 12])
def test_lookups(pkg, co, ctx, kzg_params, k):
    """k = 12: the table's 4090 usable rows are two sort tiles and a merge, and the broken row lies beyond row 2048"""
    p = pkg.fields.BN254_FR.p
    row = (1 << k) // 2 + 5
    want = {"satisfied": [], "a = 16": [(LOOKUP, 0, row), (LOOKUP, 1, row)], "wrong tag": [(LOOKUP, 1, row)],
            "table entry on an unusable row": [(LOOKUP, 0, row), (LOOKUP, 1, row)]}
    for name, kw in LOOKUP_CASES.items():
        cs, fixed, advice, asm = lookup_circuit(pkg, k, **kw(k))
        fails, counters = enumerate_failures(cs, k, p, fixed, advice, asm.mapping)
        assert fails == want[name], name
        same_report(device_report(pkg, co, ctx, kzg_params(k), cs, fixed, advice, asm), fails, counters)


@pytest.mark.gpu
def test_mod_pow_with_one_limb_too_wide(pkg, co, ctx, kzg_params, mod_pow_broken):
    m = mod_pow_broken
    assert {kind for kind, _, _ in m["fails"]} == {GATE, LOOKUP}
    same_report(device_report(pkg, co, ctx, kzg_params(14), m["cs"], m["fixed"], m["advice"], m["asm"], m["sels"], form="canonical"), m["fails"], m["counters"])


@pytest.mark.gpu
def test_copy_constraints(pkg, co, ctx, kzg_params):
    p = pkg.fields.BN254_FR.p
    cs, fixed, advice, asm = build_circuit(pkg, "R5", 6)
    bad = advice.copy()
    bad[1, 40, 0] += np.uint64(1)      # b is in no gate of R5
    fails, counters = enumerate_failures(cs, 6, p, fixed, bad, asm.mapping)
    assert fails == [(COPY, 0, Q_LO), (COPY, 1, 40)]
    same_report(device_report(pkg, co, ctx, kzg_params(6), cs, fixed, bad, asm), fails, counters)
    rep = device_report(pkg, co, ctx, kzg_params(6), cs, fixed, bad, asm, mapping=None)
    assert rep.ok and rep.copy_failures == 0 and rep.cells_in_cycles == 0 and rep.failures == []
    # an entry one past the last cell: an argument error, decided before anything follows the mapping; the context goes on working
    out_of_range = np.asarray(asm.mapping, dtype=np.uint64).copy().reshape(-1)
    out_of_range[5] = 2 * 64
    with pytest.raises(pkg.DehaloError) as e:
        device_report(pkg, co, ctx, kzg_params(6), cs, fixed, bad, asm, mapping=out_of_range)
    assert e.value.code == -1
    fails, counters = enumerate_failures(cs, 6, p, fixed, advice, asm.mapping)
    same_report(device_report(pkg, co, ctx, kzg_params(6), cs, fixed, advice, asm), fails, counters)


@pytest.mark.gpu
def test_the_check_means_what_the_verifier_says(pkg, po, co, ctx, kzg_chain):
    """a witness the check faults proves to a proof the verifier rejects; the unbroken witness is clean and its proof accepted"""
    import pairing as pr
    from dehalo2_amd import native, prover
    c = kzg_chain("R7", 6)
    params = native.ParamsKZG.create(ctx, pkg.fields.BN254, 6, c["srs"]["g"], c["srs"]["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(c["s_g2"]))
    pk = native.ProvingKey.keygen(ctx, params, c["cs"], c["fixed"], c["asm"], ())
    pk.transcript_repr = c["rep"]
    P = native.Prover(params, pk)
    bad = c["adv"].copy()
    bad[1, Q_LO + 9] = co.field_op(0, "to_mont", np.array([[5, 0, 0, 0]], dtype=np.uint64))[0]
    for adv, good in ((c["adv"], True), (bad, False)):
        rep = pk.check_witness(adv, [], assembly=c["asm"])
        assert rep.ok == good
        assert kzg_accepts(po, c, P.create_proof(adv, [], prover.SeededRng(7)).finalize()) == good
    P.release(); pk.release(); params.release()
