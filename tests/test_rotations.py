"""Circuits whose gates query rotations beyond {-1, 0, 1}: whole proofs under KZG / GWC and IPA, and the many-point evaluation behind them.

All circuits have two advice columns a, b (equality enabled on both: two permutation sets, so omega^last x is an opening point) and one fixed selector q,
on for rows 8..27; one copy constraint ties a[8] to b[40].  With `fib` = a(w^2 X) - a(w X) - a(X):
  R5     q fib                                                   rotations {last, -1, 0, 1, 2} (the prover's own four and 2)
  R7     R5 + q (b(w^5 X) - 2 b(w^-3 X))                         seven: two groups of four in the evaluation
  R9     R7 + q(w^3 X) q(w^-2 X) fib (holds wherever R5's does)  nine rotations, eight opening points
  R9all  R9 with q(w^3 X) q(w^-2 X) (a(w X) - a(X) - a(w^-1 X))  as well: a is read at -1, so all nine rotations are opening points and GWC divides in two launches
  Rlast  R5 + q (b(w^-(bf+1) X) - b(X))                          the query lands on the prover's own last rotation: still five
CPU: the restatements' proofs of every circuit are accepted under both schemes (oracle/plonk_oracle.py + oracle/verifier.py, oracle/ipa.py) and a one-value
tamper is rejected.
GPU: native proofs byte-identical to the restatements', accepted, of proof_size() bytes; dehalo_eval_polynomial_points_device against the C restatement of
eval_polynomial; a rotation-{-1, 0, 1} circuit still proves to the restatement's bytes."""
import numpy as np
import pytest

from proof_chains import S_TOXIC      # noqa: F401  (tests/test_check_witness.py takes it from here)

NAMES = ["R5", "R7", "R9", "R9all", "Rlast"]
Q_LO, Q_HI = 8, 28


def build_circuit(pkg, name, k):
    """-> (cs, fixed (1, n, 4), advice (2, n, 4) canonical, assembly)"""
    from dehalo2_amd import plonk
    P = plonk
    n = 1 << k
    cs = P.ConstraintSystem(num_advice=2, num_fixed=1, num_instance=0)
    cs.enable_equality(P.ADVICE, 0)
    cs.enable_equality(P.ADVICE, 1)
    q = cs.query_fixed(0)
    a0, a1, a2 = cs.query_advice(0, 0), cs.query_advice(0, 1), cs.query_advice(0, 2)
    fib = P.sum_(a2, ("neg", a1), ("neg", a0))
    gates = [P.mul(q, fib)]
    if name in ("R7", "R9", "R9all"):
        gates.append(P.mul(q, P.sum_(cs.query_advice(1, 5), ("neg", ("scaled", cs.query_advice(1, -3), 2)))))
    if name in ("R9", "R9all"):
        both = P.mul(cs.query_fixed(0, 3), cs.query_fixed(0, -2))      # non-zero on rows Q_LO + 2 .. Q_HI - 4 only
        gates.append(P.mul(both, fib))
        if name == "R9all":
            gates.append(P.mul(both, P.sum_(a1, ("neg", a0), ("neg", cs.query_advice(0, -1)))))      # fib one row up
    bf = cs.blinding_factors()
    if name == "Rlast":
        gates.append(P.mul(q, P.sum_(cs.query_advice(1, -(bf + 1)), ("neg", cs.query_advice(1, 0)))))
        assert cs.blinding_factors() == bf
    cs.create_gate(gates)
    fixed = np.zeros((1, n, 4), dtype=np.uint64)
    fixed[0, Q_LO:Q_HI, 0] = 1
    advice = np.zeros((2, n, 4), dtype=np.uint64)
    a = [0] * 48
    a[Q_LO], a[Q_LO + 1] = 1, 2
    for r in range(Q_LO, Q_HI):
        a[r + 2] = a[r + 1] + a[r]
    b = [0] * 48
    if name == "Rlast":
        for r in range(0, 40):
            b[r] = 3 + r % (bf + 1)                       # b(row - (bf + 1)) = b(row)
    else:
        for r in range(Q_LO - 3, Q_LO + 5):
            b[r] = 11 + r
        for r in range(Q_LO, Q_HI):
            b[r + 5] = 2 * b[r - 3]
    b[40] = a[Q_LO]
    advice[0, :48, 0], advice[1, :48, 0] = a, b
    assert 48 <= n - (bf + 1)
    asm = P.Assembly(2, n)
    asm.copy(0, Q_LO, 1, 40)
    return cs, fixed, advice, asm


def rotations_of(cs):
    bf = cs.blinding_factors()
    return sorted({0, 1, -1, -(bf + 1)} | {r for _, r in cs.advice_queries} | {r for _, r in cs.fixed_queries})


def opening_points_of(cs):
    """the distinct rotations somebody opens at: the queries, the permutation products at 0, 1 and (all sets but the last) `last`"""
    pts = {r for _, r in cs.advice_queries} | {r for _, r in cs.fixed_queries} | {0, 1}
    if cs.num_permutation_sets() > 1:
        pts.add(-(cs.blinding_factors() + 1))
    return sorted(pts)


def test_the_circuits_have_the_rotations_they_are_named_for(pkg):
    want = {"R5": (5, 4), "R7": (7, 6), "R9": (9, 8), "R9all": (9, 9), "Rlast": (5, 4)}
    for name in NAMES:
        cs = build_circuit(pkg, name, 6)[0]
        assert (len(rotations_of(cs)), len(opening_points_of(cs))) == want[name], name
        assert cs.degree() == 3 and cs.num_permutation_sets() == 2
    cs = build_circuit(pkg, "Rlast", 6)[0]
    assert (1, -(cs.blinding_factors() + 1)) in cs.advice_queries


def _chains(pkg, po, co, make):
    """(name, k) -> tests/proof_chains.py's chain of build_circuit(name, k), with the circuit"""
    cache = {}

    def get(name, k):
        if (name, k) not in cache:
            cs, fixed, advice, asm = build_circuit(pkg, name, k)
            cache[(name, k)] = dict(make(po, co, cs.description(), k, fixed, asm.mapping, advice), cs=cs, fixed=fixed, asm=asm)
        return cache[(name, k)]

    return get


@pytest.fixture(scope="module")
def kzg_chain(pkg, po, co):
    """... and `want`, the restatement's proof under ScalarStream(7)"""
    import proof_chains as PC
    get = _chains(pkg, po, co, PC.kzg_chain)

    def with_proof(name, k):
        c = get(name, k)
        if "want" not in c:
            c["want"] = PC.prove(po, c, [])[0]
        return c

    return with_proof


def kzg_accepts(po, c, proof):
    import proof_chains as PC
    return PC.accepts(po, c, proof, [])


def num_commitments(cs):
    return cs.num_advice + 3 * len(cs.lookups) + cs.num_permutation_sets() + 1 + (cs.degree() - 1)


def num_evals(cs):
    S = cs.num_permutation_sets()
    return len(cs.advice_queries) + len(cs.fixed_queries) + 1 + len(cs.permutation_columns) + (3 * S - 1) + 5 * len(cs.lookups)


def tampered(c, proof):
    import proof_chains as PC
    assert c["key"]["shape"].num_advice + c["key"]["shape"].num_sets + 1 + (c["key"]["shape"].degree - 1) == num_commitments(c["cs"])      # (no lookups here)
    return PC.tampered(c, proof)


@pytest.mark.parametrize("name", NAMES)
def test_kzg_restatement_handles_the_circuit(pkg, po, kzg_chain, name):
    c = kzg_chain(name, 6)
    cs, proof = c["cs"], c["want"]
    assert len(proof) == 32 * (num_commitments(cs) + num_evals(cs) + len(opening_points_of(cs)))
    assert kzg_accepts(po, c, proof)
    assert not kzg_accepts(po, c, tampered(c, proof))


def test_kzg_restatement_rejects_a_broken_witness(pkg, po, co, kzg_chain):
    """the wide gates are live: one b value of R7 off by one and the verifier refuses"""
    import plonk_oracle as PO
    c = kzg_chain("R7", 6)
    adv = c["adv"].copy()
    adv[1, Q_LO + 9] = co.field_op(0, "to_mont", np.array([[5, 0, 0, 0]], dtype=np.uint64))[0]
    bad, _ = PO.create_proof(po.BN254, c["srs"], c["key"], adv, [], PO.ScalarStream(7), c["rep"], 8)
    assert not kzg_accepts(po, c, bad)


@pytest.fixture(scope="module")
def ipa_chain(pkg, po, co):
    import proof_chains as PC
    return _chains(pkg, po, co, PC.ipa_chain)


def ipa_reference(pkg, po, c):
    import proof_chains as PC
    return PC.prove(po, c, [])


def ipa_accepts(pkg, po, co, c, proof):
    import proof_chains as PC
    return PC.accepts(po, c, proof, [])


@pytest.mark.parametrize("name", NAMES)
def test_ipa_restatement_handles_the_circuit(pkg, po, co, ipa_chain, name):
    c = ipa_chain(name, 6)
    cs = c["cs"]
    proof, trace = ipa_reference(pkg, po, c)
    # an advice commitment is opened at exactly the rotations its column is read at: a point set of that size exists
    assert max(cs.num_advice_queries()) in [len(ps) for ps in trace["point_sets"]]
    assert len(proof) == 32 * (num_commitments(cs) + num_evals(cs) + 1 + len(trace["point_sets"]) + 1 + 2 * 6 + 2)
    assert ipa_accepts(pkg, po, co, c, proof)
    assert not ipa_accepts(pkg, po, co, c, tampered(c, proof))


# ------------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [("R5", 6), ("R7", 6), ("R9", 6), ("R9all", 6), ("Rlast", 6), ("R7", 12)])
def test_native_kzg_proof_of_a_wide_rotation_circuit(pkg, po, ctx, kzg_chain, name, k):
    """Refused with DEHALO_ERR_UNSUPPORTED before the many-point evaluation existed.  k = 12: 4096 coefficients, two levels of the 2048-wide reduction."""
    import pairing as pr
    import plonk_oracle as PO
    from dehalo2_amd import native, prover

    c = kzg_chain(name, k)
    params = native.ParamsKZG.create(ctx, pkg.fields.BN254, k, c["srs"]["g"], c["srs"]["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(c["s_g2"]))
    pk = native.ProvingKey.keygen(ctx, params, c["cs"], c["fixed"], c["asm"], ())
    assert pk.vk_bytes() == PO.vk_bytes(po.BN254, c["key"])
    pk.transcript_repr = c["rep"]
    P = native.Prover(params, pk)
    proof = P.create_proof(c["adv"], [], prover.SeededRng(7)).finalize()
    want = c["want"]
    assert len(proof) == P.proof_size() == len(want)
    diff = [i // 32 for i in range(0, len(want), 32) if proof[i:i + 32] != want[i:i + 32]]
    assert not diff, "proof items differ from the oracle's: %r" % diff[:8]
    assert kzg_accepts(po, c, proof)
    assert P.create_proof(c["adv"], [], prover.SeededRng(7)).finalize() == want      # the prover's buffers are clean for the next proof
    P.release(); pk.release(); params.release()


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [("R5", 6), ("R7", 6), ("R9all", 6), ("Rlast", 6), ("R7", 12)])
def test_native_ipa_proof_of_a_wide_rotation_circuit(pkg, po, co, ctx, ipa_chain, name, k):
    """Byte-identical to the reference at k = 6; accepted at k = 12 (the reference comparison stops at small k, as in tests/test_ipa_proof.py)."""
    import plonk_oracle as PO
    from dehalo2_amd import native, prover

    c = ipa_chain(name, k)
    spec = pkg.fields.VESTA
    params = native.ParamsIPA.create(ctx, spec, k, c["srs"]["g"], c["srs"]["g_lagrange"], c["w"], c["u"])
    pk = native.ProvingKey.keygen(ctx, params, c["cs"], c["fixed"], c["asm"], ())
    assert pk.vk_bytes() == PO.vk_bytes(po.VESTA, dict(c["key"], fixed_commitments=c["fc"], perm_commitments=c["pc"]))
    pk.transcript_repr = c["rep"]
    P = native.Prover(params, pk)
    proof = P.create_proof(c["adv"], [], prover.SeededRng(7)).finalize()
    assert len(proof) == P.proof_size()
    if k <= 6:
        want = ipa_reference(pkg, po, c)[0]
        assert len(proof) == len(want)
        diff = [i // 32 for i in range(0, len(want), 32) if proof[i:i + 32] != want[i:i + 32]]
        assert not diff, "proof items differ from the reference's: %r" % diff[:8]
    assert ipa_accepts(pkg, po, co, c, proof)
    P.release(); pk.release(); params.release()


@pytest.fixture(scope="module")
def eval_case(pkg, co):
    """per field: 97 polynomials of 4097 coefficients, 32 points, and every value the tests compare with (computed once)"""
    cache = {}

    def get(fname):
        if fname not in cache:
            f = pkg.fields.FIELDS[fname]
            cols = np.stack([co.fill_scalars(f.id, "uniform", 4097, 700 + i) for i in range(97)])
            pts = co.fill_scalars(f.id, "uniform", 32, 19)
            cache[fname] = dict(f=f, cols=cols, pts=pts, ref={})
        return cache[fname]

    return get


def _ref(co, case, length, b, i):
    key = (length, b, i)
    if key not in case["ref"]:
        case["ref"][key] = co.eval_polynomial(case["f"].id, case["cols"][b, :length], case["pts"][i], 1)
    return case["ref"][key]


@pytest.mark.gpu
@pytest.mark.parametrize("fname", ["bn254_fr", "pasta_fp", "pasta_fq"])
@pytest.mark.parametrize("length", [1, 2047, 2048, 2049, 4097])
def test_eval_polynomial_points_vs_oracle(pkg, co, ctx, eval_case, fname, length):
    """Every num_points in {1, 4, 5, 8, 9, 32} x count in {1, 97} (one past POLY_MP_POLYS): dense against the C restatement at sampled (polynomial, point) pairs
    that cover every point and both launches of 97; sparse random masks (polynomial 0: empty) equal to the dense values where wanted and zero elsewhere."""
    import torch

    case = eval_case(fname)
    f, cols, pts = case["f"], case["cols"], case["pts"]
    d = ctx.upload(np.ascontiguousarray(cols[:, :length]))
    rng = np.random.default_rng(length)
    for npts in (1, 4, 5, 8, 9, 32):
        for count in (1, 97):
            ptrs = [d[b].data_ptr() for b in range(count)]
            out = torch.full((npts, count, 4), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ctx.eval_polynomial_points_device(f.id, ptrs, length, pts[:npts], out.data_ptr())
            ctx.synchronize()
            got = out.cpu().numpy().view(np.uint64)
            for i in range(npts):
                for b in sorted({0, (7 * i + 3) % count, count - 1}):
                    assert np.array_equal(got[i, b], _ref(co, case, length, b, i)), (npts, count, i, b)
            wanted = [int(x) & ((1 << npts) - 1) for x in rng.integers(0, 1 << 32, size=count)]
            wanted[0] = 0
            wanted[-1] = wanted[-1] if count == 1 else (1 << npts) - 1
            out2 = torch.full((npts, count, 4), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ctx.eval_polynomial_points_device(f.id, ptrs, length, pts[:npts], out2.data_ptr(), wanted=wanted)
            ctx.synchronize()
            got2 = out2.cpu().numpy().view(np.uint64)
            mask = np.array([[(wanted[b] >> i) & 1 for b in range(count)] for i in range(npts)], dtype=bool)
            assert np.array_equal(got2, np.where(mask[:, :, None], got, np.uint64(0))), (npts, count)
            assert not got2[:, 0].any()


@pytest.mark.gpu
def test_eval_polynomial_points_argument_checks(pkg, ctx, co):
    import torch
    from dehalo2_amd._lib import DehaloError

    f = pkg.fields.FIELDS["bn254_fr"]
    d = ctx.upload(co.fill_scalars(f.id, "uniform", 16, 5).reshape(1, 16, 4))
    out = torch.zeros((33, 1, 4), dtype=torch.int64, device="cuda")
    pts = co.fill_scalars(f.id, "uniform", 33, 6)
    for npts in (0, 33):
        with pytest.raises(DehaloError) as e:
            ctx.eval_polynomial_points_device(f.id, [d[0].data_ptr()], 16, pts[:npts], out.data_ptr())
        assert e.value.code == -1
    for wanted in (None, [0x1f]):      # the four-point entry points keep their contract
        with pytest.raises(DehaloError) as e:
            ctx.eval_polynomial_multi_device(f.id, [d[0].data_ptr()], 16, pts[:5], out.data_ptr(), wanted=wanted)
        assert e.value.code == -1
    ctx.eval_polynomial_points_device(f.id, [d[0].data_ptr()], 16, pts[:32], out.data_ptr())
    ctx.synchronize()


@pytest.mark.gpu
def test_narrow_rotation_circuit_is_unchanged(pkg, po, co, ctx):
    """Rotations {-1, 0, 1} only (circuits.synthesize, k = 9, range lookups): the four-point path, byte for byte the CPU restatement's proof."""
    import pairing as pr
    import plonk_oracle as PO
    import shapes
    from dehalo2_amd import circuits, native, prover

    k, s, oc = 9, 0x5EED, po.BN254
    circ = circuits.synthesize(oc.scalar.p, k, True, seed=3)
    assert rotations_of(circ.cs) == sorted([0, 1, -1, -(circ.cs.blinding_factors() + 1)])
    desc = shapes.maingate_description(True)
    srs = PO.setup_srs(oc, k, s, 8)
    key = PO.keygen(oc, srs, desc, k, circ.fixed, circ.assembly.mapping, 8)
    rep = PO.transcript_repr(oc, key, circ.selectors)
    adv = np.stack([co.field_op(0, "to_mont", circ.advice[i]) for i in range(5)])
    kzg = native.ParamsKZG.create(ctx, pkg.fields.BN254, k, srs["g"], srs["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(pr.g2_mul(s, pr.G2)))
    pk = native.ProvingKey.keygen(ctx, kzg, circ.cs, circ.fixed, circ.assembly, circ.selectors)
    pk.transcript_repr = rep
    P = native.Prover(kzg, pk)
    got = P.create_proof(adv, [[]], prover.SeededRng(7)).finalize()
    want, _ = PO.create_proof(oc, srs, key, adv, [[]], PO.ScalarStream(7), rep, 8)
    assert got == want and len(got) == P.proof_size()
    P.release(); pk.release(); kzg.release()
