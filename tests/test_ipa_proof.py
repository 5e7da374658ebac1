"""Whole ProverIPA proofs over Vesta: blinded commitments (dehalo_blind_commitments_device), committed instance columns, ProverIPA's multiopen and the
opening argument behind dehalo_create_proof with ParamsIPA.

CPU: the Python restatement of the prover (oracle/plonk_oracle.py create_proof_ipa) is accepted by the restatement of the verifier (oracle/verifier.py) at
k = 5 and 6 (and k = 9 with range lookups, the smallest size their table fits); every tampering is rejected; a proof made with Blind::default() = 0 is rejected by the verifier's 1; the query
grouping is checked on a hand-written list.
GPU: the blinding kernel against the C restatement of best_multiexp; native.Prover with ParamsIPA accepted at k = 6, 9, 11, 14, byte-identical to the
reference under one seeded stream at k = 6 and 9, of the length proof_size() reports, deterministic, fresh under OS entropy, equal with a side context; one
instance column; and the KZG path's bytes unchanged afterwards."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def F(pkg):
    return pkg.fields


@pytest.fixture(scope="module")
def ipa_chain(pkg, po, co):
    """(k, range_lookups) -> tests/proof_chains.py's IPA chain of circuits.synthesize(p, k, range_lookups, seed=3), with the circuit."""
    import proof_chains as PC
    import shapes
    from dehalo2_amd import circuits

    cache = {}

    def get(k, rl):
        if (k, rl) not in cache:
            circ = circuits.synthesize(po.VESTA.scalar.p, k, rl, seed=3)
            desc = shapes.maingate_description(rl)
            assert desc == circ.cs.description()
            cache[(k, rl)] = dict(PC.ipa_chain(po, co, desc, k, circ.fixed, circ.assembly.mapping, circ.advice, circ.selectors), circ=circ)
        return cache[(k, rl)]

    return get


def reference_proof(po, c, instances=([],), **kw):
    import proof_chains as PC
    return PC.prove(po, c, instances, **kw)


def accepts(po, c, proof, instances=([],)):
    import proof_chains as PC
    return PC.accepts(po, c, proof, instances)


def layout(po, c, k):
    """byte offsets of the proof's parts: advice commitments, evaluations, f, q_evals, the opening's c"""
    import plonk_oracle as PO
    sh = PO.Shape(c["desc"], k, po.VESTA.scalar)
    L = len(sh.lookups)
    points = sh.num_advice + 2 * L + sh.num_sets + L + 1 + (sh.degree - 1)
    evals = len(sh.instance_queries) + len(sh.advice_queries) + len(sh.fixed_queries) + 1 + len(sh.perm_columns) + (3 * sh.num_sets - 1) + 5 * L
    return dict(advice=0, eval=32 * points, f=32 * (points + evals), q_eval=32 * (points + evals + 1), evals=evals, points=points)


def tamperings(po, c, k, proof):
    lo = layout(po, c, k)
    out = {}
    for name, off in [("advice commitment", lo["advice"] + 32), ("evaluation", lo["eval"] + 64), ("f", lo["f"]), ("q_eval", lo["q_eval"] + 32), ("c", len(proof) - 64)]:
        bad = bytearray(proof)
        bad[off + 5] ^= 0x04
        out[name] = bytes(bad)
    out["truncated"] = proof[:-32]
    out["trailing byte"] = proof + b"\0"
    return out


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def test_grouping_on_a_hand_written_query_list(oracles):
    import ipa as V
    x, xw, xi = "x", "omega x", "omega^-1 x"
    queries = [("a", x), ("b", x), ("b", xw), ("z", x), ("z", xw), ("p", x), ("p", xi), ("c", xw), ("b", x), ("s", x), ("d", xi), ("d", x)]
    commitments, point_sets = V.construct_intermediate_sets(queries)
    # points by first appearance: x = 0, omega x = 1, omega^-1 x = 2; sets by first appearance over the commitments a, b, z, p, c, s, d
    assert point_sets == [[x], [x, xw], [x, xi], [xw]]
    assert [(key, si) for key, si, _ in commitments] == [("a", 0), ("b", 1), ("z", 1), ("p", 2), ("c", 3), ("s", 0), ("d", 2)]
    assert dict((key, pis) for key, _, pis in commitments)["b"] == [0, 1, 0] and dict((key, pis) for key, _, pis in commitments)["d"] == [2, 0]


def test_lagrange_eval(po):
    import ipa as V
    p = po.VESTA.scalar.p
    poly = [5, 7, 11]
    pts = [3, 10, 77]
    evs = [po.eval_polynomial(po.VESTA.scalar, poly, t) for t in pts]
    assert V.lagrange_eval(pts, evs, 123456, p) == po.eval_polynomial(po.VESTA.scalar, poly, 123456)


@pytest.mark.parametrize("k,rl", [(5, False), (6, False), (9, True)])
def test_reference_proof_is_accepted_and_tampering_rejected(po, co, F, ipa_chain, k, rl):
    """k = 5 and 6 without range lookups; with them at k = 9, the smallest size circuits.synthesize takes (the range table alone has 339 rows: at k = 5
    and 6 it refuses with "k too small for the range table")."""
    c = ipa_chain(k, rl)
    proof, trace = reference_proof(po, c)
    lo = layout(po, c, k)
    # {x}, {x, omega x}, {x, omega x, omega^last x} and, with lookups, {x, omega^-1 x}
    assert [len(ps) for ps in trace["point_sets"]] == ([1, 2, 3, 2] if rl else [1, 2, 3])
    assert len(proof) == 32 * (lo["points"] + lo["evals"] + 1 + len(trace["point_sets"]) + 1 + 2 * k + 2)
    assert accepts(po, c, proof)
    for name, bad in tamperings(po, c, k, proof).items():
        assert not accepts(po, c, bad), name
    assert not accepts(po, c, proof, instances=([1],))


def test_default_blind_is_live(pkg, po, co):
    """A prover that takes Blind::default() = 0 for the instance, fixed and sigma commitments is rejected by the verifier, which takes 1."""
    import inspect

    import ipa
    import plonk_oracle as PO
    import verifier as V
    assert ipa.DEFAULT_BLIND == 1      # ... which the prover and the verifier both take unless told otherwise
    assert all(inspect.signature(fn).parameters["default_blind"].default is ipa.DEFAULT_BLIND for fn in (PO.create_proof_ipa, V.verify_proof_ipa, ipa.ProverIPA))
    c, cs, fixed, asm, inst = _instance_chain(pkg, po, co, 5)      # (a non-empty instance column: its bare MSM is not the identity)
    assert accepts(po, c, reference_proof(po, c, instances=(inst,))[0], instances=(inst,))
    assert not accepts(po, c, reference_proof(po, c, instances=(inst,), default_blind=0)[0], instances=(inst,))
    assert not accepts(po, c, reference_proof(po, c, instances=(inst,))[0], instances=([5, 7, 10, 11],))


def test_ipa_proof_abi_is_refused_without_device(pkg):
    lib = pkg.load_library()
    assert lib.dehalo_blind_commitments_device(None, 2, None, None, 0, None, None) == -1
    assert lib.dehalo_prover_proof_size(None) == 0


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _blind_case(ctx, co, cs, jac_in, blinds_int, w):
    import torch
    d = ctx.upload(jac_in)
    b = ctx.upload(cs.scalar.encode_many([x % cs.scalar.p for x in blinds_int]))
    dw = ctx.upload(np.asarray(w, dtype=np.uint64).reshape(1, 8))
    ctx.blind_commitments_device(cs.id, d.data_ptr(), b.data_ptr(), jac_in.shape[0], dw.data_ptr(), 0)
    torch.cuda.synchronize()
    out = np.asarray(ctx.download_tensor(d)).view(np.uint64).reshape(-1, 12)
    return np.stack([co.to_affine(cs.id, row) for row in out]).reshape(-1, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", ["vesta", "pallas"])
@pytest.mark.parametrize("m", [1, 5, 64])
def test_blind_commitments_match_best_multiexp(ctx, co, F, curve_name, m):
    """C_i + [b_i] W against best_multiexp over [bases | W] with the blind as one more scalar; an identity MSM result and a zero blind included."""
    cs = F.CURVES[curve_name]
    p = cs.scalar.p
    n = 16
    bases = co.synth_bases(cs.id, n + 1)
    w = bases[n]
    rng = np.random.default_rng(40 + m)
    blinds = [int.from_bytes(rng.bytes(32), "little") % p for _ in range(m)]
    blinds[0] = 0                                                    # a zero blind: the point stays
    scal = [[int.from_bytes(rng.bytes(32), "little") % p for _ in range(n)] for _ in range(m)]
    if m > 1:
        scal[1] = [0] * n                                            # an identity MSM result: [b] W alone
        blinds[m - 1] = p - 1
    if m > 2:
        scal[2], blinds[2] = [0] * n, 0                              # both: the identity stays the identity
    jac = np.stack([co.best_multiexp(cs.id, cs.scalar.encode_many(s), bases[:n], 1) for s in scal]).reshape(m, 12)
    want = np.stack([co.to_affine(cs.id, co.best_multiexp(cs.id, cs.scalar.encode_many(s + [b]), bases, 1)) for s, b in zip(scal, blinds)]).reshape(m, 8)
    got = _blind_case(ctx, co, cs, jac, blinds, w)
    assert np.array_equal(got, want)
    if m > 2:
        assert not got[2].any() and got[1].any()


@pytest.mark.gpu
def test_blind_commitments_cancel_and_double(ctx, co, F):
    """C = [1] W with blind -1 (the identity) and blind 1 (the doubling), the edge cases of test_collapse_edge_cases."""
    cs = F.VESTA
    p = cs.scalar.p
    w = co.synth_bases(cs.id, 3)[2]
    one = co.best_multiexp(cs.id, cs.scalar.encode_many([1]), w.reshape(1, 8), 1).reshape(1, 12)
    jac = np.concatenate([one, one, one])
    blinds = [p - 1, 1, 2]
    want = np.stack([co.to_affine(cs.id, co.best_multiexp(cs.id, cs.scalar.encode_many([(1 + b) % p]), w.reshape(1, 8), 1)) for b in blinds]).reshape(3, 8)
    got = _blind_case(ctx, co, cs, jac, blinds, w)
    assert np.array_equal(got, want) and not got[0].any()


@pytest.mark.gpu
def test_blind_commitments_argument_checks(ctx, pkg, F):
    import torch
    lib = pkg.load_library()
    d = torch.zeros((8, 12), dtype=torch.int64, device="cuda")
    b = torch.zeros((8, 4), dtype=torch.int64, device="cuda")
    w = torch.zeros((1, 8), dtype=torch.int64, device="cuda")
    v = F.VESTA.id
    assert lib.dehalo_blind_commitments_device(ctx.handle, v, None, b.data_ptr(), 8, w.data_ptr(), None) == -1           # null points
    assert lib.dehalo_blind_commitments_device(ctx.handle, v, d.data_ptr(), None, 8, w.data_ptr(), None) == -1           # null blinds
    assert lib.dehalo_blind_commitments_device(ctx.handle, v, d.data_ptr(), b.data_ptr(), 8, None, None) == -1           # null W
    assert lib.dehalo_blind_commitments_device(ctx.handle, F.BN254.id, d.data_ptr(), b.data_ptr(), 8, w.data_ptr(), None) == -5      # not Pasta
    assert lib.dehalo_blind_commitments_device(ctx.handle, v, d.data_ptr(), b.data_ptr(), 1 << 29, w.data_ptr(), None) == -1        # size
    assert lib.dehalo_blind_commitments_device(ctx.handle, v, None, None, 0, w.data_ptr(), None) == 0                    # nothing to do


@pytest.fixture(scope="module")
def native_ipa(pkg, ctx, ipa_chain):
    from dehalo2_amd import native

    cache = {}

    def get(k, rl):
        if (k, rl) not in cache:
            c = ipa_chain(k, rl)
            params = native.ParamsIPA.create(ctx, pkg.fields.VESTA, k, c["srs"]["g"], c["srs"]["g_lagrange"], c["w"], c["u"])
            pk = native.ProvingKey.keygen(ctx, params, c["circ"].cs, c["circ"].fixed, c["circ"].assembly, c["circ"].selectors)
            pk.transcript_repr = c["rep"]
            cache[(k, rl)] = dict(params=params, pk=pk)
        return cache[(k, rl)]

    yield get
    for v in cache.values():
        v["pk"].release()
        v["params"].release()


@pytest.mark.gpu
@pytest.mark.parametrize("k,rl", [(6, False), (9, True), (11, False), (14, True)])
def test_native_ipa_proof_is_accepted(pkg, po, co, F, ctx, ipa_chain, native_ipa, k, rl):
    import plonk_oracle as PO
    from dehalo2_amd import native, prover

    c, d = ipa_chain(k, rl), native_ipa(k, rl)
    # the verifying key under IPA: the oracle's commitments + [Blind::default()] W
    assert d["pk"].vk_bytes() == PO.vk_bytes(po.VESTA, c["ipa_key"], c["circ"].selectors)
    P = native.Prover(d["params"], d["pk"])
    proof = P.create_proof(c["adv"], [[]], prover.SeededRng(7)).finalize()
    lo = layout(po, c, k)
    assert len(proof) == P.proof_size()
    assert len(proof) == 32 * (lo["points"] + lo["evals"] + 1 + (4 if rl else 3) + 1 + 2 * k + 2)
    assert accepts(po, c, proof)
    if k <= 9:
        for name, bad in tamperings(po, c, k, proof).items():
            assert not accepts(po, c, bad), name
    t = P.last_timings()
    assert t["total"] > 0 and t["openings"] > 0
    P.release()


@pytest.mark.gpu
@pytest.mark.parametrize("k,rl", [(6, False), (9, True)])
def test_native_ipa_proof_matches_the_reference(pkg, po, co, F, ctx, ipa_chain, native_ipa, k, rl):
    """Byte for byte under SeededRng(7); the caller's generator ends where the reference's ends."""
    import plonk_oracle as PO
    from dehalo2_amd import native, prover

    c, d = ipa_chain(k, rl), native_ipa(k, rl)
    ref = PO.ScalarStream(7)
    want = PO.create_proof_ipa(po.VESTA, c["srs"], c["u"], c["w"], c["key"], c["adv"], [[]], ref, c["rep"], 8)[0]
    P = native.Prover(d["params"], d["pk"])
    rng = prover.SeededRng(7)
    got = P.create_proof(c["adv"], [[]], rng).finalize()
    assert len(got) == len(want)
    diff = [i // 32 for i in range(0, len(want), 32) if got[i:i + 32] != want[i:i + 32]]
    assert not diff, "proof items differ from the reference's: %r" % diff[:8]
    assert np.array_equal(rng.scalars(2), ref.scalars(2))
    P.release()


@pytest.mark.gpu
def test_native_ipa_determinism_entropy_and_side_context(pkg, po, co, F, ctx, ipa_chain, native_ipa):
    from dehalo2_amd import native, prover

    k, rl = 9, True
    c, d = ipa_chain(k, rl), native_ipa(k, rl)
    P = native.Prover(d["params"], d["pk"])
    a = P.create_proof(c["adv"], [[]], prover.SeededRng(7)).finalize()
    assert P.create_proof(c["adv"], [[]], prover.SeededRng(7)).finalize() == a
    b = P.create_proof(c["adv"], [[]], prover.SeededRng(8)).finalize()
    assert b != a and accepts(po, c, b)
    p1, p2 = P.create_proof(c["adv"], [[]]).finalize(), P.create_proof(c["adv"], [[]]).finalize()
    assert p1 != p2 and len(p1) == len(a) == len(p2)
    assert accepts(po, c, p1) and accepts(po, c, p2)
    side = pkg.Context(0)
    P2 = native.Prover(d["params"], d["pk"], ctx, side)
    for _ in range(2):
        assert P2.create_proof(c["adv"], [[]], prover.SeededRng(7)).finalize() == a
    p3 = P2.create_proof(c["adv"], [[]]).finalize()
    assert p3 != a and accepts(po, c, p3)
    P.release(); P2.release(); side.close()


def _instance_circuit(pkg, po, k):
    """One advice column, one fixed selector, one instance column: q (a - instance) = 0 on the first rows; equality enabled on the advice column."""
    from dehalo2_amd import plonk

    n = 1 << k
    cs = plonk.ConstraintSystem(num_advice=1, num_fixed=1, num_instance=1)
    q, a, i = cs.query_fixed(0), cs.query_advice(0), cs.query_instance(0)
    cs.create_gate([plonk.mul(q, plonk.sum_(a, ("neg", i)))])
    cs.enable_equality(plonk.ADVICE, 0)
    desc = (1, 1, 1, (("product", ("fixed", 0, 0), ("sum", ("advice", 0, 0), ("neg", ("instance", 0, 0)))),), (), (("advice", 0),), ((0, 0),), ((0, 0),), ((0, 0),), 0)
    assert desc == cs.description()
    inst = [5, 7, 9, 11]
    fixed = np.zeros((1, n, 4), dtype=np.uint64)
    fixed[0, :len(inst), 0] = 1
    advice = np.zeros((1, n, 4), dtype=np.uint64)
    advice[0, :len(inst), 0] = inst
    return cs, desc, inst, fixed, advice, plonk.Assembly(1, n)


def _instance_chain(pkg, po, co, k):
    import proof_chains as PC

    cs, desc, inst, fixed, advice, asm = _instance_circuit(pkg, po, k)
    return PC.ipa_chain(po, co, desc, k, fixed, asm.mapping, advice), cs, fixed, asm, inst


@pytest.mark.gpu
def test_native_ipa_instance_column(pkg, po, co, F, ctx):
    """The instance column is committed, absorbed as a point, evaluated first and queried first; another instance value is rejected."""
    import plonk_oracle as PO
    from dehalo2_amd import native, prover

    k = 6
    c, cs, fixed, asm, inst = _instance_chain(pkg, po, co, k)
    srs, uw, rep, cs_ = c["srs"], (c["u"], c["w"]), c["rep"], F.VESTA
    # the reference prover and the verifier agree on this circuit first
    want = reference_proof(po, c, instances=(inst,))[0]
    assert accepts(po, c, want, instances=(inst,))
    params = native.ParamsIPA.create(ctx, cs_, k, srs["g"], srs["g_lagrange"], uw[1], uw[0])
    pk = native.ProvingKey.keygen(ctx, params, cs, fixed, asm, ())
    pk.transcript_repr = rep
    P = native.Prover(params, pk)
    proof = P.create_proof(c["adv"], [inst], prover.SeededRng(7)).finalize()
    assert len(proof) == P.proof_size()
    assert proof == want
    assert accepts(po, c, proof, instances=(inst,))
    assert not accepts(po, c, proof, instances=([5, 7, 10, 11],))
    P.release(); pk.release(); params.release()


@pytest.mark.gpu
def test_kzg_proof_is_unchanged_after_an_ipa_proof(pkg, po, co, F, ctx, ipa_chain, native_ipa):
    """The untouched path: on the same context, after an IPA proof, a KZG proof at k = 9 under SeededRng(7) equals plonk_oracle.create_proof's bytes
    and has the length proof_size() reports."""
    import pairing as pr
    import plonk_oracle as PO
    import shapes
    from dehalo2_amd import circuits, native, prover

    c, d = ipa_chain(6, False), native_ipa(6, False)
    P = native.Prover(d["params"], d["pk"])
    assert accepts(po, c, P.create_proof(c["adv"], [[]], prover.SeededRng(7)).finalize())
    P.release()
    k, rl, s = 9, True, 0x5EED
    oc = po.BN254
    circ = circuits.synthesize(oc.scalar.p, k, rl, seed=3)
    desc = shapes.maingate_description(rl)
    srs = PO.setup_srs(oc, k, s, 8)
    key = PO.keygen(oc, srs, desc, k, circ.fixed, circ.assembly.mapping, 8)
    rep = PO.transcript_repr(oc, key, circ.selectors)
    adv = np.stack([co.field_op(0, "to_mont", circ.advice[i]) for i in range(5)])
    kzg = native.ParamsKZG.create(ctx, F.BN254, k, srs["g"], srs["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(pr.g2_mul(s, pr.G2)))
    pk = native.ProvingKey.keygen(ctx, kzg, circ.cs, circ.fixed, circ.assembly, circ.selectors)
    assert pk.vk_bytes() == PO.vk_bytes(oc, key, circ.selectors)
    pk.transcript_repr = rep
    Pk = native.Prover(kzg, pk)
    got = Pk.create_proof(adv, [[]], prover.SeededRng(7)).finalize()
    want, _ = PO.create_proof(oc, srs, key, adv, [[]], PO.ScalarStream(7), rep, 8)
    assert got == want and len(got) == Pk.proof_size()
    Pk.release(); pk.release(); kzg.release()
