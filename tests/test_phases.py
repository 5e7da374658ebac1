"""Circuits with later-phase advice columns and challenges (halo2's Challenge API): whole proofs under KZG (GWC, SHPLONK) and IPA, and the witness check.

The circuits and their witness live in tests/phased_circuits.py; the phase loop is the oracle's.
CPU: the restatement's RLC3 proof is accepted under both schemes, a tampered evaluation and a witness made with a wrong c0 are rejected; the new expression
node has degree 0; the descriptor of a circuit without phases is what it was.
GPU: dehalo_create_proof_phased byte for byte against the restatement, the phase-major order, single-phase equivalence with dehalo_create_proof,
dehalo_check_witness_challenges, and every host-side refusal."""
import hashlib

import pytest

import phased_circuits as PH
import proof_chains as PC


_CHAINS = {}      # made once per process (tests/test_oracle_variants_pinned.py shares them)


def chain_of(pkg, po, co, scheme, k):
    """the RLC3 chain with `want`, `trace`, `challenges`: the restatement's proof under ScalarStream(7)"""
    if (scheme, k) not in _CHAINS:
        c = PH.chain(pkg, po, co, scheme, k)
        p = c["curve"].scalar.p
        c["p"], c["usable"] = p, c["key"]["shape"].usable
        c["want"], c["trace"] = PC.prove_circuits(po, c, [PH.mont_witness(po, co, c, PH.witness(p, k, c["usable"]))], [[]])
        c["challenges"] = c["trace"]["phase_challenges"]
        _CHAINS[(scheme, k)] = c
    return _CHAINS[(scheme, k)]


@pytest.fixture(scope="module")
def chains(pkg, po, co):
    return lambda scheme, k: chain_of(pkg, po, co, scheme, k)


# ------------------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("scheme", ["kzg", "ipa"])
def test_restatement_proves_rlc3(pkg, po, co, chains, scheme):
    c = chains(scheme, 5)
    assert PC.phase_challenges(po, c, c["want"]) == c["challenges"] and len(set(c["challenges"])) == 3 and 0 not in c["challenges"]
    assert PC.accepts(po, c, c["want"], [])
    assert not PC.accepts(po, c, PC.tampered(c, c["want"]), [])


@pytest.mark.parametrize("scheme", ["kzg", "ipa"])
def test_restatement_rejects_r_made_with_a_wrong_c0(pkg, po, co, chains, scheme):
    c = chains(scheme, 5)
    bad, _ = PC.prove_circuits(po, c, [PH.mont_witness(po, co, c, PH.witness(c["p"], 5, c["usable"], wrong_c0=True))], [[]])
    assert not PC.accepts(po, c, bad, [])


def test_a_challenge_has_degree_zero(pkg, po):
    import plonk_oracle as PO
    from dehalo2_amd import plonk
    for name in ("RLC3", "RLC3perm"):
        cs = PH.build_cs(pkg, name)
        assert plonk.degree(("challenge", 0)) == 0
        sh = PO.Shape(PO.describe(cs), 5, po.BN254.scalar)
        assert PO.expr_degree(("challenge", 0)) == 0 and (sh.phases, sh.challenge_phases) == (tuple(cs.phases()), (0, 1, 2))
        assert (cs.degree(), cs.blinding_factors()) == (sh.degree, sh.blinding_factors) == (4, 5)
        assert len(cs.description()) == 10 and cs.num_phases() == 3 and cs.challenge_phases == [0, 1, 2]
    assert PH.build_cs(pkg, "RLC3").phases() == [0, 0, 1, 1, 2] and PH.build_cs(pkg, "RLC3perm").phases() == [1, 0, 2, 0, 1]
    assert PH.build_cs(pkg, "RLC3").advice_queries == [(0, 0), (2, 0), (1, 0), (3, 0), (3, 1), (0, 1), (4, 0)]


def test_graph_builder_reads_a_challenge_as_a_source(pkg):
    from dehalo2_amd import evaluation as ev, plonk
    g = ev.GraphEvaluator()
    assert plonk.add_expression(g, ("challenge", 2), 97) == (ev.CHALLENGE, 2, 0)
    src = plonk.add_expression(g, plonk.mul(("challenge", 1), ("advice", 0, 0)), 97)
    assert src[0] == ev.INTERMEDIATE


def test_descriptor_of_a_circuit_without_phases_is_unchanged(pkg):
    """The fields dehalo_constraint_system had before the Challenge API, for maingate_cs(): pinned by digest (taken on the code before this change); the new
    pointers are NULL and the count 0, so HostCS::encode appends nothing and the substitute transcript_repr of every existing key stays what it was."""
    import ctypes as C
    from dehalo2_amd import native, plonk
    want = {True: "cffe112f1165a264", False: "74e0746b7fe163fb"}
    for rl in (True, False):
        cs = plonk.maingate_cs(rl)
        assert cs.phases() == [0] * 5 and cs.challenge_phases == [] and cs.num_phases() == 1
        d = native.ConstraintSystemDescriptor(cs, pkg.fields.BN254.scalar).struct
        assert d.advice_phases is None and d.challenge_phases is None and d.num_challenges == 0
        h = hashlib.sha256()
        h.update(repr((d.num_advice, d.num_fixed, d.num_instance, d.minimum_degree, d.num_nodes, d.num_constants, d.num_gates, d.num_lookups, d.num_permutation_columns,
                       d.num_advice_queries, d.num_fixed_queries, d.num_instance_queries)).encode())
        for ptr, count, size in ((d.nodes, d.num_nodes, 16), (d.gates, d.num_gates, 4), (d.lookup_lens, d.num_lookups, 4),
                                 (d.lookup_inputs, sum(d.lookup_lens[i] for i in range(d.num_lookups)), 4), (d.lookup_tables, sum(d.lookup_lens[i] for i in range(d.num_lookups)), 4),
                                 (d.permutation_columns, d.num_permutation_columns, 12), (d.advice_queries, d.num_advice_queries, 12),
                                 (d.fixed_queries, d.num_fixed_queries, 12), (d.instance_queries, d.num_instance_queries, 12)):
            h.update(C.string_at(ptr, count * size))
        h.update(C.string_at(d.constants, d.num_constants * 32))
        assert h.hexdigest()[:16] == want[rl], h.hexdigest()[:16]


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _mont_witness(po, co, c, k, name="RLC3", log=None):
    fn = PH.mont_witness(po, co, c, PH.witness(c["p"], k, c["usable"], name))

    def wfn(phase, challenges):
        if log is not None:
            log.append((phase, list(challenges)))
        return fn(phase, challenges)

    return wfn


def _native(pkg, ctx, po, c, k, cs=None, asm=None):
    """-> (params, pk) of the chain's SRS and circuit, vk checked against the restatement's, transcript_repr set"""
    import pairing as pr
    import plonk_oracle as PO
    from dehalo2_amd import native
    if "u" in c:
        params = native.ParamsIPA.create(ctx, pkg.fields.VESTA, k, c["srs"]["g"], c["srs"]["g_lagrange"], c["w"], c["u"])
        vk = PO.vk_bytes(po.VESTA, dict(c["key"], fixed_commitments=c["fc"], perm_commitments=c["pc"]))
    else:
        params = native.ParamsKZG.create(ctx, pkg.fields.BN254, k, c["srs"]["g"], c["srs"]["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(c["s_g2"]))
        vk = PO.vk_bytes(po.BN254, c["key"])
    pk = native.ProvingKey.keygen(ctx, params, cs if cs is not None else c["cs"], c["fixed"], asm if asm is not None else c["asm"], ())
    assert pk.vk_bytes() == vk
    pk.transcript_repr = c["rep"]
    return params, pk


def _items_differing(got, want):
    return [i // 32 for i in range(0, max(len(got), len(want)), 32) if got[i:i + 32] != want[i:i + 32]]


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,k", [("kzg", 6), ("ipa", 6), ("kzg", 9)])
def test_native_phased_proof_is_the_restatements(pkg, po, co, ctx, chains, scheme, k):
    """k = 6: 64 rows, the sub-wave case of the checking kernels; k = 9: several blocks per launch, no level of the reductions skipped."""
    from dehalo2_amd import native, prover
    c = chains(scheme, k)
    params, pk = _native(pkg, ctx, po, c, k)
    assert pk.phases() == (3, 3)
    P = native.Prover(params, pk)
    log = []
    proof = P.create_proof_phased(_mont_witness(po, co, c, k, log=log), [], prover.SeededRng(7)).finalize()
    want = c["want"]
    assert len(proof) == P.proof_size() == len(want)
    diff = _items_differing(proof, want)
    assert not diff, "proof items differ from the restatement's: %r" % diff[:8]
    assert PC.accepts(po, c, proof, []) and not PC.accepts(po, c, PC.tampered(c, proof), [])
    c0, c1, _ = PC.phase_challenges(po, c, proof)
    assert log == [(0, [0, 0, 0]), (1, [c0, 0, 0]), (2, [c0, c1, 0])]
    assert P.create_proof_phased(_mont_witness(po, co, c, k), [], prover.SeededRng(7)).finalize() == want      # the prover's buffers are clean for the next proof
    P.release(); pk.release(); params.release()


@pytest.mark.gpu
def test_native_shplonk_phased_proof(pkg, po, co, ctx, chains):
    """Everything before the multiopen is the GWC proof's; two commitments follow."""
    from dehalo2_amd import native, prover
    c = chains("kzg", 6)
    params, pk = _native(pkg, ctx, po, c, 6)
    P = native.Prover(params, pk, multiopen="shplonk")
    proof = P.create_proof_phased(_mont_witness(po, co, c, 6), [], prover.SeededRng(7)).finalize()
    cs = c["cs"]
    head = 32 * (cs.num_advice + 3 + cs.num_permutation_sets() + 1 + (cs.degree() - 1)
                 + len(cs.advice_queries) + len(cs.fixed_queries) + 1 + len(cs.permutation_columns) + (3 * cs.num_permutation_sets() - 1) + 5)
    assert proof[:head] == c["want"][:head]
    assert len(proof) == P.proof_size() == head + 64
    P.release(); pk.release(); params.release()


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["kzg", "ipa"])
def test_advice_commitments_are_phase_major(pkg, po, co, ctx, chains, scheme):
    """RLC3perm: the same circuit with its advice columns relabelled so that the phases are not monotone in the column index.  Same transcript_repr, same seed:
    the same proof, so commitments, blinding rows and blinds follow the phases and not the labels."""
    from dehalo2_amd import native, prover
    c = chains(scheme, 6)
    cs2 = PH.build_cs(pkg, "RLC3perm")
    params, pk = _native(pkg, ctx, po, c, 6, cs2, PH.assembly(pkg, cs2, 6))
    P = native.Prover(params, pk)
    proof = P.create_proof_phased(_mont_witness(po, co, c, 6, "RLC3perm"), [], prover.SeededRng(7)).finalize()
    diff = _items_differing(proof, c["want"])
    assert not diff, "proof items differ from RLC3's: %r" % diff[:8]
    P.release(); pk.release(); params.release()


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["kzg", "ipa"])
@pytest.mark.parametrize("name", ["maingate_range_k9", "R9all_k6"])
def test_phased_call_on_a_single_phase_key(pkg, po, co, ctx, scheme, name):
    """create_proof_phased calls back once and writes create_proof's bytes."""
    import test_rotations
    from dehalo2_amd import circuits, native, prover
    spec = pkg.fields.VESTA if scheme == "ipa" else pkg.fields.BN254
    oc = po.VESTA if scheme == "ipa" else po.BN254
    if name.startswith("maingate"):
        k = 9
        circ = circuits.synthesize(oc.scalar.p, k, True, seed=3)
        cs, fixed, advice, asm, sels, inst = circ.cs, circ.fixed, circ.advice, circ.assembly, circ.selectors, [[]]
    else:
        k = 6
        cs, fixed, advice, asm = test_rotations.build_circuit(pkg, "R9all", k)
        sels, inst = (), []
    if scheme == "ipa":
        pts = co.fixed_base_mul(po.CURVE_IDS["vesta"], co.fill_scalars(po.FIELD_IDS[oc.scalar.name], "uniform", (1 << k) + 2, 7))
        params = native.ParamsIPA.from_g(ctx, spec, k, pts[2:], pts[1], pts[0])
    else:
        params = native.ParamsKZG.setup(ctx, spec, k, 0x5EED)
    pk = native.ProvingKey.keygen(ctx, params, cs, fixed, asm, sels)
    assert pk.phases() == (1, 0)
    P = native.Prover(params, pk)
    want = P.create_proof(advice, inst, prover.SeededRng(7), canonical=True).finalize()
    calls = []

    def wfn(phase, challenges):
        calls.append((phase, list(challenges)))
        return advice

    got = P.create_proof_phased(wfn, inst, prover.SeededRng(7), canonical=True).finalize()
    assert got == want and len(got) == P.proof_size()
    assert calls == [(0, [])]
    P.release(); pk.release(); params.release()


@pytest.mark.gpu
def test_check_witness_with_challenges(pkg, po, co, ctx, chains):
    from dehalo2_amd import native
    from dehalo2_amd._lib import DehaloError
    k = 6
    c = chains("kzg", k)
    p, usable = c["p"], c["usable"]
    params, pk = _native(pkg, ctx, po, c, k)
    ch = [0x1234567, p - 5, 3]
    adv = PH.full_witness(p, k, usable, ch)
    rep = pk.check_witness(adv, [], c["asm"], canonical=True, challenges=ch)
    assert (rep.gate_failures, rep.lookup_failures, rep.copy_failures) == (0, 0, 0) and rep.rows == usable
    assert rep.cells_in_cycles == 2 * len(PH.copy_rows(usable)) > 0
    # r on row 3 made with another c0: gate 0 breaks there, and with it gates 2 and 3 (w was made from the right r)
    bad = adv.copy()
    a0, a1 = PH.table_row(PH.input_row(3))
    assert a1 != 0
    bad[2, 3] = PH.limbs([(a0 + (ch[0] + 1) * a1) % p], 1)[0]
    rep = pk.check_witness(bad, [], c["asm"], canonical=True, challenges=ch)
    assert rep.failures == [(native.CHECK_GATE, 0, 3), (native.CHECK_GATE, 2, 3), (native.CHECK_GATE, 3, 3)]
    assert (rep.gate_failures, rep.lookup_failures, rep.copy_failures) == (3, 0, 0)
    # a tuple that is in no table row, on a row the selector leaves alone
    row = 20
    bad = adv.copy()
    bad[1, row] = PH.limbs([4], 1)[0]
    assert (PH.table_row(PH.input_row(row))[0], 4) not in {PH.table_row(i) for i in range(16)}
    rep = pk.check_witness(bad, [], c["asm"], canonical=True, challenges=ch)
    assert rep.failures == [(native.CHECK_LOOKUP, 0, row)] and (rep.gate_failures, rep.lookup_failures, rep.copy_failures) == (0, 1, 0)
    # the same witness under other challenges satisfies nothing the challenges touch
    rep = pk.check_witness(adv, [], c["asm"], canonical=True, challenges=[ch[0] + 1, ch[1], ch[2]], cap=1)
    assert rep.gate_failures > 0 and rep.failures[0][0] == native.CHECK_GATE
    with pytest.raises(DehaloError) as e:
        pk.check_witness(adv, [], c["asm"], canonical=True)
    assert e.value.code == -1 and "dehalo_check_witness_challenges" in str(e.value)
    with pytest.raises(DehaloError) as e:
        pk.check_witness(adv, [], c["asm"], canonical=True, challenges=ch[:2])
    assert e.value.code == -1
    pk.release(); params.release()


@pytest.mark.gpu
def test_phase_argument_checks(pkg, po, co, ctx, chains):
    """Every refusal is made on the host, before anything is launched."""
    from dehalo2_amd import native, prover
    from dehalo2_amd._lib import DehaloError
    k = 6
    c = chains("kzg", k)
    params, pk = _native(pkg, ctx, po, c, k)

    def keygen_code(mutate):
        cs = PH.build_cs(pkg)
        mutate(cs)
        with pytest.raises(DehaloError) as e:
            native.ProvingKey.keygen(ctx, params, cs, c["fixed"], c["asm"], ())
        return e.value.code

    assert keygen_code(lambda cs: setattr(cs, "advice_phases", [0, 0, 2, 2, 2])) == -1                       # a phase gap
    assert keygen_code(lambda cs: setattr(cs, "advice_phases", [0, 1, 2, 3, 3])) == -5                       # four phases
    assert keygen_code(lambda cs: (setattr(cs, "advice_phases", [0, 0, 1, 1, 1]), setattr(cs, "challenge_phases", [0, 1, 2]))) == -1      # a challenge after a phase nobody has
    assert keygen_code(lambda cs: cs.create_gate([("product", ("fixed", 0, 0), ("challenge", 3))])) == -1  # challenge index out of range

    P = native.Prover(params, pk)
    adv = PH.to_mont(co, c["curve"], po, PH.full_witness(c["p"], k, c["usable"], c["challenges"]))
    with pytest.raises(DehaloError) as e:
        P.create_proof(adv, [], prover.SeededRng(7))
    assert e.value.code == -1 and "dehalo_create_proof_phased" in str(e.value)
    with pytest.raises(DehaloError) as e:
        native.create_proofs([P], adv, [prover.SeededRng(7)])
    assert e.value.code == -5
    with pytest.raises(DehaloError) as e:
        P.create_proof_circuit(native.CIRCUIT_POSE_ENC, [], prover.SeededRng(7), message=[0], key=[1, 2])
    assert e.value.code == -5
    with pytest.raises(DehaloError) as e:
        native.create_proofs_circuit([P], native.CIRCUIT_POSE_ENC, [dict(message=[0], key=[1, 2])], [prover.SeededRng(7)])
    assert e.value.code == -5
    with pytest.raises(DehaloError) as e:
        P.set_shard(0, 2, lambda pts, first, num: None)
    assert e.value.code == -5
    P.set_shard(0, 1)

    # a callback that returns 7 in phase 1: the proof ends with DEHALO_ERR_INVALID, the code in the text
    from dehalo2_amd._lib import ADVICE_FN, load_library
    lib = load_library()
    fn, keep = PH.witness(c["p"], k, c["usable"]), {}

    def raw(_user, phase, chal, count, out):
        if phase == 1:
            return 7
        keep["advice"] = PH.to_mont(co, c["curve"], po, fn(phase, [0] * count))
        out[0] = keep["advice"].ctypes.data
        return 0

    tr = native.Blake2bWrite(pk.curve)
    assert lib.dehalo_create_proof_phased(P.handle, ADVICE_FN(raw), None, None, None, 0, None, tr.handle, 0) == -1
    assert "returned 7 in phase 1" in lib.dehalo_last_error(ctx.handle).decode()
    assert lib.dehalo_create_proof_phased(P.handle, ADVICE_FN(), None, None, None, 0, None, tr.handle, 0) == -1      # no callback at all

    # the same through the wrapper, where an exception of witness_fn ends the proof; the prover then proves the next one to the restatement's bytes
    fn2 = PH.witness(c["p"], k, c["usable"])

    def failing(phase, challenges):
        if phase == 1:
            raise RuntimeError("no witness for phase 1")
        return PH.to_mont(co, c["curve"], po, fn2(phase, challenges))

    with pytest.raises(DehaloError) as e:
        P.create_proof_phased(failing, [], prover.SeededRng(7))
    assert e.value.code == -1 and isinstance(e.value.__cause__, RuntimeError)
    assert P.create_proof_phased(_mont_witness(po, co, c, k), [], prover.SeededRng(7)).finalize() == c["want"]
    P.release(); pk.release(); params.release()
