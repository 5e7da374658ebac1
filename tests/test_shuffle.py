"""The shuffle argument (ConstraintSystem::shuffle of halo2_proofs v0.3.0): whole proofs under KZG (GWC, SHPLONK) and IPA, the quotient kernel, the host logic.

The circuits and their witnesses live in tests/shuffle_circuits.py; the restatement (prover and the verifiers' PLONK part) is the oracle's.
CPU: the restatement's proofs are accepted by its verifiers, a tampered product evaluation and a witness that is no shuffle are rejected, under a description
that carries no shuffle the bytes are the pinned ones; HostCS and OpeningPlan through tests/native_host/shuffle_cs_check.cpp (g++, ASan + UBSan); the proof-size formulas.
GPU: device proofs byte for byte against the restatement under all three multiopens, through create_proof, create_proof_multi and create_proof_phased;
DEHALO_ERR_SHUFFLE; dehalo_shuffle_h_batch_device against Python integers."""
import json
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry

entry.load_oracle()      # (puts oracle/ on the path: the restatement below imports it)
import phased_circuits as PH  # noqa: E402
import plonk_oracle as PO  # noqa: E402
import shuffle_circuits as SO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CIRCUITS = [("SHUF1", 5), ("SHUF2", 6), ("SHUF5", 5), ("SHUFRLC", 5)]
K_OF = dict(CIRCUITS)


_CHAINS, _PROOFS = {}, {}      # made once per process (tests/test_oracle_variants_pinned.py shares them)


def chain_of(pkg, po, co, scheme, name):
    if (scheme, name) not in _CHAINS:
        _CHAINS[(scheme, name)] = SO.chain(pkg, po, co, scheme, name, K_OF[name])
    return _CHAINS[(scheme, name)]


def proof_of(pkg, po, co, scheme, multiopen, name, circuits=1):
    """-> (proof, trace) of the restatement under ScalarStream(7)"""
    key = (scheme, multiopen, name, circuits)
    if key not in _PROOFS:
        c = chain_of(pkg, po, co, scheme, name)
        _PROOFS[key] = SO.prove(po, co, c, witnesses_of(c, circuits), multiopen)
    return _PROOFS[key]


@pytest.fixture(scope="module")
def chains(pkg, po, co):
    return lambda scheme, name: chain_of(pkg, po, co, scheme, name)


@pytest.fixture(scope="module")
def proofs(pkg, po, co):
    return lambda scheme, multiopen, name, circuits=1: proof_of(pkg, po, co, scheme, multiopen, name, circuits)


def witnesses_of(c, circuits=1, bad=False):
    circ = c["circ"]
    if c["name"] == "SHUFRLC":
        return circ["witness"](c["curve"].scalar.p, bad)
    if c["name"] == "SHUF2":
        return [circ["witness"](bad and i == circuits - 1, variant=i) for i in range(circuits)]
    return [circ["witness"](bad)] * circuits


SCHEMES = [("kzg", "gwc"), ("kzg", "shplonk"), ("ipa", "gwc")]


# ------------------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("scheme,multiopen", SCHEMES)
@pytest.mark.parametrize("name", [n for n, _ in CIRCUITS])
def test_restatement_proves_and_verifies(po, co, chains, proofs, scheme, multiopen, name):
    c = chains(scheme, name)
    proof, trace = proofs(scheme, multiopen, name)
    sh = c["key"]["shape"]
    assert all(all(row) for row in trace["shuffles_closed"])
    assert len(proof) == PO.proof_length(sh, 1, "ipa" if scheme == "ipa" else multiopen)
    assert SO.accepts(po, c, proof, 1, multiopen)
    assert not SO.accepts(po, c, SO.tampered_product_evaluation(c, proof), 1, multiopen)


@pytest.mark.parametrize("scheme,multiopen", SCHEMES)
@pytest.mark.parametrize("name", ["SHUF1", "SHUF2", "SHUFRLC"])
def test_restatement_rejects_a_witness_that_is_no_shuffle(po, co, chains, scheme, multiopen, name):
    c = chains(scheme, name)
    proof, trace = SO.prove(po, co, c, witnesses_of(c, bad=True), multiopen)
    assert not all(all(row) for row in trace["shuffles_closed"])
    assert not SO.accepts(po, c, proof, 1, multiopen)


@pytest.mark.parametrize("multiopen", ["gwc", "shplonk"])
def test_restatement_over_two_circuits(po, co, chains, proofs, multiopen):
    c = chains("kzg", "SHUF2")
    proof, _ = proofs("kzg", multiopen, "SHUF2", 2)
    assert len(proof) == PO.proof_length(c["key"]["shape"], 2, multiopen)
    assert SO.accepts(po, c, proof, 2, multiopen)
    assert not SO.accepts(po, c, SO.tampered_product_evaluation(c, proof, 2), 2, multiopen)
    assert not SO.accepts(po, c, proof, 1, multiopen)


@pytest.mark.parametrize("scheme", ["kzg", "ipa"])
def test_without_shuffles_the_bytes_are_plonk_oracles(pkg, po, co, golden_loader, scheme):
    """R9all through the call over a list of circuits, its description carried as a Desc without shuffles: the proof pinned from the single-circuit
    restatement when it knew no shuffle (tests/golden/oracle_proof_digests.json)"""
    import proof_chains as PC
    c, inst = PC.pinned_case(pkg, po, co, scheme, "R9all_k6")
    assert inst == []
    curve = po.VESTA if scheme == "ipa" else po.BN254
    key = dict(c["key"], shape=PO.Shape(PO.Desc(c["desc"]), c["k"], curve.scalar))
    assert key["shape"].degree == c["key"]["shape"].degree and key["shape"].shuffles == ()
    got, trace = PO.create_proof_multi(curve, c["srs"], key, [c["adv"]], [[]], PO.ScalarStream(7), c["rep"], PC.THREADS, PC.scheme_of(po, c))
    assert PC.digests(got, trace) == golden_loader("oracle_proof_digests")["%s/R9all_k6" % scheme]


def test_degrees_and_sizes(pkg, po):
    from dehalo2_amd import plonk as P
    from dehalo2_amd import prover
    want = {"SHUF1": (3, 5), "SHUF2": (4, 5), "SHUF5": (5, 5), "SHUFRLC": (3, 5)}
    for name, k in CIRCUITS:
        cs = SO.build(pkg, name, k)["cs"]
        sh = PO.Shape(PO.describe(cs), k, po.BN254.scalar)
        assert (cs.degree(), cs.blinding_factors()) == (sh.degree, sh.blinding_factors) == want[name], name
        head, evals = prover.proof_layout(cs)
        for scheme in ("gwc", "shplonk"):
            groups = 2 if scheme == "shplonk" else len({pt for _, pt, _ in PO.symbolic_queries(sh, 1)})
            assert 32 * (head + evals + groups) == PO.proof_length(sh, 1, scheme)
    # a shuffle's degree rule on its own: max(2 + inputs, 2 + shuffle side), either at least 1
    cs = P.ConstraintSystem(num_advice=2)
    cs.shuffle([(("const", 3), ("const", 4))])
    assert cs.degree() == 3
    cs.shuffle([(P.mul(("advice", 0, 0), ("advice", 1, 0)), ("advice", 0, 0))])
    assert cs.degree() == 4
    cs.shuffle([(("advice", 0, 0), P.mul(P.mul(("advice", 0, 0), ("advice", 1, 0)), ("advice", 1, 0)))])
    assert cs.degree() == 5
    with pytest.raises(ValueError):
        cs.shuffle([])
    # a circuit without shuffles is described as before
    assert P.maingate_cs(True).shuffles == [] and len(P.maingate_cs(True).description()) == 10
    from dehalo2_amd import native
    d = native.ConstraintSystemDescriptor(P.maingate_cs(True), pkg.fields.BN254.scalar).struct
    assert not d.shuffle_lens and not d.shuffle_inputs and not d.shuffle_tables and d.num_shuffles == 0      # null / 0: HostCS::encode appends nothing
    d = native.ConstraintSystemDescriptor(SO.build(pkg, "SHUF2", 6)["cs"], pkg.fields.BN254.scalar).struct
    assert d.num_shuffles == 2 and [d.shuffle_lens[i] for i in range(2)] == [2, 2]


def _host_program():
    out = subprocess.run(["make", "-C", ROOT, "shuffle_cs_check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return os.path.join(ROOT, "tests", "native_host", "shuffle_cs_check")


def test_host_constraint_system_with_shuffles():
    """HostCS::load / degree / encode and the two programs of a shuffle, under ASan + UBSan"""
    run = subprocess.run([_host_program(), "cs"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("19 checks passed"), run.stdout


@pytest.mark.parametrize("circuits", [1, 2])
def test_opening_plan_with_shuffles(pkg, po, circuits):
    """OpeningPlan (csrc/opening_plan.hpp) for SHUF2 and SHUF1 against the restatement's query list, evaluation order and product order"""
    prog = _host_program()
    for name, scheme in (("SHUF2", "kzg"), ("SHUF1", "kzg"), ("SHUF5", "ipa")):
        if scheme == "ipa" and circuits > 1:
            continue
        cs = SO.build(pkg, name, K_OF[name])["cs"]
        sh = PO.Shape(PO.describe(cs), K_OF[name], (po.VESTA if scheme == "ipa" else po.BN254).scalar)
        L, S, H = len(sh.lookups), sh.num_sets, len(sh.shuffles)
        q = lambda lst: "%d %s" % (len(lst), " ".join("%d %d" % (c, r) for c, r in lst))
        line = "%d %d %d %d %d %d %d %d %d %d %d %d %s %s %s\n" % (circuits, H, sh.k, sh.num_advice, sh.num_fixed, 0, L, S, len(sh.perm_columns), sh.blinding_factors,
                                                                 sh.degree - 1, int(scheme == "ipa"), q(sh.advice_queries), q(sh.fixed_queries), q([]))
        run = subprocess.run([prog, "plan"], input=line, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        plan = json.loads(run.stdout)
        norm = lambda v: tuple(norm(i) for i in v) if isinstance(v, list) else v
        want_q = [(key, rot, ev) for key, rot, ev in PO.symbolic_queries(sh, circuits)]
        got_q = [(norm(qq["poly"]), qq["rot"], (norm(qq["eval"][0]), qq["eval"][1]) if qq["eval"] else None) for qq in plan["queries"]]
        assert got_q == want_q, name
        assert [(norm(w[0]), w[1]) for w in plan["write"]] == PO.evaluation_order(sh, circuits), name
        order = [("perm_z", c, s) for c in range(circuits) for s in range(S)] + [("lookup_z", c, l) for c in range(circuits) for l in range(L)]
        order += [("shuffle_z", c, j) for c in range(circuits) for j in range(H)] + [("random",)]
        assert [norm(k) for k in plan["product_order"]] == order, name
        mo = {"gwc": "gwc", "shplonk": "shplonk", "ipa": "ipa"}
        for scheme_name in (("ipa",) if scheme == "ipa" else ("gwc", "shplonk")):
            assert plan["proof_size"][mo[scheme_name]] == PO.proof_length(sh, circuits, scheme_name), (name, scheme_name)


# ------------------------------------------------------------------------------------------------------------------------------ GPU, whole proofs
def _native(pkg, ctx, po, c):
    """-> (params, pk) of the chain's SRS and circuit, vk checked against the restatement's, transcript_repr set"""
    import pairing as pr
    from dehalo2_amd import native
    k, circ = c["k"], c["circ"]
    if "u" in c:
        params = native.ParamsIPA.create(ctx, pkg.fields.VESTA, k, c["srs"]["g"], c["srs"]["g_lagrange"], c["w"], c["u"])
        vk = PO.vk_bytes(po.VESTA, dict(c["key"], fixed_commitments=c["fc"], perm_commitments=c["pc"]))
    else:
        params = native.ParamsKZG.create(ctx, pkg.fields.BN254, k, c["srs"]["g"], c["srs"]["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(c["s_g2"]))
        vk = PO.vk_bytes(po.BN254, c["key"])
    pk = native.ProvingKey.keygen(ctx, params, c["cs"], circ["fixed"], circ["asm"], ())
    assert pk.vk_bytes() == vk
    pk.transcript_repr = c["rep"]
    return params, pk


def _items_differing(got, want):
    return [i // 32 for i in range(0, max(len(got), len(want)), 32) if got[i:i + 32] != want[i:i + 32]]


def _device_proof(po, co, c, P, bad=False):
    from dehalo2_amd import prover
    w = witnesses_of(c, bad=bad)
    if callable(w):
        return P.create_proof_phased(PH.mont_witness(po, co, c, w), [], prover.SeededRng(7)).finalize()
    return P.create_proof(w[0], [], prover.SeededRng(7), canonical=True).finalize()


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,multiopen", SCHEMES)
@pytest.mark.parametrize("name", [n for n, _ in CIRCUITS])
def test_native_proof_is_the_restatements(pkg, po, co, ctx, chains, proofs, scheme, multiopen, name):
    from dehalo2_amd import native
    c = chains(scheme, name)
    want, _ = proofs(scheme, multiopen, name)
    params, pk = _native(pkg, ctx, po, c)
    cs = c["cs"]
    info = pk.info()
    assert info["degree"] == cs.degree() and info["blinding_factors"] == cs.blinding_factors()
    P = native.Prover(params, pk, multiopen=multiopen)
    proof = _device_proof(po, co, c, P)
    assert len(proof) == P.proof_size() == len(want)
    diff = _items_differing(proof, want)
    assert not diff, "proof items differ from the restatement's: %r" % diff[:8]
    assert _device_proof(po, co, c, P) == want      # the prover's buffers are clean for the next proof
    P.release(); pk.release(); params.release()


@pytest.mark.gpu
@pytest.mark.parametrize("multiopen", ["gwc", "shplonk"])
def test_native_proof_over_two_circuits(pkg, po, co, ctx, chains, proofs, multiopen):
    from dehalo2_amd import native, prover
    c = chains("kzg", "SHUF2")
    want, _ = proofs("kzg", multiopen, "SHUF2", 2)
    params, pk = _native(pkg, ctx, po, c)
    P = native.Prover(params, pk, multiopen=multiopen, num_circuits=2)
    proof = P.create_proof_multi(witnesses_of(c, 2), [[], []], prover.SeededRng(7), canonical=True).finalize()
    assert len(proof) == P.proof_size() == len(want)
    diff = _items_differing(proof, want)
    assert not diff, "proof items differ from the restatement's: %r" % diff[:8]
    # the second circuit's witness is no shuffle: the error names it, and the prover proves the next one
    from dehalo2_amd._lib import DehaloError
    with pytest.raises(DehaloError) as e:
        P.create_proof_multi(witnesses_of(c, 2, bad=True), [[], []], prover.SeededRng(7), canonical=True)
    assert e.value.code == -7 and "shuffle 1 of circuit 1" in str(e.value)
    assert P.create_proof_multi(witnesses_of(c, 2), [[], []], prover.SeededRng(7), canonical=True).finalize() == want
    P.release(); pk.release(); params.release()


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,name", [("kzg", "SHUF1"), ("ipa", "SHUF2"), ("kzg", "SHUFRLC")])
def test_a_witness_that_is_no_shuffle_is_refused(pkg, po, co, ctx, chains, proofs, scheme, name):
    """DEHALO_ERR_SHUFFLE, and the next proof on the same prover succeeds"""
    from dehalo2_amd import native
    from dehalo2_amd._lib import DehaloError
    c = chains(scheme, name)
    want, _ = proofs(scheme, "gwc", name)
    params, pk = _native(pkg, ctx, po, c)
    P = native.Prover(params, pk)
    with pytest.raises(DehaloError) as e:
        _device_proof(po, co, c, P, bad=True)
    assert e.value.code == -7 and "shuffle %d" % (1 if name == "SHUF2" else 0) in str(e.value)
    assert _device_proof(po, co, c, P) == want
    P.release(); pk.release(); params.release()


# ------------------------------------------------------------------------------------------------------------------------------ GPU, the kernel
SHUFFLE_LOGS = [0, 6, 7, 8, 10]      # 1 row; a partial block; one block of EVH_THREADS = 128; two; eight (a launch covers 2^log_rows rows: 127 and 129 do not exist)


def _shuffle_reference(p, values, fams, lag, y, rot_scale):
    rows = len(values)
    l0, l_last, l_active = lag
    v = list(values)
    for z, iv, sv in fams:
        for i in range(rows):
            zn = z[(i + rot_scale) % rows]
            t = v[i]
            t = (t * y + l0[i] * (1 - z[i])) % p
            t = (t * y + l_last[i] * (z[i] * z[i] - z[i])) % p
            t = (t * y + l_active[i] * (zn * sv[i] - z[i] * iv[i])) % p
            v[i] = t
    return v


def _shuffle_families(po, F, log_rows):
    """nine (z, input_value, shuffle_value) triples: uniform; columns from the edge set E; the satisfied argument (z = 1, equal sides); zeros; z(wX) sv = z iv
    with z constant; E against E at other strides; ..."""
    import quotient_inputs as QI
    import structured_inputs as SI
    rows = 1 << log_rows
    E = QI.edge_values(po, F)
    u = QI.uniform(po, F, 12 * rows, 0x5F0 + log_rows)
    col = lambda j: u[j * rows:(j + 1) * rows]
    c = SI.constant_c(F)
    fams = [(col(0), col(1), col(2)),
            (QI.cyclic(E, rows, 1, 1), QI.cyclic(E, rows, 2, 2), QI.cyclic(E, rows, 2, 4)),
            ([1] * rows, col(3), col(3)),
            ([0] * rows, [0] * rows, [0] * rows),
            ([c] * rows, col(4), col(4)),
            (QI.cyclic(E, rows, 7, 7), QI.cyclic(E, rows, 0, 1), QI.cyclic(E, rows, 3, 5)),
            (col(5), QI.cyclic(E, rows, 4, 1), col(6)),
            (QI.cyclic(E, rows, 0, 3), col(7), QI.cyclic(E, rows, 5, 2)),
            (col(8), col(9), col(10))]
    return fams


@pytest.mark.gpu
@pytest.mark.parametrize("log_rows", SHUFFLE_LOGS)
@pytest.mark.parametrize("fname", ["bn254_fr", "pasta_fp"])
def test_shuffle_h_batch_kernel(pkg, po, ctx, fname, log_rows):
    """dehalo_shuffle_h_batch_device against Python integers: counts 1, 8 and 9 (split 8 + 1), rot_scale 1 and 4 (wrapping at the last rows), both element forms,
    under uniform, indicator and E-valued Lagrange columns; a launch of nine is refused"""
    import quotient_inputs as QI
    from test_quotient_structured import _Dev
    from dehalo2_amd._lib import DehaloError
    rows = 1 << log_rows
    wants = {}      # a reference is computed once and shared by the two element forms
    for internal in (False, True):
        dev = _Dev(pkg, ctx, po, fname, internal)
        F = dev.F
        fams = _shuffle_families(po, F, log_rows)
        lags = QI.lookup_lagrange(po, F, log_rows)
        y = QI.uniform(po, F, 1, 0x5F1)[0]
        dfam = [tuple(dev.up(col) for col in fam) for fam in fams]
        for ln in ("uniform", "indicator", "edges"):
            lag = lags[ln]
            dl = [dev.up(col) for col in lag[:3]]
            for count in (1, 8, 9):
                for rs in (1, 4):
                    idx = list(range(count)) if count > 1 else [1]
                    if (ln, count, rs) not in wants:
                        wants[(ln, count, rs)] = _shuffle_reference(F.p, lag[3], [fams[i] for i in idx], lag[:3], y, rs)
                    want = wants[(ln, count, rs)]
                    values = dev.up(lag[3])
                    pkg.evaluation.shuffle_h_batch_device(ctx, dev.spec, [tuple(t.data_ptr() for t in dfam[i]) for i in idx], dl[0].data_ptr(), dl[1].data_ptr(),
                                                          dl[2].data_ptr(), y, log_rows, rs, values.data_ptr(), 0, dev.flags)
                    dev.check(values, want, (ln, count, rs, internal))
        values = dev.up(lags["uniform"][3])
        with pytest.raises(DehaloError) as e:
            ctx.shuffle_h_batch_device(dev.spec.id, [tuple(t.data_ptr() for t in dfam[i]) for i in range(9)], dl[0].data_ptr(), dl[1].data_ptr(), dl[2].data_ptr(),
                                       dev.spec.encode(y), log_rows, 1, values.data_ptr(), 0, dev.flags)
        assert e.value.code == -1


# ------------------------------------------------------------------------------------------------------------------------------ GPU, the witness check
@pytest.mark.gpu
def test_check_witness_with_shuffles(pkg, po, co, ctx, chains):
    """DEHALO_CHECK_SHUFFLE on SHUF2 (k = 6: the sub-block case of the checking kernels): a satisfied witness gives 0; one swapped value gives exactly the rows of
    the two affected tuples; duplicates count by multiplicity; order and totals hold with cap = 0"""
    from dehalo2_amd import native
    c = chains("kzg", "SHUF2")
    circ, u = c["circ"], c["circ"]["usable"]
    params, pk = _native(pkg, ctx, po, c)
    adv = circ["witness"]()
    rep = pk.check_witness(adv, [], circ["asm"], canonical=True)
    assert rep.ok and rep.failures == [] and (rep.rows, rep.shuffle_inputs, rep.lookup_inputs) == (u, 2 * u, u)
    val = lambda a, col, row: int(a[col, row, 0])      # (the witness' values fit one limb)
    tuples = lambda a: [(val(a, 0, i), val(a, 1, i)) for i in range(u)]
    # shuffle 1's side: a5[2] <-> a5[3].  The side then holds (a4[2], a5[3]) and (a4[3], a5[2]) in the place of (a4[2], a5[2]) and (a4[3], a5[3]): the input rows
    # holding one of the two displaced tuples have one partner too few; the two new tuples occur among no inputs (or, if they do, those rows have one too many)
    bad = circ["witness"](bad=True)
    gone = {(val(adv, 4, 2), val(adv, 5, 2)), (val(adv, 4, 3), val(adv, 5, 3))}
    came = {(val(bad, 4, 2), val(bad, 5, 2)), (val(bad, 4, 3), val(bad, 5, 3))}
    assert not gone & came
    rows = [i for i, t in enumerate(tuples(adv)) if t in gone or t in came]
    assert len(rows) >= 2
    rep = pk.check_witness(bad, [], circ["asm"], canonical=True)
    assert rep.failures == [(native.CHECK_SHUFFLE, 1, i) for i in rows]
    assert (rep.gate_failures, rep.lookup_failures, rep.copy_failures, rep.shuffle_failures) == (0, 0, 0, len(rows)) and not rep.ok
    # duplicates: row 5's input tuple is overwritten with another row's.  The old tuple loses a copy among the inputs, the new one gains a copy: every input row
    # holding either fails, in both shuffles (row 5 is under the selector), by multiplicity -- rows whose tuple merely repeats elsewhere do not
    dup = adv.copy()
    src = next(j for j in range(u) if j != 5 and tuples(adv)[j] != tuples(adv)[5])
    dup[0, 5], dup[1, 5] = adv[0, src], adv[1, src]
    dup[6, 5] = SO.limbs([val(dup, 0, 5) + val(dup, 1, 5)], 1)[0]      # (the gate holds; a0 stays in the table)
    old, new = tuples(adv)[5], tuples(adv)[src]
    want1 = sorted(i for i, t in enumerate(tuples(dup)) if t in (old, new))
    q_rows = int(circ["fixed"][0, :, 0].sum())
    assert 5 < q_rows
    sel = lambda i: 1 if i < q_rows else 0
    t0 = lambda a: [(sel(i) * val(a, 0, i), sel(i) * val(a, 1, i)) for i in range(u)]
    old0, new0 = t0(adv)[5], t0(dup)[5]
    want0 = [i for i, t in enumerate(t0(dup)) if t in (old0, new0)] if old0 != new0 else []
    rep = pk.check_witness(dup, [], None, canonical=True)
    assert rep.failures == [(native.CHECK_SHUFFLE, 0, i) for i in want0] + [(native.CHECK_SHUFFLE, 1, i) for i in want1]
    assert rep.shuffle_failures == len(want0) + len(want1) > 2 and rep.copy_failures == 0
    # cap = 0: the totals are exact, nothing is stored; cap = 1: the first in (kind, index, row) order
    rep0 = pk.check_witness(dup, [], None, canonical=True, cap=0)
    assert rep0.failures == [] and rep0.written == 0 and rep0.shuffle_failures == rep.shuffle_failures
    rep1 = pk.check_witness(dup, [], None, canonical=True, cap=1)
    assert rep1.failures == rep.failures[:1] and rep1.shuffle_failures == rep.shuffle_failures
    # a broken gate and a broken shuffle: GATE sorts first, SHUFFLE after everything else
    both = bad.copy()
    both[6, 1] = SO.limbs([7], 1)[0]
    rep = pk.check_witness(both, [], circ["asm"], canonical=True)
    assert rep.failures == [(native.CHECK_GATE, 0, 1)] + [(native.CHECK_SHUFFLE, 1, i) for i in rows]
    pk.release(); params.release()


@pytest.mark.gpu
def test_check_witness_shuffle_reading_a_challenge(pkg, po, co, ctx, chains):
    """SHUFRLC under the caller's challenge value; 2^5 rows: less than one wave"""
    from dehalo2_amd import native
    c = chains("kzg", "SHUFRLC")
    p, circ = c["curve"].scalar.p, c["circ"]
    params, pk = _native(pkg, ctx, po, c)
    ch = [0x1234567]
    fn = circ["witness"](p)
    fn(0, [0])
    adv = fn(1, ch).copy()
    rep = pk.check_witness(adv, [], circ["asm"], canonical=True, challenges=ch)
    assert rep.ok and rep.shuffle_inputs == circ["usable"]
    rep = pk.check_witness(adv, [], circ["asm"], canonical=True, challenges=[ch[0] + 1], cap=4)
    assert rep.shuffle_failures > 0 and rep.failures[0][0] == native.CHECK_SHUFFLE and rep.gate_failures == 0
    pk.release(); params.release()


# ------------------------------------------------------------------------------------------------------------------------------ GPU, the other entry points
@pytest.mark.gpu
def test_batch_mode_proves_shuffles(pkg, po, co, ctx, chains, proofs):
    """dehalo_create_proofs: two proofs of SHUF2 on one prover, each the restatement's"""
    from dehalo2_amd import native, prover
    c = chains("kzg", "SHUF2")
    want, _ = proofs("kzg", "gwc", "SHUF2")
    params, pk = _native(pkg, ctx, po, c)
    P = native.Prover(params, pk)
    adv = PH.to_mont(co, c["curve"], po, c["circ"]["witness"]())
    got = native.create_proofs([P], adv, [prover.SeededRng(7), prover.SeededRng(7)])
    assert [bytes(g) for g in got] == [want, want]
    P.release(); pk.release(); params.release()


@pytest.mark.gpu
def test_sharded_provers_prove_shuffles(pkg, po, co, ctx, chains, proofs):
    """dehalo_prover_set_shard with world = 2: two provers of this process, one thread and one context each, exchange their points through a barrier.  The shuffle
    products are ordinary columns of the products' phase, and the closing flags ride behind ALL its points on either rank."""
    import threading
    from dehalo2_amd import native, prover
    c = chains("kzg", "SHUF2")
    want, _ = proofs("kzg", "gwc", "SHUF2")
    params, pk = _native(pkg, ctx, po, c)
    ctx2 = pkg.Context(0)
    provers = [native.Prover(params, pk, ctx), native.Prover(params, pk, ctx2)]
    barrier, board, out = threading.Barrier(2, timeout=60), {}, {}

    def gather_of(rank):
        calls = [0]

        def gather(pts, first, num):
            call = calls[0]
            calls[0] += 1
            board[(call, rank)] = pts[first[rank]:first[rank] + num[rank]].copy()
            barrier.wait()
            other = 1 - rank
            pts[first[other]:first[other] + num[other]] = board[(call, other)]
        return gather

    def run(rank):
        try:
            provers[rank].set_shard(rank, 2, gather_of(rank))
            out[rank] = provers[rank].create_proof(c["circ"]["witness"](), [], prover.SeededRng(7), canonical=True).finalize()
        except Exception as e:      # noqa: BLE001
            out[rank] = e
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert out[0] == want and out[1] == want, (type(out[0]), type(out[1]))
    for P in provers:
        P.release()
    ctx2.close(); pk.release(); params.release()
