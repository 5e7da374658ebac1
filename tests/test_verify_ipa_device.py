"""verify_proof for IPA with a context: the device backend (one decompress launch, the instance columns' commitments over the params' Lagrange table, the fresh-bases
MSM, dehalo_ipa_s_device into one MSM over the params' resident g) against the host verifier and the oracle.

The device verifier gives the host verifier's (accept, reason) on every case of tests/verify_ipa_cases.py and on every tampered proof of the host suite; native
proofs -- create_proof over a generated ParamsIPA on Vesta and on Pallas, create_proof_phased, a shuffle circuit -- are accepted natively and by the oracle; a batch
of eight native proofs is accepted, with one tampered proof it is rejected, and the call's last MSM -- the one over g -- has the shape of ONE MSM over 2^k scalars
whatever the number of proofs (dehalo_msm_last_shape); from_ipa_vk over pk.vk_bytes() and params.write() -> ParamsIPA.read gives from_ipa's verdicts; the KZG
verifier beside the IPA verifier on one context still accepts its own proof; dehalo_ipa_verify gives ipa.verify_opening's verdicts on stand-alone openings."""
import numpy as np
import pytest

import verify_ipa_cases as VI

R_VESTA = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001


@pytest.fixture(scope="module")
def hosts(pkg, po, co):
    made = {}

    def fn(name):
        if name not in made:
            cz = VI.case(pkg, po, co, name)
            made[name] = (cz, VI.proof(pkg, po, co, name), VI.host_verifier(pkg, cz))
        return made[name]
    return fn


@pytest.fixture(scope="module")
def devices(pkg, po, co, ctx, hosts):
    """case name -> (ParamsIPA over the chain's points, the native key, the device verifier from them)"""
    from dehalo2_amd import native
    made = {}

    def fn(name):
        if name not in made:
            cz, _, _ = hosts(name)
            c = cz["c"]
            params = native.ParamsIPA.create(ctx, pkg.fields.VESTA, c["k"], c["srs"]["g"], c["srs"]["g_lagrange"], c["w"], c["u"])
            pk = native.ProvingKey.keygen(ctx, params, cz["cs"], cz["fixed"], cz["asm"], cz["selectors"])
            assert pk.vk_bytes() == cz["vk"]
            pk.transcript_repr = c["rep"]
            made[name] = (params, pk, native.Verifier.from_ipa(params, pk))
        return made[name]
    yield fn
    for params, pk, v in made.values():
        v.release(); pk.release(); params.release()


def probes(po, cz, proof):
    """the host suite's proofs of one case: the valid one, one flipped bit in every section, the malformed ones"""
    secs = VI.sections(po, cz, len(proof))
    first_eval = secs.pop("first evaluation offset")[0]
    out = [("valid", proof)] + [(label, VI.flip(proof, off)) for label, (off, _) in secs.items()]
    r = R_VESTA.to_bytes(32, "little")
    out += [("truncated by 1", proof[:-1]), ("truncated by 32", proof[:-32]), ("one trailing byte", proof + b"\0"), ("empty", b""),
            ("an evaluation replaced by r", proof[:first_eval] + r + proof[first_eval + 32:]),
            ("c replaced by r", proof[:secs["opening c"][0]] + r + proof[secs["opening c"][0] + 32:])]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", VI.NAMES)
def test_device_verifier_gives_the_host_verifiers_verdicts(po, hosts, devices, name):
    cz, proof, vh = hosts(name)
    _, _, vd = devices(name)
    assert VI.verify(vd, cz, proof) == (True, 0)
    for label, data in probes(po, cz, proof):
        assert VI.verify(vd, cz, data) == VI.verify(vh, cz, data), label
    if name == "instance":
        for wrong in ([[[5, 7, 10, 11]]], [[[5, 7, 9]]], [[[5, 7, 9, 11, 0]]]):
            assert VI.verify(vd, cz, proof, wrong) == VI.verify(vh, cz, proof, wrong) == (VI.oracle_accepts(po, cz, proof, wrong), 0 if wrong[0][0][-1] == 0 else VI.OPENING)
    t = vd.last_timings()
    assert set(t) == {"decompress", "walk", "msm", "g_sum"} and all(x >= 0 for x in t.values())


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name", ["VESTA", "PALLAS"])
def test_native_proof_under_generated_params(pkg, po, co, ctx, curve_name):
    """create_proof over ParamsIPA.generate, maingate at k = 5: accepted natively and by the oracle; from_ipa_vk over the key's and the params' bytes agrees"""
    import shapes
    from dehalo2_amd import circuits, native, prover
    spec, curve, k = getattr(pkg.fields, curve_name), getattr(po, curve_name), 5
    circ = circuits.synthesize(curve.scalar.p, k, False, seed=3)
    assert shapes.maingate_description(False) == circ.cs.description()
    params = native.ParamsIPA.generate(ctx, spec, k)
    pk = native.ProvingKey.keygen(ctx, params, circ.cs, circ.fixed, circ.assembly, circ.selectors)
    P = native.Prover(params, pk)
    inst = [[] for _ in range(circ.cs.num_instance)]
    proof = P.create_proof(circ.advice, inst, prover.SeededRng(7), canonical=True).finalize()
    v = native.Verifier.from_ipa(params, pk)
    assert v.verify(proof, inst) is True and v.last_reject == 0
    import ipa
    import verifier as V
    from dehalo2_amd import keygen
    k2, g, gl, w, u = keygen.params_ipa_from_bytes(spec, params.write())
    vk, nf = pk.vk_bytes(), circ.cs.num_fixed
    ncm = (len(vk) - 8 - len(circ.selectors) * ((1 << k) // 8)) // 64
    pts = [ipa.dec_point(curve, np.frombuffer(vk[8 + 64 * i:8 + 64 * i + 64], dtype=np.uint64)) for i in range(ncm)]
    oracle = lambda data: V.verify_proof_ipa(curve, circ.cs.description(), k, pts[:nf], pts[nf:], pk.transcript_repr, g, gl, u, w, inst, data)
    assert oracle(proof) is True
    bad = VI.flip(proof, len(proof) - 64)      # c
    assert oracle(bad) is False and v.verify(bad, inst) is False and v.last_reject == VI.OPENING
    # the verifier's side: ParamsIPA::read + VerifyingKey::read, in every format
    params2 = native.ParamsIPA.read(ctx, spec, params.write())
    for fmt in ("raw-unchecked", "raw", "processed"):
        v2 = native.Verifier.from_ipa_vk(params2, circ.cs, pk.vk_bytes(fmt) if fmt != "raw-unchecked" else vk, num_selectors=len(circ.selectors), format=fmt,
                                         transcript_repr=pk.transcript_repr)
        for data in (proof, bad, proof[:-1], VI.flip(proof, 0)):
            assert (v2.verify(data, inst), v2.last_reject) == (v.verify(data, inst), v.last_reject), fmt
        v2.release()
    # the constructors' refusals, DEHALO_ERR_INVALID each: a key of another k, a key over the other curve, ParamsKZG
    other_curve = pkg.fields.PALLAS if curve_name == "VESTA" else pkg.fields.VESTA
    for other in (native.ParamsIPA.generate(ctx, spec, k + 1), native.ParamsIPA.generate(ctx, other_curve, k), native.ParamsKZG.setup(ctx, pkg.fields.BN254, k, 0x5EED)):
        try:
            with pytest.raises(pkg.DehaloError) as e:
                native.Verifier.from_ipa(other, pk)
            assert e.value.code == -1, str(e.value)
        finally:
            other.release()
    kzg = native.ParamsKZG.setup(ctx, pkg.fields.BN254, k, 0x5EED)
    with pytest.raises(pkg.DehaloError) as e:
        native.Verifier.from_ipa_vk(kzg, circ.cs, vk, num_selectors=len(circ.selectors))
    assert e.value.code == -1 and "ParamsIPA" in str(e.value)
    kzg.release()
    v.release(); P.release(); pk.release(); params2.release(); params.release()


@pytest.mark.gpu
def test_native_phased_and_shuffle_proofs(pkg, po, co, ctx, hosts, devices):
    import phased_circuits as PH
    from dehalo2_amd import native, prover
    cz, _, _ = hosts("phased")
    params, pk, v = devices("phased")
    P = native.Prover(params, pk)
    usable = (1 << 6) - (cz["cs"].blinding_factors() + 1)
    proof = P.create_proof_phased(PH.mont_witness(po, co, cz["c"], PH.witness(po.VESTA.scalar.p, 6, usable)), [], prover.SeededRng(11)).finalize()
    assert VI.verify(v, cz, proof) == (True, 0) and VI.oracle_accepts(po, cz, proof) is True
    P.release()
    cz, _, _ = hosts("shuffle")
    params, pk, v = devices("shuffle")
    P = native.Prover(params, pk)
    proof = P.create_proof(cz["witnesses"][0], [], prover.SeededRng(11)).finalize()
    assert VI.verify(v, cz, proof) == (True, 0) and VI.oracle_accepts(po, cz, proof) is True
    bad = VI.flip(proof, VI.sections(po, cz, len(proof))["shuffle evaluation"][0])
    assert VI.verify(v, cz, bad) == (False, VI.OPENING) and VI.oracle_accepts(po, cz, bad) is False
    P.release()


@pytest.mark.gpu
def test_batch_of_eight_native_proofs_is_one_pass(pkg, po, co, ctx, hosts, devices):
    from dehalo2_amd import native, prover
    cz, _, _ = hosts("instance")
    params, pk, v = devices("instance")
    P = native.Prover(params, pk)
    proofs = [P.create_proof(cz["witnesses"][0], cz["instances"][0], prover.SeededRng(20 + i)).finalize() for i in range(8)]
    P.release()
    assert len(set(proofs)) == 8
    inst = [cz["instances"]] * 8
    # The structural condition, from what the device did: a verify call's last MSM is the one over g, and dehalo_msm_last_shape reports its (bucket, point) pairs.
    # One MSM over the 2^k generators with full-width scalars sorts the pairs of a direct commit over the same table (2^k x windows, less the zero digits: a
    # fraction 2^-c of them, so two such counts differ by a few per cent); the eight proofs' s vectors summed one by one, or the fresh-bases MSM (eight times a
    # proof's ~40 terms against 2^5 generators), would sort several times as many.
    import torch
    k = cz["c"]["k"]
    sc = ctx.upload(co.fill_scalars(po.FIELD_IDS[po.VESTA.scalar.name], "uniform", 1 << k, 31))
    aff = torch.zeros((1, 8), dtype=torch.int64, device="cuda")
    ctx._check(pkg.load_library().dehalo_params_commit_device(ctx.handle, params.handle, sc.data_ptr(), 1, 0, aff.data_ptr(), None))
    direct = ctx.msm_last_shape()["pairs"]
    sc2 = ctx.upload(co.fill_scalars(po.FIELD_IDS[po.VESTA.scalar.name], "uniform", 2 << k, 32))      # the control: two columns in one launch sort twice the pairs
    aff2 = torch.zeros((2, 8), dtype=torch.int64, device="cuda")
    ctx._check(pkg.load_library().dehalo_params_commit_device(ctx.handle, params.handle, sc2.data_ptr(), 2, 0, aff2.data_ptr(), None))
    assert direct > 0 and 1.7 * direct <= ctx.msm_last_shape()["pairs"] <= 2.3 * direct
    one_msm = lambda: 0.85 * direct <= ctx.msm_last_shape()["pairs"] <= 1.15 * direct
    assert VI.verify(v, cz, proofs[0]) == (True, 0) and one_msm()
    assert v.verify_batch(proofs, inst, num_circuits=1) is True and v.first_malformed == -1 and one_msm()
    bad = list(proofs)
    bad[5] = VI.flip(bad[5], VI.sections(po, cz, len(bad[5]))["opening f"][0])
    assert v.verify_batch(bad, inst, num_circuits=1) is False and v.first_malformed == -1 and v.last_reject == VI.OPENING and one_msm()
    assert VI.verify(v, cz, bad[5]) == (False, VI.OPENING)
    bad[2] = bad[2][:-1]
    assert v.verify_batch(bad, inst, num_circuits=1) is False and v.first_malformed == 2 and v.last_reject == VI.MALFORMED
    wrong = [cz["instances"]] * 7 + [[[[5, 7, 9, 12]]]]
    assert v.verify_batch(proofs, wrong, num_circuits=1) is False and v.last_reject == VI.OPENING
    assert v.verify_batch(proofs[:2], inst[:2], num_circuits=1) is True and one_msm()


@pytest.mark.gpu
def test_kzg_verifier_beside_the_ipa_verifier(pkg, po, co, ctx, hosts, devices):
    import verify_cases as VC
    cz, proof, _ = hosts("one")
    _, _, v = devices("one")
    kz = VC.case(pkg, po, co, "one")
    kproof = VC.proof(pkg, po, co, "one", "gwc")
    vk = VC.host_verifier(pkg, kz, "gwc", ctx=ctx)
    assert VC.verify(vk, kz, kproof) == (True, 0)
    assert VI.verify(v, cz, proof) == (True, 0)
    assert VC.verify(vk, kz, kproof) == (True, 0) and VC.verify(vk, kz, VC.flip(kproof, 40)) [0] is False
    assert VI.verify(v, cz, kproof)[0] is False      # the other scheme's bytes
    with pytest.raises(pkg.DehaloError) as e:
        from dehalo2_amd import native
        native.Verifier.from_pk(devices("one")[0], devices("one")[1])      # the KZG constructor keeps refusing ParamsIPA
    assert e.value.code == -5 and "KZG over BN254 only" in str(e.value)
    vk.release()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 6])
def test_ipa_verify_gives_verify_openings_verdicts(pkg, po, co, ctx, k):
    """stand-alone openings as tests/test_ipa.py makes them: the oracle's reference opening and the device's own, a wrong v, a wrong x3, tampered and cut bytes"""
    import ipa
    import plonk_oracle
    import verifier as V
    from dehalo2_amd import native
    from dehalo2_amd.prover import SeededRng
    spec, curve = pkg.fields.VESTA, po.VESTA
    g = co.synth_bases(spec.id, 1 << k)
    uw = co.fixed_base_mul(spec.id, co.fill_scalars(spec.scalar.id, "uniform", 2, 7))
    u, w = uw[0], uw[1]
    params = native.ParamsIPA.create(ctx, spec, k, g, g, w, u)
    rng = np.random.default_rng(k)
    poly = [int.from_bytes(rng.bytes(32), "little") % curve.scalar.p for _ in range(1 << k)]
    blind, x3 = 777 + k, 0x1234567 + k
    P = ipa.commit_reference(curve, g, w, poly, blind)
    v = po.eval_polynomial(curve.scalar, poly, x3)
    reference = ipa.open_reference(plonk_oracle.Transcript(curve), curve, g, u, w, poly, blind, x3, SeededRng(3).scalars)
    d_poly = ctx.upload(spec.scalar.encode_many(poly))
    own = params.open(d_poly.data_ptr(), blind, x3, rng=SeededRng(11)).finalize() if k == 6 else None      # (the device's own opening at the k its suite opens at)
    oracle = lambda PP, xx, vv, data: ipa.verify_opening(V.ReadTranscript(curve, data), curve, g, u, w, PP, xx, vv)
    for proof in (reference, own) if own else (reference,):
        cases = [(P, x3, v, proof), (P, x3, (v + 1) % curve.scalar.p, proof), (P, x3 + 1, v, proof), (P, x3, v, proof[:-1]), (P, x3, v, proof + b"\0"), (P, x3, v, b"")]
        for off in (0, 32, 64, 32 + 64 * k - 32, len(proof) - 64, len(proof) - 32):      # S, L_1, R_1, R_k, c, f
            cases.append((P, x3, v, VI.flip(proof, off + 3)))
        cases.append((ipa.commit_reference(curve, g, w, poly, blind + 1), x3, v, proof))
        for i, (PP, xx, vv, data) in enumerate(cases):
            assert native.ipa_verify(params, PP, xx, vv, data) is oracle(PP, xx, vv, data) is (i == 0), i
    kzg = native.ParamsKZG.setup(ctx, pkg.fields.BN254, 4, 0x5EED)
    with pytest.raises(pkg.DehaloError) as e:
        native.ipa_verify(kzg, (1, 2), 3, 4, reference)
    assert e.value.code == -1
    kzg.release(); params.release()
