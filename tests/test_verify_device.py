"""GPU suite: the device verifier (a dehalo_verifier with a context: every point of a call through one dehalo_points_decompress_device launch, the two sums of
the reduction through the fresh-bases MSM, the pairing on the host) against the host verifier and the oracle.

The device verifier gives the host verifier's verdict and reason on every case of tests/test_verify_host.py (the oracle prover's proofs, tests/verify_cases.py);
native proofs -- create_proof, create_proof_multi over two circuits, create_proof_phased, GWC and SHPLONK, create_proof_circuit of pose_enc at K = 11 -- are accepted
natively and by the oracle, and rejected by both with one evaluation byte flipped; a verifier from the key and one from the key's vk bytes agree; a batch of eight
native proofs under distinct keyed generators is accepted, rejected with proof 5 tampered, and proof 5 is rejected singly."""
import numpy as np
import pytest

import verify_cases as VC

pytestmark = pytest.mark.gpu

R_BN254 = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
@pytest.mark.parametrize("name", VC.NAMES)
def test_device_verifier_gives_the_host_verifiers_verdicts(pkg, po, co, ctx, name, multiopen):
    cz = VC.case(pkg, po, co, name)
    proof = VC.proof(pkg, po, co, name, multiopen)
    host, dev = VC.host_verifier(pkg, cz, multiopen), VC.host_verifier(pkg, cz, multiopen, ctx=ctx)
    secs = VC.sections(po, cz, multiopen)
    first_eval = secs.pop("first evaluation offset")[0]
    probes = {"valid": proof, "truncated by 1": proof[:-1], "truncated by 32": proof[:-32], "one trailing byte": proof + b"\0",
              "a scalar replaced by r": proof[:first_eval] + R_BN254.to_bytes(32, "little") + proof[first_eval + 32:]}
    probes.update({label: VC.flip(proof, off) for label, (off, _) in secs.items()})
    want = {label: VC.verify(host, cz, data) for label, data in probes.items()}
    assert want["valid"] == (True, 0) and not any(w[0] for label, w in want.items() if label != "valid")
    assert {w[1] for w in want.values()} >= {0, VC.MALFORMED, VC.PAIRING}
    for label, data in probes.items():
        assert VC.verify(dev, cz, data) == want[label], label
    assert VC.verify(dev, cz, proof) == VC.verify(dev, cz, proof) == (True, 0)      # twice in a row: no state between calls
    if name == "instance":
        wrong = [[list(cz["instances"][0][0])]]
        wrong[0][0][0] += 1
        assert VC.verify(dev, cz, proof, wrong) == VC.verify(host, cz, proof, wrong) == (False, VC.PAIRING)
        with pytest.raises(pkg.DehaloError) as e:
            dev.verify(proof, [[]], num_circuits=1)
        assert e.value.code == -1
    t = dev.last_timings()
    assert all(t[key] >= 0 for key in ("decompress", "walk", "msm", "pairing"))
    host.release(); dev.release()


def _native_key(pkg, ctx, po, cz):
    """-> (params, pk) of the case's chain: its SRS, its circuit, the oracle's transcript_repr"""
    import pairing as pr
    from dehalo2_amd import native
    c = cz["c"]
    params = native.ParamsKZG.create(ctx, pkg.fields.BN254, c["k"], c["srs"]["g"], c["srs"]["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(c["s_g2"]))
    pk = native.ProvingKey.keygen(ctx, params, cz["cs"], cz["fixed"], cz["asm"], cz["selectors"])
    assert pk.vk_bytes() == cz["vk"]
    pk.transcript_repr = c["rep"]
    return params, pk


def _evaluation_flipped(po, cz, proof, multiopen):
    return VC.flip(proof, VC.sections(po, cz, multiopen)["advice evaluation"][0])


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
@pytest.mark.parametrize("how", ["create_proof", "create_proof_multi", "create_proof_phased"])
def test_native_proofs_are_accepted_natively_and_by_the_oracle(pkg, po, co, ctx, how, multiopen):
    import phased_circuits as PH
    from dehalo2_amd import native, prover
    name = {"create_proof": "one", "create_proof_multi": "three", "create_proof_phased": "phased"}[how]
    cz = VC.case(pkg, po, co, name)
    params, pk = _native_key(pkg, ctx, po, cz)
    if how == "create_proof":
        P = native.Prover(params, pk, multiopen=multiopen)
        proof = P.create_proof(cz["witnesses"][0], cz["instances"][0], prover.SeededRng(21)).finalize()
    elif how == "create_proof_multi":      # two of the case's three witnesses: the verifier is told N = 2
        cz = dict(cz, N=2, instances=cz["instances"][:2])
        P = native.Prover(params, pk, multiopen=multiopen, num_circuits=2)
        proof = P.create_proof_multi(cz["witnesses"][:2], cz["instances"], prover.SeededRng(21)).finalize()
    else:
        P = native.Prover(params, pk, multiopen=multiopen)
        proof = P.create_proof_phased(cz["witnesses"][0], [], prover.SeededRng(21)).finalize()
    from_pk = native.Verifier.from_pk(params, pk, multiopen)
    from_vk = VC.host_verifier(pkg, cz, multiopen, vk=pk.vk_bytes(), ctx=ctx)
    host = VC.host_verifier(pkg, cz, multiopen)
    bad = _evaluation_flipped(po, cz, proof, multiopen)
    for v in (from_pk, from_vk, host):
        assert VC.verify(v, cz, proof) == (True, 0)
        assert VC.verify(v, cz, bad) == (False, VC.PAIRING)
        assert VC.verify(v, cz, proof[:-1]) == (False, VC.MALFORMED)
    assert VC.oracle_accepts(po, cz, proof, multiopen) is True and VC.oracle_accepts(po, cz, bad, multiopen) is False
    for v in (from_pk, from_vk, host):
        v.release()
    P.release(); pk.release(); params.release()


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
def test_pose_enc_proof_of_the_circuit_call(pkg, po, co, ctx, multiopen):
    """create_proof_circuit of pose_enc at K = 11 on a device-made SRS: every part of the verifier's input comes from the native objects -- the vk bytes, the
    substitute transcript_repr, g2 and s_g2 of the params -- and the oracle is given the same"""
    import pairing as pr
    import shapes
    import verifier as V
    import shplonk_oracle
    from dehalo2_amd import keygen, native, plonk, prover
    k, s, curve = 11, 0x5EED1234, pkg.fields.BN254
    inputs = dict(key=[5, 6], message=[0, 0])
    nat = native.synthesize(native.CIRCUIT_POSE_ENC, k, keygen=True, **inputs)
    cs = plonk.maingate_cs(False)
    asm = plonk.Assembly(6, 1 << k)
    asm.mapping = nat["mapping"].astype(np.int64)
    params = native.ParamsKZG.setup(ctx, curve, k, s)
    pk = native.ProvingKey.keygen(ctx, params, cs, nat["fixed"], asm, nat.get("selectors", ()))
    P = native.Prover(params, pk, multiopen=multiopen)
    proof = P.create_proof_circuit(native.CIRCUIT_POSE_ENC, [[]], prover.SeededRng(3), **inputs)[0].finalize()
    v = native.Verifier.from_pk(params, pk, multiopen)
    raw = params.write()
    g0, g2, s_g2 = np.frombuffer(raw[4:68], dtype=np.uint64), raw[-256:-128], raw[-128:]
    assert g2 == pr.g2_to_raw(pr.G2) and s_g2 == pr.g2_to_raw(pr.g2_mul(s, pr.G2))
    v2 = native.Verifier.from_vk(curve, k, g0, g2, s_g2, cs, pk.vk_bytes("processed"), num_selectors=len(nat.get("selectors", ())), format="processed", ctx=ctx,
                                 multiopen=multiopen)      # transcript_repr: the substitute, from the vk bytes alone
    sh_evals = 32 * (cs.num_advice + 3 * len(cs.lookups) + cs.num_permutation_sets() + 1 + (cs.degree() - 1))
    bad = VC.flip(proof, sh_evals)
    for ver in (v, v2):
        assert ver.verify(proof, [[]]) is True and ver.last_reject == 0
        assert ver.verify(bad, [[]]) is False and ver.last_reject == VC.PAIRING
        assert ver.verify(proof, [[]]) is True
    vk = pk.vk_bytes()
    nf, npc = cs.num_fixed, len(cs.permutation_columns)
    pts = keygen.decode_points(curve, np.frombuffer(vk[8:8 + 64 * (nf + npc)], dtype=np.uint64).reshape(-1, 8))
    oracle = shplonk_oracle.verify_proof_shplonk if multiopen == "shplonk" else V.verify_proof
    args = (po.BN254, shapes.maingate_description(False), k, pts[:nf], pts[nf:], pk.transcript_repr, (1, 2), pr.G2, pr.g2_mul(s, pr.G2), [[]])
    assert oracle(*args, proof) is True and oracle(*args, bad) is False
    v.release(); v2.release(); P.release(); pk.release(); params.release()


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
def test_batch_of_eight_native_proofs(pkg, po, co, ctx, multiopen):
    from dehalo2_amd import native, prover
    cz = VC.case(pkg, po, co, "one")
    params, pk = _native_key(pkg, ctx, po, cz)
    P = native.Prover(params, pk, multiopen=multiopen)
    proofs = native.create_proofs([P], cz["witnesses"][0], [prover.KeyedRng(bytes([i + 1]) * 32) for i in range(8)])
    assert len(set(proofs)) == 8
    v = native.Verifier.from_pk(params, pk, multiopen)
    inst = [cz["instances"]] * 8
    assert v.verify_batch(proofs, inst, num_circuits=1) is True and v.first_malformed == -1
    assert v.verify_batch(proofs, inst, rng=prover.KeyedRng(b"w" * 32), num_circuits=1) is True
    bad = list(proofs)
    bad[5] = _evaluation_flipped(po, cz, proofs[5], multiopen)
    assert v.verify_batch(bad, inst, num_circuits=1) is False and v.first_malformed == -1 and v.last_reject == VC.PAIRING
    assert [VC.verify(v, cz, p)[0] for p in bad] == [True] * 5 + [False] + [True] * 2
    assert VC.oracle_accepts(po, cz, proofs[5], multiopen) is True and VC.oracle_accepts(po, cz, bad[5], multiopen) is False
    bad[2] = bad[2][:-32]
    assert v.verify_batch(bad, inst, num_circuits=1) is False and v.first_malformed == 2
    host = VC.host_verifier(pkg, cz, multiopen)      # the same batch on the host verifier
    assert host.verify_batch(proofs, inst, num_circuits=1) is True
    host.release(); v.release(); P.release(); pk.release(); params.release()


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
def test_device_verifier_on_the_remaining_host_cases(pkg, po, co, ctx, multiopen):
    """what tests/test_verify_host.py checks beside the tampered bytes, on a verifier with a context: a wrong transcript_repr, the s_g2 of another secret, the other
    multiopen's proof, and a verifier made from the vk in each SerdeFormat -- verdict and reason are the host verifier's"""
    import pairing as pr
    import proof_chains as PC
    other = {"gwc": "shplonk", "shplonk": "gwc"}[multiopen]
    for name in ("one", "shuffle"):
        cz = VC.case(pkg, po, co, name)
        proof, foreign = VC.proof(pkg, po, co, name, multiopen), VC.proof(pkg, po, co, name, other)
        bad = VC.flip(proof, VC.sections(po, cz, multiopen)["advice evaluation"][0])
        pairs = []      # (host verifier, device verifier) made alike
        plain = dict(multiopen=multiopen)
        wrong_secret = dict(multiopen=multiopen, s_g2=pr.g2_to_raw(pr.g2_mul(PC.S_TOXIC + 1, pr.G2)))
        for kw in (plain, wrong_secret):
            pairs.append((VC.host_verifier(pkg, cz, **kw), VC.host_verifier(pkg, cz, ctx=ctx, **kw)))
        for fmt in ("processed", "raw", "raw-unchecked"):
            kw = dict(multiopen=multiopen, format=fmt, vk=VC.vk_in_format(pkg, cz, fmt))
            pairs.append((VC.host_verifier(pkg, cz, **kw), VC.host_verifier(pkg, cz, ctx=ctx, **kw)))
        wrong_repr = (VC.host_verifier(pkg, cz, multiopen), VC.host_verifier(pkg, cz, multiopen, ctx=ctx))
        for v in wrong_repr:
            v.transcript_repr = cz["c"]["rep"] + 1
        pairs.append(wrong_repr)
        verdicts = []
        for host, dev in pairs:
            for data in (proof, bad, foreign):
                want = VC.verify(host, cz, data)
                assert VC.verify(dev, cz, data) == want, (name, data is proof, data is bad)
                verdicts.append(want)
            host.release(); dev.release()
        # plain: accept, PAIRING, reject; another secret and another transcript_repr: PAIRING on the valid proof; every format as the plain one
        assert verdicts[0] == (True, 0) and verdicts[1] == (False, VC.PAIRING) and verdicts[2][0] is False
        assert verdicts[3] == (False, VC.PAIRING) and verdicts[15] == (False, VC.PAIRING)
        assert verdicts[6:9] == verdicts[9:12] == verdicts[12:15] == verdicts[0:3]


def test_params_ipa_and_pasta_are_unsupported(pkg, po, co, ctx):
    """IPA verification is not part of the library: a verifier from a ParamsIPA (which exists over Pallas and Vesta only) is DEHALO_ERR_UNSUPPORTED, whatever the
    key; so is one from a Pasta key's bytes with a context, and the error text says why"""
    from dehalo2_amd import native
    cz = VC.case(pkg, po, co, "shuffle")
    k = cz["c"]["k"]
    with pytest.raises(pkg.DehaloError) as e:      # no ParamsIPA over BN254 to make a verifier from
        native.ParamsIPA.generate(ctx, pkg.fields.BN254, k)
    assert e.value.code == -5
    kzg_params, kzg_pk = _native_key(pkg, ctx, po, cz)
    for curve in (pkg.fields.VESTA, pkg.fields.PALLAS):
        params = native.ParamsIPA.generate(ctx, curve, k)
        pk = native.ProvingKey.keygen(ctx, params, cz["cs"], cz["fixed"], cz["asm"], ())
        for p, key in ((params, pk), (params, kzg_pk), (kzg_params, pk)):      # IPA params with its own key, with a BN254 key; KZG params with a Pasta key
            with pytest.raises(pkg.DehaloError) as e:
                native.Verifier.from_pk(p, key)
            assert e.value.code == -5 and "KZG over BN254 only" in str(e.value)
        g2, s_g2 = VC.g2_raw(cz["c"])
        with pytest.raises(pkg.DehaloError) as e:
            native.Verifier.from_vk(curve, k, np.zeros(8, dtype=np.uint64), g2, s_g2, cz["cs"], pk.vk_bytes(), ctx=ctx)
        assert e.value.code == -5
        pk.release(); params.release()
    v = native.Verifier.from_pk(kzg_params, kzg_pk)      # and the KZG pair beside them is taken
    assert VC.verify(v, cz, VC.proof(pkg, po, co, "shuffle", "gwc")) == (True, 0)
    v.release(); kzg_pk.release(); kzg_params.release()
