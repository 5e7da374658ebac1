"""GPU suite: dehalo_verify_proofs_each on verifiers with a context -- every proof's weighted term lists summed apart by ONE dehalo_msm_segments launch
(csrc/msm_segments.cuh), the subset checks' pairing on the host (IPA: dehalo_ipa_s_device and the MSM over g per check) -- against the host verifier and the single
verdicts.

The batches are tests/test_verify_each_host.py's (8 and 9 proofs; bad set none, {5}, {0, last}, all; one truncated beside one flipped; count 0 and 1; copies of one
invalid proof) on a KZG verifier made from the vk bytes ("one", "three", "instance", GWC and SHPLONK), on one made from the native key, and on the IPA verifier
("one", "instance"): the reasons are verify's on each proof alone and the host verifier's on the same batch, the checks stay within the search's bound.  A batch of
eight native proofs under distinct keyed generators: all valid costs one check, proof 5 flipped is named alone."""
import pytest

import test_verify_each_host as H
import verify_cases as VC
import verify_ipa_cases as VI

pytestmark = pytest.mark.gpu


def same_as_host(dev, host):
    """the device verifier's reasons on every batch of the host suite are the host verifier's"""
    for size in (8, 9):
        for label, proofs, _ in H.batches_of(host, size):
            assert H.each(dev, proofs)[0] == H.each(host, proofs)[0], label


@pytest.mark.parametrize("name,multiopen", H.KZG)
def test_kzg_verifier_from_vk_bytes(pkg, po, co, ctx, name, multiopen):
    dev, host = H.Kzg(pkg, po, co, name, multiopen, ctx=ctx), H.Kzg(pkg, po, co, name, multiopen)
    H.run_case(dev)
    same_as_host(dev, host)
    t = dev.v.last_timings()
    assert list(t) == ["decompress", "walk", "msm", "pairing"] and all(x >= 0 for x in t.values())
    dev.v.release(); host.v.release()


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
def test_kzg_verifier_from_the_native_key(pkg, po, co, ctx, multiopen):
    import test_verify_device as TD
    from dehalo2_amd import native
    cz = VC.case(pkg, po, co, "one")
    params, pk = TD._native_key(pkg, ctx, po, cz)
    dev = H.Kzg(pkg, po, co, "one", multiopen, verifier=native.Verifier.from_pk(params, pk, multiopen))
    host = H.Kzg(pkg, po, co, "one", multiopen)
    H.run_case(dev)
    H.edge_counts(dev)
    same_as_host(dev, host)
    dev.v.release(); host.v.release(); pk.release(); params.release()


@pytest.mark.parametrize("name", H.IPA)
def test_ipa_verifier(pkg, po, co, ctx, name):
    from dehalo2_amd import native
    cz = VI.case(pkg, po, co, name)
    c = cz["c"]
    params = native.ParamsIPA.create(ctx, pkg.fields.VESTA, c["k"], c["srs"]["g"], c["srs"]["g_lagrange"], c["w"], c["u"])
    pk = native.ProvingKey.keygen(ctx, params, cz["cs"], cz["fixed"], cz["asm"], cz["selectors"])
    assert pk.vk_bytes() == cz["vk"]
    pk.transcript_repr = c["rep"]
    dev, host = H.Ipa(pkg, po, co, name, verifier=native.Verifier.from_ipa(params, pk)), H.Ipa(pkg, po, co, name)
    H.run_case(dev)
    H.edge_counts(dev)
    same_as_host(dev, host)
    dev.v.release(); host.v.release(); pk.release(); params.release()


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
def test_batch_of_eight_native_proofs(pkg, po, co, ctx, multiopen):
    import test_verify_device as TD
    from dehalo2_amd import native, prover
    cz = VC.case(pkg, po, co, "one")
    params, pk = TD._native_key(pkg, ctx, po, cz)
    P = native.Prover(params, pk, multiopen=multiopen)
    proofs = native.create_proofs([P], cz["witnesses"][0], [prover.KeyedRng(bytes([i + 1]) * 32) for i in range(8)])
    assert len(set(proofs)) == 8
    v = native.Verifier.from_pk(params, pk, multiopen)
    inst = [cz["instances"]] * 8
    assert v.verify_each(proofs, inst, num_circuits=1) == [0] * 8 and v.last_checks == 1
    assert v.verify_each(proofs, inst, rng=prover.KeyedRng(b"w" * 32), num_circuits=1) == [0] * 8 and v.last_checks == 1
    bad = list(proofs)
    bad[5] = TD._evaluation_flipped(po, cz, proofs[5], multiopen)
    assert v.verify_each(bad, inst, num_circuits=1) == [0] * 5 + [VC.PAIRING] + [0] * 2 and v.last_checks <= H.bound(8, 1)
    assert [VC.verify(v, cz, p)[0] for p in bad] == [True] * 5 + [False] + [True] * 2
    assert v.verify_batch(bad, inst, num_circuits=1) is False and v.verify_batch(proofs, inst, num_circuits=1) is True      # the batch call is what it was
    bad[2] = bad[2][:-32]
    assert v.verify_each(bad, inst, num_circuits=1) == [0, 0, VC.MALFORMED, 0, 0, VC.PAIRING, 0, 0] and v.last_checks <= H.bound(7, 1)
    host = VC.host_verifier(pkg, cz, multiopen)      # the same batch on the host verifier
    assert host.verify_each(bad, inst, num_circuits=1) == [0, 0, VC.MALFORMED, 0, 0, VC.PAIRING, 0, 0]
    host.release(); v.release(); P.release(); pk.release(); params.release()
