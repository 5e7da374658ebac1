"""GPU suite: dehalo_pairing_checks on the device (csrc/pairing.cuh: one wave per check over the line tables of fixed G2 points) against the HOST table on the
same inputs -- GT word for word, status byte for byte -- and the verifier's device mode (dehalo_verifier_set_pairing) against its host mode.

Kernel: pairs in 1, 2, 3 x checks in 1, 2, 3 and one block's checks + 1 (the kernel's own constant, dehalo_pairing_checks_per_block), check c cancelling iff
c % 3 != 1 with points of its own, so that a mixed-up index shows; the identity in either slot and in both, a = r - 1, the word x + q, a Q that is the
identity, one P off the curve between two valid checks (status 2, its neighbours 1), d_gt = NULL, the device-memory entry point, and one GT compared with the
oracle's directly.  The milliseconds of each launch are printed.
Verifier: tests/test_verify_each_host.py's batches of 8 and 9 under GWC and SHPLONK -- the reasons are host mode's, last_checks is the number of live proofs,
verify and verify_batch give host mode's verdicts; count 0 and 1; an IPA verifier refuses the mode; a verifier never switched still makes one check."""
import time

import numpy as np
import pytest

import pairing_cases as PCS
import test_verify_each_host as H
import verify_cases as VC
import verify_ipa_cases as VI
from test_pairing_host import pr  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables(pkg, ctx, pr):
    """pairs -> (device table, host table) over the same Q_j = [b_j] G2"""
    made = {}

    def fn(pairs):
        if pairs not in made:
            raws = PCS.g2_raws(pr, pairs)
            made[pairs] = (pkg.PairingTable(ctx, pkg.fields.BN254.id, raws), pkg.PairingTable(None, pkg.fields.BN254.id, raws))
        return made[pairs]
    yield fn
    for dev, host in made.values():
        dev.release(); host.release()


def same_as_host(ctx, dev, host, g1, label):
    t0 = time.perf_counter()
    status, gt = ctx.pairing_checks(dev, g1, gt=True)
    ms = (time.perf_counter() - t0) * 1e3
    print("%s: %d checks x %d pairs, %.3f ms (upload, launch, download)" % (label, g1.shape[0], g1.shape[1], ms))
    want_status, want_gt = host.checks(g1, gt=True)
    assert status.tobytes() == want_status.tobytes(), label
    assert gt.tobytes() == want_gt.tobytes(), label
    return status, gt


@pytest.mark.parametrize("pairs", [1, 2, 3])
def test_interleaved_checks_are_the_host_tables(pkg, po, pr, ctx, tables, pairs):
    dev, host = tables(pairs)
    per_block = pkg.load_library().dehalo_pairing_checks_per_block(dev.handle)
    assert per_block >= 1
    for checks in (1, 2, 3, per_block + 1):
        g1, want = PCS.interleaved(pkg, po, pr, pairs, checks)
        status, _ = same_as_host(ctx, dev, host, g1, "interleaved")
        assert status.tolist() == want.tolist(), (pairs, checks)


def test_identities_noncanonical_words_and_a_point_off_the_curve(pkg, po, pr, ctx, tables):
    dev, host = tables(2)      # Q = G2, [7] G2
    r, q, f = pr.R, pr.Q, pkg.fields.BN254.base
    W = lambda a: PCS.words(pkg, PCS.g1_mul(po, pr, a))
    rows = [(W(0), W(3), 0), (W(3), W(0), 0), (W(0), W(0), 1),                      # the identity in either slot, and in both
            (W(r - 1), W(pow(7, -1, r)), 1), (W(r - 1), W(1), 0),                   # a = r - 1: -1 + 7 / 7 = 0
            (W(-7), W(1), 1), (W(-7), W(1), 2), (W(7), W(-1), 1)]                   # a P off the curve between two valid checks
    g1 = np.stack([np.stack([a, b]) for a, b, _ in rows])
    g1[6, 1, :4] = f.encode(5)                                                       # (5, y of G1): not on the curve
    x = sum(int(v) << (64 * j) for j, v in enumerate(g1[3, 0, :4])) + q            # the word x + q
    assert x < 1 << 256
    g1[3, 0, :4] = np.frombuffer(x.to_bytes(32, "little"), dtype=np.uint64)
    status, gt = same_as_host(ctx, dev, host, g1, "special points")
    assert status.tolist() == [w for _, _, w in rows]
    assert not gt[6].any()
    assert ctx.pairing_checks(dev, g1).tobytes() == status.tobytes()                # d_gt = NULL


def test_identity_q_contributes_one(pkg, po, pr, ctx):
    raws = [bytes(128), pr.g2_to_raw(pr.G2), bytes(128)]
    dev, host = pkg.PairingTable(ctx, 0, raws), pkg.PairingTable(None, 0, raws)
    W = lambda a: PCS.words(pkg, PCS.g1_mul(po, pr, a))
    g1 = np.stack([np.stack([W(5), W(0), W(9)]), np.stack([W(5), W(2), W(9)])])
    status, _ = same_as_host(ctx, dev, host, g1, "identity Q")
    assert status.tolist() == [1, 0]
    dev.release(); host.release()


def test_device_memory_entry_point(pkg, po, pr, ctx, tables):
    import torch
    dev, host = tables(2)
    g1, want = PCS.interleaved(pkg, po, pr, 2, 3)
    d_g1 = ctx.upload(g1)
    d_status = torch.full((3,), 7, dtype=torch.uint8, device=d_g1.device)
    d_gt = torch.zeros((3, 12, 4), dtype=torch.int64, device=d_g1.device)
    ctx.pairing_checks_device(dev, d_g1.data_ptr(), 3, d_status.data_ptr(), d_gt.data_ptr())
    ctx.synchronize()
    want_status, want_gt = host.checks(g1, gt=True)
    assert d_status.cpu().numpy().tobytes() == want_status.tobytes() == want.tobytes()
    assert ctx.download_tensor(d_gt).tobytes() == want_gt.tobytes()
    ctx.pairing_checks_device(dev, 0, 0, 0)      # checks = 0 takes null arrays
    for bad in (lambda: ctx.pairing_checks_device(host, d_g1.data_ptr(), 3, d_status.data_ptr()),           # a host table
                lambda: ctx.pairing_checks_device(dev, 0, 3, d_status.data_ptr()),
                lambda: ctx.pairing_checks_device(dev, d_g1.data_ptr(), 3, 0),
                lambda: ctx.pairing_checks_device(dev, d_g1.data_ptr(), (1 << 20) + 1, d_status.data_ptr())):
        with pytest.raises(pkg.DehaloError) as e:
            bad()
        assert e.value.code == -1
    with pytest.raises(ValueError):
        ctx.pairing_checks(host, g1)


def test_device_gt_is_the_oracles(pkg, pr, ctx, tables):
    dev, _ = tables(1)
    status, gt = ctx.pairing_checks(dev, PCS.words(pkg, pr.G1).reshape(1, 1, 8), gt=True)
    assert status.tolist() == [0] and PCS.gt_to_f12(pkg, pr, gt[0]) == pr.pairing(pr.G2, pr.G1)


# ------------------------------------------------------------------------------------------------------------------------------ the verifier's device mode
@pytest.mark.parametrize("name,multiopen", [("one", mo) for mo in VC.MULTIOPENS] + [("instance", mo) for mo in VC.MULTIOPENS])
def test_verifier_device_mode_gives_host_modes_verdicts(pkg, po, co, ctx, name, multiopen):
    s = H.Kzg(pkg, po, co, name, multiopen, ctx=ctx)
    inst = lambda proofs: [s.instances] * len(proofs)
    for size in (8, 9):
        for label, proofs, _ in H.batches_of(s, size):
            s.v.set_pairing("host")
            want = H.each(s, proofs)[0]
            want_batch = s.v.verify_batch(proofs, inst(proofs), num_circuits=s.N)
            want_single = {p: s.single(p) for p in set(proofs)}
            s.v.set_pairing("device")
            reasons, checks = H.each(s, proofs)
            assert reasons == want, label
            assert checks == sum(1 for r in reasons if r in (0, VC.PAIRING)), label      # one check per live proof, no search
            assert s.v.verify_batch(proofs, inst(proofs), num_circuits=s.N) is want_batch, label
            assert {p: s.single(p) for p in set(proofs)} == want_single, label
    t = s.v.last_timings()
    assert list(t) == ["decompress", "walk", "msm", "pairing"] and all(x >= 0 for x in t.values())
    s.v.release()


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
def test_verifier_device_mode_count_zero_and_one(pkg, po, co, ctx, multiopen):
    s = H.Kzg(pkg, po, co, "one", multiopen, ctx=ctx)
    s.v.set_pairing("device")
    good, bad = s.valid[0], s.flipped(s.valid[0])
    assert H.each(s, []) == ([], 0)
    assert H.each(s, [good]) == ([0], 1)
    assert H.each(s, [bad]) == ([VC.PAIRING], 1)
    assert H.each(s, [good[:-32]]) == ([VC.MALFORMED], 0)
    assert H.each(s, [good, bad, bad, good]) == ([0, VC.PAIRING, VC.PAIRING, 0], 4)
    # each proof is checked by itself: two copies of one invalid proof under w_1 = r - 1 no longer cancel
    w = H.Weights(pkg.fields.BN254.scalar, [H.R_BN254 - 1])
    assert H.each(s, [bad, bad], rng=w) == ([VC.PAIRING] * 2, 2) and w.drawn == 1
    assert s.single(good) == (True, 0) and s.single(bad) == (False, VC.PAIRING)
    s.v.release()


def test_verifier_made_in_device_mode_and_one_never_switched(pkg, po, co, ctx):
    from dehalo2_amd import native
    cz = VC.case(pkg, po, co, "one")
    c = cz["c"]
    g2, sg2 = VC.g2_raw(c)
    proofs = [VC.proof(pkg, po, co, "one", "gwc", s) for s in H.SEEDS] * 2
    inst = [cz["instances"]] * 4
    v = native.Verifier.from_vk(pkg.fields.BN254, c["k"], np.asarray(c["srs"]["g"][0]), g2, sg2, cz["cs"], cz["vk"], num_selectors=len(cz["selectors"]), ctx=ctx,
                                transcript_repr=c["rep"], pairing="device")
    assert v.verify_each(proofs, inst, num_circuits=1) == [0] * 4 and v.last_checks == 4
    v.release()
    v = VC.host_verifier(pkg, cz, ctx=ctx)      # never switched: the search's one check on a valid batch
    assert v.verify_each(proofs, inst, num_circuits=1) == [0] * 4 and v.last_checks == 1
    v.release()


def test_ipa_verifier_refuses_the_mode(pkg, po, co, ctx):
    from dehalo2_amd import native
    cz = VI.case(pkg, po, co, "one")
    c = cz["c"]
    params = native.ParamsIPA.create(ctx, pkg.fields.VESTA, c["k"], c["srs"]["g"], c["srs"]["g_lagrange"], c["w"], c["u"])
    pk = native.ProvingKey.keygen(ctx, params, cz["cs"], cz["fixed"], cz["asm"], cz["selectors"])
    v = native.Verifier.from_ipa(params, pk)
    with pytest.raises(pkg.DehaloError) as e:
        v.set_pairing("device")
    assert e.value.code == -1
    v.set_pairing("host")
    v.release(); pk.release(); params.release()
