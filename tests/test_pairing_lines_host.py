"""CPU suite: the line tables of fixed G2 points (csrc/pairing_host.hpp: line_table, miller_table, table_checks) and dehalo_pairing_checks on a HOST table.

tests/native_host/pairing_lines_check.cpp (g++, ASan + UBSan, a program of its own) builds the table of Q in G2, [7] G2, [b] G2 and walks it for P = [a] G1,
a in 1, 5, r - 1: 102 steps, and miller_table's 48 words are miller()'s.  The identity on either side gives 1.  Through ctypes: the statuses of a host table
are dehalo_pairing_check's verdicts on tests/test_pairing_host.py's kinds of cases; GT for e(G1, G2) and one e([a] G1, [b] G2) is oracle/pairing.py's pairing()
after the change of basis (two oracle pairings, about a second each); the argument errors; and a host verifier refuses the device mode."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import pairing_cases as PCS
from conftest import ROOT
from test_pairing_host import off_subgroup, pr  # noqa: F401  (fixtures)


@pytest.fixture(scope="module")
def lines_check():
    out = subprocess.run(["make", "-C", ROOT, "pairing_lines_check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr

    def run(lines):
        r = subprocess.run([os.path.join(ROOT, "tests", "native_host", "pairing_lines_check")], input="".join(s + "\n" for s in lines), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        got = [json.loads(s) for s in r.stdout.splitlines()]
        assert len(got) == len(lines)
        return got
    return run


def _miller_line(pkg, g2_raw, P):
    return "miller %s %s" % (bytes(g2_raw).hex(), PCS.words(pkg, P).tobytes().hex())


def test_table_has_102_steps_and_walks_to_millers_words(pkg, po, pr, lines_check):
    cases = [(b, a) for b in PCS.BS for a in (1, 5, pr.R - 1)]
    got = lines_check([_miller_line(pkg, pr.g2_to_raw(pr.g2_mul(b, pr.G2)), PCS.g1_mul(po, pr, a)) for b, a in cases])
    for (b, a), g in zip(cases, got):
        assert g == {"g2": 0, "g1": 1, "built": True, "steps": 102, "one": False, "equal": True, "is_one": False}, (b, a)


def test_identities_give_one(pkg, pr, lines_check):
    q_id, p_id = lines_check([_miller_line(pkg, bytes(128), pr.G1), _miller_line(pkg, pr.g2_to_raw(pr.G2), None)])
    assert q_id == {"g2": 0, "g1": 1, "built": True, "steps": 0, "one": True, "equal": True, "is_one": True}
    assert p_id == {"g2": 0, "g1": 1, "built": True, "steps": 102, "one": False, "equal": True, "is_one": True}


def test_host_table_statuses_are_pairing_checks_verdicts(pkg, po, pr):
    """a pair that cancels, ab + 1, identities beside pairs that do and do not cancel: one check over the case's own G2 points"""
    from dehalo2_amd import native
    oc, r, G1, G2 = po.BN254, pr.R, pr.G1, pr.G2
    a, b = 5, 7
    neg = lambda P: po.ec_neg(oc, P)
    cases = {"gen and its negation": [(G1, G2), (neg(G1), G2)], "gen alone": [(G1, G2)], "identity in G1": [(None, G2)], "identity in G2": [(G1, None)],
             "bilinear": [(PCS.g1_mul(po, pr, a), pr.g2_mul(b, G2)), (neg(PCS.g1_mul(po, pr, a * b)), G2)],
             "bilinear + 1": [(PCS.g1_mul(po, pr, a), pr.g2_mul(b, G2)), (neg(PCS.g1_mul(po, pr, a * b + 1)), G2)],
             "bilinear a = r - 1": [(PCS.g1_mul(po, pr, r - 1), pr.g2_mul(3, G2)), (PCS.g1_mul(po, pr, 3), G2)],
             "identities beside a pair that cancels": [(G1, G2), (None, pr.g2_mul(9, G2)), (neg(G1), G2), (PCS.g1_mul(po, pr, 4), None)],
             "identity beside a pair that does not cancel": [(G1, G2), (None, G2)]}
    for name, pairs in cases.items():
        raw = [(P, pr.g2_to_raw(Q)) for P, Q in pairs]
        want = native.pairing_check(pkg.fields.BN254, raw)
        assert want is not (name in ("gen alone", "bilinear + 1", "identity beside a pair that does not cancel")), name
        t = pkg.PairingTable(None, pkg.fields.BN254.id, [q for _, q in raw])
        status = t.checks(np.stack([PCS.words(pkg, P) for P, _ in raw]))
        assert status.tolist() == [1 if want else 0], name
        t.release()


def test_several_checks_over_one_table(pkg, po, pr):
    """every check its own verdict: checks that cancel and do not, interleaved, and a point off the curve between two valid checks"""
    t = pkg.PairingTable(None, pkg.fields.BN254.id, PCS.g2_raws(pr, 2))
    g1, want = PCS.interleaved(pkg, po, pr, 2, 4)
    assert want.tolist() == [1, 0, 1, 1]
    f = pkg.fields.BN254.base
    g1[2, 1, :4] = f.encode(1)      # (1, y) with the y of another point
    status, gt = t.checks(g1, gt=True)
    assert status.tolist() == [1, 0, 2, 1]
    assert not gt[2].any() and gt[0].any() and gt[1].any()
    one = np.zeros((12, 4), dtype=np.uint64)
    one[0] = f.encode(1)
    assert (gt[0] == one).all() and (gt[3] == one).all() and not (gt[1] == one).all()
    assert (t.checks(g1) == status).all()      # gt = NULL
    t.release()


def test_gt_is_the_oracles_after_the_change_of_basis(pkg, po, pr):
    a, b = 5, 7
    t = pkg.PairingTable(None, pkg.fields.BN254.id, [pr.g2_to_raw(pr.G2), pr.g2_to_raw(pr.g2_mul(b, pr.G2))])
    g1 = np.zeros((2, 2, 8), dtype=np.uint64)
    g1[0, 0] = PCS.words(pkg, pr.G1)                       # e(G1, G2)
    g1[1, 1] = PCS.words(pkg, PCS.g1_mul(po, pr, a))       # e([a] G1, [b] G2)
    status, gt = t.checks(g1, gt=True)
    assert status.tolist() == [0, 0]
    e = pr.pairing(pr.G2, pr.G1)
    assert PCS.gt_to_f12(pkg, pr, gt[0]) == e
    assert PCS.gt_to_f12(pkg, pr, gt[1]) == pr.pairing(pr.g2_mul(b, pr.G2), PCS.g1_mul(po, pr, a)) == pr.f12_pow(e, a * b)
    t.release()


def test_argument_errors(pkg, pr, off_subgroup):
    lib = pkg.load_library()
    g2 = pr.g2_to_raw(pr.G2)
    buf = lambda b: np.frombuffer(bytes(b), dtype=np.uint8)
    h = C.c_void_p()
    assert lib.dehalo_pairing_table_create(None, 0, buf(g2).ctypes.data, 0, C.byref(h)) == -1                # no pairs
    assert lib.dehalo_pairing_table_create(None, 0, buf(g2 * 9).ctypes.data, 9, C.byref(h)) == -1            # more than DEHALO_PAIRING_MAX_PAIRS
    assert lib.dehalo_pairing_table_create(None, 0, None, 1, C.byref(h)) == -1
    assert lib.dehalo_pairing_table_create(None, 0, buf(g2).ctypes.data, 1, None) == -1
    assert lib.dehalo_pairing_table_create(None, 1, buf(g2).ctypes.data, 1, C.byref(h)) == -5                # Pallas
    assert lib.dehalo_pairing_table_create(None, 2, buf(g2).ctypes.data, 1, C.byref(h)) == -5                # Vesta
    assert lib.dehalo_pairing_table_create(None, 3, buf(g2).ctypes.data, 1, C.byref(h)) == -1                # no such curve
    bad = bytearray(g2)
    bad[64] ^= 1                                                                                             # off the twist
    for q in (bytes(bad), g2[:96] + pr.Q.to_bytes(32, "little"), pr.g2_to_raw(off_subgroup)):
        with pytest.raises(pkg.DehaloError) as e:
            pkg.PairingTable(None, 0, [g2, q])
        assert e.value.code == -1
    t = pkg.PairingTable(None, 0, [g2] * 8)      # the maximum
    t.release()
    t = pkg.PairingTable(None, 0, [g2])
    g1 = np.zeros((1, 8), dtype=np.uint64)
    st = np.zeros(1, dtype=np.uint8)
    assert lib.dehalo_pairing_checks(t.handle, None, 0, None, None) == 0                                     # checks = 0 takes null arrays
    assert lib.dehalo_pairing_checks(None, g1.ctypes.data, 1, st.ctypes.data, None) == -1
    assert lib.dehalo_pairing_checks(t.handle, None, 1, st.ctypes.data, None) == -1
    assert lib.dehalo_pairing_checks(t.handle, g1.ctypes.data, 1, None, None) == -1
    assert lib.dehalo_pairing_checks(t.handle, g1.ctypes.data, (1 << 20) + 1, st.ctypes.data, None) == -1     # above DEHALO_PAIRING_MAX_CHECKS
    assert lib.dehalo_pairing_checks_device(None, t.handle, g1.ctypes.data, 1, st.ctypes.data, None, None) == -1
    assert lib.dehalo_pairing_checks(t.handle, g1.ctypes.data, 1, st.ctypes.data, None) == 0 and st[0] == 1   # the identity alone
    assert t.checks(np.zeros((0, 1, 8), dtype=np.uint64)).shape == (0,)
    assert lib.dehalo_pairing_checks_per_block(t.handle) >= 1 and lib.dehalo_pairing_checks_per_block(None) >= 1
    t.release()
    lib.dehalo_pairing_table_release(None)


def test_host_and_ipa_verifiers_refuse_the_device_mode(pkg, po, co):
    import verify_cases as VC
    import verify_ipa_cases as VI
    lib = pkg.load_library()
    v = VC.host_verifier(pkg, VC.case(pkg, po, co, "one"))
    with pytest.raises(pkg.DehaloError) as e:
        v.set_pairing("device")
    assert e.value.code == -1
    v.set_pairing("host")
    assert lib.dehalo_verifier_set_pairing(v.handle, 2) == -1 and lib.dehalo_verifier_set_pairing(None, 0) == -1
    with pytest.raises(ValueError):
        v.set_pairing("gpu")
    p = VC.proof(pkg, po, co, "one", "gwc")
    assert VC.verify(v, VC.case(pkg, po, co, "one"), p) == (True, 0)      # still the host's check
    v.release()
    vi = VI.host_verifier(pkg, VI.case(pkg, po, co, "one"))
    with pytest.raises(pkg.DehaloError) as e:
        vi.set_pairing("device")
    assert e.value.code == -1
    vi.release()
