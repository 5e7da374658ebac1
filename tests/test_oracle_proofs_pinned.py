"""The CPU restatements prove today what they proved when tests/golden/oracle_proof_digests.json was written (tools/pin_oracle_proofs.py): ten proofs,
the five circuits of tests/proof_chains.py PINNED under KZG / GWC over BN254 and under IPA over Vesta, byte for byte, with the same commitments,
evaluations and challenges; each is accepted by its scheme's restated verifier and rejected with one bit of its second evaluation flipped.
And ReadTranscript.read_point, which takes square roots by Tonelli-Shanks for every curve, reads BN254 points as the (p + 1) / 4 formula does."""
import pytest

import proof_chains as PC

FIELDS = ["proof_sha256", "proof_len", "trace_sha256", "challenges"]


def test_the_golden_file_holds_exactly_the_ten_cases(golden_loader):
    want = golden_loader("oracle_proof_digests")
    assert sorted(want) == sorted(scheme + "/" + name for scheme in ("kzg", "ipa") for name in ("maingate_k5", "maingate_range_k9", "R9all_k6", "Rlast_k6", "instance_k5"))
    assert sorted(want) == sorted("%s/%s" % case for case in PC.PINNED) and len(want) == 10
    assert all(sorted(v) == sorted(FIELDS) for v in want.values())
    # ... and the test below runs every one of them, unconditionally
    marks = test_restatement_reproduces_the_pinned_proof.pytestmark
    assert [m.name for m in marks] == ["parametrize"] and list(marks[0].args[1]) == PC.PINNED


@pytest.fixture(scope="module")
def kzg_k5_proof(pkg, po, co):
    c, instances = PC.pinned_case(pkg, po, co, "kzg", "maingate_k5")
    return c, PC.prove(po, c, instances)[0]


@pytest.mark.parametrize("scheme,name", PC.PINNED)
def test_restatement_reproduces_the_pinned_proof(pkg, po, co, golden_loader, scheme, name):
    want = golden_loader("oracle_proof_digests")["%s/%s" % (scheme, name)]
    c, instances = PC.pinned_case(pkg, po, co, scheme, name)
    proof, trace = PC.prove(po, c, instances)
    got = PC.digests(proof, trace)
    for field in FIELDS:
        assert got[field] == want[field], field
    assert PC.accepts(po, c, proof, instances)
    assert not PC.accepts(po, c, PC.tampered(c, proof), instances)


def test_read_point_on_bn254_is_the_p_plus_1_over_4_formula(po, kzg_k5_proof):
    import verifier as V
    c, proof = kzg_k5_proof
    curve = po.BN254
    p = curve.base.p
    assert p % 4 == 3
    sh = c["key"]["shape"]
    num_evals = len(sh.advice_queries) + len(sh.fixed_queries) + 1 + len(sh.perm_columns) + (3 * sh.num_sets - 1) + 5 * len(sh.lookups)
    points = sh.num_advice + 3 * len(sh.lookups) + sh.num_sets + 1 + (sh.degree - 1)
    offsets = [32 * i for i in range(points)] + list(range(32 * (points + num_evals), len(proof), 32))      # the commitments, then GWC's witnesses
    assert len(offsets) > points
    for off in offsets:
        b = proof[off:off + 32]
        x, sign = int.from_bytes(b, "little") & ((1 << 255) - 1), b[31] >> 7
        y = pow((x * x * x + curve.b) % p, (p + 1) // 4, p)
        assert y * y % p == (x * x * x + curve.b) % p
        y = y if (y & 1) == sign else p - y
        assert V.ReadTranscript(curve, b).read_point() == (x, y)
    enc = lambda x, sign=0: (x | sign << 255).to_bytes(32, "little")
    off_curve = next(x for x in range(1, 50) if pow((x * x * x + curve.b) % p, (p - 1) // 2, p) == p - 1)
    for bad in [enc(p), enc(p + 1, 1), bytes(32), enc(off_curve), enc(off_curve, 1)]:      # x >= p (twice), the all-zero encoding, an x off the curve (twice)
        with pytest.raises(ValueError):
            V.ReadTranscript(curve, bad).read_point()
    assert V.ReadTranscript(curve, enc(1)).read_point() == (1, 2)      # (the generator: the reader does read what is on the curve)
