"""The CPU restatement proves over several circuits, over advice phases and with shuffle arguments what it proved when
tests/golden/oracle_variant_proof_digests.json was written (tools/pin_oracle_proofs.py variants, run on the code that still had one restatement per feature, in
tests/multi_oracle.py, tests/phased_oracle.py and tests/shuffle_oracle.py; it is not to be rewritten from the one that replaced them): per case the
proof byte for byte, the same commitments, evaluations and challenges (the phase challenges too); each proof is accepted by its verifier and rejected with the
tamper its family's tests use.  The proofs are the ones tests/test_multi_circuit.py, tests/test_phases.py and tests/test_shuffle.py make, made once per process."""
import pytest

import proof_chains as PC

KZG_CHAINS = ("maingate_k5", "maingate_range_k9", "R9all_k6", "Rlast_k6", "instance_k5")
MULTIOPENS = [("kzg", "gwc"), ("kzg", "shplonk"), ("ipa", "gwc")]
CASES = (["multi/%s/%d/%s" % (name, N, mo) for name in KZG_CHAINS for N in (1, 2, 3) for mo in ("gwc", "shplonk")]
         + ["phased/RLC3_k5/%s" % scheme for scheme in ("kzg", "ipa")]
         + ["shuffle/%s/%s/%s/1" % (name, scheme, mo) for name in ("SHUF1_k5", "SHUF2_k6", "SHUF5_k5", "SHUFRLC_k5") for scheme, mo in MULTIOPENS]
         + ["shuffle/SHUF2_k6/kzg/%s/2" % mo for mo in ("gwc", "shplonk")])
FIELDS = ["proof_sha256", "proof_len", "trace_sha256", "challenges"]


def run_case(pkg, po, co, case):
    """-> (proof, trace, accepts: proof -> bool, the tampered proof)"""
    family, name, *rest = case.split("/")
    if family == "multi":
        import test_multi_circuit as TM
        N, mo = int(rest[0]), rest[1]
        cs = TM.case_of(pkg, po, co, name)
        proof, trace = TM.reference(po, cs, N, mo)
        return proof, trace, lambda pr: TM.accepts(po, cs["chain"], pr, cs["insts"][:N], mo), TM.tampered_last_circuit_evaluation(cs["chain"]["key"]["shape"], N, proof)
    if family == "phased":
        import test_phases as TP
        c = TP.chain_of(pkg, po, co, rest[0], int(name[-1]))
        return c["want"], c["trace"], lambda pr: PC.accepts(po, c, pr, []), PC.tampered(c, c["want"])
    import shuffle_circuits as SO
    import test_shuffle as TS
    scheme, mo, circuits = rest[0], rest[1], int(rest[2])
    c = TS.chain_of(pkg, po, co, scheme, name[:-3])
    assert c["k"] == int(name[-1])
    proof, trace = TS.proof_of(pkg, po, co, scheme, mo, name[:-3], circuits)
    return proof, trace, lambda pr: SO.accepts(po, c, pr, circuits, mo), SO.tampered_product_evaluation(c, proof, circuits)


def digests(proof, trace):
    """proof_chains.digests' fields; for a key with challenge phases the phase challenges beside them"""
    out = PC.digests(proof, trace)
    if trace.get("phase_challenges"):
        out["phase_challenges"] = [hex(v) for v in trace["phase_challenges"]]
    return out


def test_the_golden_file_holds_exactly_these_cases(golden_loader):
    want = golden_loader("oracle_variant_proof_digests")
    assert sorted(want) == sorted(CASES) and len(set(CASES)) == len(CASES) == 30 + 2 + 12 + 2
    for case, v in want.items():
        phased = case.startswith("phased/") or "SHUFRLC" in case
        assert sorted(v) == sorted(FIELDS + (["phase_challenges"] if phased else [])), case
    marks = test_restatement_reproduces_the_pinned_variant.pytestmark
    assert [m.name for m in marks] == ["parametrize"] and list(marks[0].args[1]) == CASES


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_pinned_variant(pkg, po, co, golden_loader, case):
    want = golden_loader("oracle_variant_proof_digests")[case]
    proof, trace, accepts, tampered = run_case(pkg, po, co, case)
    got = digests(proof, trace)
    assert sorted(got) == sorted(want)
    for field in want:
        assert got[field] == want[field], field
    assert accepts(proof)
    assert tampered != proof and len(tampered) == len(proof) and not accepts(tampered)
