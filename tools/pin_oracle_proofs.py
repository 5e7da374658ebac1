#!/usr/bin/env python3
"""Writes tests/golden/oracle_proof_digests.json: what the CPU restatements (oracle/) prove for the ten cases of tests/proof_chains.py PINNED -- per case
the sha256 and length of the proof, the sha256 of the trace's commitments and evaluations, and the challenges.  CPU only (the C oracle must be built).
tests/test_oracle_proofs_pinned.py recomputes every case and compares; rerun this only when the restatements are meant to prove something else.
With `variants`: writes tests/golden/oracle_variant_proof_digests.json, the same record (and the phase challenges) for the cases of
tests/test_oracle_variants_pinned.py: proofs over several circuits, over advice phases and with shuffle arguments.  The committed file was written while each
of the three had a restatement of its own under tests/; it is what ties the one body in oracle/plonk_oracle.py to them, so it is not to be rewritten from that body.
usage: python tools/pin_oracle_proofs.py [variants] [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as entry      # noqa: E402


def write(out, path):
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


def variants(pkg, po, co, args):
    import test_oracle_variants_pinned as TV
    out = {}
    for case in TV.CASES:
        proof, trace, accepts, tampered = TV.run_case(pkg, po, co, case)
        assert accepts(proof) and not accepts(tampered), case
        out[case] = TV.digests(proof, trace)
        print(case, len(proof), out[case]["proof_sha256"], flush=True)
    write(out, args[0] if args else os.path.join(ROOT, "tests", "golden", "oracle_variant_proof_digests.json"))


def main():
    pkg = entry.load_package()
    po, co = entry.load_oracle()
    import proof_chains as PC
    if sys.argv[1:2] == ["variants"]:
        return variants(pkg, po, co, sys.argv[2:])
    out = {}
    for scheme, name in PC.PINNED:
        c, instances = PC.pinned_case(pkg, po, co, scheme, name)
        proof, trace = PC.prove(po, c, instances)
        assert PC.accepts(po, c, proof, instances), (scheme, name)
        out["%s/%s" % (scheme, name)] = PC.digests(proof, trace)
        print(scheme, name, len(proof), out["%s/%s" % (scheme, name)]["proof_sha256"], flush=True)
    write(out, sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "oracle_proof_digests.json"))


if __name__ == "__main__":
    main()
