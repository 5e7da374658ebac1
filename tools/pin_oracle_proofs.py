#!/usr/bin/env python3
"""Writes tests/golden/oracle_proof_digests.json: what the CPU restatements (oracle/) prove for the ten cases of tests/proof_chains.py PINNED -- per case
the sha256 and length of the proof, the sha256 of the trace's commitments and evaluations, and the challenges.  CPU only (the C oracle must be built).
tests/test_oracle_proofs_pinned.py recomputes every case and compares; rerun this only when the restatements are meant to prove something else.
usage: python tools/pin_oracle_proofs.py [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as entry      # noqa: E402


def main():
    pkg = entry.load_package()
    po, co = entry.load_oracle()
    import proof_chains as PC
    out = {}
    for scheme, name in PC.PINNED:
        c, instances = PC.pinned_case(pkg, po, co, scheme, name)
        proof, trace = PC.prove(po, c, instances)
        assert PC.accepts(po, c, proof, instances), (scheme, name)
        out["%s/%s" % (scheme, name)] = PC.digests(proof, trace)
        print(scheme, name, len(proof), out["%s/%s" % (scheme, name)]["proof_sha256"], flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "oracle_proof_digests.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
