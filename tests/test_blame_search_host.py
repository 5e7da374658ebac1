"""The search behind dehalo_verify_proofs_each (csrc/blame_search.hpp: host only, no HIP header): tests/native_host/blame_search_check.cpp -- g++, ASan + UBSan, a
program of its own -- runs it over every bad set of n = 0 .. 12 members (and every single bad member, and all bad, of 64) against the additive predicate the search
assumes, and checks the set it names, the checks it counts and the bound 1 / 1 + 2 b ceil(log2 n) on them.  No device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blame_search_names_every_bad_set_within_the_bound():
    out = subprocess.run(["make", "-C", ROOT, "blame_search_check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    run = subprocess.run([os.path.join(ROOT, "tests", "native_host", "blame_search_check")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "%d cases passed" % (sum(1 << n for n in range(13)) + 65), run.stdout
    assert "n = 12: at most 9 checks for one bad member, 23 for any bad set" in lines
