"""CPU suite: the one host home of G1 points (csrc/g1_host.hpp).  tests/native_host/g1_host_check.cpp (g++, ASan + UBSan, a program of its own) checks, on BN254,
Pallas and Vesta: compress / decompress round-trip [i]G for i = 1 .. 16 computed by G1Host, compress equals the 32 bytes dehalo_transcript::write_point appends
to a proof, the identity's encoding, the three refusals of the decoder and the texts of the status bits.  It is built and run once here."""
import os
import subprocess

from conftest import ROOT


def test_g1_host_check():
    out = subprocess.run(["make", "-C", ROOT, "g1_host_check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    r = subprocess.run([os.path.join(ROOT, "tests", "native_host", "g1_host_check")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "ok\n", r.stdout + r.stderr
