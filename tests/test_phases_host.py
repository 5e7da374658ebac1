"""The constraint system on the host with the Challenge API (csrc/plonk_host.hpp): tests/native_host/host_cs_check.cpp -- g++, ASan + UBSan, a program of its
own -- checks what HostCS::load accepts and refuses, what degree / equality / fixed-only make of a challenge node, that a one-phase circuit encodes as before and
that the graph builders emit challenge sources.  No device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_constraint_system_with_phases_and_challenges():
    out = subprocess.run(["make", "-C", ROOT, "host_cs_check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    run = subprocess.run([os.path.join(ROOT, "tests", "native_host", "host_cs_check")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("17 checks passed"), run.stdout
