"""CPU suite: the BN254 pairing check on the host (csrc/pairing_host.hpp behind dehalo_pairing_check) against oracle/pairing.py::pairing_product_is_one.

The verdict "the product is one" is compared, never a GT value: the oracle keeps Fq12 as a degree-12 extension, the library as a 2-3-2 tower.  Cases: the
generators and their negations, bilinearity e(aG1, bG2) e(-abG1, G2) = 1 for three (a, b) with a = r - 1 among them and the same with ab + 1, identities on
either side, the empty product; what is refused: a G1 point off y^2 = x^3 + 3, a G2 point off the twist, a point of the twist outside the order-r subgroup
(found here, on the CPU), a stored word not below q, a Pasta curve.  tests/native_host/pairing_check.cpp (g++, ASan + UBSan, a program of its own) prints
pairing_host.hpp's verdicts for the same cases, once, and its derived constants, which are compared with Python's integers."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

AB = [(5, 7), (0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA0987654321FEDCBA0987654321FEDCBA09)]      # and (r - 1, 3), added where r is known


@pytest.fixture(scope="module")
def pr(oracles):
    import pairing
    return pairing


@pytest.fixture(scope="module")
def off_subgroup(pr):
    """a point of the twist that [r] does not send to the identity: the first x = (c, 1) with x^3 + b' a square, tweaked by the generator"""
    from verifier import sqrt
    q = pr.Q

    def f2_sqrt(a):      # Fq2 square root through the norm (q = 3 mod 4)
        a0, a1 = a
        if a1 == 0:
            s = sqrt(a0, q)
            return (s, 0) if s is not None else (0, sqrt(-a0 % q, q))
        n = sqrt((a0 * a0 + a1 * a1) % q, q)
        if n is None:
            return None
        for t in ((a0 + n) * pow(2, -1, q) % q, (a0 - n) * pow(2, -1, q) % q):
            x0 = sqrt(t, q)
            if x0:
                cand = (x0, a1 * pow(2 * x0, -1, q) % q)
                if pr.f2_mul(cand, cand) == (a0 % q, a1 % q):
                    return cand
        return None

    for c in range(1, 200):
        x = (c, 1)
        y = f2_sqrt(pr.f2_add(pr.f2_mul(pr.f2_mul(x, x), x), pr.B2))
        if y is None:
            continue
        P = (x, y)
        assert pr.g2_on_curve(P)
        rP = pr.g2_add(pr.g2_mul(pr.R - 1, P), P)      # [r] P (g2_mul reduces its scalar mod r: multiply by r - 1 and add)
        if rP is not None:
            T = pr.g2_add(P, pr.g2_mul(3, pr.G2))      # the generator times a cofactor-coprime tweak added: still on the twist, still outside the subgroup
            assert pr.g2_on_curve(T) and pr.g2_add(pr.g2_mul(pr.R - 1, T), T) is not None
            return T
    raise AssertionError("no point outside the subgroup found")


@pytest.fixture(scope="module")
def cases(po, pr):
    """name -> ([(P in G1 | None, Q in G2 | None)], the oracle's verdict)"""
    oc, r = po.BN254, pr.R
    G1, G2 = pr.G1, pr.G2
    mul1 = lambda k: po.ec_mul(oc, k % r, G1)
    out = {"gen and its negation": [(G1, G2), (po.ec_neg(oc, G1), G2)], "gen alone": [(G1, G2)], "empty": [],
           "identity in G1": [(None, G2)], "identity in G2": [(G1, None)], "identities beside a pair that cancels": [(G1, G2), (None, pr.g2_mul(9, G2)), (po.ec_neg(oc, G1), G2), (mul1(4), None)],
           "identity beside a pair that does not cancel": [(G1, G2), (None, G2)]}
    for a, b in AB + [(r - 1, 3)]:
        out["bilinear a=%x b=%x" % (a, b)] = [(mul1(a), pr.g2_mul(b, G2)), (po.ec_neg(oc, mul1(a * b)), G2)]
        out["bilinear + 1 a=%x b=%x" % (a, b)] = [(mul1(a), pr.g2_mul(b, G2)), (po.ec_neg(oc, mul1(a * b + 1)), G2)]
    return {name: (pairs, pr.pairing_product_is_one(pairs)) for name, pairs in out.items()}


def _raw(pr, pairs):
    return [(P, pr.g2_to_raw(Q)) for P, Q in pairs]


def test_oracle_verdicts_are_the_expected_ones(cases):
    """the checker itself: the identities of the pairing it is used to judge"""
    for name, (_, verdict) in cases.items():
        want = not (name == "gen alone" or name.startswith("bilinear + 1") or "does not cancel" in name)
        assert verdict is want, name


def test_pairing_check_matches_the_oracle(pkg, pr, cases):
    from dehalo2_amd import native
    for name, (pairs, verdict) in cases.items():
        assert native.pairing_check(pkg.fields.BN254, _raw(pr, pairs)) is verdict, name


def test_count_zero_takes_null_pointers(pkg):
    lib = pkg.load_library()
    one = C.c_int(-1)
    assert lib.dehalo_pairing_check(0, None, None, 0, C.byref(one)) == 0 and one.value == 1
    assert lib.dehalo_pairing_check(0, None, None, 1, C.byref(one)) == -1
    assert lib.dehalo_pairing_check(0, None, None, 0, None) == -1


def test_points_off_curve_or_subgroup_are_invalid(pkg, po, pr, off_subgroup):
    from dehalo2_amd import native
    curve, q = pkg.fields.BN254, pr.Q
    g2 = pr.g2_to_raw(pr.G2)
    ok = [(pr.G1, g2), (po.ec_neg(po.BN254, pr.G1), g2)]
    assert native.pairing_check(curve, ok) is True
    bad_g2 = bytearray(g2)
    bad_g2[64] ^= 1                                                   # y.c0: off the twist
    word_q = g2[:96] + q.to_bytes(32, "little")                        # a stored word equal to q
    for pairs in ([((1, 3), g2)] + ok,                                 # (1, 3) is not on y^2 = x^3 + 3
                  ok + [(pr.G1, bytes(bad_g2))], ok + [(pr.G1, word_q)], ok + [(pr.G1, pr.g2_to_raw(off_subgroup))],
                  ok + [(None, pr.g2_to_raw(off_subgroup))]):          # refused even where the identity beside it makes the factor 1
        with pytest.raises(pkg.DehaloError) as e:
            native.pairing_check(curve, pairs)
        assert e.value.code == -1


def test_g1_words_stand_for_their_residues(pkg, pr):
    """a coordinate word not below q is read mod q (dehalo.h, non-canonical words (1)): x + q where it fits in 256 bits"""
    lib = pkg.load_library()
    f = pkg.fields.BN254.base
    g1 = np.zeros((2, 8), dtype=np.uint64)
    for i, P in enumerate([pr.G1, (pr.G1[0], -pr.G1[1] % pr.Q)]):
        g1[i, :4], g1[i, 4:] = f.encode(P[0]), f.encode(P[1])
    w = sum(int(v) << (64 * j) for j, v in enumerate(g1[0, :4])) + pr.Q
    assert w < 1 << 256
    g1[0, :4] = np.frombuffer(w.to_bytes(32, "little"), dtype=np.uint64)
    g2 = np.frombuffer(pr.g2_to_raw(pr.G2) * 2, dtype=np.uint8)
    one = C.c_int(-1)
    assert lib.dehalo_pairing_check(0, g1.ctypes.data, g2.ctypes.data, 2, C.byref(one)) == 0 and one.value == 1


@pytest.mark.parametrize("name", ["PALLAS", "VESTA"])
def test_pasta_is_unsupported(pkg, pr, name):
    from dehalo2_amd import native
    with pytest.raises(pkg.DehaloError) as e:
        native.pairing_check(getattr(pkg.fields, name), [(None, bytes(128))])
    assert e.value.code == -5
    one = C.c_int(-1)
    assert pkg.load_library().dehalo_pairing_check(3, None, None, 0, C.byref(one)) == -1      # no such curve


# ------------------------------------------------------------------------------------------------------------------------------ pairing_host.hpp alone, sanitized
@pytest.fixture(scope="module")
def check():
    out = subprocess.run(["make", "-C", ROOT, "pairing_check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr

    def run(lines):
        r = subprocess.run([os.path.join(ROOT, "tests", "native_host", "pairing_check")], input="".join(s + "\n" for s in lines), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        got = [json.loads(s) for s in r.stdout.splitlines()]
        assert len(got) == len(lines)
        return got
    return run


def _line(pkg, pr, pairs, curve=0):
    f = pkg.fields.BN254.base
    g1 = b"".join(bytes(64) if P is None else f.encode(P[0]).tobytes() + f.encode(P[1]).tobytes() for P, _ in pairs)
    g2 = b"".join(pr.g2_to_raw(Q) if not isinstance(Q, (bytes, bytearray)) else bytes(Q) for _, Q in pairs)
    return "check %d %d %s %s" % (curve, len(pairs), g1.hex() or "-", g2.hex() or "-")


def test_sanitized_program_prints_the_same_verdicts(pkg, pr, cases, check, off_subgroup):
    names = sorted(cases)
    got = check([_line(pkg, pr, cases[n][0]) for n in names])
    for n, g in zip(names, got):
        assert g == {"rc": 0, "is_one": int(cases[n][1])}, n
    bad_g2 = bytearray(pr.g2_to_raw(pr.G2))
    bad_g2[64] ^= 1
    refused = check([_line(pkg, pr, [((1, 3), pr.G2)]), _line(pkg, pr, [(pr.G1, bad_g2)]), _line(pkg, pr, [(pr.G1, off_subgroup)]), _line(pkg, pr, [(pr.G1, pr.G2)], curve=1)])
    assert [g["rc"] for g in refused] == [-1, -1, -1, -5]


def test_derived_constants_are_the_integers_they_claim(pr, check):
    """nothing typed in: (q^4 - q^2 + 1) / r and xi^((q - 1) / 6), computed by the program at first use, against Python's integers"""
    c = check(["constants"])[0]
    assert c["ok"] is True
    q, r = pr.Q, pr.R
    assert sum(int(w, 16) << (64 * i) for i, w in enumerate(c["hard"].split())) == (q ** 4 - q ** 2 + 1) // r and (q ** 4 - q ** 2 + 1) % r == 0
    f = bytes.fromhex(c["frob1"])
    rinv = pow(1 << 256, -1, q)
    got = tuple(int.from_bytes(f[i:i + 32], "little") * rinv % q for i in (0, 32))
    want, base, e = (1, 0), (9, 1), (q - 1) // 6
    while e:
        if e & 1:
            want = pr.f2_mul(want, base)
        base, e = pr.f2_mul(base, base), e >> 1
    assert got == want and (q - 1) % 6 == 0
