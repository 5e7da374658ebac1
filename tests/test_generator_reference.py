"""CPU: the judge of the generated points (tests/generator_reference.py) against the rule it restates (include/dehalo.h, "Generated points"), the coverage
the GPU tests of tests/test_params_ipa_generate.py rely on, and the two entry points without a device.

Every point the judge names is on its curve with the encoded parity, and every attempt before it fails for one of the rule's three reasons; the package's
Python mirror of ParamsIPA::read decodes the accepted 32 bytes to the same point; under the default key, indices 0..299 of stream 0 hold on every curve an
index accepted at once, one that needs at least 16 attempts, and 300 distinct x; dehalo_points_generate_device and dehalo_params_ipa_generate exist and
refuse a null context.  The exhausted-attempts path (256 rejections in a row) is not covered: no key that reaches it is known."""
import ctypes as C
import os
import re
import struct

import pytest

import generator_reference as G
from conftest import ROOT

NEW_SYMBOLS = ["dehalo_points_generate_device", "dehalo_params_ipa_generate"]
CURVE_NAMES = ["bn254", "pallas", "vesta"]
_CACHE = {}


def tries_0_299(curve):
    """the attempts of indices 0..299 of stream 0 under the default key, computed once per curve"""
    if curve not in _CACHE:
        _CACHE[curve] = [G.attempts(curve, None, 0, i) for i in range(300)]
    return _CACHE[curve]


def test_default_key_is_the_headers():
    assert len(G.DEFAULT_KEY) == 32 and G.DEFAULT_KEY[:30] == b"dehalo ParamsIPA generators v1" and G.DEFAULT_KEY[30:] == b"\0\0"
    txt = open(os.path.join(ROOT, "include", "dehalo.h")).read()
    m = re.search(r'#define\s+DEHALO_GENERATORS_DEFAULT_KEY\s+"([^"]*)"', txt)
    assert m and m.group(1) == "dehalo ParamsIPA generators v1\\0"      # 30 characters, a written NUL and the literal's own: 32 bytes
    assert re.search(r"#define\s+DEHALO_GENERATORS_MAX_ATTEMPTS\s+256\b", txt) and G.MAX_ATTEMPTS == 256


def test_judges_square_root():
    for name in CURVE_NAMES:
        p = G.CURVES[name]["p"]
        assert G.sqrt_mod(0, p) == 0
        residues = 0
        for a in range(1, 40):
            r = G.sqrt_mod(a, p)
            assert (r is None) == (pow(a, (p - 1) // 2, p) == p - 1)
            if r is not None:
                assert r * r % p == a
                residues += 1
        assert 5 < residues < 35


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_points_are_on_the_curve_and_rejections_have_a_reason(curve):
    c = G.CURVES[curve]
    p, b = c["p"], c["b"]
    reasons = set()
    for index, tries in enumerate(tries_0_299(curve)):
        for attempt, (enc, verdict, x, s, y) in enumerate(tries):
            assert enc == G.candidate(G.DEFAULT_KEY, 0, index, attempt) and len(enc) == 32
            v = int.from_bytes(enc, "little")
            assert x == v % (1 << 255) and s == v >> 255
            if attempt + 1 < len(tries):      # a rejection: exactly one of the three reasons, checked here without the judge's square root
                assert y is None
                rhs = (x * x * x + b) % p
                why = [x == 0, x >= p, 0 < x < p and (rhs == 0 or pow(rhs, (p - 1) // 2, p) == p - 1)]
                assert sum(why) == 1 and verdict == [G.X_ZERO, G.X_NOT_BELOW_P, G.NOT_A_NONZERO_SQUARE][why.index(True)], (index, attempt)
                reasons.add(verdict)
            else:
                assert verdict == G.ACCEPTED and 0 < x < p and 0 < y < p
                assert (y * y - x * x * x - b) % p == 0 and y & 1 == s
        assert G.point(curve, None, 0, index) == (tries[-1][2], tries[-1][4], len(tries) - 1)
    assert reasons == {G.X_NOT_BELOW_P, G.NOT_A_NONZERO_SQUARE}      # (x = 0 has probability 2^-255)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_coverage_the_gpu_tests_rely_on(curve):
    tries = tries_0_299(curve)
    last = [len(t) - 1 for t in tries]
    assert min(last) == 0, "an index accepted at attempt 0"
    assert max(last) >= 16, "an index needing at least 16 attempts"
    assert len({t[-1][2] for t in tries}) == 300, "300 distinct x"
    assert sum(1 for a in last[:50] if a >= 8) >= 2, "several indices below 50 need 8 or more attempts"


def test_judge_rejects_what_the_rule_rejects():
    for name in CURVE_NAMES:
        p = G.CURVES[name]["p"]
        assert G.judge(name, bytes(32))[0] == G.X_ZERO
        assert G.judge(name, (1 << 255).to_bytes(32, "little"))[0] == G.X_ZERO                    # x = 0 with the sign bit set
        assert G.judge(name, p.to_bytes(32, "little"))[0] == G.X_NOT_BELOW_P
        assert G.judge(name, ((1 << 255) - 1).to_bytes(32, "little"))[0] == G.X_NOT_BELOW_P
        x, y, _ = G.point(name, None, 1, 0)
        for s in (0, 1):      # both parities of one x: the two roots
            verdict, x2, s2, y2 = G.judge(name, (x | (s << 255)).to_bytes(32, "little"))
            assert verdict == G.ACCEPTED and x2 == x and s2 == s and y2 & 1 == s and y2 in (y, p - y)


def test_streams_keys_and_high_indices_differ():
    base = G.point("vesta", None, 0, 0)
    assert G.point("vesta", None, 1, 0) != base and G.point("vesta", bytes(range(32)), 0, 0) != base
    assert G.point("vesta", None, 0, 1 << 32) != base and G.point("vesta", None, 0, 1 << 47) != base      # the index reaches w13
    assert G.candidate(G.DEFAULT_KEY, 0, (1 << 32) + 5, 3) != G.candidate(G.DEFAULT_KEY, 0, 5, 3)
    g, w, u = G.params_ipa("vesta", None, 2)
    assert g == [G.point("vesta", None, 0, i)[:2] for i in range(4)] and w == G.point("vesta", None, 1, 0)[:2] and u == G.point("vesta", None, 1, 1)[:2]


@pytest.mark.parametrize("curve", ["pallas", "vesta"])
def test_params_ipa_read_mirror_decodes_the_accepted_bytes(pkg, curve):
    """keygen.params_ipa_from_bytes over a k = 5 file whose g | g_lagrange sections are the accepted candidates of indices 0..63 (w, u: 64, 65)"""
    from dehalo2_amd import keygen
    cs = {"pallas": pkg.fields.PALLAS, "vesta": pkg.fields.VESTA}[curve]
    assert cs.id == G.CURVES[curve]["id"] and cs.base.p == G.CURVES[curve]["p"]
    tries = [G.attempts(curve, None, 0, i) for i in range(66)]
    data = struct.pack("<I", 5) + b"".join(t[-1][0] for t in tries)
    k, g, gl, w, u = keygen.params_ipa_from_bytes(cs, data)
    got = keygen.decode_points(cs, g) + keygen.decode_points(cs, gl) + keygen.decode_points(cs, w) + keygen.decode_points(cs, u)
    assert k == 5 and got == [(t[-1][2], t[-1][4]) for t in tries]
    # and a rejected candidate is not an encoding of a point for the mirror either
    rejected = next(t[0][0] for t in tries if len(t) > 1 and t[0][1] == G.NOT_A_NONZERO_SQUARE)
    with pytest.raises(ValueError):
        keygen.params_ipa_from_bytes(cs, data[:4] + rejected + data[36:])


def test_header_declares_the_new_entry_points(pkg):
    txt = open(os.path.join(ROOT, "include", "dehalo.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(lib, s), s


def test_no_context_is_an_error(pkg):
    from dehalo2_amd import native
    lib = pkg.load_library()
    h = C.c_void_p()
    buf = (C.c_uint64 * 16)()
    key = (C.c_uint8 * 32)()
    for curve in (0, 1, 2):
        assert lib.dehalo_points_generate_device(None, curve, None, 0, 0, buf, 2, None) == -1
        assert lib.dehalo_points_generate_device(None, curve, key, 1, 0, buf, 0, None) == -1
        assert lib.dehalo_params_ipa_generate(None, curve, 1, None, C.byref(h)) == -1 and not h.value
        assert lib.dehalo_params_ipa_generate(None, curve, 1, key, C.byref(h)) == -1 and not h.value
    # upstream's ParamsIPA::new is still not provided
    with pytest.raises(NotImplementedError):
        native.ParamsIPA.setup(None, None, 5)
    assert hasattr(native.ParamsIPA, "generate")
