"""CPU suite: ParamsKZG's three on-disk formats on the host -- the Python mirror (keygen.params_bytes / params_from_bytes, g2_compress / g2_decompress) and
csrc/params_format.hpp, the C++ parser of the same bytes, set against each other.

The mirror round-trips in the three formats (an identity point and both parities of y among the points) and lays Processed out, at k = 1, as a compression written
out here by hand; the G2 codec round-trips the generator, [s] generator and the identity, and the generator satisfies y^2 = x^3 + 3 / (9 + i).
tests/native_host/params_format_check.cpp (g++, ASan + UBSan, a program of its own) prints params_format.hpp's layouts, header verdicts and G2 codec, once; they
are compared with the sizes stated here and with the mirror's bytes.  The header declares the eight new entry points; without a device each is an error,
not a crash."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_params_ipa_io import _points

NEW_SYMBOLS = ["dehalo_points_compress_device", "dehalo_points_decompress_device", "dehalo_points_check_device", "dehalo_params_size_custom",
               "dehalo_params_write_custom", "dehalo_params_read_custom", "dehalo_params_from_g", "dehalo_params_downsize"]
FORMATS = {"processed": 0, "raw": 1, "raw-unchecked": 2}
S = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF                # the scalar of [s] generator


def _g2_points(pkg):
    """the generator, [S] generator, the identity: ((x.c0, x.c1), (y.c0, y.c1)) canonical or None"""
    from dehalo2_amd import keygen
    F2 = keygen.Fq2Arith(pkg.fields.BN254.base.p)
    G = keygen.BN254_G2_GENERATOR
    return F2, [G, F2.point_mul(S, G), None]


# ------------------------------------------------------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("fmt", ["processed", "raw", "raw-unchecked"])
def test_mirror_round_trips(pkg, fmt):
    from dehalo2_amd import keygen
    curve, k = pkg.fields.BN254, 3
    pts = _points(pkg, curve, 16, 1000)
    pts[2] = None                                                # an identity point
    assert any(P is not None and P[1] & 1 for P in pts) and any(P is not None and not P[1] & 1 for P in pts)
    enc = keygen.encode_points(curve, pts)
    _, g2s = _g2_points(pkg)
    g2, s_g2 = keygen.g2_to_raw(curve, g2s[0]), keygen.g2_to_raw(curve, g2s[1])
    data = keygen.params_bytes(curve, k, enc[:8], enc[8:], g2, s_g2, fmt)
    assert len(data) == keygen.params_size(k, fmt) == (4 + 64 * 8 + 128 if fmt == "processed" else 4 + 128 * 8 + 256)
    k2, g, gl, a, b = keygen.params_from_bytes(curve, data, fmt)
    assert k2 == k and np.array_equal(g, enc[:8]) and np.array_equal(gl, enc[8:]) and a == g2 and b == s_g2
    assert keygen.params_bytes(curve, k2, g, gl, a, b, fmt) == data
    if fmt != "processed":      # both raw formats are the bytes the library has always written
        assert data == struct.pack("<I", k) + enc.tobytes() + g2 + s_g2
    for bad in (data[:-1], data + b"\0", struct.pack("<I", 29) + data[4:]):
        with pytest.raises(ValueError):
            keygen.params_from_bytes(curve, bad, fmt)


def test_mirror_checked_raw_refuses_what_unchecked_takes(pkg):
    from dehalo2_amd import keygen
    curve, k = pkg.fields.BN254, 1
    p = curve.base.p
    P = _points(pkg, curve, 4, 3000)
    _, g2s = _g2_points(pkg)
    g2 = keygen.g2_to_raw(curve, g2s[0])
    off = list(P)
    off[1] = (P[1][0], (P[1][1] + 1) % p)                        # (x, y + 1)
    enc = keygen.encode_points(curve, off)
    data = keygen.params_bytes(curve, k, enc[:2], enc[2:], g2, g2, "raw")
    with pytest.raises(ValueError):
        keygen.params_from_bytes(curve, data, "raw")
    assert keygen.params_bytes(curve, *keygen.params_from_bytes(curve, data, "raw-unchecked"), "raw-unchecked") == data
    good = keygen.params_bytes(curve, k, *np.split(keygen.encode_points(curve, P), 2), g2, g2, "raw")
    keygen.params_from_bytes(curve, good, "raw")
    word_p = good[:4] + p.to_bytes(32, "little") + good[36:]    # g[0].x's stored word = p
    with pytest.raises(ValueError):
        keygen.params_from_bytes(curve, word_p, "raw")
    bad_g2 = bytearray(good)
    bad_g2[-64] ^= 1                                              # s_g2's y.c0: off the twist
    with pytest.raises(ValueError):
        keygen.params_from_bytes(curve, bytes(bad_g2), "raw")


def test_processed_layout_at_k1_by_hand(pkg):
    from dehalo2_amd import keygen
    curve = pkg.fields.BN254
    P = _points(pkg, curve, 4, 2000)
    P[1] = None
    _, g2s = _g2_points(pkg)

    def comp(Q):      # G1 GroupEncoding::to_bytes by hand
        if Q is None:
            return bytes(32)
        b = bytearray(Q[0].to_bytes(32, "little"))
        b[31] |= (Q[1] & 1) << 7
        return bytes(b)

    def comp2(Q):     # G2: x.c0 | x.c1, the parity of y.c0 in the top bit of the last byte
        if Q is None:
            return bytes(64)
        b = bytearray(Q[0][0].to_bytes(32, "little") + Q[0][1].to_bytes(32, "little"))
        b[63] |= (Q[1][0] & 1) << 7
        return bytes(b)

    enc = keygen.encode_points(curve, P)
    want = struct.pack("<I", 1) + comp(P[0]) + comp(P[1]) + comp(P[2]) + comp(P[3]) + comp2(g2s[0]) + comp2(g2s[1])      # k | g[0] g[1] | gl[0] gl[1] | g2 | s_g2
    got = keygen.params_bytes(curve, 1, enc[0:2], enc[2:4], keygen.g2_to_raw(curve, g2s[0]), keygen.g2_to_raw(curve, g2s[1]), "processed")
    assert got == want and len(want) == 4 + 64 * 2 + 128 and want[:4] == b"\x01\x00\x00\x00"


def test_g2_codec_and_curve(pkg):
    from dehalo2_amd import keygen
    curve = pkg.fields.BN254
    q = curve.base.p
    assert pow(3, (q - 1) // 2, q) != 1                          # x^3 + 3 at x = 0 is a non-residue: G1's "x = 0 + sign" rule stands for BN254
    F2, pts = _g2_points(pkg)
    assert F2.mul(F2.b, (9, 1)) == (3, 0)                        # b' = 3 / (9 + i)
    G = pts[0]
    assert F2.mul(G[1], G[1]) == F2.add(F2.mul(F2.mul(G[0], G[0]), G[0]), F2.b)      # the generator is on y^2 = x^3 + 3 / (9 + i)
    assert pts[1] is not None and F2.on_curve(pts[1]) and pts[1] != G
    for P in pts:
        enc = keygen.g2_compress(curve, P)
        assert len(enc) == 64 and keygen.g2_decompress(curve, enc) == P
        assert keygen.g2_from_raw(curve, keygen.g2_to_raw(curve, P)) == P
        if P is not None:                                         # the other parity decodes to the negative
            flipped = enc[:63] + bytes([enc[63] ^ 0x80])
            assert keygen.g2_decompress(curve, flipped) == (P[0], ((-P[1][0]) % q, (-P[1][1]) % q))
    assert keygen.g2_compress(curve, None) == bytes(64)
    for bad in (q.to_bytes(32, "little") + bytes(32), bytes(32) + q.to_bytes(32, "little"), bytes(63) + b"\x80"):
        with pytest.raises(ValueError):
            keygen.g2_decompress(curve, bad)
    # a square root for a1 = 0 comes from sqrt(a0) or i sqrt(-a0)
    for a0 in (4, q - 4, 3, q - 3):
        r = F2.sqrt((a0, 0))
        assert r is not None and F2.mul(r, r) == (a0, 0)


# ------------------------------------------------------------------------------------------------------------------------------ params_format.hpp
@pytest.fixture(scope="module")
def check():
    """lines of commands -> the JSON lines the C++ program answers with (one build, under ASan + UBSan)"""
    out = subprocess.run(["make", "-C", ROOT, "params_format_check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr

    def run(lines):
        r = subprocess.run([os.path.join(ROOT, "tests", "native_host", "params_format_check")], input="".join(s + "\n" for s in lines), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        got = [json.loads(s) for s in r.stdout.splitlines()]
        assert len(got) == len(lines)
        return got
    return run


def test_cpp_layouts(check):
    cases = [(f, k) for f in (0, 1, 2) for k in (0, 1, 28)]
    for (f, k), L in zip(cases, check(["layout %d %d" % c for c in cases])):
        n, g1 = 1 << k, 32 if f == 0 else 64
        assert L == {"ok": True, "n": n, "g1": g1, "g2": 2 * g1, "off_g": 4, "off_gl": 4 + g1 * n, "off_g2": 4 + 2 * g1 * n, "off_sg2": 4 + 2 * g1 * n + 2 * g1,
                     "size": 4 + 2 * g1 * n + 4 * g1}, (f, k)
    assert check(["layout 0 0"])[0]["size"] == 4 + 64 + 128 and check(["layout 2 1"])[0]["size"] == 4 + 256 + 256
    assert check(["layout 0 29", "layout 1 29", "layout 2 4294967295", "layout 3 1", "layout -1 1"]) == [{"ok": False}] * 5


def test_cpp_header_refusals(check):
    OK, FORMAT, SHORT, K, LENGTH = 0, 1, 2, 3, 4
    lines, want = [], []
    for f in (0, 1, 2):
        for k in (0, 1, 28):
            size = 4 + (64 if f == 0 else 128) * (1 << k) + (128 if f == 0 else 256)
            lines += ["header %d %d %d" % (f, k, size), "header %d %d %d" % (f, k, size - 1), "header %d %d %d" % (f, k, size + 1)]
            want += [OK, LENGTH, LENGTH]
        lines += ["header %d 29 %d" % (f, 1 << 20), "header %d 4294967295 %d" % (f, 1 << 20), "header %d 1 3" % f, "header %d 1 0" % f]
        want += [K, K, SHORT, SHORT]
    lines += ["header 3 1 260", "header 0 1 %d" % (4 + 128 * 2 + 256), "header 1 1 %d" % (4 + 64 * 2 + 128)]      # a raw file read as Processed and the reverse
    want += [FORMAT, LENGTH, LENGTH]
    got = check(lines)
    assert [g["error"] for g in got] == want
    assert all(bool(g["text"]) == bool(g["error"]) for g in got)


def test_cpp_g2_codec_against_the_mirror(pkg, check):
    from dehalo2_amd import keygen
    curve = pkg.fields.BN254
    q = curve.base.p
    F2, pts = _g2_points(pkg)
    gen, mul = check(["gen", "mul " + S.to_bytes(32, "little").hex()])
    assert gen["on_curve"] is True                               # BN254_G2_GEN satisfies the curve equation
    assert bytes.fromhex(gen["raw"]) == keygen.g2_to_raw(curve, pts[0])
    assert bytes.fromhex(gen["b"]) == b"".join((c * (1 << 256) % q).to_bytes(32, "little") for c in F2.b)      # the twist constant, computed on both sides
    assert bytes.fromhex(mul["raw"]) == keygen.g2_to_raw(curve, pts[1])
    for P, got in zip(pts, check(["g2 " + keygen.g2_to_raw(curve, P).hex() for P in pts])):
        assert got["check"] == 0 and got["status"] == 0
        assert bytes.fromhex(got["compressed"]) == keygen.g2_compress(curve, P)
        assert bytes.fromhex(got["raw"]) == keygen.g2_to_raw(curve, P)
    # the other parity, and what is not an encoding: 1 = x not below q, 2 = not on the twist, 4 = x = 0 with the sign bit set
    enc = keygen.g2_compress(curve, pts[1])
    flipped = enc[:63] + bytes([enc[63] ^ 0x80])
    off = next(x for x in range(1, 100) if F2.sqrt(F2.add(F2.mul(F2.mul((x, 0), (x, 0)), (x, 0)), F2.b)) is None)
    cases = [(flipped, 0), (q.to_bytes(32, "little") + bytes(32), 1), (bytes(32) + q.to_bytes(32, "little"), 1), (off.to_bytes(32, "little") + bytes(32), 2),
             (bytes(63) + b"\x80", 4)]
    for (data, status), got in zip(cases, check(["dec " + d.hex() for d, _ in cases])):
        assert got["status"] == status
        if status == 0:
            assert bytes.fromhex(got["raw"]) == keygen.g2_to_raw(curve, keygen.g2_decompress(curve, data))
        else:
            with pytest.raises(ValueError):
                keygen.g2_decompress(curve, data)
    # the checked raw form: a stored word equal to q is 1, a point off the twist is 2
    raw = bytearray(keygen.g2_to_raw(curve, pts[0]))
    word_q = bytes(raw[:96]) + q.to_bytes(32, "little")
    raw[64] ^= 1
    got = check(["g2 " + word_q.hex(), "g2 " + bytes(raw).hex()])
    assert [g["check"] for g in got] == [1, 2]


# ------------------------------------------------------------------------------------------------------------------------------ the C ABI without a device
def test_header_declares_the_new_entry_points(pkg):
    txt = open(os.path.join(ROOT, "include", "dehalo.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(lib, s), s
    for name, value in (("DEHALO_SERDE_PROCESSED", 0), ("DEHALO_SERDE_RAW_BYTES", 1), ("DEHALO_SERDE_RAW_BYTES_UNCHECKED", 2)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), txt), name
    assert re.search(r"#define\s+DEHALO_KEEP_K\s+0xffffffffu", txt)
    from dehalo2_amd import native
    assert native.SERDE_FORMATS == FORMATS and native.KEEP_K == 0xFFFFFFFF


def test_no_device_means_error_not_fallback(pkg):
    lib = pkg.load_library()
    h = C.c_void_p()
    st = C.c_uint32(7)
    buf = (C.c_uint64 * 16)()
    raw = (C.c_uint8 * 516)()
    raw[0] = 1
    assert lib.dehalo_points_compress_device(None, 0, buf, 1, raw, None) == -1
    assert lib.dehalo_points_decompress_device(None, 0, raw, 1, buf, C.byref(st), None) == -1
    assert lib.dehalo_points_check_device(None, 0, buf, 1, C.byref(st), None) == -1
    assert lib.dehalo_params_size_custom(None, 0) == 0
    assert lib.dehalo_params_write_custom(None, 0, raw, 516) == -1
    for fmt, size in ((0, 260), (1, 516), (2, 516)):
        assert lib.dehalo_params_read_custom(None, 0, raw, size, fmt, 0xFFFFFFFF, C.byref(h)) == -1 and not h.value
        assert lib.dehalo_params_read_custom(None, 0, raw, size, fmt, 0, C.byref(h)) == -1 and not h.value
    assert lib.dehalo_params_from_g(None, 0, 1, buf, raw, raw, C.byref(h)) == -1 and not h.value
    assert lib.dehalo_params_downsize(None, None, 0, C.byref(h)) == -1 and not h.value
