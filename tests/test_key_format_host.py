"""CPU suite: VerifyingKey / ProvingKey in the three SerdeFormats on the host -- the Python mirror (keygen.HostProvingKey, VerifyingKey.write / read with a
format) and csrc/key_format.hpp, the C++ parser of the same bytes, set against each other.

A key made by hand at k = 2 (two fixed columns, one of them all zero with the identity for its commitment; one permutation column; one selector) is laid out
in Processed as a conversion of its RawBytes written out here: every Montgomery word w as (w R^-1 mod p) little-endian, every commitment compressed by the
documented rule.  The three formats round-trip over BN254 and Vesta; the checked formats refuse what the unchecked one takes.
tests/native_host/key_format_check.cpp (g++, ASan + UBSan, a program of its own) prints key_format.hpp's layouts, header verdicts and count / length word
verdicts, once; they are compared with the mirror's.  The header declares the eight new entry points; without a device each is an error, not a crash."""
import ctypes as C
import io
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_params_ipa_io import _points

NEW_SYMBOLS = ["dehalo_scalars_from_repr_device", "dehalo_scalars_check_device", "dehalo_vk_size_custom", "dehalo_vk_write_custom", "dehalo_pk_size_custom",
               "dehalo_pk_write_custom", "dehalo_pk_read_custom", "dehalo_keygen_pk"]
FORMATS = {"processed": 0, "raw": 1, "raw-unchecked": 2}
K, NF, NPC, NSEL, EXT = 2, 2, 1, 1, 1      # the hand-made key: degree 3 -> the extended domain has 2^(k + 1) rows


def hand_cs(pkg):
    from dehalo2_amd import plonk
    cs = plonk.ConstraintSystem(num_advice=1, num_fixed=NF)
    cs.enable_equality(plonk.ADVICE, 0)
    assert cs.degree() == 3 and len(cs.permutation_columns) == NPC
    return cs


def hand_key(pkg, curve, seed=5):
    """-> (cs, HostProvingKey): fixed column 1 is all zero and its commitment the identity; the other two commitments have an odd and an even y; the elements
    are random but for 0, 1 and p - 1 in known places"""
    from dehalo2_amd import keygen
    f, cs = curve.scalar, hand_cs(pkg)
    n, m = 1 << K, 1 << (K + EXT)
    pts = _points(pkg, curve, 6, 2000)
    odd, even = next(P for P in pts if P[1] & 1), next(P for P in pts if not P[1] & 1)
    vk = keygen.VerifyingKey(curve, K, cs, keygen.encode_points(curve, [odd, None]), keygen.encode_points(curve, [even]), [np.array([1, 0, 1, 1], dtype=bool)])
    rng = np.random.default_rng(seed)
    col = lambda cnt, ln: np.stack([f.encode_many([int.from_bytes(rng.bytes(32), "little") % f.p for _ in range(ln)]) for _ in range(cnt)]).reshape(cnt, ln, 4)
    l, fv, fp, fc, pv, pp, pc = col(3, m), col(NF, n), col(NF, n), col(NF, m), col(NPC, n), col(NPC, n), col(NPC, m)
    for a in (fv, fp, fc):
        a[1] = 0
    l[0, 0], l[0, 1], l[0, 2] = f.encode(0), f.encode(1), f.encode(f.p - 1)
    return cs, keygen.HostProvingKey(vk, l, fv, fp, fc, pv, pp, pc)


def layout_of(pkg, fmt):
    from dehalo2_amd import keygen
    return keygen.key_layout(fmt, K, NF, NPC, NSEL, EXT)


def elem_off(L, section, poly, index):
    off, cnt, ln, sl = L["polys"][section]
    assert poly < cnt and index < ln
    return off + (4 if sl else 0) + poly * (4 + 32 * ln) + 4 + 32 * index


def put(data, off, new):
    return data[:off] + new + data[off + len(new):]


# ------------------------------------------------------------------------------------------------------------------------------ the mirror
def test_processed_layout_written_out_by_hand(pkg):
    from dehalo2_amd import keygen
    curve = pkg.fields.BN254
    f, q = curve.scalar, curve.base.p
    cs, key = hand_key(pkg, curve)
    raw, proc = key.to_bytes("raw"), key.to_bytes("processed")
    assert raw == key.to_bytes("raw-unchecked")
    assert len(raw) == keygen.pk_size(cs, K, NSEL, f) and len(proc) == len(raw) - 32 * (NF + NPC)
    vk_raw, vk_proc = io.BytesIO(), io.BytesIO()
    key.vk.write(vk_raw, "raw")
    key.vk.write(vk_proc, "processed")
    assert len(vk_raw.getvalue()) == keygen.vk_size(cs, K, NSEL) and len(vk_proc.getvalue()) == keygen.vk_size(cs, K, NSEL) - 32 * (NF + NPC)
    assert raw.startswith(vk_raw.getvalue()) and proc.startswith(vk_proc.getvalue())
    # by hand, from the RawBytes: the header, the commitments compressed, the selectors, then every word out of Montgomery form
    rinv_q, rinv_p = pow(1 << 256, -1, q), pow(1 << 256, -1, f.p)
    want = raw[:8]
    for i in range(NF + NPC):
        x, y = (int.from_bytes(raw[8 + 64 * i + 32 * j:8 + 64 * i + 32 * j + 32], "little") for j in (0, 1))
        if x == 0 and y == 0:
            want += bytes(32)                                     # the identity: all zero
        else:
            e = bytearray((x * rinv_q % q).to_bytes(32, "little"))      # x canonical ...
            e[31] |= ((y * rinv_q % q) & 1) << 7                  # ... bit 255 = y is odd
            want += bytes(e)
    o = 8 + 64 * (NF + NPC)
    want += raw[o:o + 1]                                          # one selector of 4 bits
    o += 1
    n, m = 1 << K, 1 << (K + EXT)

    def poly(ln):
        nonlocal o, want
        assert struct.unpack(">I", raw[o:o + 4]) == (ln,)
        want += raw[o:o + 4]
        for j in range(ln):
            w = int.from_bytes(raw[o + 4 + 32 * j:o + 36 + 32 * j], "little")
            want += (w * rinv_p % f.p).to_bytes(32, "little")
        o += 4 + 32 * ln

    for _ in range(3):
        poly(m)
    for cnt, ln in ((NF, n), (NF, n), (NF, m), (NPC, n), (NPC, n), (NPC, m)):
        assert struct.unpack(">I", raw[o:o + 4]) == (cnt,)
        want += raw[o:o + 4]
        o += 4
        for _ in range(cnt):
            poly(ln)
    assert o == len(raw) and proc == want
    assert want[8 + 32:8 + 64] == bytes(32) and want[8 + 31] >> 7 == 1 and want[8 + 95] >> 7 == 0      # the identity, an odd y, an even y
    L = layout_of(pkg, "processed")
    assert [int.from_bytes(proc[elem_off(L, "l0", 0, j):elem_off(L, "l0", 0, j) + 32], "little") for j in range(3)] == [0, 1, f.p - 1]
    assert L["pk_size"] == len(proc) and L["vk_size"] == len(vk_proc.getvalue()) and layout_of(pkg, "raw")["pk_size"] == len(raw)


@pytest.mark.parametrize("cname", ["bn254", "vesta"])
@pytest.mark.parametrize("fmt", ["processed", "raw", "raw-unchecked"])
def test_mirror_round_trips(pkg, cname, fmt):
    from dehalo2_amd import keygen
    curve = pkg.fields.CURVES[cname]
    cs, key = hand_key(pkg, curve)
    data = key.to_bytes(fmt)
    back = keygen.HostProvingKey.from_bytes(curve, cs, data, NSEL, fmt)
    assert back.to_bytes(fmt) == data and back.to_bytes("raw") == key.to_bytes("raw")
    assert np.array_equal(back.vk.fixed_commitments, key.vk.fixed_commitments) and not back.vk.fixed_commitments[1].any()
    assert back.vk.transcript_repr == key.vk.transcript_repr
    vk = keygen.VerifyingKey.read(curve, cs, io.BytesIO(data), NSEL, fmt)
    assert np.array_equal(vk.permutation_commitments, key.vk.permutation_commitments) and np.array_equal(vk.selectors[0], key.vk.selectors[0])
    with pytest.raises(ValueError):
        key.to_bytes("compressed")
    with pytest.raises(ValueError):
        keygen.HostProvingKey.from_bytes(curve, cs, data, NSEL, "compressed")


def tamperings(pkg, curve, key, fmt):
    """name -> (bytes, the words the refusal must hold, accepted by the checked read?) over the key's bytes in `fmt` ("processed" or "raw")"""
    from dehalo2_amd import keygen
    f, q = curve.scalar, curve.base.p
    data, L = key.to_bytes(fmt), layout_of(pkg, fmt)
    out = {}
    le = lambda v: v.to_bytes(32, "little")
    kind = "an element is not below the modulus" if fmt == "processed" else "an element's stored word is not below the modulus"
    out["element = p"] = (put(data, elem_off(L, "fixed_polys", 1, 2), le(f.p)), [kind, "fixed_polys", "element %d" % ((1 << K) + 2)], False)
    out["element = p - 1"] = (put(data, elem_off(L, "permutation cosets", 0, 3), le(f.p - 1)), [], True)
    two = put(put(data, elem_off(L, "fixed_cosets", 1, 5), le(f.p + 1)), elem_off(L, "fixed_cosets", 0, 7), le((1 << 256) - 1))
    out["two bad elements in two polynomials of one slice"] = (two, [kind, "fixed_cosets", "element 7"], False)
    out["l_last"] = (put(data, elem_off(L, "l_last", 0, 1), le(f.p)), [kind, "l_last", "element 1"], False)
    if fmt == "raw":
        o = L["off_fixed_c"] + 32
        y1 = (int.from_bytes(data[o:o + 32], "little") + 1) % q
        out["(x, y + 1)"] = (put(data, o, le(y1)), ["neither on the curve", "fixed commitments"], False)
        out["coordinate word = q"] = (put(data, L["off_perm_c"], le(q)), ["stored word is not below the modulus", "permutation commitments"], False)
    else:
        x = next(x for x in range(1, 200) if pow((x ** 3 + curve.b) % q, (q - 1) // 2, q) == q - 1)
        out["x without a square root"] = (put(data, L["off_perm_c"], le(x)), ["not on the curve", "permutation commitments"], False)
        out["x = 0 with the sign bit"] = (put(data, L["off_fixed_c"] + 32, bytes(31) + b"\x80"), ["x = 0 with the sign bit", "fixed commitments"], False)
        out["x = q"] = (put(data, L["off_fixed_c"], le(q)), ["x coordinate is not below the modulus", "fixed commitments"], False)
    out["truncated"] = (data[:-1], ["length"], False)
    out["trailing byte"] = (data + b"\0", ["length"], False)
    out["wrong k"] = (struct.pack(">I", K + 1) + data[4:], ["length"], False)      # (a read has no k to compare with: the length no longer fits)
    out["wrong fixed-column count"] = (data[:4] + struct.pack(">I", NF + 1) + data[8:], ["fixed"], False)
    o = L["polys"]["fixed_polys"][0]
    out["polynomial count"] = (put(data, o, struct.pack(">I", NF - 1)), ["polynomial count", "fixed_polys"], False)
    out["polynomial length"] = (put(data, o + 4, struct.pack(">I", 3)), ["polynomial length", "fixed_polys"], False)
    return out


@pytest.mark.parametrize("cname", ["bn254", "vesta"])
@pytest.mark.parametrize("fmt", ["processed", "raw"])
def test_checked_formats_refuse_what_the_unchecked_takes(pkg, cname, fmt):
    from dehalo2_amd import keygen
    curve = pkg.fields.CURVES[cname]
    cs, key = hand_key(pkg, curve)
    for name, (bad, words, ok) in tamperings(pkg, curve, key, fmt).items():
        if ok:
            got = keygen.HostProvingKey.from_bytes(curve, cs, bad, NSEL, fmt)
            assert got.to_bytes(fmt) == bad, name
            continue
        with pytest.raises(ValueError) as e:
            keygen.HostProvingKey.from_bytes(curve, cs, bad, NSEL, fmt)
        # (the mirror reads a stream: what the C parser calls a length that does not fit is, here, a stream that ends early or goes on, or -- k + 1 in the
        # header -- the first length word, which no longer is the domain's)
        own = {"truncated": "unexpected end of file", "trailing byte": "length does not match the circuit", "wrong k": "polynomial length differs from the domain's: l0",
               "wrong fixed-column count": "fixed commitments, the circuit has"}
        assert (own[name] in str(e.value)) if name in own else all(w in str(e.value) for w in words), (name, str(e.value))
        if fmt == "raw" and len(bad) == len(key.to_bytes("raw")) and name not in ("wrong k", "wrong fixed-column count", "polynomial count", "polynomial length"):
            took = keygen.HostProvingKey.from_bytes(curve, cs, bad, NSEL, "raw-unchecked")      # the same bytes, unseen
            assert took.to_bytes("raw-unchecked") == bad, name


# ------------------------------------------------------------------------------------------------------------------------------ key_format.hpp
@pytest.fixture(scope="module")
def check():
    """lines of commands -> the JSON lines the C++ program answers with (one build, under ASan + UBSan)"""
    out = subprocess.run(["make", "-C", ROOT, "key_format_check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr

    def run(lines):
        r = subprocess.run([os.path.join(ROOT, "tests", "native_host", "key_format_check")], input="".join(s + "\n" for s in lines), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        got = [json.loads(s) for s in r.stdout.splitlines()]
        assert len(got) == len(lines)
        return got
    return run


SHAPES = [(NF, NPC, NSEL, EXT), (0, 0, 0, 1), (7, 6, 3, 2), (1, 0, 0, 0), (0, 5, 11, 3)]


def test_cpp_layouts_against_the_mirror(pkg, check):
    from dehalo2_amd import keygen
    cases = [(f, k, sh) for f in (0, 1, 2) for k in (0, 2, 9, 17, 28) for sh in SHAPES]
    names = {v: n for n, v in FORMATS.items()}
    for (f, k, sh), got in zip(cases, check(["layout %d %d %d %d %d %d" % ((f, k) + sh) for f, k, sh in cases])):
        want = keygen.key_layout(names[f], k, *sh)
        assert got.pop("ok") is True
        assert {n: tuple(v) for n, v in got.pop("polys").items()} == want["polys"], (f, k, sh)
        assert got == {n: v for n, v in want.items() if n != "polys"}, (f, k, sh)
    # the hand-made key's bytes have these sizes, and Processed is 32 bytes per commitment shorter
    cs, key = hand_key(pkg, pkg.fields.BN254)
    proc, raw = check(["layout 0 %d %d %d %d %d" % (K, NF, NPC, NSEL, EXT), "layout 1 %d %d %d %d %d" % (K, NF, NPC, NSEL, EXT)])
    assert proc["pk_size"] == len(key.to_bytes("processed")) == raw["pk_size"] - 32 * (NF + NPC) and raw["pk_size"] == len(key.to_bytes("raw"))
    assert proc["vk_size"] == raw["vk_size"] - 32 * (NF + NPC) == 8 + 32 * (NF + NPC) + 1
    assert check(["layout 0 29 1 1 1 1", "layout 3 2 1 1 1 1", "layout -1 2 1 1 1 1", "layout 1 28 1 1 1 5", "layout 1 2 1 1 1 40"]) == [{"ok": False}] * 5


def test_cpp_header_verdicts_against_the_mirror(pkg, check):
    from dehalo2_amd import keygen
    names = {0: "processed", 1: "raw", 2: "raw-unchecked", 3: "compressed"}
    lines, want = [], []
    for f in (0, 1, 2):
        for pk in (0, 1):
            for k, sh in ((2, SHAPES[0]), (9, SHAPES[2]), (0, SHAPES[1])):
                L = keygen.key_layout(names[f], k, *sh)
                size = L["pk_size"] if pk else L["vk_size"]
                for kf, nff, ln, wk in ((k, sh[0], size, -1), (k, sh[0], size, k), (k, sh[0], size - 1, -1), (k, sh[0], size + 1, -1), (k + 1, sh[0], size, -1),
                                        (k, sh[0], size, k + 1), (k, sh[0] + 1, size, -1), (29, sh[0], size, -1), (4294967295, sh[0], size, -1), (k, sh[0], 7, -1),
                                        (k, sh[0], 0, -1)):
                    lines.append("header %d %d %d %d %d %d %d %d %d %d" % ((f, kf, nff, ln) + sh + (pk, wk)))
                    want.append(keygen.key_header_error(struct.pack(">II", kf, nff)[:min(ln, 8)], names[f], *sh, pk=bool(pk), want_k=None if wk < 0 else wk, length=ln))
    lines += ["header 3 2 2 100 2 1 1 1 1 -1", "header 0 2 2 %d 2 1 1 1 1 -1" % keygen.key_layout("raw", 2, *SHAPES[0])["pk_size"]]      # a raw key read as Processed
    want += ["unknown format", "length does not match the circuit (unexpected end of input or trailing bytes)"]
    got = check(lines)
    for line, g, w in zip(lines, got, want):
        assert g["text"] == w, line
        assert bool(g["text"]) == bool(g["error"]), line
    assert len({g["error"] for g in got}) == 7      # OK and six kinds of refusal
    # (a vk without commitments has 8 bytes at every k, and one selector takes one byte at k = 2 and k = 3: those two pass with k + 1 in the header)
    assert sum(1 for g in got if g["error"] == 0) == 2 * 3 * 2 * 3 + 3 * 2


def test_cpp_poly_words_and_texts_against_the_mirror(pkg, check):
    from dehalo2_amd import keygen
    curve = pkg.fields.BN254
    cs, key = hand_key(pkg, curve)
    shape = "%d %d %d %d %d" % (K, NF, NPC, NSEL, EXT)
    n, m = 1 << K, 1 << (K + EXT)
    # section numbers as key_format.hpp counts them: 2 = l0 ... 10 = permutation cosets
    cases = [(2, 0, m, ""), (3, 0, m - 1, "polynomial length"), (5, -1, NF, ""), (5, -1, NF + 1, "polynomial count"), (6, 1, n + 1, "polynomial length"),
             (7, 1, n, "polynomial length"), (10, -1, 0, "polynomial count"), (10, 0, m, "")]
    got = check(["words 1 %s %d %d %d" % (shape, s, p, v) for s, p, v, _ in cases])
    raw, L = key.to_bytes("raw"), layout_of(pkg, "raw")
    for (s, p, v, kind), g in zip(cases, got):
        name = keygen.KEY_SECTION_NAMES[s]
        assert g["ok"] and (g["text"].startswith(kind) and g["section"] == name if kind else g["error"] == 0), (s, p, v, g)
        off, cnt, ln, sl = L["polys"][name]
        bad = put(raw, off if p < 0 else off + (4 if sl else 0) + p * (4 + 32 * ln), struct.pack(">I", v))
        if kind:
            with pytest.raises(ValueError) as e:
                keygen.HostProvingKey.from_bytes(curve, cs, bad, NSEL, "raw")
            assert kind in str(e.value) and name in str(e.value)
        else:
            assert bad == raw
    t = check(["texts"])[0]
    assert tuple(t["sections"]) == keygen.KEY_SECTION_NAMES
    with pytest.raises(ValueError) as e:
        keygen.scalars_from_repr(curve.scalar, bytes(32 * 7) + curve.scalar.p.to_bytes(32, "little"), "fixed_polys")
    assert str(e.value) == t["element_processed"]
    with pytest.raises(ValueError) as e:
        keygen.scalars_check(curve.scalar, np.frombuffer(curve.scalar.p.to_bytes(32, "little"), dtype=np.uint64), "permutation cosets")
    assert str(e.value) == t["element_raw"].replace("12345678901", "0")


# ------------------------------------------------------------------------------------------------------------------------------ the C ABI without a device
def test_header_declares_the_new_entry_points(pkg):
    txt = open(os.path.join(ROOT, "include", "dehalo.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(lib, s), s
    from dehalo2_amd import native
    assert native.SERDE_FORMATS == FORMATS
    for name in ("keygen_pk", "read", "write", "vk_bytes"):
        assert "format" in getattr(native.ProvingKey, name).__code__.co_varnames, name


def test_no_device_means_error_not_fallback(pkg):
    lib = pkg.load_library()
    h = C.c_void_p()
    st, fb = C.c_uint32(7), C.c_uint64(7)
    buf = (C.c_uint64 * 16)()
    raw = (C.c_uint8 * 4096)()
    assert lib.dehalo_scalars_from_repr_device(None, 0, raw, 1, buf, C.byref(st), C.byref(fb), None) == -1
    assert lib.dehalo_scalars_check_device(None, 0, buf, 1, C.byref(st), C.byref(fb), None) == -1
    assert lib.dehalo_scalars_from_repr_device(None, 0, None, 0, None, None, None, None) == -1
    for fmt in (0, 1, 2, 3):
        assert lib.dehalo_vk_size_custom(None, fmt) == 0 and lib.dehalo_pk_size_custom(None, fmt) == 0
        assert lib.dehalo_vk_write_custom(None, None, fmt, raw, 4096) == -1
        assert lib.dehalo_pk_write_custom(None, None, fmt, raw, 4096) == -1
        assert lib.dehalo_pk_read_custom(None, 0, None, raw, 4096, fmt, 0, C.byref(h)) == -1 and not h.value
        assert lib.dehalo_pk_read_custom(None, 0, None, None, 0, fmt, 0, None) == -1
        assert lib.dehalo_keygen_pk(None, None, None, raw, 4096, fmt, 0, buf, buf, 0, C.byref(h)) == -1 and not h.value
        assert lib.dehalo_keygen_pk(None, None, None, None, 0, fmt, 0, None, None, 0, None) == -1
