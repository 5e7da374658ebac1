"""ParamsKZG, VerifyingKey, ProvingKey and keygen: the objects the reference builds once and caches on disk
before timing `create_proof` (benches/delay_enc.rs:41-54 params, :84-115 vk / pk), device-resident, with
upstream's on-disk formats.

  ParamsKZG::{write, read}      [UPSTREAM halo2_proofs/src/poly/kzg/commitment.rs, SerdeFormat::RawBytes]
      k: u32 LE | g[0..n) | g_lagrange[0..n) | g2 | s_g2 ; a G1 point = x, y as 4 x u64 LE Montgomery limbs (64 B),
      a G2 point = x.c0, x.c1, y.c0, y.c1 (128 B).
  ParamsKZG::{write_custom, read_custom}   [the same file in the three SerdeFormats: params_bytes / params_from_bytes, g2_compress / g2_decompress]
  ParamsIPA::{write, read}      [UPSTREAM halo2_proofs/src/poly/ipa/commitment.rs]
      k: u32 LE | g[0..n) | g_lagrange[0..n) | w | u ; a point = its 32-byte GroupEncoding (params_ipa_bytes / params_ipa_from_bytes).
  VerifyingKey::{write, read}   [UPSTREAM halo2_proofs/src/plonk.rs]
      k: u32 BE | #fixed commitments: u32 BE | commitments (64 B raw each) | permutation commitments |
      selectors packed 8 bools per byte (LSB first), ceil(n / 8) bytes per selector.
  ProvingKey::{write, read}     [UPSTREAM halo2_proofs/src/plonk.rs]
      vk | l0 | l_last | l_active_row (extended polynomials) | fixed_values | fixed_polys | fixed_cosets |
      permutation values | polys | cosets ; a polynomial = len: u32 BE | elements (32 B raw Montgomery);
      a slice of polynomials = count: u32 BE | polynomials.
  Both take a format (SERDE_FORMATS): the layouts above are "raw" / "raw-unchecked"; "processed" writes a commitment as its 32-byte
  GroupEncoding and an element as its canonical integer, and the two checked formats validate what they read (HostProvingKey).
Reading a key needs the circuit's ConstraintSystem, as upstream's `read::<_, ConcreteCircuit>` does.

keygen_vk / keygen_pk [UPSTREAM halo2_proofs/src/plonk/keygen.rs] run on the device: commit_lagrange of every fixed
and permutation column, lagrange_to_coeff and coeff_to_extended of each, l0 / l_last / l_active_row.
Device arrays are torch tensors (plumbing only): int64 views of n x 4 u64 limbs.
"""
from __future__ import annotations

import hashlib
import io
import struct
from typing import List, Optional, Sequence

import numpy as np

from . import evaluation as ev
from . import plonk
from ._lib import Bases, Context
from .domain import EvaluationDomain
from .fields import CurveSpec, FieldSpec


# ---- bulk conversions --------------------------------------------------------------------------------
def ints_to_array(vals: Sequence[int]) -> np.ndarray:
    """canonical ints -> (len, 4) u64 little-endian limbs (NOT Montgomery)."""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def array_to_ints(arr) -> List[int]:
    b = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def to_device(arr):
    """host array of 64-bit words -> int64 tensor in HBM, through the library's staged upload (never `tensor.cuda()` of a pageable array: _lib.Context.upload)"""
    from ._lib import transfer_context

    with transfer_context() as c:
        return c.upload(np.ascontiguousarray(arr, dtype=np.uint64))


def to_host(t) -> np.ndarray:
    import torch
    from ._lib import transfer_context

    torch.cuda.current_stream().synchronize()      # what `t.cpu()` would have waited for
    with transfer_context() as c:
        return c.download_tensor(t.contiguous())


_RINV: dict = {}


def _rinv(p: int) -> int:
    if p not in _RINV:
        _RINV[p] = pow(1 << 256, -1, p)
    return _RINV[p]


def decode_points(curve: CurveSpec, xy) -> list:
    """(count, 8) u64 Montgomery affine -> [(x, y) | None] canonical."""
    out = []
    f = curve.base
    rinv = _rinv(f.p)
    vals = array_to_ints(np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 4))
    for i in range(0, len(vals), 2):
        x, y = vals[i], vals[i + 1]
        out.append(None if x == 0 and y == 0 else (x * rinv % f.p, y * rinv % f.p))
    return out


def encode_points(curve: CurveSpec, pts) -> np.ndarray:
    f = curve.base
    R = (1 << 256) % f.p
    flat = []
    for P in pts:
        flat += [0, 0] if P is None else [P[0] * R % f.p, P[1] * R % f.p]
    return ints_to_array(flat).reshape(-1, 8)


# ---- ParamsKZG -----------------------------------------------------------------------------------------
class ParamsKZG:
    """ParamsKZG<Bn256> (or its Pasta-curve analogue for the MSM/NTT configs): g, g_lagrange resident on the device."""

    def __init__(self, ctx: Context, curve: CurveSpec, k: int, g, g_lagrange, g2: bytes = b"", s_g2: bytes = b"", window_bits: int = 0):
        self.ctx, self.curve, self.k, self.n = ctx, curve, k, 1 << k
        self.g = np.ascontiguousarray(g, dtype=np.uint64).reshape(-1, 8)
        self.g_lagrange = np.ascontiguousarray(g_lagrange, dtype=np.uint64).reshape(-1, 8)
        if self.g.shape[0] != self.n or self.g_lagrange.shape[0] != self.n:
            raise ValueError("g and g_lagrange must hold 2^k points")
        self.g2, self.s_g2 = bytes(g2), bytes(s_g2)
        self.bases_g: Bases = ctx.register_bases(curve.id, self.g, window_bits, True)
        self.bases_g_lagrange: Bases = ctx.register_bases(curve.id, self.g_lagrange, window_bits, True)

    def release(self):
        self.bases_g.release()
        self.bases_g_lagrange.release()

    # commit / commit_lagrange on device-resident columns: `batch` polynomials of `length` <= n coefficients, n apart
    def commit_device(self, d_polys: int, batch: int, d_out: int, lagrange: bool, length: Optional[int] = None, ctx: Optional[Context] = None):
        (ctx or self.ctx).msm_device(self.bases_g_lagrange if lagrange else self.bases_g, d_polys, self.n if length is None else length, batch, d_out, 0)

    def commit_affine_device(self, d_polys: int, batch: int, d_out_affine: int, lagrange: bool, length: Optional[int] = None, ctx: Optional[Context] = None):
        """commit(..).to_affine() of `batch` columns in one call: the points the transcript absorbs."""
        (ctx or self.ctx).msm_device_affine(self.bases_g_lagrange if lagrange else self.bases_g, d_polys, self.n if length is None else length, batch, 0,
                                            d_out_affine, 0)

    def write(self, fh):
        fh.write(struct.pack("<I", self.k))
        fh.write(self.g.tobytes())
        fh.write(self.g_lagrange.tobytes())
        fh.write(self.g2.ljust(128, b"\0"))
        fh.write(self.s_g2.ljust(128, b"\0"))

    @classmethod
    def read(cls, ctx: Context, curve: CurveSpec, fh, window_bits: int = 0) -> "ParamsKZG":
        (k,) = struct.unpack("<I", _exact(fh, 4))
        if k > 28:
            raise ValueError("params: k out of range")
        n = 1 << k
        g = np.frombuffer(_exact(fh, 64 * n), dtype=np.uint64).reshape(n, 8)
        gl = np.frombuffer(_exact(fh, 64 * n), dtype=np.uint64).reshape(n, 8)
        g2, s_g2 = _exact(fh, 128), _exact(fh, 128)
        return cls(ctx, curve, k, g, gl, g2, s_g2, window_bits)


# ---- ParamsKZG::{write_custom, read_custom}: the host mirror of csrc/params_format.hpp ---------------------------------
# [UPSTREAM halo2_proofs/src/poly/kzg/commitment.rs, halo2curves 0.3.x SerdeFormat; restated from memory like the formats above]
#   k: u32 LE | g | g_lagrange | g2 | s_g2.  "processed": compressed points (G1 32 B: transcript.compress; G2 64 B: g2_compress); "raw" and "raw-unchecked":
#   Montgomery limbs (G1 64 B, G2 128 B), the first validated when read.
SERDE_FORMATS = ("processed", "raw", "raw-unchecked")
# the generator of BN254's G2 (halo2curves bn256::G2Affine::generator()): ((x.c0, x.c1), (y.c0, y.c1)), canonical
BN254_G2_GENERATOR = ((0x1800DEEF121F1E76426A00665E5C4479674322D4F75EDADD46DEBD5CD992F6ED, 0x198E9393920D483A7260BFB731FB5D25F1AA493335A9E71297E485B7AEF312C2),
                      (0x12C85EA5DB8C6DEB4AAB71808DCB408FE3D1E7690C43D37B4CE6CC0166FA7DAA, 0x090689D0585FF075EC9E99AD690C3395BC4B313370B38EF355ACDADCD122975B))


class Fq2Arith:
    """Fq2 = Fq[i] / (i^2 + 1) over pairs of Python integers (q = 3 mod 4), and the twist y^2 = x^3 + 3 / (9 + i) that BN254's G2 lives on"""

    def __init__(self, q: int):
        assert q % 4 == 3
        self.q = q
        self.b = self.mul((3, 0), self.inv((9, 1)))

    def add(self, x, y):
        return ((x[0] + y[0]) % self.q, (x[1] + y[1]) % self.q)

    def sub(self, x, y):
        return ((x[0] - y[0]) % self.q, (x[1] - y[1]) % self.q)

    def mul(self, x, y):
        return ((x[0] * y[0] - x[1] * y[1]) % self.q, (x[0] * y[1] + x[1] * y[0]) % self.q)

    def inv(self, x):
        d = pow(x[0] * x[0] + x[1] * x[1], -1, self.q)
        return (x[0] * d % self.q, -x[1] * d % self.q)

    def _sqrt_fq(self, a):
        r = pow(a, (self.q + 1) // 4, self.q)
        return r if r * r % self.q == a % self.q else None

    def sqrt(self, a):
        """a square root of a, or None: for a1 = 0, sqrt(a0) or i sqrt(-a0); otherwise through the norm"""
        q = self.q
        if a[1] == 0:
            s = self._sqrt_fq(a[0])
            if s is not None:
                return (s, 0)
            s = self._sqrt_fq(-a[0] % q)
            return None if s is None else (0, s)
        n = self._sqrt_fq((a[0] * a[0] + a[1] * a[1]) % q)
        if n is None:
            return None
        half = pow(2, -1, q)
        x0 = self._sqrt_fq((a[0] + n) * half % q)
        if x0 is None:
            x0 = self._sqrt_fq((a[0] - n) * half % q)
        if x0 is None or x0 == 0:
            return None
        r = (x0, a[1] * pow(2 * x0, -1, q) % q)
        return r if self.mul(r, r) == (a[0] % q, a[1] % q) else None

    def on_curve(self, P) -> bool:
        return P is None or self.mul(P[1], P[1]) == self.add(self.mul(self.mul(P[0], P[0]), P[0]), self.b)

    def point_add(self, P, Q):
        if P is None:
            return Q
        if Q is None:
            return P
        if P[0] == Q[0]:
            if self.add(P[1], Q[1]) == (0, 0):
                return None
            xx = self.mul(P[0], P[0])
            lam = self.mul(self.add(self.add(xx, xx), xx), self.inv(self.add(P[1], P[1])))
        else:
            lam = self.mul(self.sub(Q[1], P[1]), self.inv(self.sub(Q[0], P[0])))
        x = self.sub(self.sub(self.mul(lam, lam), P[0]), Q[0])
        return (x, self.sub(self.mul(lam, self.sub(P[0], x)), P[1]))

    def point_mul(self, s: int, P):
        acc = None
        while s:
            if s & 1:
                acc = self.point_add(acc, P)
            P = self.point_add(P, P)
            s >>= 1
        return acc


def g2_compress(curve: CurveSpec, P) -> bytes:
    """G2 GroupEncoding::to_bytes: P = ((x.c0, x.c1), (y.c0, y.c1)) canonical or None -> x.c0 | x.c1 little-endian, bit 7 of byte 63 = y.c0 is odd; None: 64 zero bytes"""
    if P is None:
        return bytes(64)
    b = bytearray(P[0][0].to_bytes(32, "little") + P[0][1].to_bytes(32, "little"))
    b[63] |= (P[1][0] & 1) << 7
    return bytes(b)


def g2_decompress(curve: CurveSpec, data: bytes):
    """G2 GroupEncoding::from_bytes; ValueError for an encoding that is not a point of the twist"""
    if len(data) != 64:
        raise ValueError("compressed G2 point must be 64 bytes")
    q = curve.base.p
    sign = data[63] >> 7
    x = (int.from_bytes(data[:32], "little"), int.from_bytes(data[32:63] + bytes([data[63] & 0x7F]), "little"))
    if x[0] >= q or x[1] >= q:
        raise ValueError("x coordinate is not canonical")
    if x == (0, 0):
        if sign:
            raise ValueError("x = 0 with the sign bit set")
        return None
    F2 = Fq2Arith(q)
    y = F2.sqrt(F2.add(F2.mul(F2.mul(x, x), x), F2.b))
    if y is None:
        raise ValueError("not on the curve")
    if (y[0] & 1) != sign:
        y = ((-y[0]) % q, (-y[1]) % q)
    return (x, y)


def g2_to_raw(curve: CurveSpec, P) -> bytes:
    """G2Affine RawBytes: x.c0 | x.c1 | y.c0 | y.c1 as Montgomery limbs (128 B); None: all zero"""
    if P is None:
        return bytes(128)
    R, q = 1 << 256, curve.base.p
    return b"".join((c * R % q).to_bytes(32, "little") for c in (P[0][0], P[0][1], P[1][0], P[1][1]))


def g2_from_raw(curve: CurveSpec, raw: bytes, checked: bool = True):
    """the inverse of g2_to_raw; checked: ValueError for a stored word not below q or a point off the twist"""
    if len(raw) != 128:
        raise ValueError("raw G2 point must be 128 bytes")
    q = curve.base.p
    w = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(4)]
    if checked and any(v >= q for v in w):
        raise ValueError("a coordinate's stored word is not below the modulus")
    if not any(w):
        return None
    c = [v * _rinv(q) % q for v in w]
    P = ((c[0], c[1]), (c[2], c[3]))
    if checked and not Fq2Arith(q).on_curve(P):
        raise ValueError("not on the curve")
    return P


def _params_sizes(format: str):
    if format not in SERDE_FORMATS:
        raise ValueError("unknown format %r" % (format,))
    return (32, 64) if format == "processed" else (64, 128)


def params_size(k: int, format: str) -> int:
    g1, g2 = _params_sizes(format)
    return 4 + 2 * g1 * (1 << k) + 2 * g2


def params_bytes(curve: CurveSpec, k: int, g, g_lagrange, g2: bytes, s_g2: bytes, format: str = "raw-unchecked") -> bytes:
    """ParamsKZG::write_custom: g, g_lagrange (2^k, 8) u64 Montgomery affine; g2, s_g2 the 128 raw bytes ParamsKZG keeps (shorter: zero-padded)"""
    from .transcript import compress

    _params_sizes(format)
    g = np.ascontiguousarray(g, dtype=np.uint64).reshape(-1, 8)
    gl = np.ascontiguousarray(g_lagrange, dtype=np.uint64).reshape(-1, 8)
    if g.shape[0] != 1 << k or gl.shape[0] != 1 << k:
        raise ValueError("g and g_lagrange must hold 2^k points")
    raw2 = [bytes(b).ljust(128, b"\0") for b in (g2, s_g2)]
    if format != "processed":
        return struct.pack("<I", k) + g.tobytes() + gl.tobytes() + raw2[0] + raw2[1]
    pts = decode_points(curve, g) + decode_points(curve, gl)
    return struct.pack("<I", k) + b"".join(compress(curve, P) for P in pts) + b"".join(g2_compress(curve, g2_from_raw(curve, b, checked=False)) for b in raw2)


def params_from_bytes(curve: CurveSpec, data: bytes, format: str = "raw-unchecked"):
    """ParamsKZG::read_custom: -> (k, g, g_lagrange, g2, s_g2) in the layout params_bytes takes; ValueError for a wrong length, k > 28, and -- "processed", "raw" --
    anything that is not a point"""
    from .transcript import decompress

    g1, g2 = _params_sizes(format)
    data = bytes(data)
    if len(data) < 4:
        raise ValueError("unexpected end of input")
    (k,) = struct.unpack("<I", data[:4])
    if k > 28:
        raise ValueError("params: k out of range")
    n = 1 << k
    if len(data) != params_size(k, format):
        raise ValueError("params: length does not match k")
    o2 = 4 + 2 * g1 * n
    tail = [data[o2:o2 + g2], data[o2 + g2:o2 + 2 * g2]]
    if format == "processed":
        pts = encode_points(curve, [decompress(curve, data[4 + 32 * i:36 + 32 * i]) for i in range(2 * n)])
        raw2 = [g2_to_raw(curve, g2_decompress(curve, b)) for b in tail]
    else:
        pts = np.frombuffer(data[4:o2], dtype=np.uint64).reshape(2 * n, 8).copy()
        raw2 = tail
        if format == "raw":
            p = curve.base.p
            words = array_to_ints(pts.reshape(-1, 4))
            if any(v >= p for v in words):
                raise ValueError("a coordinate's stored word is not below the modulus")
            for P in decode_points(curve, pts):
                if P is not None and (P[1] * P[1] - P[0] * P[0] * P[0] - curve.b) % p:
                    raise ValueError("not on the curve")
            for b in tail:
                g2_from_raw(curve, b, checked=True)
    return k, pts[:n], pts[n:], raw2[0], raw2[1]


# ---- ParamsIPA::{write, read} ----------------------------------------------------------------------------
def params_ipa_bytes(curve: CurveSpec, k: int, g, g_lagrange, w, u) -> bytes:
    """ParamsIPA::write [UPSTREAM halo2_proofs/src/poly/ipa/commitment.rs]: k: u32 LE | g | g_lagrange | w | u, every point its 32-byte GroupEncoding
    (transcript.compress).  g, g_lagrange: (2^k, 8) u64 Montgomery affine; w, u: 8 u64 each."""
    from .transcript import compress

    g, gl = decode_points(curve, g), decode_points(curve, g_lagrange)
    if len(g) != 1 << k or len(gl) != 1 << k:
        raise ValueError("g and g_lagrange must hold 2^k points")
    pts = g + gl + decode_points(curve, w) + decode_points(curve, u)
    return struct.pack("<I", k) + b"".join(compress(curve, P) for P in pts)


def params_ipa_from_bytes(curve: CurveSpec, data: bytes):
    """ParamsIPA::read: -> (k, g, g_lagrange, w, u) in the layout params_ipa_bytes takes; ValueError for a wrong length or an encoding that is not a point."""
    from .transcript import decompress

    data = bytes(data)
    if len(data) < 4:
        raise ValueError("unexpected end of input")
    (k,) = struct.unpack("<I", data[:4])
    if k > 28:
        raise ValueError("params: k out of range")
    n = 1 << k
    if len(data) != 4 + 64 * n + 64:
        raise ValueError("params: length does not match k")
    pts = encode_points(curve, [decompress(curve, data[4 + 32 * i:36 + 32 * i]) for i in range(2 * n + 2)])
    return k, pts[:n], pts[n:2 * n], pts[2 * n], pts[2 * n + 1]


def _exact(fh, nbytes: int) -> bytes:
    b = fh.read(nbytes)
    if len(b) != nbytes:
        raise ValueError("unexpected end of file")
    return b


# ---- keys in the three SerdeFormats: the host mirror of csrc/key_format.hpp and of the two device codecs ------------------
# [UPSTREAM halo2_proofs/src/plonk.rs VerifyingKey / ProvingKey::{write, read}(.., SerdeFormat), halo2curves 0.3.x SerdeObject; restated from memory]
#   "processed": a commitment is its 32-byte GroupEncoding (transcript.compress), an element its canonical integer, 32 B little-endian (to_repr);
#   "raw", "raw-unchecked": a commitment is 64 B and an element 32 B of Montgomery limbs; "raw" validates every one of them when read.
KEY_SECTION_NAMES = ("fixed commitments", "permutation commitments", "l0", "l_last", "l_active_row", "fixed_values", "fixed_polys", "fixed_cosets",
                     "permutation values", "permutation polys", "permutation cosets")


def _check_format(format: str):
    if format not in SERDE_FORMATS:
        raise ValueError("unknown format %r" % (format,))


def key_layout(format: str, k: int, nf: int, npc: int, nsel: int, ext_shift: int) -> dict:
    """where every section of a vk / pk lies (csrc/key_format.hpp key_layout): `polys` maps a section name to (off, count, len, slice) -- a slice starts with its
    count word at off, polynomial i's length word is at off + (4 if slice) + i * (4 + 32 len)"""
    _check_format(format)
    if not 0 <= k <= 28:
        raise ValueError("k out of range")
    n, point = 1 << k, 32 if format == "processed" else 64
    m = n << ext_shift
    L = dict(k=k, n=n, m=m, point=point, off_fixed_c=8, off_perm_c=8 + point * nf, off_selectors=8 + point * (nf + npc), sel_bytes=(n + 7) // 8)
    o = L["vk_size"] = L["off_selectors"] + L["sel_bytes"] * nsel
    polys = {}
    for name, cnt, ln in zip(KEY_SECTION_NAMES[2:], (1, 1, 1, nf, nf, nf, npc, npc, npc), (m, m, m, n, n, m, n, n, m)):
        sl = not name.startswith("l")
        polys[name] = (o, cnt, ln, sl)
        o += (4 if sl else 0) + cnt * (4 + 32 * ln)
    L["polys"], L["pk_size"] = polys, o
    return L


def key_header_error(data: bytes, format: str, nf: int, npc: int, nsel: int, ext_shift: int, pk: bool, want_k: Optional[int] = None, length: Optional[int] = None) -> str:
    """the verdict of csrc/key_format.hpp key_parse_header on a key's header and length: "" when it passes, the error's text otherwise.  `length`: the key's
    length when `data` is only its first eight bytes"""
    if format not in SERDE_FORMATS:
        return "unknown format"
    length = len(data) if length is None else length
    if length < 8:
        return "length: unexpected end of input"
    k, nf_file = struct.unpack(">II", data[:8])
    if k > 28:
        return "k out of range"
    if want_k is not None and k != want_k:
        return "k differs from the params'"
    if k + ext_shift > 32:
        return "k out of range"
    L = key_layout(format, k, nf, npc, nsel, ext_shift)
    if nf_file != nf:
        return "fixed-column count: the key's number of fixed commitments differs from the circuit's fixed columns"
    if length != (L["pk_size"] if pk else L["vk_size"]):
        return "length does not match the circuit (unexpected end of input or trailing bytes)"
    return ""


def scalars_to_repr(f: FieldSpec, words) -> bytes:
    """to_repr of Montgomery words ((.., 4) u64): every word w as (w R^-1 mod p), 32 bytes little-endian"""
    rinv = _rinv(f.p)
    return b"".join((w * rinv % f.p).to_bytes(32, "little") for w in array_to_ints(np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4)))


def scalars_from_repr(f: FieldSpec, data: bytes, section: str = "") -> np.ndarray:
    """from_repr: 32-byte little-endian integers -> (count, 4) u64 Montgomery words; ValueError naming the lowest index that is not below p"""
    R = (1 << 256) % f.p
    vals = [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]
    for i, v in enumerate(vals):
        if v >= f.p:
            raise ValueError("an element is not below the modulus: %s, element %d" % (section, i))
    return ints_to_array([v * R % f.p for v in vals]).reshape(-1, 4)


def scalars_check(f: FieldSpec, words, section: str = ""):
    """a checked from_raw_bytes: ValueError naming the lowest index whose stored Montgomery word is not below p"""
    for i, w in enumerate(array_to_ints(np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4))):
        if w >= f.p:
            raise ValueError("an element's stored word is not below the modulus: %s, element %d" % (section, i))


def commitments_bytes(curve: CurveSpec, pts, format: str) -> bytes:
    from .transcript import compress

    pts = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, 8)
    return pts.tobytes() if format != "processed" else b"".join(compress(curve, P) for P in decode_points(curve, pts))


def commitments_from_bytes(curve: CurveSpec, data: bytes, format: str, section: str = "") -> np.ndarray:
    """a commitment list as the format reads it -> (count, 8) u64 Montgomery affine; "processed" and "raw" raise ValueError for anything that is not a point"""
    from .transcript import decompress

    p = curve.base.p
    if format == "processed":
        out = []
        for i in range(0, len(data), 32):
            e = data[i:i + 32]
            x = int.from_bytes(e[:31] + bytes([e[31] & 0x7F]), "little")
            if x >= p:
                raise ValueError("an x coordinate is not below the modulus: " + section)
            if x == 0 and e[31] >> 7:
                raise ValueError("x = 0 with the sign bit set is not an encoding: " + section)
            try:
                out.append(decompress(curve, e))
            except ValueError:
                raise ValueError("an x coordinate is not on the curve: " + section) from None
        return encode_points(curve, out) if out else np.zeros((0, 8), dtype=np.uint64)
    pts = np.frombuffer(data, dtype=np.uint64).reshape(-1, 8).copy()
    if format == "raw":
        if any(v >= p for v in array_to_ints(pts.reshape(-1, 4))):
            raise ValueError("a coordinate's stored word is not below the modulus: " + section)
        for P in decode_points(curve, pts):
            if P is not None and (P[1] * P[1] - P[0] * P[0] * P[0] - curve.b) % p:
                raise ValueError("a point is neither on the curve nor the identity: " + section)
    return pts


def _elements_bytes(f: FieldSpec, arr, format: str) -> bytes:
    return scalars_to_repr(f, arr) if format == "processed" else np.ascontiguousarray(arr, dtype=np.uint64).tobytes()


class HostProvingKey:
    """A proving key as it lies on disk, on the host: the verifying key and the nine polynomial sections in upstream's standard Montgomery form (numpy, no device).
    l: (3, m, 4) = l0, l_last, l_active_row; the six slices: (count, len, 4).  write / read speak the three SerdeFormats; the device-resident ProvingKey goes
    through this class, and the tests build keys by hand with it."""

    SLICES = ("fixed_values", "fixed_polys", "fixed_cosets", "perm_values", "perm_polys", "perm_cosets")

    def __init__(self, vk: "VerifyingKey", l, fixed_values, fixed_polys, fixed_cosets, perm_values, perm_polys, perm_cosets):
        self.vk = vk
        self.l = np.ascontiguousarray(l, dtype=np.uint64)
        for name, a in zip(self.SLICES, (fixed_values, fixed_polys, fixed_cosets, perm_values, perm_polys, perm_cosets)):
            setattr(self, name, np.ascontiguousarray(a, dtype=np.uint64))

    def sections(self):
        """(section name, (count, len, 4) array, is a slice) in file order"""
        out = [(KEY_SECTION_NAMES[2 + i], self.l[i:i + 1], False) for i in range(3)]
        return out + [(KEY_SECTION_NAMES[5 + i], getattr(self, name), True) for i, name in enumerate(self.SLICES)]

    def write(self, fh, format: str = "raw-unchecked"):
        _check_format(format)
        f = self.vk.curve.scalar
        self.vk.write(fh, format)
        for _, arr, sl in self.sections():
            if sl:
                fh.write(struct.pack(">I", arr.shape[0]))
            for poly in arr:
                fh.write(struct.pack(">I", poly.shape[0]))
                fh.write(_elements_bytes(f, poly, format))

    def to_bytes(self, format: str = "raw-unchecked") -> bytes:
        buf = io.BytesIO()
        self.write(buf, format)
        return buf.getvalue()

    @classmethod
    def read(cls, curve: CurveSpec, cs: plonk.ConstraintSystem, fh, num_selectors: int = 0, format: str = "raw-unchecked") -> "HostProvingKey":
        """ProvingKey::read(.., SerdeFormat) on the host.  ValueError for a key that does not fit the circuit and -- "processed", "raw" -- for a commitment that is
        not a point or an element that is not below the modulus, naming the section and, for an element, its lowest index within the section.  Trailing bytes
        are the caller's to check (from_bytes does)."""
        _check_format(format)
        vk = VerifyingKey.read(curve, cs, fh, num_selectors, format)
        f = curve.scalar
        n = 1 << vk.k
        m = EvaluationDomain(None, f, cs.degree(), vk.k).extended_len()
        nf, npc = cs.num_fixed, len(cs.permutation_columns)
        got = []
        for name, cnt, ln, sl in zip(KEY_SECTION_NAMES[2:], (1, 1, 1, nf, nf, nf, npc, npc, npc), (m, m, m, n, n, m, n, n, m), (False,) * 3 + (True,) * 6):
            if sl:
                (c,) = struct.unpack(">I", _exact(fh, 4))
                if c != cnt:
                    raise ValueError("polynomial count differs from the circuit's: %s" % name)
            raw = []
            for _ in range(cnt):
                (l_,) = struct.unpack(">I", _exact(fh, 4))
                if l_ != ln:
                    raise ValueError("polynomial length differs from the domain's: %s" % name)
                raw.append(_exact(fh, 32 * ln))
            data = b"".join(raw)
            if format == "processed":
                arr = scalars_from_repr(f, data, name)
            else:
                arr = np.frombuffer(data, dtype=np.uint64).reshape(-1, 4).copy()
                if format == "raw":
                    scalars_check(f, arr, name)
            got.append(arr.reshape(cnt, ln, 4))
        return cls(vk, np.concatenate(got[:3]), *got[3:])

    @classmethod
    def from_bytes(cls, curve: CurveSpec, cs: plonk.ConstraintSystem, data: bytes, num_selectors: int = 0, format: str = "raw-unchecked") -> "HostProvingKey":
        fh = io.BytesIO(bytes(data))
        key = cls.read(curve, cs, fh, num_selectors, format)
        if fh.read(1):
            raise ValueError("length does not match the circuit (unexpected end of input or trailing bytes)")
        return key


# ---- keys -----------------------------------------------------------------------------------------------
class VerifyingKey:
    def __init__(self, curve: CurveSpec, k: int, cs: plonk.ConstraintSystem, fixed_commitments: np.ndarray, permutation_commitments: np.ndarray,
                 selectors: Sequence[np.ndarray] = ()):
        self.curve, self.k, self.cs = curve, k, cs
        self.fixed_commitments = np.ascontiguousarray(fixed_commitments, dtype=np.uint64).reshape(-1, 8)        # Montgomery affine
        self.permutation_commitments = np.ascontiguousarray(permutation_commitments, dtype=np.uint64).reshape(-1, 8)
        self.selectors = [np.asarray(s, dtype=bool) for s in selectors]
        self.transcript_repr = self._transcript_repr()

    def _transcript_repr(self) -> int:
        """vk.transcript_repr.  [UPSTREAM hashes `format!("{:?}", vk.pinned())` with Blake2b-512 personalised
        "Halo2-Verify-Key"; Rust's Debug text of the pinned key cannot be reproduced without the crate, so the same
        hash is taken over this key's RawBytes serialisation and the constraint system's description instead.]"""
        h = hashlib.blake2b(digest_size=64, person=b"Halo2-Verify-Key")
        buf = io.BytesIO()
        self.write(buf)
        body = buf.getvalue() + repr(self.cs.description()).encode()
        h.update(struct.pack("<Q", len(body)))
        h.update(body)
        return int.from_bytes(h.digest(), "little") % self.curve.scalar.p

    def write(self, fh, format: str = "raw-unchecked"):
        """VerifyingKey::write(.., SerdeFormat); both raw formats write the same bytes"""
        _check_format(format)
        fh.write(struct.pack(">I", self.k))
        fh.write(struct.pack(">I", self.fixed_commitments.shape[0]))
        fh.write(commitments_bytes(self.curve, self.fixed_commitments, format))
        fh.write(commitments_bytes(self.curve, self.permutation_commitments, format))
        for sel in self.selectors:
            fh.write(np.packbits(sel, bitorder="little").tobytes())

    @classmethod
    def read(cls, curve: CurveSpec, cs: plonk.ConstraintSystem, fh, num_selectors: int = 0, format: str = "raw-unchecked") -> "VerifyingKey":
        """VerifyingKey::read(.., SerdeFormat); "processed" and "raw" raise ValueError for a commitment that is not a point, naming the list"""
        _check_format(format)
        (k,) = struct.unpack(">I", _exact(fh, 4))
        (nf,) = struct.unpack(">I", _exact(fh, 4))
        if k > 28 and format != "raw-unchecked":      # (the default format reads as it always has)
            raise ValueError("k out of range")
        if nf != cs.num_fixed:
            raise ValueError("vk holds %d fixed commitments, the circuit has %d fixed columns" % (nf, cs.num_fixed))
        point = 32 if format == "processed" else 64
        fixed = commitments_from_bytes(curve, _exact(fh, point * nf), format, KEY_SECTION_NAMES[0])
        npc = len(cs.permutation_columns)
        perm = commitments_from_bytes(curve, _exact(fh, point * npc), format, KEY_SECTION_NAMES[1])
        n = 1 << k
        sels = [np.unpackbits(np.frombuffer(_exact(fh, (n + 7) // 8), dtype=np.uint8), bitorder="little")[:n].astype(bool) for _ in range(num_selectors)]
        return cls(curve, k, cs, fixed, perm, sels)


class ProvingKey:
    """Device-resident proving key.  Extended-domain columns are kept in the kernels' internal element form
    (dehalo.h: DEHALO_EVAL_COLUMNS_INTERNAL) and converted back only when the key is written."""

    def __init__(self, ctx: Context, vk: VerifyingKey, domain: EvaluationDomain, l_ext, fixed_values, fixed_polys, fixed_cosets, perm_values, perm_polys,
                 perm_cosets):
        self.ctx, self.vk, self.domain = ctx, vk, domain
        self.l_ext = l_ext                        # (3, ext_n, 4): l0, l_last, l_active_row -- internal form
        self.fixed_values, self.fixed_polys, self.fixed_cosets = fixed_values, fixed_polys, fixed_cosets      # cosets internal form
        self.perm_values, self.perm_polys, self.perm_cosets = perm_values, perm_polys, perm_cosets
        f = vk.curve.scalar
        p = f.p
        self.custom_gates = plonk.custom_gates_graph(vk.cs, p).compile(ctx, f)
        self.lookup_graphs = [plonk.lookup_table_value_graph(i, t, p).compile(ctx, f) for i, t in vk.cs.lookups]
        self.compress_graphs = [(plonk.compress_graph(i, p).compile(ctx, f), plonk.compress_graph(t, p).compile(ctx, f)) for i, t in vk.cs.lookups]

    def _std(self, t):
        import torch

        out = torch.empty_like(t)
        self.ctx.convert_form_device(self.vk.curve.scalar.id, t.data_ptr(), out.data_ptr(), t.numel() // 4, False, 0)
        self.ctx.synchronize()
        return to_host(out)

    def to_host_key(self) -> HostProvingKey:
        """the key's sections on the host, extended-domain columns converted out of the internal form"""
        with self.ctx.torch_stream():
            def host(t, internal=False):
                if not t.shape[0]:
                    return np.zeros(tuple(t.shape), dtype=np.uint64)
                return self._std(t) if internal else to_host(t)

            return HostProvingKey(self.vk, self._std(self.l_ext), host(self.fixed_values), host(self.fixed_polys), host(self.fixed_cosets, True),
                                  host(self.perm_values), host(self.perm_polys), host(self.perm_cosets, True))

    def write(self, fh, format: str = "raw-unchecked"):
        """ProvingKey::write(.., SerdeFormat)"""
        self.to_host_key().write(fh, format)

    @classmethod
    def read(cls, ctx: Context, curve: CurveSpec, cs: plonk.ConstraintSystem, fh, num_selectors: int = 0, format: str = "raw-unchecked") -> "ProvingKey":
        """ProvingKey::read(.., SerdeFormat); the checked formats raise ValueError (HostProvingKey.read)"""
        with ctx.torch_stream():
            return cls._read(ctx, curve, cs, fh, num_selectors, format)

    @classmethod
    def _read(cls, ctx: Context, curve: CurveSpec, cs: plonk.ConstraintSystem, fh, num_selectors: int = 0, format: str = "raw-unchecked") -> "ProvingKey":
        hk = HostProvingKey.read(curve, cs, fh, num_selectors, format)
        f = curve.scalar
        domain = EvaluationDomain(ctx, f, cs.degree(), hk.vk.k)
        dev = [to_device(a) for a in (hk.l, hk.fixed_values, hk.fixed_polys, hk.fixed_cosets, hk.perm_values, hk.perm_polys, hk.perm_cosets)]
        for t in (dev[0], dev[3], dev[6]):
            if t.numel():
                ctx.convert_form_device(f.id, t.data_ptr(), t.data_ptr(), t.numel() // 4, True, 0)
        ctx.synchronize()
        return cls(ctx, hk.vk, domain, *dev)


def vk_size(cs: plonk.ConstraintSystem, k: int, num_selectors: int) -> int:
    """Bytes VerifyingKey.write produces (RawBytes): what the reference lists as |vk| (benches/README.md:56-60)."""
    return 4 + 4 + 64 * cs.num_fixed + 64 * len(cs.permutation_columns) + num_selectors * (((1 << k) + 7) // 8)


def pk_size(cs: plonk.ConstraintSystem, k: int, num_selectors: int, field: FieldSpec) -> int:
    """Bytes ProvingKey.write produces (RawBytes): the reference's |pk|."""
    n = 1 << k
    m = EvaluationDomain(None, field, cs.degree(), k).extended_len()
    poly = lambda ln: 4 + 32 * ln
    sl = lambda cnt, ln: 4 + cnt * poly(ln)
    nf, npc = cs.num_fixed, len(cs.permutation_columns)
    return vk_size(cs, k, num_selectors) + 3 * poly(m) + sl(nf, n) + sl(nf, n) + sl(nf, m) + sl(npc, n) + sl(npc, n) + sl(npc, m)


def delta_of(f: FieldSpec) -> int:
    """PrimeField::DELTA = MULTIPLICATIVE_GENERATOR^(2^S): generates the odd-order subgroup."""
    return pow(f.gen, 1 << f.two_adicity, f.p)


def omega_powers_device(ctx: Context, domain: EvaluationDomain):
    """(n, 4) device column of omega^i, as the forward NTT of the unit vector e_1."""
    import torch

    f = domain.field
    col = torch.zeros((domain.n, 4), dtype=torch.int64, device="cuda")
    if domain.n > 1:
        col[1] = to_device(f.encode(1).reshape(1, 4))[0]
        ctx.ntt_device(f.id, col.data_ptr(), domain.k, f.encode(domain.omega), 1, 0)
    else:
        col[0] = to_device(f.encode(1).reshape(1, 4))[0]
    return col


def keygen(ctx: Context, params: ParamsKZG, cs: plonk.ConstraintSystem, fixed_canonical: np.ndarray, assembly: plonk.Assembly,
           selectors: Sequence[np.ndarray] = ()) -> ProvingKey:
    with ctx.torch_stream():           # torch's copies and fills go on the context's stream, ordered with the kernels
        return _keygen(ctx, params, cs, fixed_canonical, assembly, selectors)


def _keygen(ctx: Context, params: ParamsKZG, cs: plonk.ConstraintSystem, fixed_canonical: np.ndarray, assembly: plonk.Assembly,
            selectors: Sequence[np.ndarray] = ()) -> ProvingKey:
    """keygen_vk + keygen_pk for a circuit whose fixed columns (selectors already compressed into them) and copy
    constraints are given: fixed_canonical = (num_fixed, n, 4) u64 canonical values (rows >= usable must be zero)."""
    import torch

    curve, f, k = params.curve, params.curve.scalar, params.k
    domain = EvaluationDomain(ctx, f, cs.degree(), k)
    n, m, ek = domain.n, domain.extended_len(), domain.extended_k
    bf = cs.blinding_factors()
    if n < bf + 3:
        raise ValueError("not enough rows available")                          # upstream: Error::NotEnoughRowsAvailable
    fixed_canonical = np.ascontiguousarray(fixed_canonical, dtype=np.uint64).reshape(cs.num_fixed, n, 4)
    enc = f.encode
    c = dict(omega_inv=enc(domain.omega_inv), ifft=enc(domain.ifft_divisor), ext_omega=enc(domain.extended_omega), zeta=enc(domain.g_coset))

    def lagrange_to_all(values):
        """values (cnt, n, 4) Montgomery on device -> (commitments Montgomery affine on host, polys, cosets internal)."""
        cnt = values.shape[0]
        polys = values.clone()
        cosets = torch.zeros((cnt, m, 4), dtype=torch.int64, device="cuda")
        jac = torch.zeros((max(cnt, 1), 12), dtype=torch.int64, device="cuda")
        aff = torch.zeros((max(cnt, 1), 8), dtype=torch.int64, device="cuda")
        if cnt:
            params.commit_device(values.data_ptr(), cnt, jac.data_ptr(), True)
            ctx.to_affine_device(curve.id, jac.data_ptr(), cnt, aff.data_ptr(), 0)
            ctx.intt_scaled_device(f.id, polys.data_ptr(), k, c["omega_inv"], c["ifft"], cnt, 0)
            ctx.coset_ntt_form_device(f.id, polys.data_ptr(), k, cosets.data_ptr(), ek, c["ext_omega"], c["zeta"], cnt, ev.FORM_OUT_INTERNAL, 0)
        ctx.synchronize()
        return to_host(aff)[:cnt], polys, cosets

    # fixed columns
    fixed_values = to_device(fixed_canonical)
    if cs.num_fixed:
        ctx.field_op_device(f.id, "to_mont", fixed_values.data_ptr(), 0, fixed_values.data_ptr(), cs.num_fixed * n, 0)
    fixed_commitments, fixed_polys, fixed_cosets = lagrange_to_all(fixed_values)

    # permutation: sigma_j(omega^i) = delta^(column of the mapped cell) * omega^(its row)
    npc = len(cs.permutation_columns)
    if assembly.num_columns != npc or assembly.n != n:
        raise ValueError("assembly does not match the constraint system")
    ident = torch.zeros((npc, n, 4), dtype=torch.int64, device="cuda")
    w = omega_powers_device(ctx, domain)
    delta, dj = delta_of(f), 1
    for j in range(npc):
        ident[j].copy_(w)
        if j:
            ctx.scale_device(f.id, ident[j].data_ptr(), n, enc(dj).reshape(1, 4), 0, 0)
        dj = dj * delta % f.p
    ctx.synchronize()
    perm_values = ident.view(npc * n, 4)[to_device_index(assembly.mapping)].view(npc, n, 4).contiguous() if npc else ident
    perm_commitments, perm_polys, perm_cosets = lagrange_to_all(perm_values)

    # l0, l_last, l_active_row = 1 - (l_last + l_blind) in the extended domain
    one = to_device(enc(1).reshape(1, 4))[0]
    u = n - bf - 1
    lag = torch.zeros((3, n, 4), dtype=torch.int64, device="cuda")
    lag[0, 0] = one
    lag[1, u] = one
    lag[2, :u] = one
    _, _, l_ext = lagrange_to_all(lag)

    vk = VerifyingKey(curve, k, cs, fixed_commitments, perm_commitments, selectors)
    return ProvingKey(ctx, vk, domain, l_ext, fixed_values, fixed_polys, fixed_cosets, perm_values, perm_polys, perm_cosets)


def to_device_index(idx: np.ndarray):
    from ._lib import transfer_context

    with transfer_context() as c:
        return c.upload(np.ascontiguousarray(idx, dtype=np.int64))
