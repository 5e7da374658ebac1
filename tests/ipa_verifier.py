"""The IPA opening argument on Python integers -- TEST INFRASTRUCTURE ONLY.

`verify_opening` restates upstream's verifier of one opening [UPSTREAM halo2_proofs @ v2023_04_20: poly/ipa/commitment/verifier.rs
`verify_proof`, poly/ipa/strategy.rs `GuardIPA` (compute_s, compute_b)] from the published protocol: read S, xi, z, the k rounds' (L_j, R_j, u_j)
and c, f, then check

    P - [v] G_0 + [xi] S + sum_j ([u_j^-1] L_j + [u_j] R_j) - [c] <s, G> - [c b z] U - [f] W = 0

with one multi-exponentiation (coracle.best_multiexp, the C restatement of best_multiexp) over [G | P, S, L_j, R_j, U, W].

`open_reference` is the prover side, commitment::create_proof, written out with naive group arithmetic (pyoracle): slow, for k <= 6.

The item order (S; xi, z; per round L_j, R_j, u_j; c, f) and the draw order (s_poly, s_poly_blind, then l_rand, r_rand per round) are restated
from the published protocol; no upstream source was at hand to pin them byte for byte.  Acceptance by this verifier shows the device's proofs
are sound openings; it does not show they equal upstream's bytes.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np

import pyoracle as po
from plonk_oracle import Transcript
from verifier import ReadTranscript


def _sqrt(a: int, p: int) -> Optional[int]:
    """Tonelli-Shanks (the Pasta fields are 1 mod 4: the oracle's reader takes p = 3 mod 4 only)."""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    q, s = p - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % p, i + 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    return r


class PastaReadTranscript(ReadTranscript):
    """Blake2bRead over a Pasta curve: GroupEncoding of Ep / Eq (x little-endian, bit 255 = sign of y; all zero = identity, refused)."""

    def read_point(self):
        b = self._take()
        sign = b[31] >> 7
        x = int.from_bytes(b[:31] + bytes([b[31] & 0x7F]), "little")
        p = self.curve.base.p
        if x >= p:
            raise ValueError("non-canonical x")
        if x == 0 and sign == 0:
            raise ValueError("identity in proof")
        y = _sqrt(x * x % p * x + self.curve.b, p)
        if y is None:
            raise ValueError("not on curve")
        if (y & 1) != sign:
            y = p - y
        self.h.update(b"\x01" + x.to_bytes(32, "little") + y.to_bytes(32, "little"))
        return (x, y)


def compute_s(us: Sequence[int], init: int, p: int) -> List[int]:
    v = [0] * (1 << len(us))
    v[0] = init % p
    for i, u in enumerate(reversed(us)):
        ln = 1 << i
        for t in range(ln):
            v[ln + t] = v[t] * u % p
    return v


def compute_b(x: int, us: Sequence[int], p: int) -> int:
    tmp, cur = 1, x % p
    for u in reversed(us):
        tmp = tmp * (1 + u * cur) % p
        cur = cur * cur % p
    return tmp


def verify_opening(co, curve_spec, curve: po.Curve, g_mont: np.ndarray, u_mont: np.ndarray, w_mont: np.ndarray, commitment, x3: int, v: int,
                   proof: bytes) -> bool:
    """commitment = P as canonical (x, y); g_mont / u_mont / w_mont as the library takes them (Montgomery {x, y}); x3, v canonical."""
    g_mont = np.ascontiguousarray(g_mont, dtype=np.uint64).reshape(-1, 8)
    n = g_mont.shape[0]
    k = n.bit_length() - 1
    f = curve.scalar
    p = f.p
    T = PastaReadTranscript(curve, proof)
    try:
        S = T.read_point()
        xi, z = T.challenge(), T.challenge()
        rounds = []
        for _ in range(k):
            L, R = T.read_point(), T.read_point()
            rounds.append((L, R, T.challenge()))
        c, fv = T.read_scalar(), T.read_scalar()
    except ValueError:
        return False
    if T.pos != len(proof):
        return False
    us = [u for (_, _, u) in rounds]
    if any(u == 0 for u in us):
        return False
    s = compute_s(us, -c, p)
    s[0] = (s[0] - v) % p
    b = compute_b(x3, us, p)
    enc_b = curve_spec.base.encode
    pts, scs = [], []
    for P, sc in [(commitment, 1), (S, xi)] + [(L, pow(u, -1, p)) for (L, _, u) in rounds] + [(R, u) for (_, R, u) in rounds]:
        pts.append(np.concatenate([enc_b(P[0]), enc_b(P[1])]))
        scs.append(sc)
    bases = np.concatenate([g_mont, np.stack(pts), np.asarray(u_mont, dtype=np.uint64).reshape(1, 8), np.asarray(w_mont, dtype=np.uint64).reshape(1, 8)])
    scalars = curve_spec.scalar.encode_many([x % p for x in s + scs + [-c * b * z, -fv]])
    acc = co.to_affine(curve_spec.id, co.best_multiexp(curve_spec.id, scalars, bases, 4))
    return not np.asarray(acc).any()


def _dec_points(curve_spec, arr) -> List[Optional[tuple]]:
    arr = np.asarray(arr, dtype=np.uint64).reshape(-1, 8)
    return [None if not row.any() else (curve_spec.base.decode(row[:4]), curve_spec.base.decode(row[4:])) for row in arr]


def open_reference(curve_spec, curve: po.Curve, g_mont, u_mont, w_mont, poly: Sequence[int], blind: int, x3: int, draw: Callable[[int], np.ndarray],
                   transcript: Optional[Transcript] = None) -> bytes:
    """commitment::create_proof on integers.  draw(count) -> count x 4 u64 Montgomery representations (prover.SeededRng.scalars)."""
    f = curve.scalar
    p = f.p
    G = _dec_points(curve_spec, g_mont)
    U = _dec_points(curve_spec, u_mont)[0]
    W = _dec_points(curve_spec, w_mont)[0]
    n = len(G)
    k = n.bit_length() - 1
    dec = curve_spec.scalar.decode_many
    s_poly = dec(draw(n))
    s_blind = dec(draw(1))[0]
    rands = dec(draw(2 * k))
    T = transcript if transcript is not None else Transcript(curve)
    s_at = po.eval_polynomial(f, s_poly, x3)
    s_poly[0] = (s_poly[0] - s_at) % p
    T.write_point(po.ec_add(curve, po.msm_naive(curve, s_poly, G), po.ec_mul(curve, s_blind, W)))
    xi, z = T.challenge(), T.challenge()
    pp = [(a + xi * b) % p for a, b in zip(poly, s_poly)]
    pp[0] = (pp[0] - po.eval_polynomial(f, pp, x3)) % p
    fsum = (s_blind * xi + blind) % p
    bvec = [pow(x3, i, p) for i in range(n)]
    g = list(G)
    for j in range(k):
        half = len(pp) // 2
        lr, rr = rands[2 * j], rands[2 * j + 1]
        vl = sum(a * b for a, b in zip(pp[half:], bvec[:half])) % p
        vr = sum(a * b for a, b in zip(pp[:half], bvec[half:])) % p
        L = po.msm_naive(curve, pp[half:] + [vl * z % p, lr], g[:half] + [U, W])
        R = po.msm_naive(curve, pp[:half] + [vr * z % p, rr], g[half:] + [U, W])
        T.write_point(L)
        T.write_point(R)
        u = T.challenge()
        ui = pow(u, -1, p)
        pp = [(pp[i] + pp[i + half] * ui) % p for i in range(half)]
        bvec = [(bvec[i] + bvec[i + half] * u) % p for i in range(half)]
        g = [po.ec_add(curve, g[i], po.ec_mul(curve, u, g[i + half])) for i in range(half)]
        fsum = (fsum + lr * ui + rr * u) % p
    T.write_scalar(pp[0])
    T.write_scalar(fsum)
    return bytes(T.proof)


def commit_reference(co, curve_spec, g_mont, w_mont, poly: Sequence[int], blind: int):
    """P = MSM(poly, g) + [blind] W (ParamsIPA::commit) as canonical (x, y), through the C restatement of best_multiexp."""
    p = curve_spec.scalar.p
    bases = np.concatenate([np.asarray(g_mont, dtype=np.uint64).reshape(-1, 8), np.asarray(w_mont, dtype=np.uint64).reshape(1, 8)])
    scalars = curve_spec.scalar.encode_many([x % p for x in list(poly) + [blind]])
    return _dec_points(curve_spec, co.to_affine(curve_spec.id, co.best_multiexp(curve_spec.id, scalars, bases, 4)))[0]
