"""CPU restatement of the SHPLONK multiopen over KZG / BN254: ProverSHPLONK (a scheme object for plonk_oracle.create_proof) and verify_proof_shplonk (over
verifier.read_plonk and pairing.pairing_product_is_one).  TEST INFRASTRUCTURE ONLY, beside the oracle's GWC and IPA restatements.

Follows [UPSTREAM halo2_proofs @ v2023_04_20: poly/kzg/multiopen/shplonk.rs, shplonk/prover.rs, shplonk/verifier.rs] from the published algorithm (the crate is
not at hand): parity with upstream's bytes is unpinned; what pins the prover is the pairing check of the verifier below.

The queries (key, point, item, eval) arrive in plonk_oracle.plonk_queries' order.  construct_intermediate_sets: every distinct commitment (by `key`), in order of
first appearance, gets the set of points it is opened at; commitments with equal point sets form one rotation set, sets and the commitments inside a set in order
of first appearance; super_point_set is the union.  (Upstream keeps the points of a set in a BTreeSet; nothing written to the proof depends on their order.  Its
prover tells commitments apart by polynomial and its verifier by point: two identical fixed columns behave differently there, which is out of scope here.)

The prover is worded as upstream words it -- per polynomial the low-degree equivalent R_ij through its evaluations is SUBTRACTED and the difference divided by
(X - z) for every point of the set in turn (co.kate_division) -- and not with the partial-fraction identity of the device's one-pass quotient, which
tests/test_shplonk.py pins separately (partial_fraction_quotient below)."""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np

import coracle as co
import pairing as pr
import plonk_oracle as PO
import pyoracle as po
import verifier as V


# ---- polynomials over Python integers (coefficients low to high) ------------------------------------------------------
def poly_mul_linear(a: Sequence[int], z: int, p: int) -> List[int]:
    """a(X) (X - z)"""
    out = [0] * (len(a) + 1)
    for i, c in enumerate(a):
        out[i] = (out[i] - z * c) % p
        out[i + 1] = (out[i + 1] + c) % p
    return out


def interpolate(points: Sequence[int], evals: Sequence[int], p: int) -> List[int]:
    """lagrange_interpolate: the polynomial of degree < len(points) through (points[t], evals[t])"""
    out = [0] * len(points)
    for t, (zt, et) in enumerate(zip(points, evals)):
        num, den = [1], 1
        for s, zs in enumerate(points):
            if s != t:
                num = poly_mul_linear(num, zs, p)
                den = den * (zt - zs) % p
        c = et * pow(den, -1, p) % p
        for i, nc in enumerate(num):
            out[i] = (out[i] + c * nc) % p
    return out


def evaluate(a: Sequence[int], x: int, p: int) -> int:
    acc = 0
    for c in reversed(a):
        acc = (acc * x + c) % p
    return acc


def kate(a: Sequence[int], z: int, p: int) -> List[int]:
    """arithmetic::kate_division: (a(X) - a(z)) / (X - z), len(a) - 1 coefficients"""
    q, acc = [0] * (len(a) - 1), 0
    for i in range(len(a) - 1, 0, -1):
        acc = (a[i] + z * acc) % p
        q[i - 1] = acc
    return q


def chained_quotient(a: Sequence[int], points: Sequence[int], p: int) -> List[int]:
    """a div prod (X - z), remainders dropped, by one kate division per point: len(a) - len(points) coefficients"""
    q = list(a)
    for z in points:
        q = kate(q, z, p)
    return q


def partial_fraction_quotient(a: Sequence[int], points: Sequence[int], p: int) -> List[int]:
    """the same quotient as sum_t w_t kate(a, z_t), w_t = 1 / prod_{s != t} (z_t - z_s): len(a) - 1 coefficients, the top len(points) - 1 zero"""
    out = [0] * (len(a) - 1)
    for t, zt in enumerate(points):
        den = 1
        for s, zs in enumerate(points):
            if s != t:
                den = den * (zt - zs) % p
        w = pow(den, -1, p)
        for i, c in enumerate(kate(a, zt, p)):
            out[i] = (out[i] + w * c) % p
    return out


# ---- the intermediate sets ----------------------------------------------------------------------------------------
def intermediate_sets(Q):
    """-> (sets, super_points); sets = [(points, [(item, {point: eval}), ...]), ...] in order of first appearance"""
    order, by_key = [], {}
    for key, pt, item, e in Q:
        if key not in by_key:
            by_key[key] = (item, {})
            order.append(key)
        by_key[key][1].setdefault(pt, e)
    sets, index = [], {}
    for key in order:
        item, evals = by_key[key]
        pts = frozenset(evals)
        if pts not in index:
            index[pts] = len(sets)
            sets.append((sorted(pts), []))
        sets[index[pts]][1].append((item, evals))
    super_points = []
    for _, pt, _, _ in Q:
        if pt not in super_points:
            super_points.append(pt)
    return sets, super_points


def _prod(xs, p):
    acc = 1
    for x in xs:
        acc = acc * x % p
    return acc


class ProverSHPLONK(PO.ProverGWC):
    """create_proof's scheme object for KZG with the SHPLONK multiopen: ProverGWC's commitments and instance handling, another `open`."""

    def open(self, T, Q, rng, write_commit) -> dict:
        F = PO.Fld(self.curve.scalar)
        p, fid = F.p, F.id
        y, v = T.challenge(), T.challenge()
        sets, super_points = intermediate_sets(Q)
        n = None
        pad = lambda a: np.concatenate([a.reshape(-1, 4), np.zeros((n - a.reshape(-1, 4).shape[0], 4), dtype=np.uint64)])
        quotients, folded, lows = [], [], []
        for points, members in sets:
            n = members[0][0][0].shape[0] if n is None else n
            # sum_j y^j (P_ij - R_ij), then the division by every (X - z) of the set in turn
            polys = [poly for (poly, _), _ in members]
            ys = [pow(y, j, p) for j in range(len(polys))]
            low = [interpolate(points, [evals[z] for z in points], p) for _, evals in members]
            low_batch = [sum(c * r[i] for c, r in zip(ys, low)) % p for i in range(len(points))]
            batch = co.lincomb(fid, polys, F.many(ys))
            diff = co.lincomb(fid, [batch, pad(F.many(low_batch))], F.many([1, p - 1]))
            q = diff
            for z in points:
                q = co.kate_division(fid, q, F.m(z))
            quotients.append(pad(q))
            folded.append(batch)
            lows.append(low_batch)
        h = co.lincomb(fid, quotients, F.many([pow(v, i, p) for i in range(len(sets))]))
        write_commit(self.srs["g"], h, F.m(0))      # Blind::default(), dropped under KZG
        u = T.challenge()
        zt = _prod([(u - z) % p for z in super_points], p)
        zdiff = [_prod([(u - z) % p for z in super_points if z not in points], p) for points, _ in sets]
        z0_inv = pow(zdiff[0], -1, p)
        coefs = [pow(v, i, p) * zd % p * z0_inv % p for i, zd in enumerate(zdiff)]
        const = sum(c * evaluate(low, u, p) for c, low in zip(coefs, lows)) % p
        L = co.lincomb(fid, folded + [h], F.many(coefs + [-zt * z0_inv % p]), F.m(const))
        assert F.un(co.eval_polynomial(fid, L, F.m(u), self.threads)) == 0, "L(u) != 0"
        write_commit(self.srs["g"], pad(co.kate_division(fid, L, F.m(u))), F.m(0))
        return dict(challenges=dict(y_open=y, v=v, u=u), point_sets=[points for points, _ in sets])


def create_proof(curve: po.Curve, srs, key: dict, advice_mont, instances, rng, vk_repr: int, threads: int = 1):
    return PO.create_proof(curve, srs, key, advice_mont, instances, rng, vk_repr, threads, "shplonk")


def verify_proof_shplonk(curve: po.Curve, desc, k: int, fixed_commitments, perm_commitments, vk_repr: int, g0, g2, s_g2, instances, proof: bytes, circuits=None) -> bool:
    """VerifierSHPLONK::verify_proof behind plonk/verifier.rs: with c_i = v^i zdiff_i / zdiff_0 and z_0 = Z_0(u),
    M = sum_i c_i sum_j y^j [P_ij] - (sum_i c_i sum_j y^j r_ij) G - z_0 [h] + u [h'];  accept iff e([h'], [s]G2) = e(M, G2) and no bytes trail."""
    p, C = curve.scalar.p, curve
    T = V.ReadTranscript(curve, proof)
    try:
        Q, _ = V.read_plonk(T, curve, desc, k, fixed_commitments, perm_commitments, vk_repr, instances, None, circuits)
        y, v = T.challenge(), T.challenge()
        h = T.read_point()
        u = T.challenge()
        h2 = T.read_point()
    except ValueError:
        return False
    if T.pos != len(T.data):
        return False
    sets, super_points = intermediate_sets(Q)
    zdiff = [_prod([(u - z) % p for z in super_points if z not in points], p) for points, _ in sets]
    z0_inv = pow(zdiff[0], -1, p) if zdiff[0] else 0
    z_0 = _prod([(u - z) % p for z in sets[0][0]], p)
    M, r_total = None, 0
    for i, ((points, members), zd) in enumerate(zip(sets, zdiff)):
        c = pow(v, i, p) * zd % p * z0_inv % p
        inner, r_inner = None, 0
        for j, (cm, evals) in enumerate(members):
            yj = pow(y, j, p)
            inner = po.ec_add(C, inner, po.ec_mul(C, yj, cm))
            r_inner = (r_inner + yj * evaluate(interpolate(points, [evals[z] for z in points], p), u, p)) % p
        M = po.ec_add(C, M, po.ec_mul(C, c, inner))
        r_total = (r_total + c * r_inner) % p
    M = po.ec_add(C, M, po.ec_neg(C, po.ec_mul(C, r_total, g0)))
    M = po.ec_add(C, M, po.ec_neg(C, po.ec_mul(C, z_0, h)))
    M = po.ec_add(C, M, po.ec_mul(C, u, h2))
    return pr.pairing_product_is_one([(h2, s_g2), (po.ec_neg(C, M), g2)])
