"""IPACommitmentScheme on the CPU oracle's primitives: commitments, the opening argument and the IPA multiopen, prover and verifier side.
TEST INFRASTRUCTURE ONLY.

Restated from the published protocol [UPSTREAM halo2_proofs @ v2023_04_20: poly/ipa/commitment/{prover,verifier}.rs, poly/ipa/strategy.rs `GuardIPA`
(compute_s, compute_b), poly/ipa/multiopen.rs construct_intermediate_sets, poly/ipa/multiopen/{prover,verifier}.rs].  `verify_opening` reads S, xi, z,
the k rounds' (L_j, R_j, u_j) and c, f from a transcript, then checks

    P - [v] G_0 + [xi] S + sum_j ([u_j^-1] L_j + [u_j] R_j) - [c] <s, G> - [c b z] U - [f] W = 0

with one multi-exponentiation (coracle.best_multiexp, the C restatement of best_multiexp) over [G | P, S, L_j, R_j, U, W].  `open_reference` is the prover
side, commitment::create_proof, written out with naive group arithmetic (pyoracle): slow, for k <= 6 (a whole proof at k = 9 takes seconds).

No halo2 source was at hand: the item order (S; xi, z; per round L_j, R_j, u_j; c, f), the draw order (s_poly, s_poly_blind, then l_rand, r_rand per
round), the multiopen's item order and Blind::default() = Blind(F::ONE) are restated from the published protocol and from memory; parity with upstream's
bytes is unpinned.  Acceptance by these verifiers shows the device's proofs are sound for this restatement; it does not show they equal upstream's bytes.
What pins the CPU prover and the device's to each other is byte equality under one seeded scalar stream.

Points and scalars in arrays are Montgomery limbs as the library takes them ({x, y} rows of 8 u64, scalars of 4); everything else is Python integers.
"""
from __future__ import annotations

from typing import Callable, List, Sequence, Tuple

import numpy as np

import coracle as co
import pyoracle as po

# Blind::default(): the blind of the verifying key's fixed and permutation commitments and of the instance commitments.  The library's twin is
# IPA_DEFAULT_BLIND (csrc/whole_call.hpp).
DEFAULT_BLIND = 1


# ---- codecs ------------------------------------------------------------------------------------------------------------------------------------------
def enc(f: po.Field, xs: Sequence[int]) -> np.ndarray:
    """canonical integers -> len x 4 Montgomery limbs"""
    return np.frombuffer(b"".join((x % f.p * f.R % f.p).to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


def dec(f: po.Field, arr) -> List[int]:
    b = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") * f.R_inv % f.p for i in range(0, len(b), 32)]


def dec_point(curve: po.Curve, row):
    """Montgomery {x, y} row -> canonical (x, y) | None for the identity (all zero)."""
    row = np.asarray(row, dtype=np.uint64).reshape(8)
    return tuple(dec(curve.base, row)) if row.any() else None


def enc_point(curve: po.Curve, P) -> np.ndarray:
    return enc(curve.base, P).reshape(8)


# ---- commitments -------------------------------------------------------------------------------------------------------------------------------------
def commit_blinded(curve: po.Curve, bases, w_mont, scalars, blind_mont, threads: int = 4):
    """MSM(scalars, bases[:len]) + [blind] W as canonical (x, y) | None: W rides as one more base, the blind (Montgomery limbs) as one more scalar."""
    cid = po.CURVE_IDS[curve.name]
    sc = np.concatenate([np.asarray(scalars, dtype=np.uint64).reshape(-1, 4), np.asarray(blind_mont, dtype=np.uint64).reshape(1, 4)])
    bs = np.concatenate([np.asarray(bases, dtype=np.uint64).reshape(-1, 8)[:sc.shape[0] - 1], np.asarray(w_mont, dtype=np.uint64).reshape(1, 8)])
    return dec_point(curve, co.to_affine(cid, co.best_multiexp(cid, sc, bs, threads)))


def commit_reference(curve: po.Curve, g_mont, w_mont, poly: Sequence[int], blind: int):
    """ParamsIPA::commit / commit_lagrange on integers."""
    return commit_blinded(curve, g_mont, w_mont, enc(curve.scalar, poly), enc(curve.scalar, [blind]))


def blinded_key_commitments(curve: po.Curve, key: dict, w_mont, default_blind: int = DEFAULT_BLIND):
    """The verifying key's commitments under IPA: plonk_oracle.keygen's bare MSMs + [Blind::default()] W."""
    bw = po.ec_mul(curve, default_blind, dec_point(curve, w_mont))
    return ([po.ec_add(curve, c, bw) for c in key["fixed_commitments"]], [po.ec_add(curve, c, bw) for c in key["perm_commitments"]])


# ---- the opening argument ----------------------------------------------------------------------------------------------------------------------------
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


def verify_opening(T, curve: po.Curve, g_mont, u_mont, w_mont, commitment, x3: int, v: int) -> bool:
    """The rest of transcript T (verifier.ReadTranscript: a whole proof's, under way, or a fresh one over a stand-alone opening's bytes) opens
    `commitment` = P, canonical (x, y), to v at x3, and nothing follows it."""
    g_mont = np.ascontiguousarray(g_mont, dtype=np.uint64).reshape(-1, 8)
    k = g_mont.shape[0].bit_length() - 1
    p = curve.scalar.p
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
    if T.pos != len(T.data):
        return False
    us = [u for (_, _, u) in rounds]
    if any(u == 0 for u in us) or commitment is None:
        return False
    s = compute_s(us, -c, p)
    s[0] = (s[0] - v) % p
    b = compute_b(x3, us, p)
    opened = [(commitment, 1), (S, xi)] + [(L, pow(u, -1, p)) for (L, _, u) in rounds] + [(R, u) for (_, R, u) in rounds]
    bases = np.concatenate([g_mont, np.stack([enc_point(curve, P) for P, _ in opened]), np.asarray(u_mont, dtype=np.uint64).reshape(1, 8),
                            np.asarray(w_mont, dtype=np.uint64).reshape(1, 8)])
    scalars = enc(curve.scalar, s + [sc for _, sc in opened] + [-c * b * z, -fv])
    cid = po.CURVE_IDS[curve.name]
    return not co.to_affine(cid, co.best_multiexp(cid, scalars, bases, 4)).any()


def open_reference(T, curve: po.Curve, g_mont, u_mont, w_mont, poly: Sequence[int], blind: int, x3: int, draw: Callable[[int], np.ndarray]) -> bytes:
    """commitment::create_proof on integers, written to transcript T (plonk_oracle.Transcript) -> T's proof bytes so far.
    draw(count) -> count x 4 u64 Montgomery representations (prover.SeededRng.scalars)."""
    f = curve.scalar
    p = f.p
    G = [dec_point(curve, row) for row in np.asarray(g_mont, dtype=np.uint64).reshape(-1, 8)]
    U, W = dec_point(curve, u_mont), dec_point(curve, w_mont)
    n = len(G)
    k = n.bit_length() - 1
    s_poly = dec(f, draw(n))
    s_blind = dec(f, draw(1))[0]
    rands = dec(f, draw(2 * k))
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


# ---- the multiopen -----------------------------------------------------------------------------------------------------------------------------------
def construct_intermediate_sets(queries: Sequence[Tuple[object, object]]):
    """queries: (commitment key, point) in order -> (commitments, point_sets).
    commitments: [(key, set index, [point index of each of its queries, in query order])] in order of first appearance; two queries name the same
    commitment when their keys are equal.  Points are numbered in order of first appearance; a commitment's point set is the ascending set of its
    point indices; sets are numbered in order of first appearance over the commitments.  point_sets[set] = the points, ascending by point index."""
    points: List[object] = []
    keys: List[object] = []
    cpoints: List[List[int]] = []
    for key, pt in queries:
        if pt not in points:
            points.append(pt)
        pi = points.index(pt)
        if key not in keys:
            keys.append(key)
            cpoints.append([])
        cpoints[keys.index(key)].append(pi)
    sets: List[Tuple[int, ...]] = []
    commitments = []
    for key, pis in zip(keys, cpoints):
        s = tuple(sorted(set(pis)))
        if s not in sets:
            sets.append(s)
        commitments.append((key, sets.index(s), pis))
    return commitments, [[points[i] for i in s] for s in sets]


def lagrange_eval(points: Sequence[int], evals: Sequence[int], x: int, p: int) -> int:
    """The value at x of the polynomial of degree < len(points) through (points[i], evals[i])."""
    acc = 0
    for i, (xi, yi) in enumerate(zip(points, evals)):
        num, den = 1, 1
        for j, xj in enumerate(points):
            if j != i:
                num = num * (x - xj) % p
                den = den * (xi - xj) % p
        acc = (acc + yi * num % p * pow(den, -1, p)) % p
    return acc


class ProverIPA:
    """What plonk_oracle.create_proof takes as its scheme under IPA: every commitment is MSM + [blind] W, the instance columns are committed with
    Blind::default() (a test passes 0 to show the verifier's constant is live), absorbed as points and queried, and the queries are opened by
    ProverIPA::create_proof ending in open_reference on the same transcript and scalar stream."""
    query_instance = True

    def __init__(self, curve: po.Curve, srs, u_mont, w_mont, threads: int = 1, default_blind: int = DEFAULT_BLIND):
        self.curve, self.srs, self.u, self.w, self.threads, self.default_blind = curve, srs, u_mont, w_mont, threads, default_blind % curve.scalar.p

    def commit(self, bases, scalars, blind_mont):
        return commit_blinded(self.curve, bases, self.w, scalars, blind_mont, self.threads)

    def absorb_instance(self, T, values: Sequence[int], column: np.ndarray):
        T.common_point(self.commit(self.srs["g_lagrange"], column, enc(self.curve.scalar, [self.default_blind])))

    def open(self, T, Q, rng, write_commit) -> dict:
        """Q: plonk_oracle.plonk_queries' (key, point, (polynomial, blind), eval); write_commit(bases, scalars, blind_mont) -> blind.  f's blind and
        the opening's draws come from rng behind the PLONK body's."""
        f = self.curve.scalar
        p, fid, g = f.p, po.FIELD_IDS[f.name], self.srs["g"]
        n = np.asarray(g).reshape(-1, 8).shape[0]
        ev = lambda poly, pt: dec(f, co.eval_polynomial(fid, poly, enc(f, [pt]), self.threads))[0]
        x1, x2 = T.challenge(), T.challenge()
        commitments, point_sets = construct_intermediate_sets([(key, pt) for key, pt, _, _ in Q])
        item = {key: it for key, _, it, _ in Q}
        q_polys, q_blinds = [None] * len(point_sets), [0] * len(point_sets)
        for key, si, _ in commitments:
            poly, blind = item[key]
            q_polys[si] = poly if q_polys[si] is None else co.lincomb(fid, [q_polys[si], poly], enc(f, [x1, 1]))
            q_blinds[si] = (q_blinds[si] * x1 + blind) % p
        f_poly = None
        for pts, q in zip(point_sets, q_polys):
            for pt in pts:                                                                   # the remainder is dropped at every step
                q = np.concatenate([co.kate_division(fid, q, enc(f, [pt])).reshape(-1, 4)[:n - 1], np.zeros((1, 4), dtype=np.uint64)])
            f_poly = q if f_poly is None else co.lincomb(fid, [f_poly, q], enc(f, [x2, 1]))
        f_blind = write_commit(g, f_poly, rng.scalars(1)[0])
        x3 = T.challenge()
        q_evals = [ev(q, x3) for q in q_polys]
        for e in q_evals:
            T.write_scalar(e)
        x4 = T.challenge()
        p_poly, p_blind = f_poly, f_blind
        for q, b in zip(q_polys, q_blinds):
            p_poly = co.lincomb(fid, [p_poly, q], enc(f, [x4, 1]))
            p_blind = (p_blind * x4 + b) % p
        open_reference(T, self.curve, g, self.u, self.w, dec(f, p_poly), p_blind, x3, rng.scalars)
        return dict(challenges=dict(x1=x1, x2=x2, x3=x3, x4=x4), point_sets=point_sets, q_evals=q_evals)


def verify_multiopen(T, curve: po.Curve, g_mont, u_mont, w_mont, Q) -> bool:
    """VerifierIPA::verify_proof on the rest of transcript T.  Q: plonk_oracle.plonk_queries' (key, point, commitment, eval): x_1, x_2, the q
    commitments and evaluation sets, f, x_3, the q evaluations, the value of f at x_3 from the interpolants, x_4, the final commitment and value;
    then the opening argument's check."""
    p = curve.scalar.p
    x1, x2 = T.challenge(), T.challenge()
    commitments, point_sets = construct_intermediate_sets([(key, pt) for key, pt, _, _ in Q])
    item = {key: cm for key, _, cm, _ in Q}
    evals_of = {(key, pt): e for key, pt, _, e in Q}
    q_commitments = [None] * len(point_sets)
    q_eval_sets = [[0] * len(ps) for ps in point_sets]
    for key, si, _ in commitments:
        q_commitments[si] = po.ec_add(curve, po.ec_mul(curve, x1, q_commitments[si]) if q_commitments[si] is not None else None, item[key])
        for j, pt in enumerate(point_sets[si]):
            q_eval_sets[si][j] = (q_eval_sets[si][j] * x1 + evals_of[(key, pt)]) % p
    try:
        f_commitment = T.read_point()
        x3 = T.challenge()
        q_evals = [T.read_scalar() for _ in point_sets]
    except ValueError:
        return False
    f_eval = 0
    for pts, evs, u_i in zip(point_sets, q_eval_sets, q_evals):
        e = (u_i - lagrange_eval(pts, evs, x3, p)) % p
        for pt in pts:
            if (x3 - pt) % p == 0:
                return False
            e = e * pow((x3 - pt) % p, -1, p) % p
        f_eval = (f_eval * x2 + e) % p
    x4 = T.challenge()
    P, v = f_commitment, f_eval
    for qc, u_i in zip(q_commitments, q_evals):
        P = po.ec_add(curve, po.ec_mul(curve, x4, P), qc)
        v = (v * x4 + u_i) % p
    return verify_opening(T, curve, g_mont, u_mont, w_mont, P, x3, v)
