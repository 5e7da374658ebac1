"""verify_proof over IPACommitmentScheme / VerifierIPA on Python integers -- TEST INFRASTRUCTURE ONLY.

Restates upstream's verifier under IPA [UPSTREAM halo2_proofs @ v2023_04_20: plonk/verifier.rs with QUERY_INSTANCE = true,
poly/ipa/multiopen.rs construct_intermediate_sets, poly/ipa/multiopen/verifier.rs, poly/ipa/commitment/verifier.rs] from the published protocol:
the PLONK part of oracle/verifier.py with the instance columns committed (commit_lagrange with Blind::default(), absorbed as points), their
evaluations read first and queried first; then x_1, x_2, the q commitments and evaluation sets, f, x_3, the q evaluations, the value of f at x_3
from the interpolants, x_4, the final commitment and value; then the opening argument's check (ipa_verifier's, on the same transcript).

No halo2 source was at hand: item order and Blind::default() = Blind(F::ONE) are restated from memory, parity with upstream's bytes is unpinned.
Acceptance shows a proof is a sound proof for this restatement of the protocol.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

import pyoracle as po
from ipa_verifier import PastaReadTranscript, compute_b, compute_s
from plonk_oracle import Shape
from verifier import eval_expr

# Blind::default(): the blind of the verifying key's fixed and permutation commitments and of the instance commitments.  The library's twin is
# IPA_DEFAULT_BLIND (csrc/whole_call.hpp).
DEFAULT_BLIND = 1


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


def dec_point(curve_spec, row):
    row = np.asarray(row, dtype=np.uint64).reshape(8)
    return None if not row.any() else (curve_spec.base.decode(row[:4]), curve_spec.base.decode(row[4:]))


def commit_ints(co, curve_spec, bases_mont, w_mont, scalars: Sequence[int], blind: int):
    """MSM(scalars, bases[:len]) + [blind] W as a canonical (x, y) | None, through the C restatement of best_multiexp."""
    p = curve_spec.scalar.p
    bases = np.concatenate([np.asarray(bases_mont, dtype=np.uint64).reshape(-1, 8)[:len(scalars)], np.asarray(w_mont, dtype=np.uint64).reshape(1, 8)])
    sc = curve_spec.scalar.encode_many([x % p for x in list(scalars) + [blind]])
    return dec_point(curve_spec, co.to_affine(curve_spec.id, co.best_multiexp(curve_spec.id, sc, bases, 4)))


def blinded_key_commitments(curve: po.Curve, curve_spec, key: dict, w_mont, default_blind: int = DEFAULT_BLIND):
    """The verifying key's commitments under IPA: plonk_oracle.keygen's bare MSMs + [Blind::default()] W."""
    bw = po.ec_mul(curve, default_blind, dec_point(curve_spec, w_mont))
    return ([po.ec_add(curve, c, bw) for c in key["fixed_commitments"]], [po.ec_add(curve, c, bw) for c in key["perm_commitments"]])


def verify_opening_on(T, co, curve_spec, curve: po.Curve, g_mont, u_mont, w_mont, commitment, x3: int, v: int) -> bool:
    """ipa_verifier.verify_opening reading from a transcript that is already under way (a whole proof's): the same check, the same equation."""
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
    enc_b = curve_spec.base.encode
    pts, scs = [], []
    for P, sc in [(commitment, 1), (S, xi)] + [(L, pow(u, -1, p)) for (L, _, u) in rounds] + [(R, u) for (_, R, u) in rounds]:
        pts.append(np.concatenate([enc_b(P[0]), enc_b(P[1])]))
        scs.append(sc)
    bases = np.concatenate([g_mont, np.stack(pts), np.asarray(u_mont, dtype=np.uint64).reshape(1, 8), np.asarray(w_mont, dtype=np.uint64).reshape(1, 8)])
    scalars = curve_spec.scalar.encode_many([x % p for x in s + scs + [-c * b * z, -fv]])
    acc = co.to_affine(curve_spec.id, co.best_multiexp(curve_spec.id, scalars, bases, 4))
    return not np.asarray(acc).any()


def plonk_queries(sh: Shape, rotate, x, C: Dict[str, list], E: Dict[str, list], bf: int):
    """The opening queries in upstream's order (instance, advice, permutation products, lookups, fixed, sigma, h, random) as (key, point, item, eval):
    `key` names the commitment, `item` is whatever the caller opens (a commitment for the verifier, a (polynomial, blind) for the prover)."""
    x_next, x_inv, x_last = rotate(1), rotate(-1), rotate(-(bf + 1))
    Q = []
    for (c, r), e in zip(sh.instance_queries, E["instance"]):
        Q.append((("instance", c), rotate(r), C["instance"][c], e))
    for (c, r), e in zip(sh.advice_queries, E["advice"]):
        Q.append((("advice", c), rotate(r), C["advice"][c], e))
    for s, (zc, (e0, e1, _)) in enumerate(zip(C["perm_z"], E["perm"])):
        Q += [(("perm_z", s), x, zc, e0), (("perm_z", s), x_next, zc, e1)]
    for s in reversed(range(max(0, len(C["perm_z"]) - 1))):      # sets.iter().rev().skip(1)
        Q.append((("perm_z", s), x_last, C["perm_z"][s], E["perm"][s][2]))
    for l, ((ai, ti), zc, (z0, z1, a0, am1, s0)) in enumerate(zip(C["lookup_permuted"], C["lookup_z"], E["lookup"])):
        Q += [(("lookup_z", l), x, zc, z0), (("lookup_a", l), x, ai, a0), (("lookup_s", l), x, ti, s0), (("lookup_a", l), x_inv, ai, am1), (("lookup_z", l), x_next, zc, z1)]
    for (c, r), e in zip(sh.fixed_queries, E["fixed"]):
        Q.append((("fixed", c), rotate(r), C["fixed"][c], e))
    for j, (sc, e) in enumerate(zip(C["sigma"], E["sigma"])):
        Q.append((("sigma", j), x, sc, e))
    Q.append((("h",), x, C["h"], E["h"]))
    Q.append((("random",), x, C["random"], E["random"]))
    return Q


def verify_proof(co, curve: po.Curve, curve_spec, desc, k: int, fixed_commitments, perm_commitments, vk_repr: int, g_mont, g_lagrange_mont, u_mont, w_mont,
                 instances: Sequence[Sequence[int]], proof: bytes, default_blind: int = DEFAULT_BLIND) -> bool:
    f = curve.scalar
    p = f.p
    sh = Shape(desc, k, f)
    d, n, bf = sh.dom, sh.n, sh.blinding_factors
    T = PastaReadTranscript(curve, proof)
    try:
        T.common_scalar(vk_repr)
        instance_commitments = []
        for vals in instances:
            P = commit_ints(co, curve_spec, g_lagrange_mont, w_mont, list(vals), default_blind)
            if P is None:
                return False
            T.h.update(b"\x01" + P[0].to_bytes(32, "little") + P[1].to_bytes(32, "little"))      # common_point
            instance_commitments.append(P)
        advice_commitments = [T.read_point() for _ in range(sh.num_advice)]
        theta = T.challenge()
        lookups_permuted = [(T.read_point(), T.read_point()) for _ in sh.lookups]
        beta, gamma = T.challenge(), T.challenge()
        perm_z_commitments = [T.read_point() for _ in range(sh.num_sets)]
        lookup_z_commitments = [T.read_point() for _ in sh.lookups]
        random_commitment = T.read_point()
        y = T.challenge()
        h_commitments = [T.read_point() for _ in range(sh.degree - 1)]
        x = T.challenge()
        instance_evals = [T.read_scalar() for _ in sh.instance_queries]
        advice_evals = [T.read_scalar() for _ in sh.advice_queries]
        fixed_evals = [T.read_scalar() for _ in sh.fixed_queries]
        random_eval = T.read_scalar()
        sigma_evals = [T.read_scalar() for _ in sh.perm_columns]
        perm_evals = []
        for s in range(sh.num_sets):
            e0, e1 = T.read_scalar(), T.read_scalar()
            perm_evals.append((e0, e1, T.read_scalar() if s != sh.num_sets - 1 else None))
        lookup_evals = [tuple(T.read_scalar() for _ in range(5)) for _ in sh.lookups]
    except ValueError:
        return False
    xn = pow(x, n, p)
    rotate = lambda r: x * pow(d.omega if r >= 0 else d.omega_inv, abs(r), p) % p

    def l_i(i):
        wi = pow(d.omega, i % n, p)
        return wi * (xn - 1) % p * pow(n * (x - wi) % p, -1, p) % p
    l_evals = [l_i(-i) for i in range(bf + 2)]
    l_0, l_last = l_evals[0], l_evals[bf + 1]
    l_blind = sum(l_evals[1:bf + 1]) % p
    inst = {q: e for q, e in zip(sh.instance_queries, instance_evals)}
    fx = {q: e for q, e in zip(sh.fixed_queries, fixed_evals)}
    av = {q: e for q, e in zip(sh.advice_queries, advice_evals)}
    exprs: List[int] = [eval_expr(g, p, fx, av, inst) for g in sh.gates]
    if sh.num_sets:
        colval = lambda ck, ci: {"advice": av, "fixed": fx, "instance": inst}[ck][(ci, 0)]
        exprs.append(l_0 * (1 - perm_evals[0][0]) % p)
        zl = perm_evals[-1][0]
        exprs.append(l_last * (zl * zl - zl) % p)
        for s in range(1, sh.num_sets):
            exprs.append(l_0 * (perm_evals[s][0] - perm_evals[s - 1][2]) % p)
        delta = pow(f.gen, 1 << f.S, p)
        for s in range(sh.num_sets):
            cols = sh.perm_columns[s * sh.chunk_len:(s + 1) * sh.chunk_len]
            left = perm_evals[s][1]
            for j, (ck, ci) in enumerate(cols, start=s * sh.chunk_len):
                left = left * (colval(ck, ci) + beta * sigma_evals[j] + gamma) % p
            right = perm_evals[s][0]
            cur = beta * x % p * pow(delta, s * sh.chunk_len, p) % p
            for ck, ci in cols:
                right = right * (colval(ck, ci) + cur + gamma) % p
                cur = cur * delta % p
            exprs.append((left - right) * (1 - (l_last + l_blind)) % p)
    active = (1 - (l_last + l_blind)) % p
    for (ins, tabs), (z0, z1, a0, am1, s0) in zip(sh.lookups, lookup_evals):
        def compress(es):
            acc = 0
            for e in es:
                acc = (acc * theta + eval_expr(e, p, fx, av, inst)) % p
            return acc
        left = z1 * (a0 + beta) % p * (s0 + gamma) % p
        right = z0 * (compress(ins) + beta) % p * (compress(tabs) + gamma) % p
        exprs += [l_0 * (1 - z0) % p, l_last * (z0 * z0 - z0) % p, (left - right) * active % p, l_0 * (a0 - s0) % p, (a0 - s0) * (a0 - am1) % p * active % p]
    expected_h = 0
    for e in exprs:
        expected_h = (expected_h * y + e) % p
    expected_h = expected_h * pow(xn - 1, -1, p) % p
    C = curve
    h_commitment = None
    for hc in reversed(h_commitments):
        h_commitment = po.ec_add(C, po.ec_mul(C, xn, h_commitment) if h_commitment is not None else None, hc)
    Q = plonk_queries(sh, rotate, x,
                      dict(instance=instance_commitments, advice=advice_commitments, perm_z=perm_z_commitments, lookup_permuted=lookups_permuted,
                           lookup_z=lookup_z_commitments, fixed=fixed_commitments, sigma=perm_commitments, h=h_commitment, random=random_commitment),
                      dict(instance=instance_evals, advice=advice_evals, perm=perm_evals, lookup=lookup_evals, fixed=fixed_evals, sigma=sigma_evals,
                           h=expected_h, random=random_eval), bf)
    # ---- VerifierIPA::verify_proof
    x1, x2 = T.challenge(), T.challenge()
    commitments, point_sets = construct_intermediate_sets([(key, pt) for key, pt, _, _ in Q])
    item = {key: cm for key, _, cm, _ in Q}
    evals_of = {}
    for key, pt, _, e in Q:
        evals_of[(key, pt)] = e
    q_commitments = [None] * len(point_sets)
    q_eval_sets = [[0] * len(ps) for ps in point_sets]
    for key, si, _ in commitments:
        q_commitments[si] = po.ec_add(C, po.ec_mul(C, x1, q_commitments[si]) if q_commitments[si] is not None else None, item[key])
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
        P = po.ec_add(C, po.ec_mul(C, x4, P), qc)
        v = (v * x4 + u_i) % p
    return verify_opening_on(T, co, curve_spec, curve, g_mont, u_mont, w_mont, P, x3, v)
