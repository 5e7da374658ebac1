"""verify_proof over KZG / GWC and over IPA on Python integers.  TEST INFRASTRUCTURE ONLY.

The reference's only check of the hot path's results is `assert!(accept)` after
`verify_proof::<KZGCommitmentScheme<Bn256>, VerifierGWC<_>, Challenge255<_>, Blake2bRead<_, _, _>, SingleStrategy<_>>`
(benches/delay_enc.rs:147-165).  This restates that verifier [UPSTREAM halo2_proofs @ v2023_04_20: plonk/verifier.rs,
plonk/{lookup,permutation,vanishing}/verifier.rs, poly/kzg/multiopen/gwc/verifier.rs, poly/kzg/strategy.rs] from the published
protocol: read the proof through the transcript, recompute h(x) from the evaluations, and check the batched KZG openings
with one pairing product.  A proof is accepted only if every commitment, evaluation and quotient in it is consistent --
which is what ties the device's MSM / NTT results to the mathematics rather than to this repository's own oracles.

One PLONK part (`read_plonk`) serves every scheme, proofs over several circuits, keys with later advice phases and challenges, and shuffle arguments.  Under IPA (`verify_proof_ipa`, plonk/verifier.rs with QUERY_INSTANCE = true) the instance columns
are committed (commit_lagrange with Blind::default()) and absorbed as points, their evaluations read first and queried first, and the queries go to
ipa.verify_multiopen.  No halo2 source was at hand for the IPA side: parity with upstream's bytes is unpinned (see ipa.py); acceptance shows a proof
is a sound proof for this restatement of the protocol.

Inputs are plain data: the circuit description tuple (see plonk_oracle.py), the verifying key's commitments as canonical
affine points, g[0], g2 and s_g2 (KZG) or g, g_lagrange, u, w as Montgomery rows (IPA).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import ipa
import pairing as pr
import pyoracle as po
from plonk_oracle import Shape, Transcript, evaluation_order, plonk_queries


def sqrt(a: int, p: int) -> Optional[int]:
    """Tonelli-Shanks: exact for every odd prime (BN254's base field is 3 mod 4, where it is a^((p + 1) / 4); the Pasta fields are 1 mod 4)."""
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


class ReadTranscript(Transcript):
    """Blake2bRead: points as x little-endian with bit 255 = sign of y; all zero = the identity, refused."""

    def __init__(self, curve: po.Curve, proof: bytes):
        super().__init__(curve)
        self.data, self.pos = bytes(proof), 0

    def _take(self) -> bytes:
        if self.pos + 32 > len(self.data):
            raise ValueError("proof too short")
        self.pos += 32
        return self.data[self.pos - 32:self.pos]

    def read_scalar(self) -> int:
        s = int.from_bytes(self._take(), "little")
        if s >= self.curve.scalar.p:
            raise ValueError("non-canonical scalar")
        self.common_scalar(s)
        return s

    def read_point(self):
        b = self._take()
        sign = b[31] >> 7
        x = int.from_bytes(b[:31] + bytes([b[31] & 0x7F]), "little")
        p = self.curve.base.p
        if x >= p:
            raise ValueError("non-canonical x")
        if x == 0 and sign == 0:
            raise ValueError("identity in proof")
        y = sqrt(x * x % p * x + self.curve.b, p)
        if y is None:
            raise ValueError("not on curve")
        if (y & 1) != sign:
            y = p - y
        self.common_point((x, y))
        return (x, y)


def eval_expr(e, p, fixed, advice, instance, challenges=()) -> int:
    """Expression::evaluate with the queried evaluations: fixed / advice / instance are dicts (column, rotation) -> value, challenges a list."""
    k = e[0]
    sub = lambda x: eval_expr(x, p, fixed, advice, instance, challenges)
    if k == "const": return e[1] % p
    if k == "fixed": return fixed[(e[1], e[2])]
    if k == "advice": return advice[(e[1], e[2])]
    if k == "instance": return instance[(e[1], e[2])]
    if k == "challenge": return challenges[e[1]]
    if k == "neg": return -sub(e[1]) % p
    if k == "sum": return (sub(e[1]) + sub(e[2])) % p
    if k == "product": return sub(e[1]) * sub(e[2]) % p
    if k == "scaled": return sub(e[1]) * e[2] % p
    raise ValueError(k)


def read_plonk(T: ReadTranscript, curve: po.Curve, desc, k: int, fixed_commitments, perm_commitments, vk_repr: int, instances, instance_commitments=None,
               circuits: Optional[int] = None):
    """The PLONK part of verify_proof: reads T up to the evaluations, squeezing each phase's challenges where its advice commitments end, rebuilds expected_h
    (every circuit's gate, permutation, lookup and shuffle expressions folded into one value with y) and the folded h commitment -> (the opening queries
    (key, point, commitment, eval) in plonk_queries' order, the phase challenges); raises ValueError on a malformed proof.
    circuits None: a proof over one circuit, `instances` its instance columns; N: over N circuits, instances[c] circuit c's columns.
    instance_commitments None (KZG, QUERY_INSTANCE = false): the instance values are absorbed as scalars and their evaluations interpolated here; given
    (IPA, one circuit): absorbed as points, evaluations read."""
    if circuits is None:
        instances, circuits = [instances], 1
    f = curve.scalar
    p = f.p
    sh = Shape(desc, k, f)
    d, n, bf, N, last = sh.dom, sh.n, sh.blinding_factors, circuits, -(sh.blinding_factors + 1)
    L, S, H = len(sh.lookups), sh.num_sets, len(sh.shuffles)
    query_instance = instance_commitments is not None
    assert N == 1 or not query_instance
    if len(instances) != N or any(len(inst) != sh.num_instance for inst in instances):
        raise ValueError("instances.len() != num_instance_columns")
    T.common_scalar(vk_repr)
    C = {("fixed", i): P for i, P in enumerate(fixed_commitments)}
    C.update({("sigma", j): P for j, P in enumerate(perm_commitments)})
    if query_instance:
        for i, P in enumerate(instance_commitments):
            T.common_point(P)
            C[("instance", 0, i)] = P
    else:
        for inst in instances:
            for vals in inst:
                for v in vals:
                    T.common_scalar(v)
    challenges = [0] * len(sh.challenge_phases)
    for ph in range(sh.num_phases):
        C.update({("advice", c, col): T.read_point() for c in range(N) for col in range(sh.num_advice) if sh.phases[col] == ph})
        for j, q in enumerate(sh.challenge_phases):
            if q == ph:
                challenges[j] = T.challenge()
    theta = T.challenge()
    for c in range(N):
        for l in range(L):
            C[("lookup_a", c, l)], C[("lookup_s", c, l)] = T.read_point(), T.read_point()
    beta, gamma = T.challenge(), T.challenge()
    for name, count in (("perm_z", S), ("lookup_z", L), ("shuffle_z", H)):      # every circuit's permutation products, then lookup, then shuffle products
        C.update({(name, c, i): T.read_point() for c in range(N) for i in range(count)})
    C[("random",)] = T.read_point()
    y = T.challenge()
    h_commitments = [T.read_point() for _ in range(sh.degree - 1)]
    x = T.challenge()
    E = {item: T.read_scalar() for item in evaluation_order(sh, N, query_instance)}
    xn = pow(x, n, p)
    rotate = lambda r: x * pow(d.omega if r >= 0 else d.omega_inv, abs(r), p) % p
    # l_i(x) for i in [-(bf+1), 0] (domain.l_i_range): l_i(x) = omega^i (x^n - 1) / (n (x - omega^i))
    def l_i(i):
        wi = pow(d.omega, i % n, p)
        return wi * (xn - 1) % p * pow(n * (x - wi) % p, -1, p) % p
    l_evals = [l_i(-i) for i in range(bf + 2)]            # l_0, l_{-1}, ..., l_{-(bf+1)}
    l_0, l_last = l_evals[0], l_evals[bf + 1]
    l_blind = sum(l_evals[1:bf + 1]) % p
    active = (1 - (l_last + l_blind)) % p
    fx = {q: E[(("fixed", q[0]), q[1])] for q in sh.fixed_queries}
    sigma_evals = [E[(("sigma", j), 0)] for j in range(len(sh.perm_columns))]
    delta = pow(f.gen, 1 << f.S, p)
    expected_h = 0
    for c in range(N):
        if query_instance:
            inst = {q: E[(("instance", c, q[0]), q[1])] for q in sh.instance_queries}
        else:                                              # interpolated by the verifier
            inst = {(col, r): sum(v * l_i(j - r) for j, v in enumerate(instances[c][col])) % p for (col, r) in sh.instance_queries}
        av = {q: E[(("advice", c, q[0]), q[1])] for q in sh.advice_queries}
        value = lambda e: eval_expr(e, p, fx, av, inst, challenges)

        def compress(es):
            acc = 0
            for e in es:
                acc = (acc * theta + value(e)) % p
            return acc
        exprs: List[int] = [value(g) for g in sh.gates]
        # permutation::verifier::Evaluated::expressions
        if S:
            pz = [tuple(E.get((("perm_z", c, s), r)) for r in (0, 1, last)) for s in range(S)]
            colval = lambda ck, ci: {"advice": av, "fixed": fx, "instance": inst}[ck][(ci, 0)]
            exprs.append(l_0 * (1 - pz[0][0]) % p)
            zl = pz[-1][0]
            exprs.append(l_last * (zl * zl - zl) % p)
            for s in range(1, S):
                exprs.append(l_0 * (pz[s][0] - pz[s - 1][2]) % p)
            for s in range(S):
                cols = sh.perm_columns[s * sh.chunk_len:(s + 1) * sh.chunk_len]
                left = pz[s][1]
                for j, (ck, ci) in enumerate(cols, start=s * sh.chunk_len):
                    left = left * (colval(ck, ci) + beta * sigma_evals[j] + gamma) % p
                right = pz[s][0]
                cur = beta * x % p * pow(delta, s * sh.chunk_len, p) % p
                for ck, ci in cols:
                    right = right * (colval(ck, ci) + cur + gamma) % p
                    cur = cur * delta % p
                exprs.append((left - right) * active % p)
        # lookup::verifier::Evaluated::expressions
        for l, (ins, tabs) in enumerate(sh.lookups):
            z0, z1, a0, am1, s0 = (E[((name, c, l), r)] for name, r in (("lookup_z", 0), ("lookup_z", 1), ("lookup_a", 0), ("lookup_a", -1), ("lookup_s", 0)))
            left = z1 * (a0 + beta) % p * (s0 + gamma) % p
            right = z0 * (compress(ins) + beta) % p * (compress(tabs) + gamma) % p
            exprs += [l_0 * (1 - z0) % p, l_last * (z0 * z0 - z0) % p, (left - right) * active % p, l_0 * (a0 - s0) % p, (a0 - s0) * (a0 - am1) % p * active % p]
        # the shuffles': l0 (1 - z), l_last (z^2 - z), l_active (z(wx)(S + gamma) - z(x)(A + gamma))
        for j, (ins, sides) in enumerate(sh.shuffles):
            z0, z1 = E[(("shuffle_z", c, j), 0)], E[(("shuffle_z", c, j), 1)]
            exprs += [l_0 * (1 - z0) % p, l_last * (z0 * z0 - z0) % p, (z1 * (compress(sides) + gamma) - z0 * (compress(ins) + gamma)) % p * active % p]
        for e in exprs:
            expected_h = (expected_h * y + e) % p
    E[(("h",), 0)] = expected_h * pow(xn - 1, -1, p) % p
    # h commitment folded with x^n
    for hc in reversed(h_commitments):
        C[("h",)] = po.ec_add(curve, po.ec_mul(curve, xn, C[("h",)]) if ("h",) in C else None, hc)
    return plonk_queries(sh, N, query_instance, rotate, C.__getitem__, lambda key, r: E[(key, r)]), challenges


def verify_proof(curve: po.Curve, desc, k: int, fixed_commitments, perm_commitments, vk_repr: int, g0, g2, s_g2, instances, proof: bytes,
                 circuits: Optional[int] = None) -> bool:
    """instances, circuits: read_plonk's"""
    p, C = curve.scalar.p, curve
    T = ReadTranscript(curve, proof)
    try:
        Q, _ = read_plonk(T, curve, desc, k, fixed_commitments, perm_commitments, vk_repr, instances, None, circuits)
    except ValueError:
        return False
    # VerifierGWC::verify_proof
    v = T.challenge()
    groups = {}                                          # by point, in order of first appearance
    for _, pt, cm, e in Q:
        groups.setdefault(pt, []).append((cm, e))
    try:
        ws = [T.read_point() for _ in groups]
    except ValueError:
        return False
    if T.pos != len(T.data):
        return False                                     # trailing bytes
    u = T.challenge()
    commitment_multi, eval_multi, witness, witness_with_aux = None, 0, None, None
    pu = 1
    for (pt, group), wi in zip(groups.items(), ws):
        cb, eb, pv = None, 0, 1
        for cm, e in group:
            cb = po.ec_add(C, cb, po.ec_mul(C, pv, cm))
            eb = (eb + pv * e) % p
            pv = pv * v % p
        commitment_multi = po.ec_add(C, commitment_multi, po.ec_mul(C, pu, cb))
        eval_multi = (eval_multi + pu * eb) % p
        witness_with_aux = po.ec_add(C, witness_with_aux, po.ec_mul(C, pu * pt % p, wi))
        witness = po.ec_add(C, witness, po.ec_mul(C, pu, wi))
        pu = pu * u % p
    right = po.ec_add(C, po.ec_add(C, witness_with_aux, commitment_multi), po.ec_neg(C, po.ec_mul(C, eval_multi, g0)))
    # e(witness, [s]G2) == e(right, G2)
    return pr.pairing_product_is_one([(witness, s_g2), (po.ec_neg(C, right), g2)])


def verify_proof_ipa(curve: po.Curve, desc, k: int, fixed_commitments, perm_commitments, vk_repr: int, g_mont, g_lagrange_mont, u_mont, w_mont,
                     instances: Sequence[Sequence[int]], proof: bytes, default_blind: int = ipa.DEFAULT_BLIND, circuits: Optional[int] = None) -> bool:
    """fixed_commitments, perm_commitments: ipa.blinded_key_commitments'.  instances, circuits: read_plonk's (one circuit)."""
    assert circuits in (None, 1), "IPA proves one circuit"
    instance_commitments = [ipa.commit_reference(curve, g_lagrange_mont, w_mont, list(vals), default_blind) for vals in (instances if circuits is None else instances[0])]
    if None in instance_commitments:
        return False
    T = ReadTranscript(curve, proof)
    try:
        Q, _ = read_plonk(T, curve, desc, k, fixed_commitments, perm_commitments, vk_repr, instances, instance_commitments, circuits)
    except ValueError:
        return False
    return ipa.verify_multiopen(T, curve, g_mont, u_mont, w_mont, Q)
