"""verify_proof over KZG / GWC and over IPA on Python integers.  TEST INFRASTRUCTURE ONLY.

The reference's only check of the hot path's results is `assert!(accept)` after
`verify_proof::<KZGCommitmentScheme<Bn256>, VerifierGWC<_>, Challenge255<_>, Blake2bRead<_, _, _>, SingleStrategy<_>>`
(benches/delay_enc.rs:147-165).  This restates that verifier [UPSTREAM halo2_proofs @ v2023_04_20: plonk/verifier.rs,
plonk/{lookup,permutation,vanishing}/verifier.rs, poly/kzg/multiopen/gwc/verifier.rs, poly/kzg/strategy.rs] from the published
protocol: read the proof through the transcript, recompute h(x) from the evaluations, and check the batched KZG openings
with one pairing product.  A proof is accepted only if every commitment, evaluation and quotient in it is consistent --
which is what ties the device's MSM / NTT results to the mathematics rather than to this repository's own oracles.

One PLONK part (`read_plonk`) serves both schemes.  Under IPA (`verify_proof_ipa`, plonk/verifier.rs with QUERY_INSTANCE = true) the instance columns
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
from plonk_oracle import Shape, Transcript, plonk_queries


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


def eval_expr(e, p, fixed, advice, instance) -> int:
    """Expression::evaluate with the queried evaluations: fixed / advice / instance are dicts (column, rotation) -> value."""
    k = e[0]
    if k == "const": return e[1] % p
    if k == "fixed": return fixed[(e[1], e[2])]
    if k == "advice": return advice[(e[1], e[2])]
    if k == "instance": return instance[(e[1], e[2])]
    if k == "neg": return -eval_expr(e[1], p, fixed, advice, instance) % p
    if k == "sum": return (eval_expr(e[1], p, fixed, advice, instance) + eval_expr(e[2], p, fixed, advice, instance)) % p
    if k == "product": return eval_expr(e[1], p, fixed, advice, instance) * eval_expr(e[2], p, fixed, advice, instance) % p
    if k == "scaled": return eval_expr(e[1], p, fixed, advice, instance) * e[2] % p
    raise ValueError(k)


def read_plonk(T: ReadTranscript, curve: po.Curve, desc, k: int, fixed_commitments, perm_commitments, vk_repr: int, instances: Sequence[Sequence[int]],
               instance_commitments=None):
    """The PLONK part of verify_proof: reads T up to the evaluations, rebuilds expected_h and the folded h commitment -> the opening queries
    (key, point, commitment, eval) in plonk_queries' order; raises ValueError on a malformed proof.  instance_commitments None (KZG, QUERY_INSTANCE =
    false): the instance values are absorbed as scalars and their evaluations interpolated here; given (IPA): absorbed as points, evaluations read."""
    f = curve.scalar
    p = f.p
    sh = Shape(desc, k, f)
    d, n, bf = sh.dom, sh.n, sh.blinding_factors
    T.common_scalar(vk_repr)
    if instance_commitments is None:
        for vals in instances:
            for v in vals:
                T.common_scalar(v)
    else:
        for P in instance_commitments:
            T.common_point(P)
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
    instance_evals = [T.read_scalar() for _ in sh.instance_queries] if instance_commitments is not None else []
    advice_evals = [T.read_scalar() for _ in sh.advice_queries]
    fixed_evals = [T.read_scalar() for _ in sh.fixed_queries]
    random_eval = T.read_scalar()
    sigma_evals = [T.read_scalar() for _ in sh.perm_columns]
    perm_evals = []
    for s in range(sh.num_sets):
        e0, e1 = T.read_scalar(), T.read_scalar()
        perm_evals.append((e0, e1, T.read_scalar() if s != sh.num_sets - 1 else None))
    lookup_evals = [tuple(T.read_scalar() for _ in range(5)) for _ in sh.lookups]     # product, product_next, permuted_input, permuted_input_inv, permuted_table
    xn = pow(x, n, p)
    rotate = lambda r: x * pow(d.omega if r >= 0 else d.omega_inv, abs(r), p) % p
    # l_i(x) for i in [-(bf+1), 0] (domain.l_i_range): l_i(x) = omega^i (x^n - 1) / (n (x - omega^i))
    def l_i(i):
        wi = pow(d.omega, i % n, p)
        return wi * (xn - 1) % p * pow(n * (x - wi) % p, -1, p) % p
    l_evals = [l_i(-i) for i in range(bf + 2)]            # l_0, l_{-1}, ..., l_{-(bf+1)}
    l_0, l_last = l_evals[0], l_evals[bf + 1]
    l_blind = sum(l_evals[1:bf + 1]) % p
    if instance_commitments is None:                       # interpolated by the verifier
        inst = {(c, r): sum(v * l_i(j - r) for j, v in enumerate(instances[c])) % p for (c, r) in sh.instance_queries}
    else:
        inst = {q: e for q, e in zip(sh.instance_queries, instance_evals)}
    fx = {q: e for q, e in zip(sh.fixed_queries, fixed_evals)}
    av = {q: e for q, e in zip(sh.advice_queries, advice_evals)}
    # expressions, folded with y
    exprs: List[int] = [eval_expr(g, p, fx, av, inst) for g in sh.gates]
    # permutation::verifier::Evaluated::expressions
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
    # lookup::verifier::Evaluated::expressions
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
    # h commitment folded with x^n
    h_commitment = None
    for hc in reversed(h_commitments):
        h_commitment = po.ec_add(curve, po.ec_mul(curve, xn, h_commitment) if h_commitment is not None else None, hc)
    return plonk_queries(sh, rotate, x,
                         dict(instance=instance_commitments, advice=advice_commitments, perm_z=perm_z_commitments, lookup_permuted=lookups_permuted,
                              lookup_z=lookup_z_commitments, fixed=fixed_commitments, sigma=perm_commitments, h=h_commitment, random=random_commitment),
                         dict(instance=instance_evals, advice=advice_evals, perm=perm_evals, lookup=lookup_evals, fixed=fixed_evals, sigma=sigma_evals,
                              h=expected_h, random=random_eval))


def verify_proof(curve: po.Curve, desc, k: int, fixed_commitments, perm_commitments, vk_repr: int, g0, g2, s_g2, instances: Sequence[Sequence[int]], proof: bytes) -> bool:
    p, C = curve.scalar.p, curve
    T = ReadTranscript(curve, proof)
    try:
        Q = read_plonk(T, curve, desc, k, fixed_commitments, perm_commitments, vk_repr, instances)
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
                     instances: Sequence[Sequence[int]], proof: bytes, default_blind: int = ipa.DEFAULT_BLIND) -> bool:
    """fixed_commitments, perm_commitments: ipa.blinded_key_commitments'."""
    instance_commitments = [ipa.commit_reference(curve, g_lagrange_mont, w_mont, list(vals), default_blind) for vals in instances]
    if None in instance_commitments:
        return False
    T = ReadTranscript(curve, proof)
    try:
        Q = read_plonk(T, curve, desc, k, fixed_commitments, perm_commitments, vk_repr, instances, instance_commitments)
    except ValueError:
        return False
    return ipa.verify_multiopen(T, curve, g_mont, u_mont, w_mont, Q)
