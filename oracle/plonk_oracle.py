"""CPU restatement of keygen + create_proof (KZG / GWC, and IPA through ipa.py) for the parity tests.  TEST INFRASTRUCTURE ONLY: importable from
tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg; the product never imports it.

Follows [UPSTREAM halo2_proofs @ v2023_04_20: plonk/keygen.rs, plonk/prover.rs, plonk/lookup/prover.rs,
plonk/permutation/{keygen,prover}.rs, plonk/vanishing/prover.rs, plonk/evaluation.rs, poly/domain.rs,
poly/kzg/multiopen/gwc/prover.rs, transcript.rs] -- the code behind the reference's calls at
benches/delay_enc.rs:86,103 (keygen) and :123-131 (create_proof) -- written from the published algorithm (the crate is
not in the container): **parity unpinned** against upstream itself; what pins it is oracle/verifier.py accepting the
proofs (the reference's own end-to-end check, `assert!(accept)`, benches/delay_enc.rs:147-165).
One create_proof body (`create_proof_multi`) proves under every commitment scheme, over one or several circuits of a key, with or without later advice
phases, challenges and shuffle arguments; what differs between the schemes is a scheme object's (ProverGWC here, ipa.ProverIPA, tests/shplonk_oracle.py's).

The heavy steps go through oracle.c (best_multiexp, best_fft, evaluate_h's row loops, permute_expression_pair, batch
inversion) with upstream's serial / chunk-per-thread structure; everything else is Python integers.
The circuit arrives as plain data: `desc` = (num_advice, num_fixed, num_instance, gates, lookups, permutation_columns,
advice_queries, fixed_queries, instance_queries, minimum_degree) with expressions as nested tuples
("const", c) ("fixed" | "advice" | "instance", index, rotation) ("challenge", index) ("neg", e) ("sum", a, b) ("product", a, b) ("scaled", e, c).
What a constraint system has beside that tuple -- shuffle arguments, the advice columns' phases, the challenges' phases -- travels on it: `Desc`.
"""
from __future__ import annotations

import hashlib
import struct
from typing import Dict, List, Sequence, Tuple

import numpy as np

import coracle as co
import ipa
import pyoracle as po


# ---- small helpers -----------------------------------------------------------------------------------------
class Fld:
    """A scalar field with its Montgomery codec on 4 x u64 limbs."""

    def __init__(self, f: po.Field):
        self.f, self.p, self.id = f, f.p, po.FIELD_IDS[f.name]
        self.R, self.Rinv = f.R, f.R_inv

    def m(self, x: int) -> np.ndarray:
        return ipa.enc(self.f, [x])[0]

    def many(self, xs: Sequence[int]) -> np.ndarray:
        return ipa.enc(self.f, xs)

    def un(self, limbs) -> int:
        return ipa.dec(self.f, limbs)[0]

    def un_many(self, arr) -> List[int]:
        return ipa.dec(self.f, arr)


def expr_degree(e) -> int:
    k = e[0]
    if k in ("const", "challenge"): return 0
    if k in ("fixed", "advice", "instance"): return 1
    if k in ("neg", "scaled"): return expr_degree(e[1])
    if k == "sum": return max(expr_degree(e[1]), expr_degree(e[2]))
    return expr_degree(e[1]) + expr_degree(e[2])


class Desc(tuple):
    """The description tuple + the shuffles [(inputs, shuffle side)], the phase of every advice column and the phase after which each challenge is squeezed.
    A plain 10-tuple is a description with none of them."""
    shuffles, phases, challenge_phases = (), (), ()

    def __new__(cls, desc, shuffles=(), phases=(), challenge_phases=()):
        self = super().__new__(cls, tuple(desc))
        self.shuffles = tuple((tuple(i), tuple(s)) for i, s in shuffles)
        self.phases, self.challenge_phases = tuple(phases) or (0,) * self[0], tuple(challenge_phases)
        return self


def describe(cs) -> Desc:
    """the Desc of a constraint system object (description(), shuffles, phases(), challenge_phases)"""
    return Desc(cs.description(), cs.shuffles, cs.phases(), cs.challenge_phases)


class Shape:
    """ConstraintSystem::{degree, blinding_factors} and EvaluationDomain::new from the plain description."""

    def __init__(self, desc, k: int, field: po.Field):
        (self.num_advice, self.num_fixed, self.num_instance, self.gates, self.lookups, self.perm_columns, self.advice_queries, self.fixed_queries,
         self.instance_queries, self.minimum_degree) = desc
        self.shuffles, self.challenge_phases = getattr(desc, "shuffles", ()), getattr(desc, "challenge_phases", ())
        self.phases = getattr(desc, "phases", ()) or (0,) * self.num_advice
        self.num_phases = max(self.phases + (0,)) + 1
        cnt = [0] * self.num_advice
        for c, _ in self.advice_queries:
            cnt[c] += 1
        self.blinding_factors = max(3, max(cnt or [1])) + 2
        d = 3                                                  # permutation::Argument::required_degree() is 3 whether or not a column is enabled
        for ins, tabs in self.lookups:
            d = max(d, max(4, 2 + max([1] + [expr_degree(e) for e in ins]) + max([1] + [expr_degree(e) for e in tabs])))
        for ins, sides in self.shuffles:
            d = max(d, 2 + max([1] + [expr_degree(e) for e in ins]), 2 + max([1] + [expr_degree(e) for e in sides]))
        for g in self.gates:
            d = max(d, expr_degree(g))
        self.degree = max(d, self.minimum_degree)
        self.chunk_len = self.degree - 2
        self.k, self.n = k, 1 << k
        self.dom = po.Domain(field, k, self.degree)
        self.ext_k, self.ext_n = self.dom.extended_k, 1 << self.dom.extended_k
        self.usable = self.n - (self.blinding_factors + 1)
        self.num_sets = (len(self.perm_columns) + self.chunk_len - 1) // self.chunk_len if self.perm_columns else 0


# ---- expressions as GraphEvaluator programs, compiled naively (one calculation per node, no simplification) ----
class Prog:
    def __init__(self, p: int):
        self.p, self.constants, self.rotations, self.calcs, self.n_int = p, [0, 1, 2], [], [], 0

    def const(self, c: int):
        c %= self.p
        if c not in self.constants:
            self.constants.append(c)
        return (po.SRC_CONSTANT, self.constants.index(c), 0)

    def rot(self, r: int) -> int:
        if r not in self.rotations:
            self.rotations.append(r)
        return self.rotations.index(r)

    def calc(self, op, a, b=(po.SRC_CONSTANT, 0, 0), parts=()):
        self.calcs.append((op, a, b, tuple(parts), self.n_int))
        self.n_int += 1
        return (po.SRC_INTERMEDIATE, self.n_int - 1, 0)

    def expr(self, e):
        k = e[0]
        if k == "const": return self.const(e[1])
        if k == "fixed": return (po.SRC_FIXED, e[1], self.rot(e[2]))
        if k == "advice": return (po.SRC_ADVICE, e[1], self.rot(e[2]))
        if k == "instance": return (po.SRC_INSTANCE, e[1], self.rot(e[2]))
        if k == "challenge": return (po.SRC_CHALLENGE, e[1], 0)
        if k == "neg": return self.calc(po.CALC_NEGATE, self.expr(e[1]))
        if k == "sum": return self.calc(po.CALC_ADD, self.expr(e[1]), self.expr(e[2]))
        if k == "product": return self.calc(po.CALC_MUL, self.expr(e[1]), self.expr(e[2]))
        if k == "scaled": return self.calc(po.CALC_MUL, self.expr(e[1]), self.const(e[2]))
        raise ValueError(k)

    def run(self, F: Fld, fixed, advice, instance, challenges, beta, gamma, theta, y, log_rows, rot_scale, previous, threads):
        mm = lambda v: None if v is None else F.m(v)
        ch = F.many(challenges) if challenges else None
        return co.graph_evaluate(F.id, F.many(self.constants), self.rotations, self.calcs, self.n_int, fixed, advice, instance, ch, mm(beta), mm(gamma), mm(theta),
                                 mm(y), log_rows, rot_scale, previous, threads)


# ---- transcript (Blake2bWrite<_, _, Challenge255>) ------------------------------------------------------------------
class Transcript:
    def __init__(self, curve: po.Curve):
        self.curve, self.h, self.proof = curve, hashlib.blake2b(digest_size=64, person=b"Halo2-Transcript"), bytearray()

    def challenge(self) -> int:
        self.h.update(b"\x00")
        return int.from_bytes(self.h.copy().digest(), "little") % self.curve.scalar.p

    def common_scalar(self, s: int):
        self.h.update(b"\x02" + int(s).to_bytes(32, "little"))

    def write_scalar(self, s: int):
        self.common_scalar(s)
        self.proof += int(s).to_bytes(32, "little")

    def common_point(self, P):
        assert P is not None, "cannot write points at infinity to the transcript"
        self.h.update(b"\x01" + P[0].to_bytes(32, "little") + P[1].to_bytes(32, "little"))

    def write_point(self, P):
        self.common_point(P)
        b = bytearray(P[0].to_bytes(32, "little"))
        b[31] |= (P[1] & 1) << 7
        self.proof += b


# ---- SRS ------------------------------------------------------------------------------------------------------
def setup_srs(curve: po.Curve, k: int, s: int, threads: int = 1) -> Dict[str, np.ndarray]:
    """ParamsKZG::setup with the toxic waste `s` given: g[i] = [s^i]G, g_lagrange[i] = [L_i(s)]G, L_i(s) = omega^i (s^n - 1) / (n (s - omega^i))
    [UPSTREAM poly/kzg/commitment.rs setup]."""
    F, cid = Fld(curve.scalar), po.CURVE_IDS[curve.name]
    p, n = F.p, 1 << k
    omega = curve.scalar.omega(k)
    powers = co.powers(F.id, F.m(s), F.m(1), n)
    g = co.fixed_base_mul(cid, powers, threads)
    w = co.powers(F.id, F.m(omega), F.m(1), n)
    den = co.field_op(F.id, "sub", np.tile(F.m(s), (n, 1)), w)                      # s - omega^i
    den = co.batch_invert(F.id, den)
    c = (pow(s, n, p) - 1) * pow(n, -1, p) % p
    lag = co.field_op(F.id, "mul", co.field_op(F.id, "mul", den, w), np.tile(F.m(c), (n, 1)))
    gl = co.fixed_base_mul(cid, lag, threads)
    return {"k": k, "g": g, "g_lagrange": gl, "s": s}


# ---- keygen ---------------------------------------------------------------------------------------------------
def commit(curve: po.Curve, bases: np.ndarray, scalars: np.ndarray, threads: int):
    """params.commit / commit_lagrange -> affine (x, y) canonical | None."""
    cid = po.CURVE_IDS[curve.name]
    return ipa.dec_point(curve, co.to_affine(cid, co.best_multiexp(cid, scalars, bases[:scalars.shape[0]], threads)))


def keygen(curve: po.Curve, srs, desc, k: int, fixed_canonical: np.ndarray, mapping: np.ndarray, threads: int = 1) -> dict:
    """keygen_vk + keygen_pk.  fixed_canonical: (num_fixed, n, 4) canonical limbs; mapping: flat cell -> flat cell
    (column * n + row) of the permutation's cycles."""
    F = Fld(curve.scalar)
    sh = Shape(desc, k, curve.scalar)
    d, n, p = sh.dom, sh.n, F.p
    mm = F.m
    l2c = lambda a: co.lagrange_to_coeff(F.id, a, k, mm(d.omega_inv), mm(d.ifft_divisor), threads)
    c2e = lambda a: co.coeff_to_extended(F.id, a, k, sh.ext_k, mm(d.ext_omega), mm(d.g_coset), threads)
    fixed_values = [co.field_op(F.id, "to_mont", np.ascontiguousarray(fixed_canonical[i])) for i in range(sh.num_fixed)]
    fixed_polys = [l2c(v) for v in fixed_values]
    fixed_cosets = [c2e(c) for c in fixed_polys]
    fixed_commitments = [commit(curve, srs["g_lagrange"], v, threads) for v in fixed_values]
    # permutation: sigma_j(omega^i) = delta^(col') omega^(row') for the cell (col', row') that (j, i) maps to
    npc = len(sh.perm_columns)
    delta = pow(curve.scalar.gen, 1 << curve.scalar.S, p)
    w = co.powers(F.id, mm(d.omega), mm(1), n)
    ident = np.concatenate([co.field_op(F.id, "mul", w, np.tile(mm(pow(delta, j, p)), (n, 1))) for j in range(npc)]) if npc else np.zeros((0, 4), dtype=np.uint64)
    perm_values = [ident[np.asarray(mapping[j * n:(j + 1) * n])] for j in range(npc)]
    perm_polys = [l2c(v) for v in perm_values]
    perm_cosets = [c2e(c) for c in perm_polys]
    perm_commitments = [commit(curve, srs["g_lagrange"], v, threads) for v in perm_values]
    one = mm(1)
    u = sh.usable
    l0 = np.zeros((n, 4), dtype=np.uint64); l0[0] = one
    l_last = np.zeros((n, 4), dtype=np.uint64); l_last[u] = one
    l_blind = np.zeros((n, 4), dtype=np.uint64); l_blind[u + 1:] = one
    l0e, l_last_e, l_blind_e = c2e(l2c(l0)), c2e(l2c(l_last)), c2e(l2c(l_blind))
    ones = np.tile(one, (sh.ext_n, 1))
    l_active = co.field_op(F.id, "sub", ones, co.field_op(F.id, "add", l_last_e, l_blind_e))
    return dict(shape=sh, fixed_values=fixed_values, fixed_polys=fixed_polys, fixed_cosets=fixed_cosets, fixed_commitments=fixed_commitments,
                perm_values=perm_values, perm_polys=perm_polys, perm_cosets=perm_cosets, perm_commitments=perm_commitments, l0=l0e, l_last=l_last_e,
                l_active=l_active, delta=delta, desc=desc)


def vk_bytes(curve: po.Curve, key: dict, selectors: Sequence[np.ndarray] = ()) -> bytes:
    """VerifyingKey::write, SerdeFormat::RawBytes."""
    B = curve.base
    raw = lambda P: b"".join((c * B.R % B.p).to_bytes(32, "little") for c in (P if P is not None else (0, 0)))
    out = struct.pack(">I", key["shape"].k) + struct.pack(">I", len(key["fixed_commitments"]))
    out += b"".join(raw(P) for P in key["fixed_commitments"]) + b"".join(raw(P) for P in key["perm_commitments"])
    for sel in selectors:
        out += np.packbits(np.asarray(sel, dtype=bool), bitorder="little").tobytes()
    return out


def description_text(desc) -> str:
    """What transcript_repr hashes of a description: the tuple's text; with phases or challenges (description, phases, challenge phases)'s; with shuffles
    (description, shuffles, phases, challenge phases)'s."""
    shuffles, phases, challenge_phases = getattr(desc, "shuffles", ()), getattr(desc, "phases", ()), getattr(desc, "challenge_phases", ())
    if shuffles:
        return repr((tuple(desc), shuffles, phases, challenge_phases))
    if challenge_phases or any(phases):
        return repr((tuple(desc), phases, challenge_phases))
    return repr(desc)


def transcript_repr(curve: po.Curve, key: dict, selectors=()) -> int:
    body = vk_bytes(curve, key, selectors) + description_text(key["desc"]).encode()
    h = hashlib.blake2b(digest_size=64, person=b"Halo2-Verify-Key")
    h.update(struct.pack("<Q", len(body)) + body)
    return int.from_bytes(h.digest(), "little") % curve.scalar.p


class ScalarStream:
    """The checker's own reproducible source of "random" scalars (tests and bench only): numpy's PCG64 seeded with `seed`, four 64-bit outputs per
    scalar, least-significant word first, the top word masked to 61 bits -- a raw 253-bit value, taken as a Montgomery representation (below all
    four moduli).  create_proof consumes it in upstream's program order (one `Scheme::Scalar::random(&mut rng)` at a time, [UPSTREAM]
    plonk/prover.rs); the product's seeded generators (Python and C++) have to produce this same stream for the proofs to be comparable byte for byte."""

    def __init__(self, seed: int):
        self.gen = np.random.Generator(np.random.PCG64(seed))

    def scalars(self, count: int) -> np.ndarray:
        a = self.gen.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 61) - 1)
        return a


# ---- the order of things: one statement each, over circuits and shuffles ------------------------------------------------------------------------
# A commitment or evaluation of a circuit's own is keyed (name, circuit, index); what the proof has once is keyed (name, index), ("random",), ("h",).
def evaluation_order(sh: Shape, circuits: int = 1, query_instance: bool = False):
    """The evaluations a proof over `circuits` circuits writes, in upstream's order, as (key, rotation): per circuit instance (where queried) | per circuit
    advice | fixed | random | sigma | per circuit permutation products | per circuit lookups | per circuit shuffles."""
    L, S, H, last = len(sh.lookups), sh.num_sets, len(sh.shuffles), -(sh.blinding_factors + 1)
    W = [(("instance", c, col), r) for c in range(circuits) for col, r in sh.instance_queries] if query_instance else []
    W += [(("advice", c, col), r) for c in range(circuits) for col, r in sh.advice_queries]
    W += [(("fixed", col), r) for col, r in sh.fixed_queries] + [(("random",), 0)] + [(("sigma", j), 0) for j in range(len(sh.perm_columns))]
    for c in range(circuits):
        for s in range(S):
            W += [(("perm_z", c, s), 0), (("perm_z", c, s), 1)] + ([(("perm_z", c, s), last)] if s != S - 1 else [])
    for c in range(circuits):
        for l in range(L):
            W += [(("lookup_z", c, l), 0), (("lookup_z", c, l), 1), (("lookup_a", c, l), 0), (("lookup_a", c, l), -1), (("lookup_s", c, l), 0)]
    for c in range(circuits):
        for j in range(H):
            W += [(("shuffle_z", c, j), 0), (("shuffle_z", c, j), 1)]
    return W


def plonk_queries(sh: Shape, circuits: int, query_instance: bool, rotate, item, ev):
    """The opening queries in upstream's order as (key, point, item(key), ev(key, rotation)): circuit after circuit its instance (where queried), advice,
    permutation product, lookup and shuffle queries, then once fixed, sigma, h, random.  `item` gives whatever the caller opens (a commitment for a
    verifier, a (polynomial, blind) for a prover), `ev` the evaluation.  The one statement of that order: every prover and verifier lists its queries here.
    [UPSTREAM permutation::{prover,verifier}: the products at x and omega x set by set, then at omega^last x over sets.iter().rev().skip(1)]"""
    L, S, H, last = len(sh.lookups), sh.num_sets, len(sh.shuffles), -(sh.blinding_factors + 1)
    Q = []
    q = lambda key, r: Q.append((key, rotate(r), item(key), ev(key, r)))
    for c in range(circuits):
        for col, r in (sh.instance_queries if query_instance else ()):
            q(("instance", c, col), r)
        for col, r in sh.advice_queries:
            q(("advice", c, col), r)
        for s in range(S):
            q(("perm_z", c, s), 0), q(("perm_z", c, s), 1)
        for s in reversed(range(max(0, S - 1))):      # sets.iter().rev().skip(1)
            q(("perm_z", c, s), last)
        for l in range(L):
            q(("lookup_z", c, l), 0), q(("lookup_a", c, l), 0), q(("lookup_s", c, l), 0), q(("lookup_a", c, l), -1), q(("lookup_z", c, l), 1)
        for j in range(H):
            q(("shuffle_z", c, j), 0), q(("shuffle_z", c, j), 1)
    for col, r in sh.fixed_queries:
        q(("fixed", col), r)
    for j in range(len(sh.perm_columns)):
        q(("sigma", j), 0)
    q(("h",), 0), q(("random",), 0)
    return Q


def symbolic_queries(sh: Shape, circuits: int = 1, query_instance: bool = False):
    """plonk_queries with rotations for points and (key, rotation) for evaluations (None: the folded h's) -> [(key, rotation, eval)]"""
    Q = plonk_queries(sh, circuits, query_instance, lambda r: r, lambda key: key, lambda key, r: None if key == ("h",) else (key, r))
    return [(key, pt, e) for key, pt, _, e in Q]


def proof_length(sh: Shape, circuits: int, scheme: str) -> int:
    """KZG: 32 [N (A + 3 L + S + H) + 1 + pieces + groups] + 32 [N (|advice_q| + (3 S - 1 if S) + 5 L + 2 H) + |fixed_q| + 1 + npc]; SHPLONK: 2 for `groups`.
    IPA (N = 1): 32 [A + 3 L + S + H + 1 + pieces + 1 (f) + 1 (S) + 2 k] + 32 [|instance_q| + evaluations + point sets + 2]"""
    A, L, S, H, N = sh.num_advice, len(sh.lookups), sh.num_sets, len(sh.shuffles), circuits
    Q = symbolic_queries(sh, circuits, scheme == "ipa")
    evals = N * (len(sh.advice_queries) + (3 * S - 1 if S else 0) + 5 * L + 2 * H) + len(sh.fixed_queries) + 1 + len(sh.perm_columns)
    head = N * (A + 3 * L + S + H) + 1 + (sh.degree - 1)
    if scheme == "ipa":
        sets = {}
        for key, pt, _ in Q:
            sets.setdefault(key, set()).add(pt)
        return 32 * (head + 2 + 2 * sh.k) + 32 * (N * len(sh.instance_queries) + evals + len({frozenset(v) for v in sets.values()}) + 2)
    groups = 2 if scheme == "shplonk" else len({pt for _, pt, _ in Q})
    return 32 * (head + groups) + 32 * evals


# ---- create_proof ---------------------------------------------------------------------------------------------
class ProverGWC:
    """What create_proof takes as its scheme under KZG: bare MSM commitments (the blinds are drawn and dropped), instance values absorbed as scalars
    and not queried (QUERY_INSTANCE = false), GWC's multiopen.  ipa.ProverIPA is the other scheme."""
    query_instance = False
    default_blind = 0

    def __init__(self, curve: po.Curve, srs, threads: int = 1):
        self.curve, self.srs, self.threads = curve, srs, threads

    def commit(self, bases, scalars, blind_mont):
        return commit(self.curve, bases, scalars, self.threads)

    def absorb_instance(self, T, values: Sequence[int], column: np.ndarray):
        for v in values:
            T.common_scalar(v)

    def open(self, T, Q, rng, write_commit) -> dict:
        """[UPSTREAM poly/kzg/multiopen/gwc/prover.rs]: per distinct point, in order of first appearance, one witness over its queries batched with v."""
        F = Fld(self.curve.scalar)
        p = F.p
        v = T.challenge()
        groups: Dict[int, list] = {}
        for _, pt, (poly, _), e in Q:
            groups.setdefault(pt, []).append((poly, e))
        for pt, group in groups.items():
            coefs = [pow(v, i, p) for i in range(len(group))]
            eval_batch = sum(c * e for c, (_, e) in zip(coefs, group)) % p
            poly_batch = co.lincomb(F.id, [q for q, _ in group], F.many(coefs), F.m(eval_batch))
            write_commit(self.srs["g"], co.kate_division(F.id, poly_batch, F.m(pt)), F.m(0))
        return dict(challenges=dict(v=v))


def scheme_object(curve: po.Curve, srs, threads: int, scheme):
    """"gwc" (or None), "shplonk" (tests/shplonk_oracle.py's) or a scheme object as it is"""
    if scheme is None or scheme == "gwc":
        return ProverGWC(curve, srs, threads)
    if scheme == "shplonk":
        import shplonk_oracle
        return shplonk_oracle.ProverSHPLONK(curve, srs, threads)
    return scheme


def create_proof_multi(curve: po.Curve, srs, key: dict, witnesses: Sequence, instances: Sequence[Sequence[Sequence[int]]], rng, vk_repr: int, threads: int = 1,
                       scheme=None):
    """One proof over len(witnesses) circuits of one key -> (proof bytes, trace) -- trace holds every commitment, challenge and evaluation in order, and h's
    coefficients.  witnesses[c]: (num_advice, n, 4) Montgomery advice, or for a key with later phases a function (phase, challenges) -> such an array with
    the columns of phases <= phase filled; instances[c]: circuit c's instance columns.  rng.scalars(count) -> (count, 4) Montgomery, consumed in upstream's
    order (one body draws for every scheme, the multiopen's draws behind it).  scheme: "gwc" (the default), "shplonk" or a scheme object (ProverGWC,
    ipa.ProverIPA) -- how instances enter the transcript and whether they are queried, commit(bases, scalars, blind) and open(T, Q, rng, write_commit).

    [UPSTREAM plonk/prover.rs] takes `&[circuit]` and `&[instances]`: every step that concerns a witness loops over the circuits, every step that concerns the
    key or the quotient happens once.
      instances        for each circuit, for each instance column: absorbed
      advice           for each phase: for each circuit the blinding rows of the phase's columns (ascending), one blind per column, the commitments;
                       then one challenge per challenge of that phase                                                     -> theta
      lookups          for each circuit, for each lookup: the permuted pair                                               -> beta, gamma
      products         every circuit's permutation products (last_z starts again at 1) | every circuit's lookup products | every circuit's shuffle
                       products: z[0] = 1, z[i + 1] = z[i] (A[i] + gamma) / (S[i] + gamma), A and S the sides compressed with theta as a lookup's are
      vanishing        the random polynomial, once                                                                        -> y
      evaluate_h       one running value: for each circuit its gates, its permutation terms, its lookup terms, per shuffle
                       l0 (1 - z), l_last (z^2 - z), l_active (z(wX)(S + gamma) - z(X)(A + gamma)); / t(X); the pieces committed once   -> x
      evaluations      `evaluation_order`;  queries  `plonk_queries`
    Several circuits are proved under KZG only, and only where the key has one phase and no challenge."""
    scheme = scheme_object(curve, srs, threads, scheme)
    N = len(witnesses)
    F = Fld(curve.scalar)
    sh: Shape = key["shape"]
    assert N >= 1 and len(instances) == N
    assert N == 1 or not scheme.query_instance, "IPA proves one circuit"
    assert N == 1 or (sh.num_phases == 1 and not sh.challenge_phases), "later phases and challenges: one circuit"
    d, n, p, k, u, bf = sh.dom, sh.n, F.p, sh.k, sh.usable, sh.blinding_factors
    mm = F.m
    T = Transcript(curve)
    trace = {"commitments": [], "challenges": {}, "evals": []}
    l2c = lambda a: co.lagrange_to_coeff(F.id, a, k, mm(d.omega_inv), mm(d.ifft_divisor), threads)
    c2e = lambda a: co.coeff_to_extended(F.id, a, k, sh.ext_k, mm(d.ext_omega), mm(d.g_coset), threads)
    mul = lambda a, b: co.field_op(F.id, "mul", a, b)
    add = lambda a, b: co.field_op(F.id, "add", a, b)
    sub = lambda a, b: co.field_op(F.id, "sub", a, b)
    bc = lambda v, rows=n: np.tile(mm(v), (rows, 1))

    def write_commit(bases, scalars, blind_mont):
        P = scheme.commit(bases, scalars, blind_mont)
        T.write_point(P)
        trace["commitments"].append(P)
        return F.un(blind_mont)

    T.common_scalar(vk_repr)
    circuits = [dict(advice=[None] * sh.num_advice, advice_blinds=[None] * sh.num_advice) for _ in range(N)]
    # instances: circuit after circuit
    for cc, inst in zip(circuits, instances):
        assert len(inst) == sh.num_instance, "instances.len() != num_instance_columns"
        cc["inst_values"] = []
        for vals in inst:
            assert len(vals) <= u, "instance column too long"
            col = np.zeros((n, 4), dtype=np.uint64)
            if len(vals):
                col[:len(vals)] = F.many(vals)
            cc["inst_values"].append(col)
            scheme.absorb_instance(T, vals, col)
        cc["inst_polys"] = [l2c(v) for v in cc["inst_values"]]
    # advice, phase by phase: the phase's rows, its blinds, its commitments, its challenges
    challenges = [0] * len(sh.challenge_phases)
    for ph in range(sh.num_phases):
        cols = [c for c in range(sh.num_advice) if sh.phases[c] == ph]
        for cc, witness in zip(circuits, witnesses):
            advice_mont = witness(ph, list(challenges)) if callable(witness) else witness
            for c in cols:
                cc["advice"][c] = np.array(advice_mont[c], dtype=np.uint64).reshape(n, 4)
                cc["advice"][c][u:] = rng.scalars(n - u)
            for c, b in zip(cols, rng.scalars(len(cols))):
                cc["advice_blinds"][c] = write_commit(srs["g_lagrange"], cc["advice"][c], b)
        for j, q in enumerate(sh.challenge_phases):
            if q == ph:
                challenges[j] = T.challenge()
    theta = T.challenge()
    # lookups: compress, permute
    fixed_v = key["fixed_values"]

    def compress(cc, exprs):
        acc = np.zeros((n, 4), dtype=np.uint64)
        for e in exprs:
            pr = Prog(p)
            pr.calc(po.CALC_STORE, pr.expr(e))
            val = pr.run(F, fixed_v, cc["advice"], cc["inst_values"], challenges, None, None, None, None, k, 1, None, threads)
            acc = add(mul(acc, bc(theta)), val)
        return acc

    for cc in circuits:
        cc["lookups"] = []
        for ins, tabs in sh.lookups:
            ci, ct = compress(cc, ins), compress(cc, tabs)
            res = co.permute_expression_pair(F.id, ci, ct, u)
            assert res is not None, "lookup input not in table (ConstraintSystemFailure)"
            pi, pt = (np.concatenate([v, np.zeros((n - u, 4), dtype=np.uint64)]) for v in res)
            pi[u:] = rng.scalars(n - u)
            pt[u:] = rng.scalars(n - u)
            bi, bt = rng.scalars(2)
            cc["lookups"].append(dict(ci=ci, ct=ct, pi=pi, pt=pt, pi_blind=write_commit(srs["g_lagrange"], pi, bi), pt_blind=write_commit(srs["g_lagrange"], pt, bt)))
    beta, gamma = T.challenge(), T.challenge()
    # permutation products of every circuit
    w = co.powers(F.id, mm(d.omega), mm(1), n)
    for cc in circuits:
        colvals = {"advice": cc["advice"], "fixed": fixed_v, "instance": cc["inst_values"]}
        cc["perm_z"], cc["perm_z_blinds"] = [], []
        last_z, dcur = 1, 1
        for s in range(sh.num_sets):
            cols_s = sh.perm_columns[s * sh.chunk_len:(s + 1) * sh.chunk_len]
            den = np.tile(mm(1), (n, 1))
            for j, (ck, cidx) in enumerate(cols_s, start=s * sh.chunk_len):
                den = mul(den, add(add(mul(bc(beta), key["perm_values"][j]), bc(gamma)), colvals[ck][cidx]))
            modified = co.batch_invert(F.id, den)
            for ck, cidx in cols_s:
                modified = mul(modified, add(add(mul(w, bc(dcur * beta % p)), bc(gamma)), colvals[ck][cidx]))
                dcur = dcur * key["delta"] % p
            z = co.field_op(F.id, "mul", co.grand_product(F.id, modified, np.tile(mm(1), (n, 1))), bc(last_z))
            z[n - bf:] = rng.scalars(bf)
            zb = rng.scalars(1)[0]
            last_z = F.un(z[u])
            cc["perm_z"].append(z)
            cc["perm_z_blinds"].append(write_commit(srs["g_lagrange"], z, zb))
    # then the lookup products of every circuit
    for cc in circuits:
        for lk in cc["lookups"]:
            den = mul(add(lk["pi"], bc(beta)), add(lk["pt"], bc(gamma)))
            num = mul(add(lk["ci"], bc(beta)), add(lk["ct"], bc(gamma)))
            z = co.grand_product(F.id, num, den)
            z[n - bf:] = rng.scalars(bf)
            lk["z"] = z
            lk["z_blind"] = write_commit(srs["g_lagrange"], z, rng.scalars(1)[0])
    # then the shuffle products of every circuit
    for cc in circuits:
        cc["shuffles"] = []
        for ins, sides in sh.shuffles:
            z = co.grand_product(F.id, add(compress(cc, ins), bc(gamma)), add(compress(cc, sides), bc(gamma)))
            closed = F.un(z[u]) == 1
            z[n - bf:] = rng.scalars(bf)
            cc["shuffles"].append(dict(z=z, closed=closed, z_blind=write_commit(srs["g_lagrange"], z, rng.scalars(1)[0])))
    # vanishing: the random polynomial, once
    random_poly = rng.scalars(n)
    random_blind = write_commit(srs["g"], random_poly, rng.scalars(1)[0])
    y = T.challenge()
    # evaluate_h: one running value over the circuits
    fixed_c = key["fixed_cosets"]
    rot_scale = sh.ext_n // n
    h = None
    for cc in circuits:
        cc["advice_polys"] = [l2c(a) for a in cc["advice"]]
        cc["perm_z_polys"] = [l2c(z) for z in cc["perm_z"]]
        for lk in cc["lookups"]:
            lk["pi_poly"], lk["pt_poly"], lk["z_poly"] = l2c(lk["pi"]), l2c(lk["pt"]), l2c(lk["z"])
        for sf in cc["shuffles"]:
            sf["z_poly"] = l2c(sf["z"])
        advice_c, inst_c = [c2e(a) for a in cc["advice_polys"]], [c2e(a) for a in cc["inst_polys"]]
        run = lambda pr, beta, gamma, theta, y, previous: pr.run(F, fixed_c, advice_c, inst_c, challenges, beta, gamma, theta, y, sh.ext_k, rot_scale, previous, threads)
        pr = Prog(p)
        parts = [pr.expr(g) for g in sh.gates]
        pr.calc(po.CALC_HORNER, (po.SRC_PREVIOUS, 0, 0), (po.SRC_Y, 0, 0), parts)
        h = run(pr, None, None, None, y, h)
        if sh.num_sets:
            cmap = {"advice": advice_c, "fixed": fixed_c, "instance": inst_c}
            pcols = [cmap[ck][ci] for ck, ci in sh.perm_columns]
            h = co.permutation_h(F.id, h, [c2e(zp) for zp in cc["perm_z_polys"]], pcols, key["perm_cosets"], sh.chunk_len, -(bf + 1), key["l0"], key["l_last"],
                                 key["l_active"], mm(beta), mm(gamma), mm(y), mm(key["delta"]), mm(beta * d.g_coset % p), mm(d.ext_omega), sh.ext_k, rot_scale, threads)
        for (ins, tabs), lk in zip(sh.lookups, cc["lookups"]):
            pr = Prog(p)
            ci = pr.calc(po.CALC_HORNER, (po.SRC_CONSTANT, 0, 0), (po.SRC_THETA, 0, 0), [pr.expr(e) for e in ins])
            ct = pr.calc(po.CALC_HORNER, (po.SRC_CONSTANT, 0, 0), (po.SRC_THETA, 0, 0), [pr.expr(e) for e in tabs])
            pr.calc(po.CALC_MUL, pr.calc(po.CALC_ADD, ci, (po.SRC_BETA, 0, 0)), pr.calc(po.CALC_ADD, ct, (po.SRC_GAMMA, 0, 0)))
            tv = run(pr, beta, gamma, theta, None, None)
            h = co.lookup_h(F.id, h, c2e(lk["z_poly"]), c2e(lk["pi_poly"]), c2e(lk["pt_poly"]), tv, key["l0"], key["l_last"], key["l_active"], mm(beta), mm(gamma), mm(y),
                            sh.ext_k, rot_scale, threads)
        for (ins, sides), sf in zip(sh.shuffles, cc["shuffles"]):      # element-wise, on Montgomery columns of the extended domain
            def side_value(exprs):
                pr = Prog(p)
                cv = pr.calc(po.CALC_HORNER, (po.SRC_CONSTANT, 0, 0), (po.SRC_THETA, 0, 0), [pr.expr(e) for e in exprs])
                pr.calc(po.CALC_ADD, cv, (po.SRC_GAMMA, 0, 0))
                return run(pr, None, gamma, theta, None, None)
            iv, sv = side_value(ins), side_value(sides)
            z = c2e(sf["z_poly"])
            z_next = np.roll(z, -rot_scale, axis=0)
            for term, lag in ((sub(bc(1, sh.ext_n), z), key["l0"]), (sub(mul(z, z), z), key["l_last"]), (sub(mul(z_next, sv), mul(z, iv)), key["l_active"])):
                h = add(mul(h, bc(y, sh.ext_n)), mul(term, lag))
    # divide by t(X), back to coefficients, split, commit: once
    orig, step = pow(d.g_coset, n, p), pow(d.ext_omega, n, p)
    t_inv = F.many([pow((orig * pow(step, i, p) - 1) % p, -1, p) for i in range(rot_scale)])
    h = co.scale_periodic(F.id, h, t_inv)
    hc = co.extended_to_coeff(F.id, h, sh.ext_k, mm(d.ext_omega_inv), mm(d.ext_ifft_divisor), mm(d.g_coset), threads)
    pieces_n = sh.degree - 1
    pieces = [np.ascontiguousarray(hc[i * n:(i + 1) * n]) for i in range(pieces_n)]
    h_blinds = [write_commit(srs["g"], pc, b) for pc, b in zip(pieces, rng.scalars(pieces_n))]
    x = T.challenge()
    xn = pow(x, n, p)
    rotate = lambda r: x * pow(d.omega if r >= 0 else d.omega_inv, abs(r), p) % p
    ev = lambda poly, pt: F.un(co.eval_polynomial(F.id, poly, mm(pt), threads))
    # what is opened, key -> (polynomial, blind), and the evaluations, in evaluation_order
    db = scheme.default_blind
    opened = {("random",): (random_poly, random_blind)}
    opened.update({("fixed", i): (q, db) for i, q in enumerate(key["fixed_polys"])})
    opened.update({("sigma", j): (q, db) for j, q in enumerate(key["perm_polys"])})
    for c, cc in enumerate(circuits):
        opened.update({("instance", c, i): (q, db) for i, q in enumerate(cc["inst_polys"])})
        opened.update({("advice", c, i): item for i, item in enumerate(zip(cc["advice_polys"], cc["advice_blinds"]))})
        opened.update({("perm_z", c, s): item for s, item in enumerate(zip(cc["perm_z_polys"], cc["perm_z_blinds"]))})
        for l, lk in enumerate(cc["lookups"]):
            opened.update({("lookup_z", c, l): (lk["z_poly"], lk["z_blind"]), ("lookup_a", c, l): (lk["pi_poly"], lk["pi_blind"]),
                           ("lookup_s", c, l): (lk["pt_poly"], lk["pt_blind"])})
        opened.update({("shuffle_z", c, j): (sf["z_poly"], sf["z_blind"]) for j, sf in enumerate(cc["shuffles"])})
    E = {}
    for key_, r in evaluation_order(sh, N, scheme.query_instance):
        E[(key_, r)] = ev(opened[key_][0], rotate(r))
        T.write_scalar(E[(key_, r)])
        trace["evals"].append(E[(key_, r)])
    hfold = co.lincomb(F.id, pieces, F.many([pow(xn, i, p) for i in range(pieces_n)]))
    opened[("h",)] = (hfold, sum(b * pow(xn, i, p) for i, b in enumerate(h_blinds)) % p)      # the blinds folded with x^n as the pieces are
    E[(("h",), 0)] = ev(hfold, x)
    Q = plonk_queries(sh, N, scheme.query_instance, rotate, opened.__getitem__, lambda key_, r: E[(key_, r)])
    multiopen = scheme.open(T, Q, rng, write_commit)
    trace["challenges"] = dict(theta=theta, beta=beta, gamma=gamma, y=y, x=x, **multiopen.pop("challenges"))
    trace.update(multiopen)
    last = -(bf + 1)
    trace["perm_last_evals"] = [E[(("perm_z", c, s), last)] for c in range(N) for s in range(sh.num_sets - 1)]      # as written to the transcript: set 0, 1, ...
    trace["x_last_group"] = [e for _, pt, _, e in Q if pt == rotate(last)] if sh.num_sets > 1 else []      # as GWC batches them with 1, v, v^2, ...
    trace["h_coeffs"] = hc
    trace["phase_challenges"] = challenges
    trace["shuffles_closed"] = [[sf["closed"] for sf in cc["shuffles"]] for cc in circuits]
    return bytes(T.proof), trace


def create_proof(curve: po.Curve, srs, key: dict, advice_mont, instances: Sequence[Sequence[int]], rng, vk_repr: int, threads: int = 1, scheme=None):
    """create_proof_multi over one circuit: advice_mont its witness, instances its instance columns."""
    return create_proof_multi(curve, srs, key, [advice_mont], [instances], rng, vk_repr, threads, scheme)


def create_proof_ipa(curve: po.Curve, srs, u_mont, w_mont, key: dict, advice_mont, instances: Sequence[Sequence[int]], rng, vk_repr: int,
                     threads: int = 1, default_blind: int = ipa.DEFAULT_BLIND):
    """create_proof over IPACommitmentScheme / ProverIPA [UPSTREAM plonk/prover.rs with QUERY_INSTANCE = true, poly/ipa/multiopen/prover.rs].
    srs: {"g", "g_lagrange"} (Montgomery points), u_mont / w_mont one point each; key: keygen's (bare commitments; the transcript representation is
    taken over ipa.blinded_key_commitments').  The trace also holds point_sets and q_evals."""
    return create_proof(curve, srs, key, advice_mont, instances, rng, vk_repr, threads, ipa.ProverIPA(curve, srs, u_mont, w_mont, threads, default_blind))
