"""One proof over several circuits of one proving key on the CPU restatements, without touching oracle/: create_proof over a list of witnesses and the
PLONK part of the verifier over a list of instance lists.  TEST INFRASTRUCTURE ONLY, beside tests/shplonk_oracle.py and tests/phased_oracle.py.

[UPSTREAM halo2_proofs @ v2023_04_20 plonk/prover.rs, plonk/verifier.rs]: create_proof takes `&[circuit]` and `&[instances]`; every step that concerns a
witness loops over the circuits, every step that concerns the key or the quotient happens once.  Written from the published loop structure (the crate is not at
hand): parity with upstream's bytes is unpinned, as for the rest of the oracle; what pins it is the restated verifiers accepting the proofs, and the single-circuit
restatement being its N = 1 case byte for byte.

  instances        for each circuit, for each instance column: absorbed (KZG: every value as a scalar)
  advice           for each circuit: blinding rows column after column, one blind per column, the commitments          -> theta
  lookups          for each circuit, for each lookup: the permuted pair                                               -> beta, gamma
  products         for each circuit its permutation products (last_z starts again at 1); THEN for each circuit its lookup products
  vanishing        the random polynomial, once                                                                        -> y
  evaluate_h       one running value: for each circuit its gates, its permutation terms, its lookup terms; / t(X); the pieces committed once   -> x
  evaluations      per circuit advice | fixed | random | sigma | per circuit permutation products | per circuit lookups      (`evaluation_order`)
  queries          per circuit (advice, permutation products, lookups) | fixed, sigma, h, random                             (`multi_queries`)

A commitment or evaluation of a circuit's own is keyed (name, circuit, index); what the proof has once keeps plonk_oracle's key."""
from __future__ import annotations

from typing import Sequence

import numpy as np

import coracle as co
import plonk_oracle as PO
import pyoracle as po
import verifier as V


def _tag(key, c):
    return (key[0], c) + tuple(key[1:])


def multi_queries(sh, rotate, x, circuit_C: Sequence[dict], circuit_E: Sequence[dict], shared_C: dict, shared_E: dict):
    """The opening queries of a proof over len(circuit_C) circuits, as plonk_queries gives them for one: circuit after circuit its advice, permutation product
    and lookup queries, then once the fixed, sigma, h and random queries.  circuit_C[c] / circuit_E[c]: advice, perm_z, lookup_permuted, lookup_z / advice,
    perm, lookup of circuit c; shared_C / shared_E: fixed, sigma, h, random."""
    none_C = dict(instance=[], advice=[], perm_z=[], lookup_permuted=[], lookup_z=[], fixed=[], sigma=[], h=None, random=None)
    none_E = dict(instance=[], advice=[], perm=[], lookup=[], fixed=[], sigma=[], h=None, random=None)
    Q = []
    for c, (C, E) in enumerate(zip(circuit_C, circuit_E)):
        own = PO.plonk_queries(sh, rotate, x, dict(none_C, **C), dict(none_E, **E))[:-2]      # (less the h and random queries plonk_queries always ends with)
        Q += [(_tag(key, c), pt, item, e) for key, pt, item, e in own]
    return Q + PO.plonk_queries(sh, rotate, x, dict(none_C, **shared_C), dict(none_E, **shared_E))


def evaluation_order(sh, circuits: int):
    """The evaluations a KZG proof over `circuits` circuits writes, in order, as (key, rotation)."""
    L, S, last = len(sh.lookups), sh.num_sets, -(sh.blinding_factors + 1)
    W = [(("advice", c, col), r) for c in range(circuits) for col, r in sh.advice_queries]
    W += [(("fixed", col), r) for col, r in sh.fixed_queries] + [(("random",), 0)] + [(("sigma", j), 0) for j in range(len(sh.perm_columns))]
    for c in range(circuits):
        for s in range(S):
            W += [(("perm_z", c, s), 0), (("perm_z", c, s), 1)] + ([(("perm_z", c, s), last)] if s != S - 1 else [])
    for c in range(circuits):
        for l in range(L):
            W += [(("lookup_z", c, l), 0), (("lookup_z", c, l), 1), (("lookup_a", c, l), 0), (("lookup_a", c, l), -1), (("lookup_s", c, l), 0)]
    return W


def symbolic_queries(sh, circuits: int):
    """multi_queries with keys for commitments, rotations for points and (key, rotation) for evaluations (None: the folded h's) -> [(key, rotation, eval)]"""
    L, S, last = len(sh.lookups), sh.num_sets, -(sh.blinding_factors + 1)
    Cs, Es = [], []
    for c in range(circuits):
        Cs.append(dict(advice=[("advice", col) for col in range(sh.num_advice)], perm_z=[("perm_z", s) for s in range(S)],
                       lookup_permuted=[(("lookup_a", l), ("lookup_s", l)) for l in range(L)], lookup_z=[("lookup_z", l) for l in range(L)]))
        Es.append(dict(advice=[(("advice", c, col), r) for col, r in sh.advice_queries],
                       perm=[tuple((("perm_z", c, s), r) for r in (0, 1, last)) for s in range(S)],
                       lookup=[((("lookup_z", c, l), 0), (("lookup_z", c, l), 1), (("lookup_a", c, l), 0), (("lookup_a", c, l), -1), (("lookup_s", c, l), 0)) for l in range(L)]))
    shared_C = dict(fixed=[("fixed", col) for col in range(sh.num_fixed)], sigma=[("sigma", j) for j in range(len(sh.perm_columns))], h=("h",), random=("random",))
    shared_E = dict(fixed=[(("fixed", col), r) for col, r in sh.fixed_queries], sigma=[(("sigma", j), 0) for j in range(len(sh.perm_columns))], h=None, random=(("random",), 0))
    return [(key, pt, e) for key, pt, _, e in multi_queries(sh, lambda r: r, 0, Cs, Es, shared_C, shared_E)]


def proof_length(sh, circuits: int, scheme: str) -> int:
    """32 [N (A + 3 L + S) + 1 + pieces + groups] + 32 [N (|advice_q| + (3 S - 1 if S else 0) + 5 L) + |fixed_q| + 1 + npc]; SHPLONK: 2 for `groups`"""
    A, L, S, N = sh.num_advice, len(sh.lookups), sh.num_sets, circuits
    groups = 2 if scheme == "shplonk" else len({pt for _, pt, _ in symbolic_queries(sh, circuits)})
    return 32 * (N * (A + 3 * L + S) + 1 + (sh.degree - 1) + groups) + 32 * (N * (len(sh.advice_queries) + (3 * S - 1 if S else 0) + 5 * L) + len(sh.fixed_queries) + 1 + len(sh.perm_columns))


def scheme_object(curve, srs, threads, scheme):
    if scheme is None or scheme == "gwc":
        return PO.ProverGWC(curve, srs, threads)
    if scheme == "shplonk":
        import shplonk_oracle
        return shplonk_oracle.ProverSHPLONK(curve, srs, threads)
    return scheme


def create_proof_multi(curve: po.Curve, srs, key: dict, advices: Sequence[np.ndarray], instances: Sequence[Sequence[Sequence[int]]], rng, vk_repr: int, threads: int = 1,
                       scheme=None):
    """-> (proof bytes, trace).  advices[c]: (num_advice, n, 4) Montgomery; instances[c]: circuit c's instance columns; scheme: "gwc" (the default), "shplonk" or a
    scheme object of plonk_oracle.create_proof's kind whose instance columns are not queried."""
    scheme = scheme_object(curve, srs, threads, scheme)
    assert not scheme.query_instance and len(advices) == len(instances) and len(advices) >= 1
    N = len(advices)
    F = PO.Fld(curve.scalar)
    sh: PO.Shape = key["shape"]
    d, n, p, k, u, bf = sh.dom, sh.n, F.p, sh.k, sh.usable, sh.blinding_factors
    mm = F.m
    T = PO.Transcript(curve)
    trace = {"commitments": [], "challenges": {}, "evals": []}
    l2c = lambda a: co.lagrange_to_coeff(F.id, a, k, mm(d.omega_inv), mm(d.ifft_divisor), threads)
    c2e = lambda a: co.coeff_to_extended(F.id, a, k, sh.ext_k, mm(d.ext_omega), mm(d.g_coset), threads)
    mul = lambda a, b: co.field_op(F.id, "mul", a, b)
    add = lambda a, b: co.field_op(F.id, "add", a, b)
    bc = lambda v: np.tile(mm(v), (n, 1))

    def write_commit(bases, scalars, blind_mont):
        P = scheme.commit(bases, scalars, blind_mont)
        T.write_point(P)
        trace["commitments"].append(P)
        return F.un(blind_mont)

    T.common_scalar(vk_repr)
    circuits = [dict() for _ in range(N)]
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
    # advice: circuit c's rows, circuit c's blinds, circuit c's commitments
    for cc, advice_mont in zip(circuits, advices):
        cc["advice"] = [np.array(advice_mont[i], dtype=np.uint64).reshape(n, 4) for i in range(sh.num_advice)]
        for a in cc["advice"]:
            a[u:] = rng.scalars(n - u)
        cc["advice_blinds"] = [write_commit(srs["g_lagrange"], a, b) for a, b in zip(cc["advice"], rng.scalars(sh.num_advice))]
    theta = T.challenge()
    # lookups: compress, permute
    fixed_v = key["fixed_values"]
    for cc in circuits:
        cc["lookups"] = []
        for ins, tabs in sh.lookups:
            def compress(exprs):
                acc = np.zeros((n, 4), dtype=np.uint64)
                for e in exprs:
                    pr = PO.Prog(p)
                    pr.calc(po.CALC_STORE, pr.expr(e))
                    val = pr.run(F, fixed_v, cc["advice"], cc["inst_values"], None, None, None, None, None, k, 1, None, threads)
                    acc = add(mul(acc, bc(theta)), val)
                return acc
            ci, ct = compress(ins), compress(tabs)
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
        advice_c, inst_c = [c2e(a) for a in cc["advice_polys"]], [c2e(a) for a in cc["inst_polys"]]
        pr = PO.Prog(p)
        parts = [pr.expr(g) for g in sh.gates]
        pr.calc(po.CALC_HORNER, (po.SRC_PREVIOUS, 0, 0), (po.SRC_Y, 0, 0), parts)
        h = pr.run(F, fixed_c, advice_c, inst_c, None, None, None, None, y, sh.ext_k, rot_scale, h, threads)
        if sh.num_sets:
            cmap = {"advice": advice_c, "fixed": fixed_c, "instance": inst_c}
            pcols = [cmap[ck][ci] for ck, ci in sh.perm_columns]
            h = co.permutation_h(F.id, h, [c2e(zp) for zp in cc["perm_z_polys"]], pcols, key["perm_cosets"], sh.chunk_len, -(bf + 1), key["l0"], key["l_last"],
                                 key["l_active"], mm(beta), mm(gamma), mm(y), mm(key["delta"]), mm(beta * d.g_coset % p), mm(d.ext_omega), sh.ext_k, rot_scale, threads)
        for (ins, tabs), lk in zip(sh.lookups, cc["lookups"]):
            pr = PO.Prog(p)
            ci = pr.calc(po.CALC_HORNER, (po.SRC_CONSTANT, 0, 0), (po.SRC_THETA, 0, 0), [pr.expr(e) for e in ins])
            ct = pr.calc(po.CALC_HORNER, (po.SRC_CONSTANT, 0, 0), (po.SRC_THETA, 0, 0), [pr.expr(e) for e in tabs])
            pr.calc(po.CALC_MUL, pr.calc(po.CALC_ADD, ci, (po.SRC_BETA, 0, 0)), pr.calc(po.CALC_ADD, ct, (po.SRC_GAMMA, 0, 0)))
            tv = pr.run(F, fixed_c, advice_c, inst_c, None, beta, gamma, theta, None, sh.ext_k, rot_scale, None, threads)
            h = co.lookup_h(F.id, h, c2e(lk["z_poly"]), c2e(lk["pi_poly"]), c2e(lk["pt_poly"]), tv, key["l0"], key["l_last"], key["l_active"], mm(beta), mm(gamma), mm(y),
                            sh.ext_k, rot_scale, threads)
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
    # the evaluations, in evaluation_order
    polys = {("random",): random_poly}
    polys.update({("fixed", i): q for i, q in enumerate(key["fixed_polys"])})
    polys.update({("sigma", j): q for j, q in enumerate(key["perm_polys"])})
    for c, cc in enumerate(circuits):
        polys.update({("advice", c, i): q for i, q in enumerate(cc["advice_polys"])})
        polys.update({("perm_z", c, s): q for s, q in enumerate(cc["perm_z_polys"])})
        for l, lk in enumerate(cc["lookups"]):
            polys.update({("lookup_z", c, l): lk["z_poly"], ("lookup_a", c, l): lk["pi_poly"], ("lookup_s", c, l): lk["pt_poly"]})
    E = {}
    for key_, r in evaluation_order(sh, N):
        E[(key_, r)] = ev(polys[key_], rotate(r))
        T.write_scalar(E[(key_, r)])
        trace["evals"].append(E[(key_, r)])
    hfold = co.lincomb(F.id, pieces, F.many([pow(xn, i, p) for i in range(pieces_n)]))
    h_blind = sum(b * pow(xn, i, p) for i, b in enumerate(h_blinds)) % p
    db, last = scheme.default_blind, -(bf + 1)
    Cs, Es = [], []
    for c, cc in enumerate(circuits):
        Cs.append(dict(advice=list(zip(cc["advice_polys"], cc["advice_blinds"])), perm_z=list(zip(cc["perm_z_polys"], cc["perm_z_blinds"])),
                       lookup_permuted=[((lk["pi_poly"], lk["pi_blind"]), (lk["pt_poly"], lk["pt_blind"])) for lk in cc["lookups"]],
                       lookup_z=[(lk["z_poly"], lk["z_blind"]) for lk in cc["lookups"]]))
        Es.append(dict(advice=[E[(("advice", c, col), r)] for col, r in sh.advice_queries],
                       perm=[(E[(("perm_z", c, s), 0)], E[(("perm_z", c, s), 1)], E.get((("perm_z", c, s), last))) for s in range(sh.num_sets)],
                       lookup=[(E[(("lookup_z", c, l), 0)], E[(("lookup_z", c, l), 1)], E[(("lookup_a", c, l), 0)], E[(("lookup_a", c, l), -1)], E[(("lookup_s", c, l), 0)])
                               for l in range(len(sh.lookups))]))
    shared_C = dict(fixed=[(q, db) for q in key["fixed_polys"]], sigma=[(q, db) for q in key["perm_polys"]], h=(hfold, h_blind), random=(random_poly, random_blind))
    shared_E = dict(fixed=[E[(("fixed", col), r)] for col, r in sh.fixed_queries], sigma=[E[(("sigma", j), 0)] for j in range(len(sh.perm_columns))], h=ev(hfold, x),
                    random=E[(("random",), 0)])
    Q = multi_queries(sh, rotate, x, Cs, Es, shared_C, shared_E)
    opened = scheme.open(T, Q, rng, write_commit)
    trace["challenges"] = dict(theta=theta, beta=beta, gamma=gamma, y=y, x=x, **opened.pop("challenges"))
    trace.update(opened)
    trace["h_coeffs"] = hc
    return bytes(T.proof), trace


def read_plonk_multi(T, curve: po.Curve, desc, k: int, fixed_commitments, perm_commitments, vk_repr: int, instances: Sequence[Sequence[Sequence[int]]],
                     instance_commitments=None):
    """verifier.read_plonk for a proof over len(instances) circuits: instances[c] are circuit c's instance columns.  KZG only (the instance values are absorbed as
    scalars and their evaluations interpolated here)."""
    assert instance_commitments is None
    f = curve.scalar
    p = f.p
    sh = PO.Shape(desc, k, f)
    d, n, bf = sh.dom, sh.n, sh.blinding_factors
    N = len(instances)
    T.common_scalar(vk_repr)
    for inst in instances:
        if len(inst) != sh.num_instance:
            raise ValueError("instances.len() != num_instance_columns")
        for vals in inst:
            for v in vals:
                T.common_scalar(v)
    advice_commitments = [[T.read_point() for _ in range(sh.num_advice)] for _ in range(N)]
    theta = T.challenge()
    lookups_permuted = [[(T.read_point(), T.read_point()) for _ in sh.lookups] for _ in range(N)]
    beta, gamma = T.challenge(), T.challenge()
    perm_z_commitments = [[T.read_point() for _ in range(sh.num_sets)] for _ in range(N)]
    lookup_z_commitments = [[T.read_point() for _ in sh.lookups] for _ in range(N)]
    random_commitment = T.read_point()
    y = T.challenge()
    h_commitments = [T.read_point() for _ in range(sh.degree - 1)]
    x = T.challenge()
    E = {item: T.read_scalar() for item in evaluation_order(sh, N)}
    last = -(bf + 1)
    xn = pow(x, n, p)
    rotate = lambda r: x * pow(d.omega if r >= 0 else d.omega_inv, abs(r), p) % p

    def l_i(i):
        wi = pow(d.omega, i % n, p)
        return wi * (xn - 1) % p * pow(n * (x - wi) % p, -1, p) % p
    l_evals = [l_i(-i) for i in range(bf + 2)]
    l_0, l_last = l_evals[0], l_evals[bf + 1]
    l_blind = sum(l_evals[1:bf + 1]) % p
    active = (1 - (l_last + l_blind)) % p
    fx = {q: E[(("fixed", q[0]), q[1])] for q in sh.fixed_queries}
    sigma_evals = [E[(("sigma", j), 0)] for j in range(len(sh.perm_columns))]
    delta = pow(f.gen, 1 << f.S, p)
    expected_h = 0                                                  # every circuit's expressions folded into one value with y
    Cs, Es = [], []
    for c in range(N):
        inst = {(col, r): sum(v * l_i(j - r) for j, v in enumerate(instances[c][col])) % p for (col, r) in sh.instance_queries}
        av = {q: E[(("advice", c, q[0]), q[1])] for q in sh.advice_queries}
        perm_evals = [(E[(("perm_z", c, s), 0)], E[(("perm_z", c, s), 1)], E.get((("perm_z", c, s), last))) for s in range(sh.num_sets)]
        lookup_evals = [(E[(("lookup_z", c, l), 0)], E[(("lookup_z", c, l), 1)], E[(("lookup_a", c, l), 0)], E[(("lookup_a", c, l), -1)], E[(("lookup_s", c, l), 0)])
                        for l in range(len(sh.lookups))]
        exprs = [V.eval_expr(g, p, fx, av, inst) for g in sh.gates]
        if sh.num_sets:
            colval = lambda ck, ci: {"advice": av, "fixed": fx, "instance": inst}[ck][(ci, 0)]
            exprs.append(l_0 * (1 - perm_evals[0][0]) % p)
            zl = perm_evals[-1][0]
            exprs.append(l_last * (zl * zl - zl) % p)
            for s in range(1, sh.num_sets):
                exprs.append(l_0 * (perm_evals[s][0] - perm_evals[s - 1][2]) % p)
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
                exprs.append((left - right) * active % p)
        for (ins, tabs), (z0, z1, a0, am1, s0) in zip(sh.lookups, lookup_evals):
            def compress(es):
                acc = 0
                for e in es:
                    acc = (acc * theta + V.eval_expr(e, p, fx, av, inst)) % p
                return acc
            left = z1 * (a0 + beta) % p * (s0 + gamma) % p
            right = z0 * (compress(ins) + beta) % p * (compress(tabs) + gamma) % p
            exprs += [l_0 * (1 - z0) % p, l_last * (z0 * z0 - z0) % p, (left - right) * active % p, l_0 * (a0 - s0) % p, (a0 - s0) * (a0 - am1) % p * active % p]
        for e in exprs:
            expected_h = (expected_h * y + e) % p
        Cs.append(dict(advice=advice_commitments[c], perm_z=perm_z_commitments[c], lookup_permuted=lookups_permuted[c], lookup_z=lookup_z_commitments[c]))
        Es.append(dict(advice=[av[q] for q in sh.advice_queries], perm=perm_evals, lookup=lookup_evals))
    expected_h = expected_h * pow(xn - 1, -1, p) % p
    h_commitment = None
    for hc in reversed(h_commitments):
        h_commitment = po.ec_add(curve, po.ec_mul(curve, xn, h_commitment) if h_commitment is not None else None, hc)
    return multi_queries(sh, rotate, x, Cs, Es, dict(fixed=fixed_commitments, sigma=perm_commitments, h=h_commitment, random=random_commitment),
                         dict(fixed=[fx[q] for q in sh.fixed_queries], sigma=sigma_evals, h=expected_h, random=E[(("random",), 0)]))


def accepts(po_, c, proof, instances, scheme="gwc"):
    """the restated verifier of `scheme` on a proof over len(instances) circuits of chain c (tests/proof_chains.py), read_plonk_multi patched in"""
    import pairing as pr
    import shplonk_oracle
    from phased_oracle import patched
    verify = shplonk_oracle.verify_proof_shplonk if scheme == "shplonk" else V.verify_proof
    instances = [[list(v) for v in inst] for inst in instances]
    with patched(V, "read_plonk", read_plonk_multi):
        return verify(po_.BN254, c["desc"], c["k"], c["key"]["fixed_commitments"], c["key"]["perm_commitments"], c["rep"], (1, 2), pr.G2, c["s_g2"], instances, proof)
