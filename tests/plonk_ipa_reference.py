"""create_proof over IPACommitmentScheme / ProverIPA on the CPU oracle's primitives -- TEST INFRASTRUCTURE ONLY.

plonk_oracle.create_proof with the blinds USED (every commitment is MSM + [blind] W), the instance columns committed and opened, and ProverIPA's
multiopen in place of GWC's [UPSTREAM halo2_proofs @ v2023_04_20: plonk/prover.rs with QUERY_INSTANCE = true, poly/ipa/multiopen/prover.rs], ending
in ipa_verifier.open_reference on the same transcript and scalar stream.  The draw order is plonk_oracle's (upstream's program order) with f's blind
and the opening's draws behind it.  Parity with upstream's bytes is unpinned (no halo2 source at hand); what pins the two provers to each other is
byte equality under one seeded stream, and both to the protocol the verifier of plonk_ipa_verifier.py.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

import coracle as co
import pyoracle as po
from ipa_verifier import open_reference
from plonk_ipa_verifier import DEFAULT_BLIND, construct_intermediate_sets, dec_point, plonk_queries
from plonk_oracle import Fld, Prog, Shape, Transcript


def create_proof(curve: po.Curve, curve_spec, srs, u_mont, w_mont, key: dict, advice_mont: np.ndarray, instances: Sequence[Sequence[int]], rng, vk_repr: int,
                 threads: int = 1, default_blind: int = DEFAULT_BLIND):
    """-> (proof bytes, trace).  srs: {"g", "g_lagrange"} (Montgomery points), u_mont / w_mont one point each; key: plonk_oracle.keygen's;
    advice_mont: (num_advice, n, 4) Montgomery; rng.scalars(count) -> (count, 4) Montgomery (consumed in upstream's order); default_blind: Blind::default()
    (a test passes 0 to show the verifier's constant is live)."""
    F = Fld(curve.scalar)
    sh: Shape = key["shape"]
    d, n, p, k, u, bf = sh.dom, sh.n, F.p, sh.k, sh.usable, sh.blinding_factors
    mm = F.m
    T = Transcript(curve)
    trace = {"commitments": [], "challenges": {}, "evals": []}
    l2c = lambda a: co.lagrange_to_coeff(F.id, a, k, mm(d.omega_inv), mm(d.ifft_divisor), threads)
    c2e = lambda a: co.coeff_to_extended(F.id, a, k, sh.ext_k, mm(d.ext_omega), mm(d.g_coset), threads)
    mul = lambda a, b: co.field_op(F.id, "mul", a, b)
    add = lambda a, b: co.field_op(F.id, "add", a, b)
    bc = lambda x: np.tile(mm(x), (n, 1))

    cid = po.CURVE_IDS[curve.name]
    w_row = np.asarray(w_mont, dtype=np.uint64).reshape(1, 8)

    def commit_blinded(bases, scalars, blind_mont):
        """MSM(scalars, bases) + [blind] W: W rides as one more base, the blind (Montgomery limbs, as drawn) as one more scalar"""
        sc = np.concatenate([np.asarray(scalars, dtype=np.uint64).reshape(-1, 4), np.asarray(blind_mont, dtype=np.uint64).reshape(1, 4)])
        return dec_point(curve_spec, co.to_affine(cid, co.best_multiexp(cid, sc, np.concatenate([bases[:sc.shape[0] - 1], w_row]), threads)))

    def write_commit(bases, scalars, blind_mont):
        P = commit_blinded(bases, scalars, blind_mont)
        T.write_point(P)
        trace["commitments"].append(P)
        return F.un(blind_mont)

    T.common_scalar(vk_repr)
    # instances
    inst_values = []
    for vals in instances:                                  # QUERY_INSTANCE = true: committed with Blind::default(), absorbed as points
        col = np.zeros((n, 4), dtype=np.uint64)
        if len(vals):
            col[:len(vals)] = F.many(vals)
        inst_values.append(col)
        P = commit_blinded(srs["g_lagrange"], col, mm(default_blind))
        assert P is not None, "cannot write points at infinity to the transcript"
        T.h.update(b"\x01" + P[0].to_bytes(32, "little") + P[1].to_bytes(32, "little"))
    inst_polys = [l2c(v) for v in inst_values]
    # advice
    advice = [np.array(advice_mont[i], dtype=np.uint64).reshape(n, 4) for i in range(sh.num_advice)]
    for a in advice:
        a[u:] = rng.scalars(n - u)
    advice_blinds = [write_commit(srs["g_lagrange"], a, b) for a, b in zip(advice, rng.scalars(sh.num_advice))]
    theta = T.challenge()
    # lookups: compress, permute
    fixed_v = key["fixed_values"]
    lookups = []
    for ins, tabs in sh.lookups:
        def compress(exprs):
            acc = np.zeros((n, 4), dtype=np.uint64)
            for e in exprs:
                pr = Prog(p)
                pr.calc(po.CALC_STORE, pr.expr(e))
                val = pr.run(F, fixed_v, advice, inst_values, None, None, None, None, None, k, 1, None, threads)
                acc = add(mul(acc, bc(theta)), val)
            return acc
        ci, ct = compress(ins), compress(tabs)
        res = co.permute_expression_pair(F.id, ci, ct, u)
        assert res is not None, "lookup input not in table (ConstraintSystemFailure)"
        pi, pt = (np.concatenate([x, np.zeros((n - u, 4), dtype=np.uint64)]) for x in res)
        pi[u:] = rng.scalars(n - u)
        pt[u:] = rng.scalars(n - u)
        bi, bt = rng.scalars(2)
        lookups.append(dict(ci=ci, ct=ct, pi=pi, pt=pt, pi_blind=write_commit(srs["g_lagrange"], pi, bi), pt_blind=write_commit(srs["g_lagrange"], pt, bt)))
    beta, gamma = T.challenge(), T.challenge()
    # permutation argument
    colvals = {"advice": advice, "fixed": fixed_v, "instance": inst_values}
    w = co.powers(F.id, mm(d.omega), mm(1), n)
    perm_z, perm_z_blinds, last_z, dcur = [], [], 1, 1
    for s in range(sh.num_sets):
        cols_s = sh.perm_columns[s * sh.chunk_len:(s + 1) * sh.chunk_len]
        den = np.tile(mm(1), (n, 1))
        for j, (ck, cidx) in enumerate(cols_s, start=s * sh.chunk_len):
            den = mul(den, add(add(mul(bc(beta), key["perm_values"][j]), bc(gamma)), colvals[ck][cidx]))
        den = co.batch_invert(F.id, den)
        modified = den
        for ck, cidx in cols_s:
            modified = mul(modified, add(add(mul(w, bc(dcur * beta % p)), bc(gamma)), colvals[ck][cidx]))
            dcur = dcur * key["delta"] % p
        z = co.field_op(F.id, "mul", co.grand_product(F.id, modified, np.tile(mm(1), (n, 1))), bc(last_z))
        z[n - bf:] = rng.scalars(bf)
        zb = rng.scalars(1)[0]
        last_z = F.un(z[u])
        perm_z.append(z)
        perm_z_blinds.append(write_commit(srs["g_lagrange"], z, zb))
    # lookup products
    for lk in lookups:
        den = mul(add(lk["pi"], bc(beta)), add(lk["pt"], bc(gamma)))
        num = mul(add(lk["ci"], bc(beta)), add(lk["ct"], bc(gamma)))
        z = co.grand_product(F.id, num, den)
        z[n - bf:] = rng.scalars(bf)
        lk["z"] = z
        lk["z_blind"] = write_commit(srs["g_lagrange"], z, rng.scalars(1)[0])
    # vanishing: random polynomial
    random_poly = rng.scalars(n)
    random_blind = write_commit(srs["g"], random_poly, rng.scalars(1)[0])
    y = T.challenge()
    # coefficient forms, cosets
    advice_polys = [l2c(a) for a in advice]
    perm_z_polys = [l2c(z) for z in perm_z]
    for lk in lookups:
        lk["pi_poly"], lk["pt_poly"], lk["z_poly"] = l2c(lk["pi"]), l2c(lk["pt"]), l2c(lk["z"])
    advice_c, inst_c = [c2e(a) for a in advice_polys], [c2e(a) for a in inst_polys]
    fixed_c = key["fixed_cosets"]
    rot_scale = sh.ext_n // n
    # evaluate_h
    pr = Prog(p)
    parts = [pr.expr(g) for g in sh.gates]
    pr.calc(po.CALC_HORNER, (po.SRC_PREVIOUS, 0, 0), (po.SRC_Y, 0, 0), parts)
    h = pr.run(F, fixed_c, advice_c, inst_c, None, None, None, None, y, sh.ext_k, rot_scale, None, threads)
    if sh.num_sets:
        cmap = {"advice": advice_c, "fixed": fixed_c, "instance": inst_c}
        pcols = [cmap[ck][ci] for ck, ci in sh.perm_columns]
        h = co.permutation_h(F.id, h, [c2e(zp) for zp in perm_z_polys], pcols, key["perm_cosets"], sh.chunk_len, -(bf + 1), key["l0"], key["l_last"], key["l_active"],
                             mm(beta), mm(gamma), mm(y), mm(key["delta"]), mm(beta * d.g_coset % p), mm(d.ext_omega), sh.ext_k, rot_scale, threads)
    for (ins, tabs), lk in zip(sh.lookups, lookups):
        pr = Prog(p)
        ci = pr.calc(po.CALC_HORNER, (po.SRC_CONSTANT, 0, 0), (po.SRC_THETA, 0, 0), [pr.expr(e) for e in ins])
        ct = pr.calc(po.CALC_HORNER, (po.SRC_CONSTANT, 0, 0), (po.SRC_THETA, 0, 0), [pr.expr(e) for e in tabs])
        pr.calc(po.CALC_MUL, pr.calc(po.CALC_ADD, ci, (po.SRC_BETA, 0, 0)), pr.calc(po.CALC_ADD, ct, (po.SRC_GAMMA, 0, 0)))
        tv = pr.run(F, fixed_c, advice_c, inst_c, None, beta, gamma, theta, None, sh.ext_k, rot_scale, None, threads)
        h = co.lookup_h(F.id, h, c2e(lk["z_poly"]), c2e(lk["pi_poly"]), c2e(lk["pt_poly"]), tv, key["l0"], key["l_last"], key["l_active"], mm(beta), mm(gamma), mm(y),
                        sh.ext_k, rot_scale, threads)
    # divide by t(X), back to coefficients, split, commit
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

    def write_eval(poly, pt):
        e = ev(poly, pt)
        T.write_scalar(e)
        trace["evals"].append(e)
        return e

    inst_evals = [write_eval(inst_polys[c], rotate(r)) for c, r in sh.instance_queries]
    adv_evals = [write_eval(advice_polys[c], rotate(r)) for c, r in sh.advice_queries]
    fix_evals = [write_eval(key["fixed_polys"][c], rotate(r)) for c, r in sh.fixed_queries]
    hfold = co.lincomb(F.id, pieces, F.many([pow(xn, i, p) for i in range(pieces_n)]))
    random_eval = write_eval(random_poly, x)
    sigma_evals = [write_eval(sp, x) for sp in key["perm_polys"]]
    x_next, x_inv, x_last = rotate(1), rotate(-1), rotate(-(bf + 1))
    pz_evals = []
    for s, zp in enumerate(perm_z_polys):
        e0, e1 = write_eval(zp, x), write_eval(zp, x_next)
        el = write_eval(zp, x_last) if s != len(perm_z_polys) - 1 else None
        pz_evals.append((e0, e1, el))
    lk_evals = []
    for lk in lookups:
        lk_evals.append((write_eval(lk["z_poly"], x), write_eval(lk["z_poly"], x_next), write_eval(lk["pi_poly"], x), write_eval(lk["pi_poly"], x_inv),
                         write_eval(lk["pt_poly"], x)))
    # queries, in upstream's order; the opened item is (polynomial, blind)
    h_blind = sum(b * pow(xn, i, p) for i, b in enumerate(h_blinds)) % p      # folded with x^n as the pieces are
    Q = plonk_queries(sh, rotate, x,
                      dict(instance=[(q, default_blind % p) for q in inst_polys], advice=list(zip(advice_polys, advice_blinds)), perm_z=list(zip(perm_z_polys, perm_z_blinds)),
                           lookup_permuted=[((lk["pi_poly"], lk["pi_blind"]), (lk["pt_poly"], lk["pt_blind"])) for lk in lookups],
                           lookup_z=[(lk["z_poly"], lk["z_blind"]) for lk in lookups], fixed=[(q, default_blind % p) for q in key["fixed_polys"]],
                           sigma=[(q, default_blind % p) for q in key["perm_polys"]], h=(hfold, h_blind), random=(random_poly, random_blind)),
                      dict(instance=inst_evals, advice=adv_evals, perm=pz_evals, lookup=lk_evals, fixed=fix_evals, sigma=sigma_evals, h=None, random=random_eval), bf)
    # ---- ProverIPA::create_proof
    x1, x2 = T.challenge(), T.challenge()
    commitments, point_sets = construct_intermediate_sets([(key_, pt) for key_, pt, _, _ in Q])
    item = {key_: it for key_, _, it, _ in Q}
    q_polys, q_blinds = [None] * len(point_sets), [0] * len(point_sets)
    for key_, si, _ in commitments:
        poly, blind = item[key_]
        q_polys[si] = poly if q_polys[si] is None else co.lincomb(F.id, [q_polys[si], poly], F.many([x1, 1]))
        q_blinds[si] = (q_blinds[si] * x1 + blind) % p
    f_poly = None
    for pts, q in zip(point_sets, q_polys):
        for pt in pts:                                                                   # the remainder is dropped at every step
            q = np.concatenate([co.kate_division(F.id, q, mm(pt)).reshape(-1, 4)[:n - 1], np.zeros((1, 4), dtype=np.uint64)])
        f_poly = q if f_poly is None else co.lincomb(F.id, [f_poly, q], F.many([x2, 1]))
    f_blind = write_commit(srs["g"], f_poly, rng.scalars(1)[0])
    x3 = T.challenge()
    q_evals = [ev(q, x3) for q in q_polys]
    for e in q_evals:
        T.write_scalar(e)
    x4 = T.challenge()
    p_poly, p_blind = f_poly, f_blind
    for q, b in zip(q_polys, q_blinds):
        p_poly = co.lincomb(F.id, [p_poly, q], F.many([x4, 1]))
        p_blind = (p_blind * x4 + b) % p
    open_reference(curve_spec, curve, srs["g"], u_mont, w_mont, F.un_many(p_poly), p_blind, x3, rng.scalars, T)
    trace["challenges"] = dict(theta=theta, beta=beta, gamma=gamma, y=y, x=x, x1=x1, x2=x2, x3=x3, x4=x4)
    trace["point_sets"], trace["q_evals"] = point_sets, q_evals
    return bytes(T.proof), trace
