"""ProverSHPLONK: KZG proofs with the SHPLONK multiopen, and the division by a point set's vanishing polynomial behind it.

CPU: the restatement (tests/shplonk_oracle.py: upstream's wording, R_ij subtracted and a chain of kate divisions) against its pairing verifier on the pinned
KZG chains of tests/proof_chains.py -- accepted, of the GWC proof's length less 32 x (opening points - 2), rejected after a one-bit tamper of an evaluation or of
h', and a GWC proof is no SHPLONK proof; the partial-fraction identity the device's quotient rests on, in Python integers.
GPU: dehalo_vanishing_quotient_batch_device against chained co.kate_division (block edges, the two-block carry, groups of four points, the cap of 32, eight
polynomials a call, exact zeros on top over a poisoned buffer, argument checks that launch nothing); whole proofs through native.Prover(multiopen="shplonk")
byte for byte the restatement's and accepted; the switch (IPA refuses it, back on "gwc" the GWC bytes return); batch mode over two SHPLONK provers.
The kernel's carries are kate_apply_body's over the block sums (no recursion of its own), so the longest length is the two-level 4097."""
import numpy as np
import pytest

KZG_NAMES = ["maingate_k5", "maingate_range_k9", "R9all_k6", "Rlast_k6", "instance_k5"]


def shplonk_accepts(po, c, proof, instances):
    import pairing as pr
    import shplonk_oracle as SO
    return SO.verify_proof_shplonk(po.BN254, c["desc"], c["k"], c["key"]["fixed_commitments"], c["key"]["perm_commitments"], c["rep"], (1, 2), pr.G2, c["s_g2"],
                                   [list(v) for v in instances], proof)


def shplonk_prove(po, c, instances, seed=7):
    import plonk_oracle as PO
    import shplonk_oracle as SO
    return SO.create_proof(po.BN254, c["srs"], c["key"], c["adv"], [list(v) for v in instances], PO.ScalarStream(seed), c["rep"], 8)


def opening_points(c):
    """the distinct points the chain's circuit is opened at"""
    sh = c["key"]["shape"]
    pts = {r for _, r in sh.advice_queries} | {r for _, r in sh.fixed_queries} | {0}
    if sh.num_sets or sh.lookups:
        pts.add(1)
    if sh.lookups:
        pts.add(-1)
    if sh.num_sets > 1:
        pts.add(-(sh.blinding_factors + 1))
    return len(pts)


@pytest.fixture(scope="module")
def pinned(pkg, po, co):
    """name -> (chain, instances, SHPLONK proof, trace, GWC proof) of the restatements under ScalarStream(7), computed once"""
    import proof_chains as PC
    cache = {}

    def get(name):
        if name not in cache:
            c, inst = PC.pinned_case(pkg, po, co, "kzg", name)
            proof, trace = shplonk_prove(po, c, inst)
            cache[name] = (c, inst, proof, trace, PC.prove(po, c, inst)[0])
        return cache[name]

    return get


@pytest.mark.parametrize("name", KZG_NAMES)
def test_restatement_proof_is_accepted_and_tampering_is_not(pkg, po, pinned, name):
    import proof_chains as PC
    c, inst, proof, trace, gwc = pinned(name)
    assert shplonk_accepts(po, c, proof, inst)
    assert len(proof) == len(gwc) - 32 * (opening_points(c) - 2)
    assert proof[:len(proof) - 64] == gwc[:len(proof) - 64]      # one PLONK part: the proofs differ in the multiopen alone
    assert not shplonk_accepts(po, c, PC.tampered(c, proof), inst)
    bad = bytearray(proof)
    bad[len(proof) - 32 + 3] ^= 0x10                             # one bit of h'
    assert not shplonk_accepts(po, c, bytes(bad), inst)
    assert not shplonk_accepts(po, c, proof + b"\0" * 32, inst)
    assert not shplonk_accepts(po, c, gwc, inst)
    assert not PC.accepts(po, c, proof, inst)                    # nor the other way round
    assert max(len(ps) for ps in trace["point_sets"]) == {"R9all_k6": 4, "maingate_range_k9": 3}.get(name, max(len(ps) for ps in trace["point_sets"]))


@pytest.mark.parametrize("m", [1, 2, 4, 5])
def test_partial_fractions_equal_the_chained_division(po, m):
    """sum_t w_t kate(a, z_t) = the m-deep chain of kate divisions = (a - R) / Z, R the interpolation of a's values on the points: a of 40 coefficients."""
    import shplonk_oracle as SO
    p = po.BN254_FR.p
    rng = np.random.default_rng(100 + m)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % p
    a = [rnd() for _ in range(40)]
    pts = [rnd() for _ in range(m)]
    chain = SO.chained_quotient(a, pts, p)
    assert len(chain) == 40 - m
    pf = SO.partial_fraction_quotient(a, pts, p)
    assert pf[:40 - m] == chain and not any(pf[40 - m:])
    # (a - R) = chain * Z exactly
    R = SO.interpolate(pts, [SO.evaluate(a, z, p) for z in pts], p)
    prod = chain
    for z in pts:
        prod = SO.poly_mul_linear(prod, z, p)
    assert prod == [(x - (R[i] if i < m else 0)) % p for i, x in enumerate(a)]


# ------------------------------------------------------------------------------------------------------------------------------ GPU
M_ALL = [1, 2, 3, 4, 5, 9, 32]


@pytest.fixture(scope="module")
def vq_case(pkg, co):
    """per field: eight polynomials of 4097 coefficients and 32 points; the chained references by (polynomial, length, m), computed once"""
    cache = {}

    def get(fname):
        if fname not in cache:
            f = pkg.fields.FIELDS[fname]
            cache[fname] = dict(f=f, a=np.stack([co.fill_scalars(f.id, "uniform", 4097, 900 + i) for i in range(8)]), pts=co.fill_scalars(f.id, "uniform", 32, 23), ref={})
        return cache[fname]

    return get


def _chain_ref(co, case, b, length, m):
    key = (b, length, m)
    if key not in case["ref"]:
        q = np.ascontiguousarray(case["a"][b, :length])
        for t in range(m):
            q = co.kate_division(case["f"].id, q, case["pts"][t]) if q.shape[0] > 1 else np.zeros((0, 4), dtype=np.uint64)
        case["ref"][key] = q
    return case["ref"][key]


def _run_vq(ctx, f, cols, length, point_sets):
    """-> (count, length, 4) u64 outputs over a poisoned buffer"""
    import torch
    d = ctx.upload(np.ascontiguousarray(cols[:, :length]))
    out = torch.full((len(point_sets), length, 4), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.vanishing_quotient_batch_device(f.id, [d[i].data_ptr() for i in range(len(point_sets))], length, point_sets, [out[i].data_ptr() for i in range(len(point_sets))])
    ctx.synchronize()
    return out.cpu().numpy().view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("fname", ["bn254_fr", "pasta_fp"])
@pytest.mark.parametrize("m", M_ALL)
def test_vanishing_quotient_vs_chained_division(pkg, co, ctx, vq_case, fname, m):
    """len in {m, m + 1} (a zero and a one-coefficient quotient), 2047 / 2048 / 2049 (the block edge) and 4097 (three blocks: carries): the quotient equals the chain
    of m kate divisions and the top m outputs are exactly zero over a buffer of all-ones words."""
    case = vq_case(fname)
    for length in (m, m + 1, 2047, 2048, 2049, 4097):
        got = _run_vq(ctx, case["f"], case["a"][:1], length, [case["pts"][:m]])[0]
        want = _chain_ref(co, case, 0, length, m)
        assert want.shape[0] == length - m
        assert np.array_equal(got[:length - m], want), (length, m)
        assert not got[length - m:].any(), (length, m)


@pytest.mark.gpu
@pytest.mark.parametrize("fname", ["bn254_fr", "pasta_fp"])
@pytest.mark.parametrize("length", [2049, 4097])
def test_vanishing_quotient_eight_polynomials_of_different_m(pkg, co, ctx, vq_case, fname, length):
    case = vq_case(fname)
    ms = [1, 2, 3, 4, 5, 9, 32, 4]
    got = _run_vq(ctx, case["f"], case["a"], length, [case["pts"][:m] for m in ms])
    for b, m in enumerate(ms):
        assert np.array_equal(got[b, :length - m], _chain_ref(co, case, b, length, m)), (b, m)
        assert not got[b, length - m:].any(), (b, m)


@pytest.mark.gpu
def test_vanishing_quotient_argument_checks_launch_nothing(pkg, co, ctx, vq_case):
    import ctypes as C
    import torch
    from dehalo2_amd._lib import DehaloError

    case = vq_case("bn254_fr")
    f, pts = case["f"], case["pts"]
    d = ctx.upload(np.ascontiguousarray(case["a"][:, :64]))
    out = torch.full((9, 64, 4), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptrs, outs = [d[i % 8].data_ptr() for i in range(9)], [out[i].data_ptr() for i in range(9)]
    twice = np.stack([pts[0], pts[1], pts[0]])
    more = np.concatenate([pts, pts[:1] * 0 + 5])      # 33 points
    bad = [(ptrs[:1], [pts[:0]], outs[:1]),            # m = 0
           (ptrs[:1], [more], outs[:1]),               # m = 33
           (ptrs, [pts[:2]] * 9, outs),                # count = 9
           (ptrs[:2], [pts[:2], twice], outs[:2]),     # two equal points in the second set
           ([ptrs[0], 0], [pts[:2]] * 2, outs[:2]),    # a null polynomial
           (ptrs[:1], [pts[:2]], [0]),                 # a null output
           (ptrs[:1], [pts[:2]], ptrs[:1])]            # output = input
    for a, sets, q in bad:
        with pytest.raises(DehaloError) as e:
            ctx.vanishing_quotient_batch_device(f.id, a, 64, sets, q)
        assert e.value.code == -1
    lib = ctx.lib
    one = (C.c_void_p * 1)(ptrs[0])
    assert lib.dehalo_vanishing_quotient_batch_device(ctx.handle, f.id, one, 64, None, None, one, 1, None) == -1      # null point table
    ctx.synchronize()
    assert (out.cpu().numpy() == -1).all()             # nothing was launched
    assert (d.cpu().numpy().view(np.uint64) == case["a"][:, :64]).all()
    ctx.vanishing_quotient_batch_device(f.id, ptrs[:1], 64, [pts[:32]], outs[:1])
    ctx.synchronize()


def _native_kzg(pkg, po, ctx, c):
    import pairing as pr
    import plonk_oracle as PO
    from dehalo2_amd import native
    params = native.ParamsKZG.create(ctx, pkg.fields.BN254, c["k"], c["srs"]["g"], c["srs"]["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(c["s_g2"]))
    pk = native.ProvingKey.keygen(ctx, params, c["cs"], c["fixed"], c["asm"], c.get("selectors", ()))
    assert pk.vk_bytes() == PO.vk_bytes(po.BN254, c["key"], c.get("selectors", ()))
    pk.transcript_repr = c["rep"]
    return params, pk


@pytest.fixture(scope="module")
def proof_case(pkg, po, co):
    """name -> the KZG chain with what native keygen needs (cs, fixed, asm, selectors), the instances, and `want`: the restatement's SHPLONK proof"""
    import proof_chains as PC
    import test_ipa_proof
    import test_rotations
    from dehalo2_amd import circuits
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        base, k = name.rsplit("_k", 1)
        k = int(k)
        if base == "maingate_range":
            circ = circuits.synthesize(po.BN254.scalar.p, k, True, seed=3)
            c = dict(PC.kzg_chain(po, co, circ.cs.description(), k, circ.fixed, circ.assembly.mapping, circ.advice, circ.selectors), cs=circ.cs, fixed=circ.fixed,
                     asm=circ.assembly, selectors=circ.selectors)
            inst = [[]]
        elif base == "instance":
            cs, desc, inst1, fixed, advice, asm = test_ipa_proof._instance_circuit(pkg, po, k)
            c = dict(PC.kzg_chain(po, co, desc, k, fixed, asm.mapping, advice), cs=cs, fixed=fixed, asm=asm)
            inst = [inst1]
        else:
            cs, fixed, advice, asm = test_rotations.build_circuit(pkg, base, k)
            c = dict(PC.kzg_chain(po, co, cs.description(), k, fixed, asm.mapping, advice), cs=cs, fixed=fixed, asm=asm)
            inst = []
        c["inst"] = inst
        c["want"] = shplonk_prove(po, c, inst)[0]
        cache[name] = c
        return c

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["R5_k6", "R9all_k6", "Rlast_k6", "maingate_range_k9", "instance_k5", "R7_k12"])
def test_native_shplonk_proof_equals_the_restatement(pkg, po, ctx, proof_case, name):
    """R9all: a four-point set; maingate_range: lookups and a {x, omega x, omega^last x} set; R7 at k = 12: two 2048-blocks, the quotient's carries."""
    from dehalo2_amd import native, prover
    c = proof_case(name)
    params, pk = _native_kzg(pkg, po, ctx, c)
    P = native.Prover(params, pk, multiopen="shplonk")
    proof = P.create_proof(c["adv"], c["inst"], prover.SeededRng(7)).finalize()
    want = c["want"]
    assert len(proof) == P.proof_size() == len(want)
    diff = [i // 32 for i in range(0, len(want), 32) if proof[i:i + 32] != want[i:i + 32]]
    assert not diff, "proof items differ from the restatement's: %r" % diff[:8]
    assert shplonk_accepts(po, c, proof, c["inst"])
    assert P.create_proof(c["adv"], c["inst"], prover.SeededRng(7)).finalize() == want      # the prover's buffers are clean for the next proof
    P.release(); pk.release(); params.release()


@pytest.mark.gpu
def test_the_switch(pkg, po, co, ctx, proof_case):
    """Default GWC; "shplonk" and back reproduce each scheme's bytes on one prover; proof_size follows; other values are refused; a prover over ParamsIPA has no switch."""
    import proof_chains as PC
    import test_rotations
    from dehalo2_amd import native, prover
    from dehalo2_amd._lib import DehaloError

    c = proof_case("R9all_k6")
    gwc = PC.prove(po, c, [])[0]
    params, pk = _native_kzg(pkg, po, ctx, c)
    P = native.Prover(params, pk)
    assert P.proof_size() == len(gwc) and P.create_proof(c["adv"], [], prover.SeededRng(7)).finalize() == gwc
    for _ in range(2):      # idempotent
        P.set_multiopen("shplonk")
    assert P.proof_size() == len(c["want"]) and P.create_proof(c["adv"], [], prover.SeededRng(7)).finalize() == c["want"]
    for value in (2, -1):
        with pytest.raises(DehaloError) as e:
            P.set_multiopen(value)
        assert e.value.code == -1
    assert P.proof_size() == len(c["want"])      # a refused value changes nothing
    P.set_multiopen("gwc")
    assert P.proof_size() == len(gwc) and P.create_proof(c["adv"], [], prover.SeededRng(7)).finalize() == gwc
    P.release(); pk.release(); params.release()
    # IPA
    cs, fixed, advice, asm = test_rotations.build_circuit(pkg, "R5", 6)
    ci = PC.ipa_chain(po, co, cs.description(), 6, fixed, asm.mapping, advice)
    iparams = native.ParamsIPA.create(ctx, pkg.fields.VESTA, 6, ci["srs"]["g"], ci["srs"]["g_lagrange"], ci["w"], ci["u"])
    ipk = native.ProvingKey.keygen(ctx, iparams, cs, fixed, asm, ())
    IP = native.Prover(iparams, ipk)
    size = IP.proof_size()
    for value in ("shplonk", "gwc"):
        with pytest.raises(DehaloError) as e:
            IP.set_multiopen(value)
        assert e.value.code == -5
    assert IP.proof_size() == size
    with pytest.raises(DehaloError) as e:
        native.Prover(iparams, ipk, multiopen="shplonk")
    assert e.value.code == -5
    IP.release(); ipk.release(); iparams.release()


@pytest.mark.gpu
def test_batch_mode_over_two_shplonk_provers(pkg, po, ctx, proof_case):
    from dehalo2_amd import native, prover
    c = proof_case("R5_k6")
    params, pk = _native_kzg(pkg, po, ctx, c)
    lone = native.Prover(params, pk, multiopen="shplonk")
    seeds = [7, 8, 9, 10, 11]
    alone = [lone.create_proof(c["adv"], [], prover.SeededRng(s)).finalize() for s in seeds]
    assert alone[0] == c["want"] and len(set(alone)) == len(seeds)
    ctxs = [pkg.Context(0) for _ in range(2)]
    provers = [native.Prover(params, pk, cx, multiopen="shplonk") for cx in ctxs]
    got = native.create_proofs(provers, c["adv"], [prover.SeededRng(s) for s in seeds])
    assert got == alone
    for P in provers + [lone]:
        P.release()
    for cx in ctxs:
        cx.close()
    pk.release(); params.release()
