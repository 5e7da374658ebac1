"""One proof over several circuits of one proving key (KZG: GWC and SHPLONK): the oracle's create_proof_multi against the pinned single-circuit proofs and the
restated verifiers (CPU), the opening plan's circuit dimension against the restatement's lists (CPU, a sanitized program of its own), and whole proofs through
native.Prover(num_circuits=N).create_proof_multi against the restatement byte for byte (GPU).

Circuits 1, 2, ... of a case take other satisfying witnesses of the same key: the maingate circuits' witness moved along a direction its gate allows (another seed of
circuits.synthesize changes the fixed columns too), other start values for the rotation circuits' recurrences, other instance values for instance_k5."""
import json
import os
import subprocess

import numpy as np
import pytest

KZG_CHAINS = ("maingate_k5", "maingate_range_k9", "R9all_k6", "Rlast_k6", "instance_k5")
SCHEMES = ("gwc", "shplonk")
MAX_N = 4      # (the fourth witness: the lookup chain's case beyond the batched kernels' tiles)
SEED = 7


# ---- witnesses ------------------------------------------------------------------------------------------------------------------------------------------
def _rotation_witness(pkg, name, k, variant):
    """tests/test_rotations.py build_circuit's advice with other start values (variant 0: its own)"""
    import test_rotations as TR
    cs, fixed, advice, asm = TR.build_circuit(pkg, name, k)
    if variant == 0:
        return advice
    bf, lo, hi = cs.blinding_factors(), TR.Q_LO, TR.Q_HI
    a = [0] * 48
    a[lo], a[lo + 1] = 1 + 2 * variant, 2 + 5 * variant
    for r in range(lo, hi):
        a[r + 2] = a[r + 1] + a[r]
    b = [0] * 48
    if name == "Rlast":
        for r in range(0, 40):
            b[r] = 3 + 7 * variant + r % (bf + 1)
    else:
        for r in range(lo - 3, lo + 5):
            b[r] = 11 + 13 * variant + r
        for r in range(lo, hi):
            b[r + 5] = 2 * b[r - 3]
    b[40] = a[lo]
    out = np.zeros_like(advice)
    out[0, :48, 0], out[1, :48, 0] = a, b
    return out


def _maingate_witness(circ, p, variant):
    """Another satisfying witness of circuits.synthesize's circuit, its fixed columns and permutation untouched (another seed changes both): on an arithmetic row
    a b + c - e + s_d d + s_next e(next) + constant = 0, so c and e move together, where the row has no c d term, the row above does not read this e and
    neither cell is tied by a copy constraint.  The lookups' selectors are off on such rows."""
    from dehalo2_amd import plonk
    n = 1 << circ.k
    col = lambda i: [int(circ.fixed[i, r, 0]) | int(circ.fixed[i, r, 1]) << 64 | int(circ.fixed[i, r, 2]) << 128 | int(circ.fixed[i, r, 3]) << 192 for r in range(n)]
    mab, mcd, nxt, sc, se = col(plonk.MG_MUL_AB), col(plonk.MG_MUL_CD), col(plonk.MG_NEXT), col(plonk.MG_SC), col(plonk.MG_SE)
    free = lambda c, r: circ.assembly.mapping[c * n + r] == c * n + r
    out, moved = circ.advice.copy(), 0
    for r in range(circ.used_rows):
        if mab[r] == 1 and sc[r] == 1 and se[r] == p - 1 and mcd[r] == 0 and (r == 0 or nxt[r - 1] == 0) and free(2, r) and free(4, r):
            for c in (2, 4):
                value = (sum(int(out[c, r, j]) << (64 * j) for j in range(4)) + variant * (r + 1)) % p
                out[c, r] = [(value >> (64 * j)) & ((1 << 64) - 1) for j in range(4)]
            moved += 1
    assert moved >= 4
    return out


def build_case(pkg, po, co, name):
    """-> dict(chain, advs: MAX_N Montgomery witnesses, insts: their instance lists (one list of columns per circuit))"""
    import plonk_oracle as PO
    import proof_chains as PC
    from dehalo2_amd import circuits
    chain, inst0 = PC.pinned_case(pkg, po, co, "kzg", name)
    fid = PO.Fld(po.BN254.scalar).id
    mont = lambda canonical: np.stack([co.field_op(fid, "to_mont", np.ascontiguousarray(canonical[i])) for i in range(canonical.shape[0])])
    advs, insts = [chain["adv"]], [[list(v) for v in inst0]]
    for v in range(1, MAX_N):
        if name.startswith("maingate"):
            k, rl = (9, True) if "range" in name else (5, False)
            advs.append(mont(_maingate_witness(circuits.synthesize(po.BN254.scalar.p, k, rl, seed=3), po.BN254.scalar.p, v)))
            insts.append([[]])
        elif name == "instance_k5":
            inst = [5 + 100 * v, 7 + v, 9, 11 + 3 * v]
            adv = np.zeros((1, 1 << 5, 4), dtype=np.uint64)
            adv[0, :len(inst), 0] = inst
            advs.append(mont(adv))
            insts.append([inst])
        else:
            advs.append(mont(_rotation_witness(pkg, name[:-3], 6, v)))
            insts.append([])
    return dict(chain=chain, advs=advs, insts=insts, name=name)


_CASES = {}


def case_of(pkg, po, co, name):
    """build_case, made once per process (tests/test_oracle_variants_pinned.py shares it)"""
    if name not in _CASES:
        _CASES[name] = build_case(pkg, po, co, name)
    return _CASES[name]


@pytest.fixture(scope="module")
def case(pkg, po, co):
    return lambda name: case_of(pkg, po, co, name)


_PROOFS, _STREAMS = {}, {}


def reference(po, cs, N, scheme, order=None, seed=SEED):
    """the restatement's (proof, trace) over the first N witnesses of case `cs` (or those of `order`), made once"""
    import plonk_oracle as PO
    import proof_chains as PC
    order = tuple(order if order is not None else range(N))
    key = (cs["name"], order, scheme, seed)
    if key not in _PROOFS:
        c = cs["chain"]
        stream = PO.ScalarStream(seed)
        _PROOFS[key] = PO.create_proof_multi(po.BN254, c["srs"], c["key"], [cs["advs"][i] for i in order], [cs["insts"][i] for i in order], stream, c["rep"],
                                             PC.THREADS, scheme)
        _STREAMS[key] = stream.gen.bit_generator.state      # where the restatement's draws ended
    return _PROOFS[key]


def layout(sh, N):
    """byte offsets in a proof: (advice commitment j of circuit c) -> offset, the first evaluation, the number of evaluations"""
    A, L, S = sh.num_advice, len(sh.lookups), sh.num_sets
    first_eval = 32 * (N * (A + 3 * L + S) + 1 + (sh.degree - 1))
    n_evals = N * (len(sh.advice_queries) + (3 * S - 1 if S else 0) + 5 * L) + len(sh.fixed_queries) + 1 + len(sh.perm_columns)
    return first_eval, n_evals


def tampered_last_circuit_evaluation(sh, N, proof):
    """one bit of the last evaluation of the last circuit flipped: its last lookup's or permutation product's, else its last advice query"""
    first_eval, n_evals = layout(sh, N)
    offset = first_eval + 32 * (n_evals - 1) if (len(sh.lookups) or sh.num_sets) else first_eval + 32 * (N * len(sh.advice_queries) - 1)
    bad = bytearray(proof)
    bad[offset + 5] ^= 0x04
    return bytes(bad)


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------------------------------------
def accepts(po, chain, proof, insts, scheme):
    """the restated verifier of `scheme` on a proof over len(insts) circuits"""
    import proof_chains as PC
    return PC.accepts(po, chain, proof, insts, scheme, len(insts))


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("name", KZG_CHAINS)
def test_restatement_with_one_circuit_is_the_single_circuit_oracle(po, case, golden_loader, name, scheme):
    """The one-circuit calls and the call over a list of one write the bytes pinned when the single-circuit and the multi-circuit restatement were two functions
    (tests/golden/oracle_variant_proof_digests.json; under GWC also oracle_proof_digests.json's, taken from the single-circuit one alone)."""
    import plonk_oracle as PO
    import proof_chains as PC
    import shplonk_oracle as SO
    cs = case(name)
    c = cs["chain"]
    want = golden_loader("oracle_variant_proof_digests")["multi/%s/1/%s" % (name, scheme)]
    single = SO.create_proof if scheme == "shplonk" else PO.create_proof
    for proof, trace in (single(po.BN254, c["srs"], c["key"], c["adv"], cs["insts"][0], PO.ScalarStream(SEED), c["rep"], PC.THREADS), reference(po, cs, 1, scheme)):
        assert PC.digests(proof, trace) == want
        if scheme == "gwc":
            assert PC.digests(proof, trace) == golden_loader("oracle_proof_digests")["kzg/" + name]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("N", (2, 3))
@pytest.mark.parametrize("name", KZG_CHAINS)
def test_restatement_proofs_are_accepted_and_tampering_rejected(po, case, name, N, scheme):
    import plonk_oracle as PO
    cs = case(name)
    sh = cs["chain"]["key"]["shape"]
    proof, _ = reference(po, cs, N, scheme)
    insts = cs["insts"][:N]
    other = "shplonk" if scheme == "gwc" else "gwc"
    assert len(proof) == PO.proof_length(sh, N, scheme)
    assert accepts(po, cs["chain"], proof, insts, scheme)
    assert not accepts(po, cs["chain"], proof, insts, other), "a proof of one multiopen passes for the other's"
    assert not accepts(po, cs["chain"], tampered_last_circuit_evaluation(sh, N, proof), insts, scheme), "an evaluation of the last circuit"
    bad = bytearray(proof)
    bad[32 * sh.num_advice + 3] ^= 0x04
    assert not accepts(po, cs["chain"], bytes(bad), insts, scheme), "an advice commitment of circuit 1"
    assert not accepts(po, cs["chain"], proof + proof[-32:], insts, scheme), "32 trailing bytes"
    assert not accepts(po, cs["chain"], proof, cs["insts"][:N - 1], scheme), "one circuit fewer"
    if name == "instance_k5":
        swapped = [insts[1], insts[0]] + insts[2:]
        assert swapped != insts and not accepts(po, cs["chain"], proof, swapped, scheme), "two circuits' instance lists exchanged"


@pytest.mark.parametrize("name", ("Rlast_k6", "instance_k5"))
def test_swapping_two_witnesses_gives_another_accepted_proof(po, case, name):
    cs = case(name)
    a, _ = reference(po, cs, 2, "gwc")
    b, _ = reference(po, cs, 2, "gwc", order=(1, 0))
    assert a != b and len(a) == len(b)
    assert accepts(po, cs["chain"], b, [cs["insts"][1], cs["insts"][0]], "gwc")


# ---- CPU: the opening plan's circuit dimension -----------------------------------------------------------------------------------------------------------
PLAN_CHAINS = ("maingate_range_k9", "Rlast_k6", "R9all_k6", "instance_k5")
PLAN_CASES = [(name, N) for name in PLAN_CHAINS for N in (1, 2, 3)]


def plan_shapes(pkg, po):
    """the four chains' shapes from their descriptions alone (no key is made for this)"""
    import plonk_oracle as PO
    import shapes
    import test_ipa_proof
    import test_rotations
    descs = {"maingate_range_k9": (shapes.maingate_description(True), 9), "instance_k5": (test_ipa_proof._instance_circuit(pkg, po, 5)[1], 5)}
    for name in ("Rlast_k6", "R9all_k6"):
        descs[name] = (test_rotations.build_circuit(pkg, name[:-3], 6)[0].description(), 6)
    return {name: PO.Shape(desc, k, po.BN254.scalar) for name, (desc, k) in descs.items()}


def shape_line(sh, N):
    out = [N, sh.k, sh.num_advice, sh.num_fixed, sh.num_instance, len(sh.lookups), sh.num_sets, len(sh.perm_columns), sh.blinding_factors, sh.degree - 1, 0]
    for qs in (sh.advice_queries, sh.fixed_queries, sh.instance_queries):
        out.append(len(qs))
        for c, r in qs:
            out += [c, r]
    return " ".join(str(v) for v in out)


@pytest.fixture(scope="module")
def plans(pkg, po):
    from conftest import ROOT
    out = subprocess.run(["make", "-C", ROOT, "opening_plan_multi_check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    shs = plan_shapes(pkg, po)
    lines = "".join(shape_line(shs[name], N) + "\n" for name, N in PLAN_CASES)
    ipa_line = shape_line(shs["instance_k5"], 2).split()
    ipa_line[10] = "1"
    lines += " ".join(ipa_line) + "\n" + shape_line(shs["instance_k5"], 0) + "\n"
    run = subprocess.run([os.path.join(ROOT, "tests", "native_host", "opening_plan_multi_check")], input=lines, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    printed = [json.loads(s) for s in run.stdout.splitlines()]
    assert len(printed) == len(PLAN_CASES) + 2
    return shs, dict(zip(PLAN_CASES, printed)), printed[-2:]


def tup(x):
    return tuple(tup(v) for v in x) if isinstance(x, list) else x


def test_opening_plan_refuses_what_it_cannot_order(plans):
    _, _, (ipa_two, none) = plans
    assert set(ipa_two) == {"refused"} and set(none) == {"refused"}


@pytest.mark.parametrize("name,N", PLAN_CASES)
def test_opening_plan_equals_the_restatements_lists(plans, name, N):
    import ipa as IPA
    import plonk_oracle as PO
    shs, printed, _ = plans
    sh, P = shs[name], printed[(name, N)]
    A, NF, L, S, npc, pieces = sh.num_advice, sh.num_fixed, len(sh.lookups), sh.num_sets, len(sh.perm_columns), sh.degree - 1
    last = -(sh.blinding_factors + 1)
    assert P["circuits"] == N and P["NC"] == N * (A + 3 * L + S) + 1
    # the numbering: per-circuit blocks first, what the proof has once behind them
    polys = [("advice", c, j) for c in range(N) for j in range(A)] + [(kind, c, l) for c in range(N) for l in range(L) for kind in ("lookup_a", "lookup_s")]
    for c in range(N):
        polys += [("perm_z", c, s) for s in range(S)] + [("lookup_z", c, l) for l in range(L)]
    polys += [("random",)] + [("fixed", j) for j in range(NF)] + [("sigma", j) for j in range(npc)] + [("hpiece", i) for i in range(pieces)]
    assert [tup(k) for k in P["polys"]] == polys + [("h",)] and P["num_polys"] == len(polys)
    # the products' commitments are written permutation products first, whatever the columns' order
    written = [polys[P["o_pz"] + o] for o in P["product_order"]]
    assert written == [("perm_z", c, s) for c in range(N) for s in range(S)] + [("lookup_z", c, l) for c in range(N) for l in range(L)] + [("random",)]
    rots = sorted({0, 1, -1, last} | {r for _, r in sh.advice_queries} | {r for _, r in sh.fixed_queries})
    assert P["rots"] == rots and P["eval_count"] == len(rots) * len(polys)

    def decode(slot):
        if slot == -1:
            return None
        assert 0 <= slot < P["eval_count"]
        return (polys[slot % len(polys)], rots[slot // len(polys)])

    assert decode(P["hpiece0"]) == (("hpiece", 0), 0)
    # ---- the transcript's order
    W = PO.evaluation_order(sh, N)
    assert [decode(s) for s in P["write"]] == W
    # ---- the queries
    Q = PO.symbolic_queries(sh, N)
    assert [(tup(q["poly"]), q["rot"]) for q in P["queries"]] == [(key, pt) for key, pt, _ in Q]
    assert [decode(q["eval"]) for q in P["queries"]] == [e for _, _, e in Q]
    assert len({q["blind"] for q in P["queries"] if tup(q["poly"])[0] not in ("fixed", "sigma")}) == len({key for key, _, _ in Q if key[0] not in ("fixed", "sigma")})
    # ---- GWC's groups
    groups = {}
    for key, pt, e in Q:
        groups.setdefault(pt, []).append((key, e))
    assert [g["rot"] for g in P["groups"]] == list(groups)
    for g, members in zip(P["groups"], groups.values()):
        assert [(tup(k), decode(s)) for k, s in zip(g["polys"], g["evals"])] == members and len(g["polys"]) == len(g["evals"])
    # ---- the intermediate sets
    commitments, point_sets = IPA.construct_intermediate_sets([(key, pt) for key, pt, _ in Q])
    points = list(groups)
    assert P["point_rot"] == points
    assert [[P["point_rot"][pi] for pi in ps] for ps in P["point_sets"]] == point_sets
    assert [(tup(c["poly"]), c["set"]) for c in P["commitments"]] == [(key, si) for key, si, _ in commitments]
    for c in P["commitments"]:
        first = [next(e for k2, pt, e in Q if k2 == tup(c["poly"]) and pt == points[pi]) for pi in P["point_sets"][c["set"]]]
        assert [decode(s) for s in c["evals"]] == first
    assert P["set_members"] == [[ci for ci, c in enumerate(P["commitments"]) if c["set"] == si] for si in range(len(point_sets))]
    # ---- who reads which value
    read = set(W) | {e for _, _, e in Q if e is not None} | {(("hpiece", i), 0) for i in range(pieces)}
    assert P["eval_wanted"] == [sum(1 << ri for ri, r in enumerate(rots) if (key, r) in read) for key in polys]
    # ---- the length of the proof
    assert P["proof_size"] == dict(gwc=PO.proof_length(sh, N, "gwc"), shplonk=PO.proof_length(sh, N, "shplonk"))
    if name == "R9all_k6":
        assert len(points) > 8


# ---- GPU: whole proofs through native.Prover(num_circuits=N).create_proof_multi ------------------------------------------------------------------------
def native_circuit(pkg, po, name):
    """-> (cs, fixed, assembly, selectors) of a chain: what ProvingKey.keygen takes"""
    import test_ipa_proof
    import test_rotations
    from dehalo2_amd import circuits
    if name.startswith("maingate"):
        k, rl = (9, True) if "range" in name else (5, False)
        circ = circuits.synthesize(po.BN254.scalar.p, k, rl, seed=3)
        return circ.cs, circ.fixed, circ.assembly, circ.selectors
    if name == "instance_k5":
        cs, _, _, fixed, _, asm = test_ipa_proof._instance_circuit(pkg, po, 5)
        return cs, fixed, asm, ()
    cs, fixed, _, asm = test_rotations.build_circuit(pkg, name[:-3], 6)
    return cs, fixed, asm, ()


_NATIVE = {}


@pytest.fixture(scope="module")
def native_key(pkg, po, ctx, case):
    """name -> (params, proving key) on the device, made once; released with the module"""
    import pairing as pr
    import plonk_oracle as PO
    from dehalo2_amd import native

    def get(name):
        if name not in _NATIVE:
            c = case(name)["chain"]
            cs, fixed, asm, selectors = native_circuit(pkg, po, name)
            params = native.ParamsKZG.create(ctx, pkg.fields.BN254, c["k"], c["srs"]["g"], c["srs"]["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(c["s_g2"]))
            pk = native.ProvingKey.keygen(ctx, params, cs, fixed, asm, selectors)
            assert pk.vk_bytes() == PO.vk_bytes(po.BN254, c["key"], selectors)
            pk.transcript_repr = c["rep"]
            _NATIVE[name] = (params, pk)
        return _NATIVE[name]
    yield get
    for params, pk in _NATIVE.values():
        pk.release(); params.release()
    _NATIVE.clear()


@pytest.fixture(scope="module")
def side_ctx(pkg, ctx):
    c = pkg.Context(0)
    yield c
    c.close()


def first_difference(got, want):
    return [i // 32 for i in range(0, max(len(got), len(want)), 32) if got[i:i + 32] != want[i:i + 32]][:8]


GPU_CASES = [(name, N) for name in ("maingate_k5", "Rlast_k6", "R9all_k6", "instance_k5") for N in (1, 2, 3)] + [("maingate_range_k9", 1), ("maingate_range_k9", 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("with_side", (False, True), ids=("one_context", "side_context"))
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("name,N", GPU_CASES)
def test_native_proof_over_several_circuits_equals_the_restatement(pkg, po, ctx, side_ctx, case, native_key, name, N, scheme, with_side):
    import plonk_oracle as PO
    from dehalo2_amd import native, prover
    cs = case(name)
    params, pk = native_key(name)
    want, _ = reference(po, cs, N, scheme)
    P = native.Prover(params, pk, side_ctx=side_ctx if with_side else None, multiopen=scheme, num_circuits=N)
    try:
        assert P.proof_size() == len(want) == PO.proof_length(cs["chain"]["key"]["shape"], N, scheme)
        rng = prover.SeededRng(SEED)
        proof = P.create_proof_multi(cs["advs"][:N], cs["insts"][:N], rng).finalize()
        assert len(proof) == len(want) and not first_difference(proof, want), "proof items differ from the restatement's: %r" % first_difference(proof, want)
        assert rng.gen.bit_generator.state == _STREAMS[(name, tuple(range(N)), scheme, SEED)], "the generator is not where the restatement's draws ended"
        assert accepts(po, cs["chain"], proof, cs["insts"][:N], scheme)
    finally:
        P.release()


@pytest.mark.gpu
@pytest.mark.parametrize("with_side", (False, True), ids=("one_context", "side_context"))
def test_native_proof_beyond_the_batch_tiles(pkg, po, ctx, side_ctx, case, native_key, with_side):
    """N L = 20 > 16 (the permutation's batch tile) and N (S + L) = 28 > 8 (the lookup pass's launch tile): N = 4 is the smallest N of the lookup chain past both"""
    from dehalo2_amd import native, prover
    cs, N = case("maingate_range_k9"), 4
    sh = cs["chain"]["key"]["shape"]
    assert N * len(sh.lookups) > 16 and (N - 1) * len(sh.lookups) <= 16 and N * (sh.num_sets + len(sh.lookups)) > 8
    params, pk = native_key("maingate_range_k9")
    want, _ = reference(po, cs, N, "gwc")
    P = native.Prover(params, pk, side_ctx=side_ctx if with_side else None, num_circuits=N)
    try:
        proof = P.create_proof_multi(cs["advs"][:N], cs["insts"][:N], prover.SeededRng(SEED)).finalize()
        assert not first_difference(proof, want), first_difference(proof, want)
        assert accepts(po, cs["chain"], proof, cs["insts"][:N], "gwc")
    finally:
        P.release()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("maingate_range_k9", "instance_k5"))
def test_native_one_circuit_through_the_multi_call_is_create_proof(pkg, po, ctx, case, native_key, name):
    from dehalo2_amd import native, prover
    cs = case(name)
    params, pk = native_key(name)
    P = native.Prover(params, pk)
    try:
        single = P.create_proof(cs["advs"][0], cs["insts"][0], prover.SeededRng(SEED)).finalize()
        multi = P.create_proof_multi(cs["advs"][:1], cs["insts"][:1], prover.SeededRng(SEED)).finalize()
        assert single == multi == reference(po, cs, 1, "gwc")[0]
    finally:
        P.release()


@pytest.mark.gpu
def test_native_two_proofs_in_a_row_and_device_entropy(pkg, po, ctx, side_ctx, case, native_key):
    from dehalo2_amd import native, prover
    cs = case("Rlast_k6")
    params, pk = native_key("Rlast_k6")
    first, _ = reference(po, cs, 2, "gwc")
    second, _ = reference(po, cs, 2, "gwc", order=(1, 0))
    P = native.Prover(params, pk, side_ctx=side_ctx, num_circuits=2)
    try:
        assert P.create_proof_multi(cs["advs"][:2], cs["insts"][:2], prover.SeededRng(SEED)).finalize() == first
        assert P.create_proof_multi([cs["advs"][1], cs["advs"][0]], [cs["insts"][1], cs["insts"][0]], prover.SeededRng(SEED)).finalize() == second      # a fresh prover's
        assert P.create_proof_multi(cs["advs"][:2], cs["insts"][:2], prover.SeededRng(SEED)).finalize() == first
        hidden = P.create_proof_multi(cs["advs"][:2], cs["insts"][:2], None).finalize()      # device ChaCha
        assert hidden != first and len(hidden) == len(first) and accepts(po, cs["chain"], hidden, cs["insts"][:2], "gwc")
    finally:
        P.release()


def _code(pkg, call):
    with pytest.raises((pkg.DehaloError, ValueError)) as e:
        call()
    return getattr(e.value, "code", -1)      # (native.py raises ValueError for DEHALO_ERR_INVALID about instances)


INVALID, UNSUPPORTED, NOT_IN_TABLE = -1, -5, -6


@pytest.mark.gpu
def test_native_error_table(pkg, po, co, ctx, case, native_key):
    import proof_chains as PC
    from dehalo2_amd import native, prover
    cs = case("instance_k5")
    params, pk = native_key("instance_k5")
    advs, insts = cs["advs"], cs["insts"]
    assert _code(pkg, lambda: native.Prover(params, pk, num_circuits=0)) == INVALID
    P2, P1 = native.Prover(params, pk, num_circuits=2), native.Prover(params, pk)
    try:
        assert _code(pkg, lambda: P2.create_proof_multi(advs[:3], insts[:3], prover.SeededRng(SEED))) == INVALID                     # other than the prover's
        assert _code(pkg, lambda: P1.create_proof_multi(advs[:2], insts[:2], prover.SeededRng(SEED))) == INVALID
        assert _code(pkg, lambda: P2.create_proof_multi(advs[:2], insts[:2], prover.SeededRng(SEED), num_circuits=0)) == INVALID
        assert _code(pkg, lambda: P2.create_proof(advs[0], insts[0], prover.SeededRng(SEED))) == INVALID                              # create_proof on N > 1
        assert _code(pkg, lambda: P2.create_proof_multi(advs[:2], [insts[0], [insts[1][0], [1]]], prover.SeededRng(SEED))) == INVALID   # circuit 1: two columns
        too_long = [1] * ((1 << 5) - 5)
        assert _code(pkg, lambda: P2.create_proof_multi(advs[:2], [insts[0], [too_long]], prover.SeededRng(SEED))) == INVALID        # circuit 1: beyond the usable rows
        assert _code(pkg, lambda: P2.set_shard(0, 2, lambda *a: None)) == UNSUPPORTED
        assert _code(pkg, lambda: native.create_proofs([P2], [advs[0]], [prover.SeededRng(SEED)])) == UNSUPPORTED
        assert _code(pkg, lambda: P2.create_proof_phased(lambda ph, ch: advs[0], insts[0], prover.SeededRng(SEED))) == UNSUPPORTED
        assert _code(pkg, lambda: P2.create_proof_circuit(0, insts[0], prover.SeededRng(SEED), **native_inputs())) == UNSUPPORTED
        assert _code(pkg, lambda: native.create_proofs_circuit([P2], 0, [native_inputs()], [prover.SeededRng(SEED)])) == UNSUPPORTED
        # the prover is still good after every refusal
        assert P2.create_proof_multi(advs[:2], insts[:2], prover.SeededRng(SEED)).finalize() == reference(po, cs, 2, "gwc")[0]
    finally:
        P2.release(); P1.release()
    # ParamsIPA, and a key with later-phase advice
    import phased_circuits as PH
    import pairing as pr
    ic, _ = PC.pinned_case(pkg, po, co, "ipa", "instance_k5")
    ip = native.ParamsIPA.create(ctx, pkg.fields.VESTA, 5, ic["srs"]["g"], ic["srs"]["g_lagrange"], ic["w"], ic["u"])
    cs5, fixed5, asm5, _ = native_circuit(pkg, po, "instance_k5")
    ipk = native.ProvingKey.keygen(ctx, ip, cs5, fixed5, asm5, ())
    try:
        assert _code(pkg, lambda: native.Prover(ip, ipk, num_circuits=2)) == UNSUPPORTED
        native.Prover(ip, ipk, num_circuits=1).release()
    finally:
        ipk.release(); ip.release()
    pc = PH.chain(pkg, po, co, "kzg", 6)
    pp = native.ParamsKZG.create(ctx, pkg.fields.BN254, 6, pc["srs"]["g"], pc["srs"]["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(pc["s_g2"]))
    ppk = native.ProvingKey.keygen(ctx, pp, pc["cs"], pc["fixed"], pc["asm"], ())
    try:
        assert _code(pkg, lambda: native.Prover(pp, ppk, num_circuits=2)) == UNSUPPORTED
    finally:
        ppk.release(); pp.release()


def native_inputs():
    """inputs of the smallest synthesized circuit (the call is refused before they are read)"""
    return dict()


@pytest.mark.gpu
def test_native_lookup_input_missing_in_circuit_one_only(pkg, po, ctx, case, native_key):
    from dehalo2_amd import native, prover
    cs = case("maingate_range_k9")
    params, pk = native_key("maingate_range_k9")
    sh = cs["chain"]["key"]["shape"]
    # the first limb of a composition row (the lookups' selector is on there) set beyond every table value
    circ_fixed = native_circuit(pkg, po, "maingate_range_k9")[1]
    from dehalo2_amd import plonk
    row = int(np.nonzero(circ_fixed[plonk.RC_S_COMPOSITION, :, 0])[0][0])
    import plonk_oracle as PO
    bad = cs["advs"][1].copy()
    bad[0, row] = PO.Fld(po.BN254.scalar).m(1 << 200)      # no range table holds it
    P = native.Prover(params, pk, num_circuits=2)
    try:
        assert _code(pkg, lambda: P.create_proof_multi([cs["advs"][0], bad], cs["insts"][:2], prover.SeededRng(SEED))) == NOT_IN_TABLE
        assert P.create_proof_multi(cs["advs"][:2], cs["insts"][:2], prover.SeededRng(SEED)).finalize() == reference(po, cs, 2, "gwc")[0]
    finally:
        P.release()
    assert sh.lookups
