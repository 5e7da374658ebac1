"""CPU suite: the prover's opening plan (csrc/opening_plan.hpp) against the oracle driven symbolically.

The plan says which polynomial is opened at which rotation, in which order, under which blind, and where its evaluation lands -- for GWC, SHPLONK and IPA alike.
tests/native_host/opening_plan_check.cpp (g++, ASan + UBSan, a program of its own) prints it for every shape below, once; here each printed plan is compared,
by exact equality, with what oracle/plonk_oracle.py symbolic_queries (plonk_queries with commitments their keys, points their rotations and evaluations the pairs
(key, rotation)) and oracle/ipa.py construct_intermediate_sets make of the same shape.  The oracle keys what a circuit has of its own (name, circuit, index):
the printed (name, index) are read as circuit 0's.  The transcript's write order, the layouts and the proof sizes are this file's
own statement of upstream's."""
import json
import os
import subprocess

import pytest

K = 6
REFUSAL = "33 distinct opening rotations: more than 32"


def _wide(columns):
    """`columns` advice columns, column c queried once at rotation 2 + c: no column is queried twice, so bf stays 5 and `last` -6"""
    return (columns, 0, 0, (), (), (), tuple((c, 2 + c) for c in range(columns)), (), (), 0)


def descriptions(pkg):
    import shapes
    from test_rotations import NAMES, build_circuit
    d = {"maingate_lookups": shapes.maingate_description(True),                       # S = 2, L = 5, one instance column
         "maingate_plain": shapes.maingate_description(False)}                        # degree 3: chunks of one column, S = 6, five queries at omega^last x in reverse
    for name in NAMES:                                                                # a fixed column at two rotations, a query on `last`, more than four rotations
        d[name] = build_circuit(pkg, name, K)[0].description()
    d["one_perm_column"] = (1, 0, 0, (), (), (("advice", 0),), ((0, 0),), (), (), 0)  # S = 1: nobody reads at `last`, which stays a rotation
    d["one_advice"] = (1, 0, 0, (), (), (), ((0, 0),), (), (), 0)
    d["lookup_and_minus_one"] = (2, 1, 0, (), (((("advice", 0, 0),), (("fixed", 0, 0),)),), (), ((0, 0), (1, -1)), ((0, 0),), (), 0)      # b(w^-1 x) shares the lookup's point
    d["instance_two_rotations"] = (1, 0, 1, (), (), (), ((0, 0),), (), ((0, 3), (0, 0)), 0)      # IPA: the first point is one nothing else uses
    d["rotations_32"] = _wide(28)                                                     # {-6, -1, 0, 1} and 2 .. 29
    d["rotations_33"] = _wide(29)
    return d


CASES = [(name, scheme) for name in ("maingate_lookups", "maingate_plain", "R5", "R7", "R9", "R9all", "Rlast", "one_perm_column", "one_advice", "lookup_and_minus_one",
                                     "rotations_32", "rotations_33") for scheme in ("kzg", "ipa")] + [("instance_two_rotations", "ipa")]


def shape_line(sh, ipa):
    out = [K, sh.num_advice, sh.num_fixed, sh.num_instance, len(sh.lookups), sh.num_sets, len(sh.perm_columns), sh.blinding_factors, sh.degree - 1, int(ipa)]
    for qs in (sh.advice_queries, sh.fixed_queries, sh.instance_queries):
        out.append(len(qs))
        for c, r in qs:
            out += [c, r]
    return " ".join(str(v) for v in out)


@pytest.fixture(scope="module")
def plans(pkg, po):
    """(name, scheme) -> (the oracle's Shape, the printed plan): one build, one run over every case"""
    import plonk_oracle as PO
    from conftest import ROOT
    out = subprocess.run(["make", "-C", ROOT, "opening_plan_check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    desc = descriptions(pkg)
    shs = {name: PO.Shape(desc[name], K, po.BN254.scalar) for name in desc}
    lines = "".join(shape_line(shs[name], scheme == "ipa") + "\n" for name, scheme in CASES)
    run = subprocess.run([os.path.join(ROOT, "tests", "native_host", "opening_plan_check")], input=lines, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr and run.stderr == "", run.stdout + run.stderr
    printed = [json.loads(s) for s in run.stdout.splitlines()]
    assert len(printed) == len(CASES)
    return {case: (shs[case[0]], plan) for case, plan in zip(CASES, printed)}


OWN = ("instance", "advice", "perm_z", "lookup_a", "lookup_s", "lookup_z")      # a circuit's own: keyed (name, circuit, index)


def tup(x):
    """a printed value as the oracle spells it: lists are tuples, a circuit's own polynomial is circuit 0's"""
    if not isinstance(x, list):
        return x
    x = tuple(tup(v) for v in x)
    return (x[0], 0) + x[1:] if x and x[0] in OWN else x


def transcript_order(sh, ipa):
    """upstream's order of the evaluations in the proof, as (key, rotation): the instance queries, then the rest"""
    L, S, last = len(sh.lookups), sh.num_sets, -(sh.blinding_factors + 1)
    inst = [(("instance", 0, c), r) for c, r in sh.instance_queries] if ipa else []
    W = [(("advice", 0, c), r) for c, r in sh.advice_queries] + [(("fixed", c), r) for c, r in sh.fixed_queries] + [(("random",), 0)]
    W += [(("sigma", j), 0) for j in range(len(sh.perm_columns))]
    for s in range(S):
        W += [(("perm_z", 0, s), 0), (("perm_z", 0, s), 1)] + ([(("perm_z", 0, s), last)] if s != S - 1 else [])
    for l in range(L):
        W += [(("lookup_z", 0, l), 0), (("lookup_z", 0, l), 1), (("lookup_a", 0, l), 0), (("lookup_a", 0, l), -1), (("lookup_s", 0, l), 0)]
    return inst, W


@pytest.mark.parametrize("name,scheme", CASES)
def test_opening_plan_equals_the_oracles(plans, name, scheme):
    import ipa as IPA
    import plonk_oracle as PO
    sh, P = plans[(name, scheme)]
    ipa = scheme == "ipa"
    if name == "rotations_33":
        assert P == {"refused": REFUSAL}
        return
    A, NF, I, L, S, npc = sh.num_advice, sh.num_fixed, sh.num_instance, len(sh.lookups), sh.num_sets, len(sh.perm_columns)
    bf, pieces = sh.blinding_factors, sh.degree - 1
    last = -(bf + 1)

    # ---- layouts: columns, polynomial numbering, blinds
    assert P["columns"] == dict(o_adv=0, o_perm=A, o_pz=A + 2 * L, o_lz=A + 2 * L + S, o_rand=A + 3 * L + S, NC=A + 3 * L + S + 1)
    polys = [("advice", 0, c) for c in range(A)] + [(kind, 0, l) for l in range(L) for kind in ("lookup_a", "lookup_s")] + [("perm_z", 0, s) for s in range(S)]
    polys += [("lookup_z", 0, l) for l in range(L)] + [("random",)] + [("fixed", c) for c in range(NF)] + [("sigma", j) for j in range(npc)]
    polys += [("hpiece", i) for i in range(pieces)] + ([("instance", 0, c) for c in range(I)] if ipa else [])
    assert [tup(k) for k in P["polys"]] == polys + [("h",)] and P["num_polys"] == len(polys)
    B = dict(bi_adv=0, bi_perm=A, bi_prod=A + 2 * L, bi_rand=A + 3 * L + S)
    B.update(bi_h=B["bi_rand"] + 1, bi_hfold=B["bi_rand"] + 1 + pieces, bi_f=B["bi_rand"] + 2 + pieces, bi_def=B["bi_rand"] + 3 + pieces, bi_count=B["bi_rand"] + 3 + pieces + max(I, 1))
    assert P["blinds"] == B
    hiding = {("advice", 0, c): c for c in range(A)}
    hiding.update({("lookup_a", 0, l): A + 2 * l for l in range(L)})
    hiding.update({("lookup_s", 0, l): A + 2 * l + 1 for l in range(L)})
    hiding.update({("perm_z", 0, s): B["bi_prod"] + s for s in range(S)})
    hiding.update({("lookup_z", 0, l): B["bi_prod"] + S + l for l in range(L)})
    hiding.update({("random",): B["bi_rand"], ("h",): B["bi_hfold"]})
    hiding.update({("hpiece", i): B["bi_h"] + i for i in range(pieces)})
    assert len(set(hiding.values()) | {B["bi_f"], B["bi_def"]}) == len(hiding) + 2 and max(hiding.values()) < B["bi_f"] < B["bi_def"] < B["bi_count"]

    def blind_of(key):
        return B["bi_def"] if key[0] in ("fixed", "sigma", "instance") else hiding[key]

    # ---- rotations and slots
    rots = sorted({0, 1, -1, last} | {r for _, r in sh.advice_queries} | {r for _, r in sh.fixed_queries} | ({r for _, r in sh.instance_queries} if ipa else set()))
    assert P["rots"] == rots and P["eval_count"] == len(rots) * len(polys)
    if name == "rotations_32":
        assert len(rots) == 32 and bf == 5

    def decode(slot):      # -> (key, rotation); None for the folded h's -1
        if slot == -1:
            return None
        assert 0 <= slot < P["eval_count"]
        return (polys[slot % len(polys)], rots[slot // len(polys)])

    assert decode(P["hpiece0"]) == (("hpiece", 0), 0)

    # ---- the queries
    Q = PO.symbolic_queries(sh, 1, ipa)
    assert [(tup(q["poly"]), q["rot"]) for q in P["queries"]] == [(key, pt) for key, pt, _ in Q]
    assert [decode(q["eval"]) for q in P["queries"]] == [e for _, _, e in Q]
    assert [q["blind"] for q in P["queries"]] == [blind_of(key) for key, _, _ in Q]
    assert [q["eval"] for q in P["queries"] if tup(q["poly"]) == ("h",)] == [-1]

    # ---- GWC: by point in order of first appearance (ProverGWC.open), members in query order
    groups = {}
    for key, pt, e in Q:
        groups.setdefault(pt, []).append((key, e))
    assert [g["rot"] for g in P["groups"]] == list(groups)
    for g, members in zip(P["groups"], groups.values()):
        assert [(tup(k), decode(s)) for k, s in zip(g["polys"], g["evals"])] == members and len(g["polys"]) == len(g["evals"])

    # ---- the intermediate sets
    commitments, point_sets = IPA.construct_intermediate_sets([(key, pt) for key, pt, _ in Q])
    points = list(groups)      # numbered by first appearance
    assert P["point_rot"] == points
    assert [[P["point_rot"][pi] for pi in ps] for ps in P["point_sets"]] == point_sets and all(ps == sorted(ps) for ps in P["point_sets"])
    assert [(tup(c["poly"]), c["set"]) for c in P["commitments"]] == [(key, si) for key, si, _ in commitments]
    for c in P["commitments"]:
        key = tup(c["poly"])
        assert c["blind"] == blind_of(key)
        first = [next(e for k2, pt, e in Q if k2 == key and pt == points[pi]) for pi in P["point_sets"][c["set"]]]
        assert [decode(s) for s in c["evals"]] == first
    if (name, scheme) == ("maingate_lookups", "ipa"):
        assert (len(Q), len(commitments), point_sets) == (60, 46, [[0], [0, 1], [0, 1, -6], [0, -1]])
    assert P["set_members"] == [[ci for ci, c in enumerate(P["commitments"]) if c["set"] == si] for si in range(len(point_sets))]

    # ---- the transcript's order
    inst, W = transcript_order(sh, ipa)
    assert [decode(s) for s in P["instance_write"]] == inst and [decode(s) for s in P["write"]] == W
    assert -1 not in P["instance_write"] + P["write"]

    # ---- who reads which value: no bit more
    read = set(inst) | set(W) | {e for _, _, e in Q if e is not None} | {(("hpiece", i), 0) for i in range(pieces)}
    assert P["eval_wanted"] == [sum(1 << ri for ri, r in enumerate(rots) if (key, r) in read) for key in polys]
    assert P["eval_wanted8"] == (P["eval_wanted"] if len(rots) <= 4 else None)
    if name == "one_perm_column":
        assert last in rots and all(not (w >> rots.index(last)) & 1 for w in P["eval_wanted"])

    # ---- proof sizes: 32 bytes per commitment, opening and scalar (a prover over IPA has the one multiopen: the other two sizes are nobody's there)
    n_commit, n_evals = A + 3 * L + S + 1 + pieces, len(inst) + len(W)
    sizes = dict(gwc=32 * (n_commit + len(points) + n_evals), shplonk=32 * (n_commit + 2 + n_evals), ipa=32 * (n_commit + 2 + 2 * K + n_evals + len(point_sets) + 2))
    assert set(P["proof_size"]) == set(sizes)
    for multiopen in (["ipa"] if ipa else ["gwc", "shplonk", "ipa"]):
        assert P["proof_size"][multiopen] == sizes[multiopen], multiopen
