"""The shuffle argument's test circuits: SHUF1, SHUF2, SHUF5, SHUFRLC, their witnesses (satisfying, and ones that are no shuffle) and their chains.  TEST
INFRASTRUCTURE ONLY; the prover and the verifiers are the oracle's (oracle/plonk_oracle.py, oracle/verifier.py), which read a key's shuffles, phases and
challenges from its description (plonk_oracle.Desc).  Circuits without instance columns."""
import numpy as np

import phased_circuits as PH
import plonk_oracle as PO


def limbs(values, n):
    return PH.limbs(values, n)


def build(pkg, name, k):
    """-> dict(cs, k, fixed (canonical), asm, witness): witness(bad=False) -> (num_advice, n, 4) canonical advice for a single-phase circuit, or, for SHUFRLC,
    a function (phase, challenges) -> advice.  bad: one value changed so that one shuffle's sides are no permutation of each other."""
    from dehalo2_amd import plonk as P
    n = 1 << k
    if name == "SHUF1":      # input [a0], shuffle [a1]; one fixed column nobody reads, no permutation
        cs = P.ConstraintSystem(num_advice=2, num_fixed=1, num_instance=0)
        cs.shuffle([(cs.query_advice(0), cs.query_advice(1))])
        u = n - (cs.blinding_factors() + 1)
        a0 = [(3 * i + 1) % 7 for i in range(u)]      # with repeats
        perm = [(5 * i + 2) % u for i in range(u)] if u % 5 else list(reversed(range(u)))

        def witness(bad=False):
            a1 = [a0[j] for j in perm]
            if bad:
                a1[3] = (a1[3] + 1) % 7 + 100
            adv = np.zeros((2, n, 4), dtype=np.uint64)
            adv[0], adv[1] = limbs(a0, n), limbs(a1, n)
            return adv
        return dict(cs=cs, k=k, fixed=np.zeros((1, n, 4), dtype=np.uint64), asm=P.Assembly(0, n), witness=witness, usable=u)
    if name == "SHUF5":      # input [q a0 a1] (degree 3), shuffle [a2]: the key's degree is 5, the quotient has four pieces
        cs = P.ConstraintSystem(num_advice=3, num_fixed=1, num_instance=0)
        q = cs.query_fixed(0)
        cs.shuffle([(P.mul(P.mul(q, cs.query_advice(0)), cs.query_advice(1)), cs.query_advice(2))])
        cs.enable_equality(P.ADVICE, 2)
        u = n - (cs.blinding_factors() + 1)
        R = u - 5
        fixed = np.zeros((1, n, 4), dtype=np.uint64)
        fixed[0, :R, 0] = 1
        a0 = [i + 2 for i in range(u)]
        a1 = [(i * i) % 13 + 1 for i in range(u)]
        prod = [a0[i] * a1[i] if i < R else 0 for i in range(u)]
        perm = list(reversed(range(u)))

        def witness(bad=False):
            a2 = [prod[j] for j in perm]
            if bad:
                a2[0] += 1
            adv = np.zeros((3, n, 4), dtype=np.uint64)
            adv[0], adv[1], adv[2] = limbs(a0, n), limbs(a1, n), limbs(a2, n)
            return adv
        asm = P.Assembly(1, n)
        asm.copy(0, 0, 0, 1)      # a2[0] = a2[1] = 0: both are images of rows the selector switches off
        return dict(cs=cs, k=k, fixed=fixed, asm=asm, witness=witness, usable=u)
    if name == "SHUF2":
        # fixed q (selector, rows [0, R)), t (table 0 .. 15); advice a0 .. a5, g
        #   shuffle 0   [q a0, q a1]  ~  [q a2, q a3(wX)]        shuffle 1   [a0, a1]  ~  [a4, a5]
        #   gate        q (a0 + a1 - g)                          lookup      a0 in t              equality on a0, a1 with one copy each
        cs = P.ConstraintSystem(num_advice=7, num_fixed=2, num_instance=0)
        q, t = cs.query_fixed(0), cs.query_fixed(1)
        cs.enable_equality(P.ADVICE, 0)
        cs.enable_equality(P.ADVICE, 1)
        a = [cs.query_advice(i) for i in range(3)]
        a3n = cs.query_advice(3, 1)
        a4, a5, g = cs.query_advice(4), cs.query_advice(5), cs.query_advice(6)
        cs.create_gate([P.mul(q, P.sum_(a[0], a[1], ("neg", g)))])
        cs.lookup([(a[0], t)])
        cs.shuffle([(P.mul(q, a[0]), P.mul(q, a[2])), (P.mul(q, a[1]), P.mul(q, a3n))])
        cs.shuffle([(a[0], a4), (a[1], a5)])
        u = n - (cs.blinding_factors() + 1)
        R = u - 18
        assert R > 16 and R % 13 and u % 5
        fixed = np.zeros((2, n, 4), dtype=np.uint64)
        fixed[0, :R, 0] = 1
        fixed[1, :, 0] = np.arange(n) % 16
        asm = P.Assembly(2, n)
        asm.copy(0, 1, 0, 17)       # a0 has period 16
        asm.copy(1, 1, 1, 10)       # 1 and 100 are both 1 mod 11

        def witness(bad=False, variant=0):
            a0 = [(7 * i + 3 + variant) % 16 for i in range(u)]
            a1 = [(i * i) % 11 + 100 + 1000 * variant for i in range(u)]
            p0 = [(13 * i + 5) % R for i in range(R)]
            p1 = [(5 * i + 7) % u for i in range(u)]
            a2 = [a0[p0[i]] if i < R else 77 for i in range(u)]
            a3 = [9] + [a1[p0[i]] if i < R else 55 for i in range(u - 1)]      # a3[i + 1] pairs with a2[i]
            a4, a5 = [a0[j] for j in p1], [a1[j] for j in p1]
            if bad:
                a5[2], a5[3] = a5[3], a5[2]      # the columns stay permutations of each other; the TUPLES do not (unless the two values are equal)
                assert a5[2] != a5[3] and a4[2] != a4[3]
            adv = np.zeros((7, n, 4), dtype=np.uint64)
            for i, col in enumerate((a0, a1, a2, a3, a4, a5, [x + y for x, y in zip(a0, a1)])):
                adv[i] = limbs(col, n)
            return adv
        return dict(cs=cs, k=k, fixed=fixed, asm=asm, witness=witness, usable=u)
    if name == "SHUFRLC":      # a0, a1 in phase 0, b in phase 1, c0 squeezed after phase 0: [a0 + c0 a1] ~ [b]
        cs = P.ConstraintSystem(num_advice=3, num_fixed=1, num_instance=0)
        cs.advice_phases = [0, 0, 1]
        c0 = cs.challenge_usable_after(0)
        cs.enable_equality(P.ADVICE, 0)
        cs.shuffle([(P.sum_(cs.query_advice(0), P.mul(c0, cs.query_advice(1))), cs.query_advice(2))])
        u = n - (cs.blinding_factors() + 1)
        a0 = [(3 * i) % 5 for i in range(u)]
        a1 = [(i * i + 1) % 7 for i in range(u)]
        perm = list(reversed(range(u)))

        def witness(p, bad=False):
            adv = np.zeros((3, n, 4), dtype=np.uint64)
            adv[0], adv[1] = limbs(a0, n), limbs(a1, n)

            def fn(phase, challenges):
                if phase == 1:
                    c = (challenges[0] + (1 if bad else 0)) % p
                    rlc = [(x + c * y) % p for x, y in zip(a0, a1)]
                    adv[2] = limbs([rlc[j] for j in perm], n)
                return adv
            return fn
        return dict(cs=cs, k=k, fixed=np.zeros((1, n, 4), dtype=np.uint64), asm=P.Assembly(1, n), witness=witness, usable=u)
    raise ValueError(name)


def chain(pkg, po, co, scheme, name, k):
    """tests/proof_chains.py's chain for circuit `name`: SRS, key and the transcript representation over (description, shuffles, phases, challenge phases)."""
    import proof_chains as PC
    circ = build(pkg, name, k)
    cs = circ["cs"]
    dummy = np.zeros((cs.num_advice, 1 << k, 4), dtype=np.uint64)
    c = (PC.ipa_chain if scheme == "ipa" else PC.kzg_chain)(po, co, PO.describe(cs), k, circ["fixed"], circ["asm"].mapping, dummy)
    c = dict(c, circ=circ, cs=cs, curve=po.VESTA if scheme == "ipa" else po.BN254, name=name, scheme=scheme)
    del c["adv"]
    return c


def prove(po, co, c, witnesses, multiopen="gwc", seed=7):
    """-> (proof, trace).  witnesses: a list of canonical advice arrays (one per circuit), or for a phased circuit a function (phase, challenges) -> advice."""
    import proof_chains as PC
    ws = [PH.mont_witness(po, co, c, witnesses)] if callable(witnesses) else [PH.to_mont(co, c["curve"], po, w) for w in witnesses]
    return PC.prove_circuits(po, c, ws, [[]] * len(ws), multiopen, seed)


def accepts(po, c, proof, circuits=1, multiopen="gwc"):
    """the restated verifier of the chain's scheme (KZG: of `multiopen`) on a proof over `circuits` circuits"""
    import proof_chains as PC
    return PC.accepts(po, c, proof, [[]] * circuits, multiopen, circuits)


def tampered_product_evaluation(c, proof, circuits=1):
    """z(x) of circuit 0's first shuffle with one bit flipped"""
    sh = c["key"]["shape"]
    A, L, S, H = sh.num_advice, len(sh.lookups), sh.num_sets, len(sh.shuffles)
    head = circuits * (A + 3 * L + S + H) + 1 + (sh.degree - 1)
    before = circuits * (len(sh.advice_queries) + (3 * S - 1 if S else 0) + 5 * L) + len(sh.fixed_queries) + 1 + len(sh.perm_columns)
    bad = bytearray(proof)
    bad[32 * (head + before) + 3] ^= 0x10
    return bytes(bad)
