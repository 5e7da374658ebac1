"""Later-phase advice and challenges: the circuits RLC3 / RLC3perm, their witness as a function of the challenges, and their chain.  TEST INFRASTRUCTURE ONLY;
the prover and the verifiers are the oracle's (oracle/plonk_oracle.py create_proof_multi, oracle/verifier.py read_plonk), which commit and read the advice phase by
phase and squeeze each phase's challenges themselves.

RLC3's phases are non-decreasing in the column index; RLC3perm relabels its columns so that they are not, and is only ever compared with RLC3 byte for byte."""
import numpy as np

Q_ROWS = 16      # the selector is on for rows 0 .. 15


# ---- the circuits ---------------------------------------------------------------------------------------------------------------------------------
# advice by role; RLC3 numbers them in this order, RLC3perm relabels them (phases not monotone in the column index, the order inside a phase kept)
ROLES = ("a0", "a1", "r", "s", "w")
ROLE_PHASE = dict(a0=0, a1=0, r=1, s=1, w=2)
LABELS = dict(RLC3=dict(a0=0, a1=1, r=2, s=3, w=4), RLC3perm=dict(a0=1, a1=3, r=0, s=4, w=2))


def build_cs(pkg, name="RLC3"):
    """fixed q, t0, t1; advice a0, a1 (phase 0), r, s (phase 1), w (phase 2); challenges c0 after phase 0, c1 after phase 1, c2 after phase 2.
         gate 0   q (r - (a0 + c0 a1))                     gate 1   q (s(wX) - c0 s(X) - a0(wX))
         gate 2   q (w - c1 r)                             gate 3   q c2 (w - c1 r)
         lookup   (a0 + c0 a1) in (t0 + c0 t1)             equality on a0 and r"""
    from dehalo2_amd import plonk as P
    lab = LABELS[name]
    cs = P.ConstraintSystem(num_advice=5, num_fixed=3, num_instance=0)
    cs.advice_phases = [ROLE_PHASE[role] for role in sorted(ROLES, key=lambda role: lab[role])]
    c0, c1, c2 = (cs.challenge_usable_after(ph) for ph in (0, 1, 2))
    cs.enable_equality(P.ADVICE, lab["a0"])
    cs.enable_equality(P.ADVICE, lab["r"])
    q, t0, t1 = (cs.query_fixed(i) for i in range(3))
    a0, a1, r = cs.query_advice(lab["a0"]), cs.query_advice(lab["a1"]), cs.query_advice(lab["r"])
    s, s_next, a0_next = cs.query_advice(lab["s"]), cs.query_advice(lab["s"], 1), cs.query_advice(lab["a0"], 1)
    w = cs.query_advice(lab["w"])
    rlc = P.sum_(a0, P.mul(c0, a1))
    wr = P.sum_(w, ("neg", P.mul(c1, r)))
    cs.create_gate([P.mul(q, P.sum_(r, ("neg", rlc))),
                    P.mul(q, P.sum_(s_next, ("neg", P.mul(c0, s)), ("neg", a0_next))),
                    P.mul(q, wr),
                    P.mul(P.mul(q, c2), wr)])
    cs.lookup([(rlc, P.sum_(t0, P.mul(c0, t1)))])
    return cs


def table_row(i):
    return (i % 16) % 8, (3 * (i % 16)) % 5


def input_row(i):
    """the table row whose tuple advice row i holds"""
    return (5 * i + 2) % 16


def fixed_columns(k):
    n = 1 << k
    fixed = np.zeros((3, n, 4), dtype=np.uint64)
    fixed[0, :Q_ROWS, 0] = 1
    for i in range(n):
        fixed[1, i, 0], fixed[2, i, 0] = table_row(i)
    return fixed


def copy_rows(usable):
    """rows whose a1 is zero: there r = a0 whatever c0 is, and the two cells are tied by a copy constraint"""
    return [i for i in range(min(usable, 64)) if table_row(input_row(i))[1] == 0]


def assembly(pkg, cs, k):
    from dehalo2_amd import plonk as P
    asm = P.Assembly(2, 1 << k)
    for i in copy_rows((1 << k) - (cs.blinding_factors() + 1)):
        asm.copy(0, i, 1, i)
    return asm


def limbs(values, n):
    out = np.zeros((n, 4), dtype=np.uint64)
    for i, v in enumerate(values):
        for j in range(4):
            out[i, j] = (v >> (64 * j)) & ((1 << 64) - 1)
    return out


def witness(p, k, usable, name="RLC3", wrong_c0=False):
    """-> fn(phase, challenges) -> (5, n, 4) canonical advice with the columns of phases <= phase filled.  wrong_c0: r is computed with c0 + 1."""
    n, lab = 1 << k, LABELS[name]
    a0 = [table_row(input_row(i))[0] for i in range(usable)]
    a1 = [table_row(input_row(i))[1] for i in range(usable)]
    adv = np.zeros((5, n, 4), dtype=np.uint64)
    adv[lab["a0"]], adv[lab["a1"]] = limbs(a0, n), limbs(a1, n)
    state = {}

    def fn(phase, challenges):
        if phase == 1:
            c0 = challenges[0]
            cr = (c0 + 1) % p if wrong_c0 else c0
            state["r"] = [(x + cr * y) % p for x, y in zip(a0, a1)]
            s = [0] * usable
            s[0] = a0[0]
            for i in range(Q_ROWS):
                s[i + 1] = (c0 * s[i] + a0[i + 1]) % p
            adv[lab["r"]], adv[lab["s"]] = limbs(state["r"], n), limbs(s, n)
        if phase == 2:
            adv[lab["w"]] = limbs([challenges[1] * x % p for x in state["r"]], n)
        return adv

    return fn


def full_witness(p, k, usable, challenges, name="RLC3"):
    """the whole witness under given challenge values (what check_witness takes)"""
    fn = witness(p, k, usable, name)
    for ph in range(3):
        adv = fn(ph, list(challenges))
    return adv.copy()


# ---- chains -----------------------------------------------------------------------------------------------------------------------------------------
def chain(pkg, po, co, scheme, k):
    """tests/proof_chains.py's chain for RLC3 at k, key and `rep` from the description with its phases and challenge nodes; `adv` is absent -- the witness is
    a function (`witness`)."""
    import plonk_oracle as PO
    import proof_chains as PC
    cs = build_cs(pkg)
    fixed, asm = fixed_columns(k), assembly(pkg, cs, k)
    dummy = np.zeros((cs.num_advice, 1 << k, 4), dtype=np.uint64)
    c = (PC.ipa_chain if scheme == "ipa" else PC.kzg_chain)(po, co, PO.describe(cs), k, fixed, asm.mapping, dummy)
    c = dict(c, cs=cs, curve=po.VESTA if scheme == "ipa" else po.BN254, fixed=fixed, asm=asm)
    del c["adv"]
    return c


def to_mont(co, curve, po, canonical):
    import plonk_oracle as PO
    fid = PO.Fld(curve.scalar).id
    return np.stack([co.field_op(fid, "to_mont", np.ascontiguousarray(canonical[i])) for i in range(canonical.shape[0])])


def mont_witness(po, co, c, fn):
    """a witness function's advice in Montgomery form: what the oracle's prover and create_proof_phased take"""
    return lambda phase, challenges: to_mont(co, c["curve"], po, fn(phase, challenges))
