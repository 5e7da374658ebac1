"""Later-phase advice and challenges on the CPU restatements, without touching oracle/: the circuits RLC3 / RLC3perm, their witness as a function of the
challenges, and the oracle's prover and verifiers taught the phase loop from outside.  TEST INFRASTRUCTURE ONLY, beside tests/shplonk_oracle.py.

[UPSTREAM halo2_proofs @ v2023_04_20 plonk/prover.rs, plonk/verifier.rs]: after the instances, for each phase in order the advice commitments of its columns are
written and then one challenge is squeezed per challenge of that phase; theta follows the last phase.  A challenge is a constant of the rest of the proof.  So:

  * the challenges of a proof are recovered by reading its advice commitments through a transcript that squeezes at the phase boundaries (`recover`);
  * every ("challenge", j) of the description becomes ("const", value) -- same degree, same Shape -- and the oracle's verifiers run as they are, their
    ReadTranscript replaced by one that squeezes at the same boundaries (`accepts`);
  * the oracle's create_proof runs as it is on the substituted description, its Transcript replaced likewise and its ScalarStream wrapped so that the advice
    blinding rows and blinds come from their phase-major positions in the stream (`prove`).  The challenge values it needs beforehand come from `phase_loop`,
    which restates only the loop above over the scheme objects' own commit; `prove` asserts that the patched transcript squeezed those same values.

A circuit whose phases are non-decreasing in the column index has its commitments in column order in the proof, which is what the oracle reads and writes: RLC3
is such a circuit, RLC3perm is not and is only ever compared with RLC3 byte for byte."""
from contextlib import contextmanager

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


# ---- substitution -----------------------------------------------------------------------------------------------------------------------------------
def substitute(e, challenges):
    if e[0] == "challenge":
        return ("const", challenges[e[1]])
    return tuple(substitute(x, challenges) if isinstance(x, tuple) else x for x in e)


def substituted_description(cs, challenges):
    d = cs.description()
    gates = tuple(substitute(g, challenges) for g in d[3])
    lookups = tuple((tuple(substitute(e, challenges) for e in i), tuple(substitute(e, challenges) for e in t)) for i, t in d[4])
    return d[:3] + (gates, lookups) + d[5:]


class Layout:
    """where the phase boundaries are, for a circuit whose phases are non-decreasing in the column index"""

    def __init__(self, cs):
        self.phases, self.challenge_phases = cs.phases(), list(cs.challenge_phases)
        assert self.phases == sorted(self.phases), "the oracle reads and writes advice commitments in column order"
        self.num_phases = max(self.phases) + 1
        self.cols = [[c for c, ph in enumerate(self.phases) if ph == q] for q in range(self.num_phases)]
        # after this many advice commitments: the challenges to squeeze, in index order
        self.squeeze_after, done = {}, 0
        for q in range(self.num_phases):
            done += len(self.cols[q])
            self.squeeze_after[done] = [j for j, ph in enumerate(self.challenge_phases) if ph == q]


def phased(base, layout):
    """`base` (the oracle's Transcript or ReadTranscript) squeezing the phases' challenges behind the advice commitments: the first points written / read after
    construction are the advice commitments (instance commitments are absorbed with common_point)."""

    class Phased(base):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.points, self.phase_challenges = 0, {}

        def _point(self):
            self.points += 1
            for j in layout.squeeze_after.get(self.points, ()):
                self.phase_challenges[j] = self.challenge()

        def write_point(self, P):
            super().write_point(P)
            self._point()

        def read_point(self):
            P = super().read_point()
            self._point()
            return P

    return Phased


@contextmanager
def patched(module, attr, value):
    old = getattr(module, attr)
    setattr(module, attr, value)
    try:
        yield
    finally:
        setattr(module, attr, old)


# ---- chains -----------------------------------------------------------------------------------------------------------------------------------------
def chain(pkg, po, co, scheme, k, name="RLC3"):
    """tests/proof_chains.py's chain for RLC3 at k: the key is made from the description with every challenge 0 (keygen reads degrees only), `rep` is taken
    over the description with the challenge nodes and the phases; `adv` is absent -- the witness is a function (`witness_fn`)."""
    import plonk_oracle as PO
    import proof_chains as PC
    cs = build_cs(pkg, name)
    curve = po.VESTA if scheme == "ipa" else po.BN254
    fixed, asm = fixed_columns(k), assembly(pkg, cs, k)
    zero_desc = substituted_description(cs, [0] * len(cs.challenge_phases))
    dummy = np.zeros((cs.num_advice, 1 << k, 4), dtype=np.uint64)
    c = (PC.ipa_chain if scheme == "ipa" else PC.kzg_chain)(po, co, zero_desc, k, fixed, asm.mapping, dummy)
    tagged = (cs.description(), tuple(cs.phases()), tuple(cs.challenge_phases))
    rep_key = dict(c["ipa_key"] if scheme == "ipa" else c["key"], desc=tagged)
    c = dict(c, cs=cs, curve=curve, fixed=fixed, asm=asm, layout=Layout(cs) if name == "RLC3" else None, rep=PO.transcript_repr(curve, rep_key))
    del c["adv"]
    return c


def to_mont(co, curve, po, canonical):
    import plonk_oracle as PO
    fid = PO.Fld(curve.scalar).id
    return np.stack([co.field_op(fid, "to_mont", np.ascontiguousarray(canonical[i])) for i in range(canonical.shape[0])])


def scheme_of(po, c):
    import ipa
    import plonk_oracle as PO
    import proof_chains as PC
    if "u" in c:
        return ipa.ProverIPA(po.VESTA, c["srs"], c["u"], c["w"], PC.THREADS, ipa.DEFAULT_BLIND)
    return PO.ProverGWC(po.BN254, c["srs"], PC.THREADS)


class PhaseMajorStream:
    """The oracle draws every advice column's blinding rows and then every column's blind; upstream draws them phase by phase.  Serves the oracle's first
    num_advice + 1 requests from the phase-major positions of the underlying stream, everything later as it comes."""

    def __init__(self, inner, layout, rows):
        A = len(layout.phases)
        raw = inner.scalars(A * rows + A)
        self.inner, self.queue = inner, []
        col_rows, col_blind, off = {}, {}, 0
        for cols in layout.cols:
            for j, c in enumerate(cols):
                col_rows[c] = raw[off + j * rows:off + (j + 1) * rows]
                col_blind[c] = raw[off + len(cols) * rows + j]
            off += len(cols) * (rows + 1)
        self.queue = [col_rows[c] for c in range(A)] + [np.stack([col_blind[c] for c in range(A)])]
        self.col_rows, self.col_blind = col_rows, col_blind

    def scalars(self, count):
        if self.queue:
            out = self.queue.pop(0)
            assert out.shape[0] == count
            return out.copy()
        return self.inner.scalars(count)


def phase_loop(po, co, c, witness_fn, seed=7):
    """The phase loop alone: -> (the challenges, the final advice in Montgomery form)."""
    import plonk_oracle as PO
    curve, sh, lay = c["curve"], c["key"]["shape"], c["layout"]
    scheme, F = scheme_of(po, c), PO.Fld(c["curve"].scalar)
    rows = sh.n - sh.usable
    stream = PhaseMajorStream(PO.ScalarStream(seed), lay, rows)
    T = PO.Transcript(curve)
    T.common_scalar(c["rep"])
    challenges = [0] * len(lay.challenge_phases)
    adv = None
    for ph in range(lay.num_phases):
        adv = to_mont(co, curve, po, witness_fn(ph, list(challenges)))
        for col in lay.cols[ph]:
            a = adv[col].copy()
            a[sh.usable:] = stream.col_rows[col]
            T.write_point(scheme.commit(c["srs"]["g_lagrange"], a, stream.col_blind[col]))
        for j, q in enumerate(lay.challenge_phases):
            if q == ph:
                challenges[j] = T.challenge()
    return challenges, adv


def prove(po, co, c, witness_fn, seed=7):
    """-> (proof, trace, challenges): the oracle's create_proof / create_proof_ipa on the substituted description, phase squeezes and phase-major draws patched in."""
    import plonk_oracle as PO
    import proof_chains as PC
    challenges, adv = phase_loop(po, co, c, witness_fn, seed)
    desc = substituted_description(c["cs"], challenges)
    sh = PO.Shape(desc, c["k"], c["curve"].scalar)
    key = dict(c["key"], shape=sh, desc=desc)
    made = []

    class Recording(phased(PO.Transcript, c["layout"])):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    rng = PhaseMajorStream(PO.ScalarStream(seed), c["layout"], sh.n - sh.usable)
    with patched(PO, "Transcript", Recording):
        if "u" in c:
            proof, trace = PO.create_proof_ipa(po.VESTA, c["srs"], c["u"], c["w"], key, adv, [], rng, c["rep"], PC.THREADS)
        else:
            proof, trace = PO.create_proof(po.BN254, c["srs"], key, adv, [], rng, c["rep"], PC.THREADS)
    assert [made[0].phase_challenges[j] for j in range(len(challenges))] == challenges, "the restatement squeezed other challenges than the phase loop"
    return proof, trace, challenges


def recover(po, c, proof):
    """the challenges of a proof, read from its advice commitments; None for a proof too short or malformed there"""
    import verifier as V
    T = phased(V.ReadTranscript, c["layout"])(c["curve"], proof)
    T.common_scalar(c["rep"])
    try:
        for _ in range(len(c["layout"].phases)):
            T.read_point()
    except ValueError:
        return None
    return [T.phase_challenges[j] for j in range(len(c["layout"].challenge_phases))]


def accepts(po, c, proof):
    """the scheme's restated verifier, the description substituted with the proof's own challenges"""
    import proof_chains as PC
    import verifier as V
    challenges = recover(po, c, proof)
    if challenges is None:
        return False
    with patched(V, "ReadTranscript", phased(V.ReadTranscript, c["layout"])):
        return PC.accepts(po, dict(c, desc=substituted_description(c["cs"], challenges)), proof, [])


def tampered(c, proof):
    import proof_chains as PC
    return PC.tampered(c, proof)
