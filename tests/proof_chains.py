"""The chains the whole-proof tests share: SRS, key, transcript representation and advice for one circuit under KZG (BN254) or IPA (Vesta), the
restatements' prove / verify calls on such a chain, and the ten cases whose proofs tests/golden/oracle_proof_digests.json pins.

Every chain takes the SRS trapdoor S_TOXIC and 8 threads; IPA chains take u, w from two seeded fixed-base multiples and blind the key's commitments with
Blind::default().  A chain is a plain dict; `"u" in c` tells an IPA chain from a KZG one."""
import hashlib

import numpy as np

S_TOXIC = 0x2468ACE02468ACE13579BDF13579BDF
THREADS = 8


def _chain(curve, co, desc, k, fixed, mapping, advice):
    import plonk_oracle as PO
    srs = PO.setup_srs(curve, k, S_TOXIC, THREADS)
    key = PO.keygen(curve, srs, desc, k, fixed, mapping, THREADS)
    adv = np.stack([co.field_op(PO.Fld(curve.scalar).id, "to_mont", advice[i]) for i in range(desc[0])])
    return dict(desc=desc, k=k, srs=srs, key=key, adv=adv)


def kzg_chain(po, co, desc, k, fixed, mapping, advice, selectors=()):
    import pairing as pr
    import plonk_oracle as PO
    c = _chain(po.BN254, co, desc, k, fixed, mapping, advice)
    return dict(c, rep=PO.transcript_repr(po.BN254, c["key"], selectors), s_g2=pr.g2_mul(S_TOXIC, pr.G2))


def ipa_chain(po, co, desc, k, fixed, mapping, advice, selectors=()):
    """fc, pc / ipa_key: the key's commitments + [Blind::default()] W, which `rep` is taken over."""
    import ipa
    import plonk_oracle as PO
    c = _chain(po.VESTA, co, desc, k, fixed, mapping, advice)
    uw = co.fixed_base_mul(po.CURVE_IDS["vesta"], co.fill_scalars(po.FIELD_IDS[po.VESTA.scalar.name], "uniform", 2, 7))
    fc, pc = ipa.blinded_key_commitments(po.VESTA, c["key"], uw[1])
    ipa_key = dict(c["key"], fixed_commitments=fc, perm_commitments=pc)
    return dict(c, u=uw[0], w=uw[1], fc=fc, pc=pc, ipa_key=ipa_key, rep=PO.transcript_repr(po.VESTA, ipa_key, selectors))


def scheme_of(po, c, multiopen="gwc"):
    """what create_proof takes as its scheme on chain c: ProverIPA for an IPA chain, else the KZG multiopen's name"""
    import ipa
    return ipa.ProverIPA(po.VESTA, c["srs"], c["u"], c["w"], THREADS, ipa.DEFAULT_BLIND) if "u" in c else multiopen


def prove(po, c, instances, seed=7, **kw):
    """-> (proof, trace) of the scheme's restated prover under ScalarStream(seed)."""
    import plonk_oracle as PO
    instances = [list(v) for v in instances]
    if "u" in c:
        return PO.create_proof_ipa(po.VESTA, c["srs"], c["u"], c["w"], c["key"], c["adv"], instances, PO.ScalarStream(seed), c["rep"], THREADS, **kw)
    return PO.create_proof(po.BN254, c["srs"], c["key"], c["adv"], instances, PO.ScalarStream(seed), c["rep"], THREADS)


def prove_circuits(po, c, witnesses, instances, multiopen="gwc", seed=7):
    """-> (proof, trace) over len(witnesses) circuits of chain c: Montgomery advice arrays or, for a phased key, a function (phase, challenges) -> advice"""
    import plonk_oracle as PO
    curve = po.VESTA if "u" in c else po.BN254
    return PO.create_proof_multi(curve, c["srs"], c["key"], witnesses, instances, PO.ScalarStream(seed), c["rep"], THREADS, scheme_of(po, c, multiopen))


def accepts(po, c, proof, instances, multiopen="gwc", circuits=None):
    """The scheme's restated verifier (KZG: of `multiopen`) on `proof`.  circuits None: over one circuit, `instances` its columns; N: instances[c] circuit c's."""
    import pairing as pr
    import shplonk_oracle
    import verifier as V
    instances = [list(v) for v in instances] if circuits is None else [[list(v) for v in inst] for inst in instances]
    if "u" in c:
        return V.verify_proof_ipa(po.VESTA, c["desc"], c["k"], c["fc"], c["pc"], c["rep"], c["srs"]["g"], c["srs"]["g_lagrange"], c["u"], c["w"], instances, proof,
                                  circuits=circuits)
    verify = shplonk_oracle.verify_proof_shplonk if multiopen == "shplonk" else V.verify_proof
    return verify(po.BN254, c["desc"], c["k"], c["key"]["fixed_commitments"], c["key"]["perm_commitments"], c["rep"], (1, 2), pr.G2, c["s_g2"], instances, proof, circuits)


def phase_challenges(po, c, proof):
    """the phase challenges the verifier squeezes while it reads `proof` (a chain without instance columns); None for a proof malformed before its evaluations end"""
    import verifier as V
    curve, ipa_ = (po.VESTA, True) if "u" in c else (po.BN254, False)
    fc, pc = (c["fc"], c["pc"]) if ipa_ else (c["key"]["fixed_commitments"], c["key"]["perm_commitments"])
    try:
        return V.read_plonk(V.ReadTranscript(curve, proof), curve, c["desc"], c["k"], fc, pc, c["rep"], [], [] if ipa_ else None)[1]
    except ValueError:
        return None


def tampered(c, proof):
    """one evaluation (the second) with one bit flipped"""
    sh = c["key"]["shape"]
    bad = bytearray(proof)
    bad[32 * (sh.num_advice + 3 * len(sh.lookups) + sh.num_sets + 1 + (sh.degree - 1)) + 32 + 5] ^= 0x04
    return bytes(bad)


# ---- the pinned cases ------------------------------------------------------------------------------------------------------------------------------
PINNED = [(scheme, name) for scheme in ("kzg", "ipa") for name in ("maingate_k5", "maingate_range_k9", "R9all_k6", "Rlast_k6", "instance_k5")]


def pinned_case(pkg, po, co, scheme, name):
    """-> (chain, instances) of one case of PINNED.  maingate_*: circuits.synthesize(p, k, range lookups, seed=3); R9all / Rlast: tests/test_rotations.py's
    build_circuit; instance_k5: the one-instance-column circuit of tests/test_ipa_proof.py at the k its CPU test takes."""
    import shapes
    from dehalo2_amd import circuits
    import test_ipa_proof
    import test_rotations

    curve = po.VESTA if scheme == "ipa" else po.BN254
    chain = lambda *a: (ipa_chain if scheme == "ipa" else kzg_chain)(po, co, *a)
    if name.startswith("maingate"):
        k, rl = (9, True) if "range" in name else (5, False)
        circ = circuits.synthesize(curve.scalar.p, k, rl, seed=3)
        desc = shapes.maingate_description(rl)
        assert desc == circ.cs.description()
        return chain(desc, k, circ.fixed, circ.assembly.mapping, circ.advice, circ.selectors), [[]]
    if name == "instance_k5":
        cs, desc, inst, fixed, advice, asm = test_ipa_proof._instance_circuit(pkg, po, 5)
        return chain(desc, 5, fixed, asm.mapping, advice), [inst]
    cs, fixed, advice, asm = test_rotations.build_circuit(pkg, name[:-3], 6)
    return chain(cs.description(), 6, fixed, asm.mapping, advice), []


def digests(proof, trace):
    """what the golden file records of one proof"""
    return dict(proof_sha256=hashlib.sha256(proof).hexdigest(), proof_len=len(proof),
                trace_sha256=hashlib.sha256((repr(trace["commitments"]) + repr(trace["evals"])).encode()).hexdigest(),
                challenges={name: hex(v) for name, v in trace["challenges"].items()})
