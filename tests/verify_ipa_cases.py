"""What the IPA verifier's CPU and GPU suites share: the circuits a native IPA verifier is judged on (the existing IPA chains over Vesta, at the smallest k their
own suites use), their proofs from the ORACLE prover (oracle/plonk_oracle.py with ipa.ProverIPA), the byte offsets of a proof's sections and the oracle's verdicts
(oracle/verifier.py verify_proof_ipa).  TEST INFRASTRUCTURE ONLY.  Every proof and every oracle verdict is computed once per session and shared.

Cases:
  one        maingate at k = 5: gates and a permutation, selectors in the vk, an instance column that holds no value
  phased     RLC3 at k = 6: three advice phases, three challenges, a lookup whose expressions read a challenge
  shuffle    SHUF1 at k = 5: a shuffle and nothing else (no permutation: a key without sigma columns)
  rotations  R9all at k = 6: nine distinct rotations
  instance   one instance column of four values at k = 5: a committed, queried instance column"""
import numpy as np

import phased_circuits as PH
import proof_chains as PC

NAMES = ["one", "phased", "shuffle", "rotations", "instance"]
MALFORMED, OPENING = 1, 3      # dehalo_reject_reason

_cases, _proofs, _verdicts = {}, {}, {}


def case(pkg, po, co, name):
    """-> dict(c: the IPA chain, cs, selectors, N = 1, instances: [circuit][column], witnesses, vk: the blinded key's bytes, fixed, asm: what keygen takes)"""
    if name in _cases:
        return _cases[name]
    import plonk_oracle as PO
    import shuffle_circuits as SC
    import test_ipa_proof
    import test_rotations
    from dehalo2_amd import circuits
    sel = ()
    if name == "one":
        circ = circuits.synthesize(po.VESTA.scalar.p, 5, False, seed=3)
        c = PC.ipa_chain(po, co, circ.cs.description(), 5, circ.fixed, circ.assembly.mapping, circ.advice, circ.selectors)
        cs, sel, wit, fixed, asm = circ.cs, circ.selectors, [c["adv"]], circ.fixed, circ.assembly
    elif name == "phased":
        c = PH.chain(pkg, po, co, "ipa", 6)
        cs, fixed, asm = c["cs"], c["fixed"], c["asm"]
        usable = (1 << 6) - (cs.blinding_factors() + 1)
        wit = [PH.mont_witness(po, co, c, PH.witness(po.VESTA.scalar.p, 6, usable))]
    elif name == "shuffle":
        c = SC.chain(pkg, po, co, "ipa", "SHUF1", 5)
        cs, fixed, asm = c["cs"], c["circ"]["fixed"], c["circ"]["asm"]
        wit = [PH.to_mont(co, po.VESTA, po, c["circ"]["witness"]())]
    elif name == "rotations":
        cs, fixed, advice, asm = test_rotations.build_circuit(pkg, "R9all", 6)
        c = PC.ipa_chain(po, co, cs.description(), 6, fixed, asm.mapping, advice)
        wit = [c["adv"]]
    elif name == "instance":
        cs, desc, values, fixed, advice, asm = test_ipa_proof._instance_circuit(pkg, po, 5)
        c = PC.ipa_chain(po, co, desc, 5, fixed, asm.mapping, advice)
        wit = [c["adv"]]
    else:
        raise ValueError(name)
    inst = [[values]] if name == "instance" else [[[] for _ in range(cs.num_instance)]]
    _cases[name] = dict(name=name, c=c, cs=cs, selectors=sel, N=1, instances=inst, witnesses=wit, vk=PO.vk_bytes(po.VESTA, c["ipa_key"], sel), fixed=fixed, asm=asm)
    return _cases[name]


def proof(pkg, po, co, name, seed=7):
    key = (name, seed)
    if key not in _proofs:
        cz = case(pkg, po, co, name)
        _proofs[key] = PC.prove_circuits(po, cz["c"], cz["witnesses"], cz["instances"], "ipa", seed)[0]
    return _proofs[key]


def oracle_accepts(po, cz, data, instances=None):
    """verify_proof_ipa's verdict on `data`, remembered per (case, bytes, instances)"""
    inst = cz["instances"] if instances is None else instances
    key = (cz["name"], bytes(data), repr(inst))
    if key not in _verdicts:
        _verdicts[key] = PC.accepts(po, cz["c"], bytes(data), inst, "ipa", 1)
    return _verdicts[key]


def sections(po, cz, proof_len):
    """name -> (byte offset of the section's first 32 bytes, "point" | "scalar") for every section a tampered proof is made from: each commitment phase, each kind
    of evaluation, then the multiopen's f, a q evaluation, and the opening's S, an L_j, an R_j, c and f"""
    import plonk_oracle as PO
    sh, k = cz["c"]["key"]["shape"], cz["c"]["k"]
    A, L, S, H, pieces = sh.num_advice, len(sh.lookups), sh.num_sets, len(sh.shuffles), sh.degree - 1
    last = -(sh.blinding_factors + 1)
    out, at = {}, 0
    out["advice commitment"] = (0, "point")
    at += A
    if L:
        out["permuted lookup commitment"] = (32 * at, "point")
    at += 2 * L
    if S + L + H:
        out["product commitment"] = (32 * at, "point")
    at += S + L + H
    out["random commitment"] = (32 * at, "point")
    at += 1
    out["h piece"] = (32 * (at + pieces - 1), "point")
    at += pieces
    order = PO.evaluation_order(sh, 1, True)
    first = lambda pred: next((i for i, (key, r) in enumerate(order) if pred(key, r)), None)
    wanted = {"instance evaluation": lambda key, r: key[0] == "instance", "advice evaluation": lambda key, r: key[0] == "advice",
              "fixed evaluation": lambda key, r: key[0] == "fixed", "random evaluation": lambda key, r: key[0] == "random",
              "sigma evaluation": lambda key, r: key[0] == "sigma", "permutation product at x": lambda key, r: key[0] == "perm_z" and r == 0,
              "permutation product at omega x": lambda key, r: key[0] == "perm_z" and r == 1,
              "permutation product at omega^last x": lambda key, r: key[0] == "perm_z" and r == last, "lookup evaluation": lambda key, r: key[0] == "lookup_a" and r == -1,
              "lookup product evaluation": lambda key, r: key[0] == "lookup_z" and r == 1, "shuffle evaluation": lambda key, r: key[0] == "shuffle_z" and r == 1}
    for label, pred in wanted.items():
        i = first(pred)
        if i is not None:
            out[label] = (32 * (at + i), "scalar")
    out["first evaluation offset"] = (32 * at, "scalar")
    at += len(order)
    tail = 1 + 2 * k + 2                              # S, the rounds' (L_j, R_j), c and f
    ns = proof_len // 32 - at - 1 - tail              # the q evaluations: one per point set
    assert ns >= 1 and proof_len % 32 == 0
    out["multiopen f commitment"] = (32 * at, "point")
    out["first q evaluation"] = (32 * (at + 1), "scalar")
    out["last q evaluation"] = (32 * (at + ns), "scalar")
    at += 1 + ns
    out["opening S"] = (32 * at, "point")
    out["opening L_1"] = (32 * (at + 1), "point")
    out["opening R_1"] = (32 * (at + 2), "point")
    out["opening L_k"] = (32 * (at + 2 * k - 1), "point")
    out["opening R_k"] = (32 * (at + 2 * k), "point")
    out["opening c"] = (32 * (at + 2 * k + 1), "scalar")
    out["opening f"] = (32 * (at + 2 * k + 2), "scalar")
    assert 32 * (at + 2 * k + 3) == proof_len
    return out


def flip(data, offset):
    """the lowest bit of the byte at `offset` flipped"""
    bad = bytearray(data)
    bad[offset] ^= 1
    return bytes(bad)


def expected_reason(po, data, offset, kind):
    """what a reader makes of the 32 bytes at `offset`: MALFORMED where the oracle's ReadTranscript refuses them, else OPENING"""
    from verifier import ReadTranscript
    T = ReadTranscript(po.VESTA, data[offset:offset + 32])
    try:
        T.read_point() if kind == "point" else T.read_scalar()
    except ValueError:
        return MALFORMED
    return OPENING


def host_verifier(pkg, cz, format="raw-unchecked", vk=None, srs=None, w=None, u=None):
    """a host verifier from the raw parts: g, g_lagrange, w, u, the constraint system and the blinded key's vk bytes; the oracle's transcript_repr set"""
    from dehalo2_amd import native
    c = cz["c"]
    srs = c["srs"] if srs is None else srs
    return native.Verifier.from_ipa_host(pkg.fields.VESTA, c["k"], srs["g"], srs["g_lagrange"], c["w"] if w is None else w, c["u"] if u is None else u, cz["cs"],
                                         cz["vk"] if vk is None else vk, num_selectors=len(cz["selectors"]), format=format, transcript_repr=c["rep"])


def verify(v, cz, data, instances=None):
    """-> (accept, reason) of a native verifier on one proof of the case"""
    inst = cz["instances"] if instances is None else instances
    ok = v.verify(data, inst, num_circuits=1)
    return ok, v.last_reject


def vk_in_format(pkg, cz, format):
    """the case's vk bytes in a SerdeFormat: both raw formats are the RawBytes vk, Processed compresses the commitments"""
    from dehalo2_amd import keygen
    raw, key = cz["vk"], cz["c"]["ipa_key"]
    if format != "processed":
        return raw
    count = len(key["fixed_commitments"]) + len(key["perm_commitments"])
    pts = np.frombuffer(raw[8:8 + 64 * count], dtype=np.uint64).reshape(-1, 8)
    return raw[:8] + keygen.commitments_bytes(pkg.fields.VESTA, pts, "processed") + raw[8 + 64 * count:]
