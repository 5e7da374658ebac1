"""What the verifier's CPU and GPU suites share: the circuits a native verifier is judged on, their proofs from the ORACLE prover (oracle/plonk_oracle.py
create_proof_multi with "gwc" and "shplonk"), the byte offsets of a proof's sections and the oracle's verdicts.  TEST INFRASTRUCTURE ONLY.  Every proof and every
oracle verdict is computed once per session and shared (a two-pair pairing in Python integers takes a fifth of a second).

Cases (smallest k the circuits' own suites use):
  one        maingate at k = 5: one circuit, gates and a permutation, selectors in the vk
  three      SHUF2 at k = 6 over N = 3 circuits: a lookup, two shuffles, a gate, a permutation
  phased     RLC3 at k = 6: three advice phases, three challenges, a lookup whose expressions read a challenge
  shuffle    SHUF1 at k = 5: a shuffle and nothing else (no permutation: a key without sigma columns)
  rotations  R9all at k = 6: nine distinct rotations
  instance   one instance column of four values at k = 5"""
import numpy as np

import phased_circuits as PH
import proof_chains as PC

NAMES = ["one", "three", "phased", "shuffle", "rotations", "instance"]
MULTIOPENS = ["gwc", "shplonk"]
MALFORMED, PAIRING = 1, 2      # dehalo_reject_reason

_cases, _proofs, _verdicts = {}, {}, {}


def case(pkg, po, co, name):
    """-> dict(c: the chain, cs, selectors, N, instances: [circuit][column], witnesses)"""
    if name in _cases:
        return _cases[name]
    import plonk_oracle as PO
    import shuffle_circuits as SC      # (imports the oracle at its top: only once the oracle's directory is on the path)
    import test_ipa_proof
    import test_rotations
    from dehalo2_amd import circuits
    mont = lambda c, adv: PH.to_mont(co, po.BN254, po, adv)
    sel = ()
    if name == "one":
        circ = circuits.synthesize(po.BN254.scalar.p, 5, False, seed=3)
        c = PC.kzg_chain(po, co, circ.cs.description(), 5, circ.fixed, circ.assembly.mapping, circ.advice, circ.selectors)
        cs, sel, N, inst, wit = circ.cs, circ.selectors, 1, [[]], [c["adv"]]
    elif name == "three":
        c = SC.chain(pkg, po, co, "kzg", "SHUF2", 6)
        cs, N, inst = c["cs"], 3, [[], [], []]
        wit = [mont(c, c["circ"]["witness"](variant=v)) for v in range(3)]
    elif name == "phased":
        c = PH.chain(pkg, po, co, "kzg", 6)
        cs, N, inst = c["cs"], 1, [[]]
        usable = (1 << 6) - (cs.blinding_factors() + 1)
        wit = [PH.mont_witness(po, co, c, PH.witness(po.BN254.scalar.p, 6, usable))]
    elif name == "shuffle":
        c = SC.chain(pkg, po, co, "kzg", "SHUF1", 5)
        cs, N, inst = c["cs"], 1, [[]]
        wit = [mont(c, c["circ"]["witness"]())]
    elif name == "rotations":
        cs, fixed, advice, asm = test_rotations.build_circuit(pkg, "R9all", 6)
        c = PC.kzg_chain(po, co, cs.description(), 6, fixed, asm.mapping, advice)
        N, inst, wit = 1, [[]], [c["adv"]]
    elif name == "instance":
        cs, desc, values, fixed, advice, asm = test_ipa_proof._instance_circuit(pkg, po, 5)
        c = PC.kzg_chain(po, co, desc, 5, fixed, asm.mapping, advice)
        N, inst, wit = 1, [[values]], [c["adv"]]
    else:
        raise ValueError(name)
    if name != "instance":      # (maingate has an instance column that holds no value)
        inst = [[[] for _ in range(cs.num_instance)] for _ in range(N)]
    if name == "one":
        fixed, asm = circ.fixed, circ.assembly
    elif name in ("three", "shuffle"):
        fixed, asm = c["circ"]["fixed"], c["circ"]["asm"]
    elif name == "phased":
        fixed, asm = c["fixed"], c["asm"]
    _cases[name] = dict(name=name, c=c, cs=cs, selectors=sel, N=N, instances=inst, witnesses=wit, vk=PO.vk_bytes(po.BN254, c["key"], sel), fixed=fixed, asm=asm)
    return _cases[name]


def proof(pkg, po, co, name, multiopen, seed=7):
    key = (name, multiopen, seed)
    if key not in _proofs:
        cz = case(pkg, po, co, name)
        _proofs[key] = PC.prove_circuits(po, cz["c"], cz["witnesses"], cz["instances"], multiopen, seed)[0]
    return _proofs[key]


def oracle_accepts(po, cz, data, multiopen, instances=None):
    """the oracle's verdict on `data`, remembered per (case, multiopen, bytes, instances)"""
    inst = cz["instances"] if instances is None else instances
    key = (cz["name"], multiopen, bytes(data), repr(inst))
    if key not in _verdicts:
        _verdicts[key] = PC.accepts(po, cz["c"], bytes(data), inst, multiopen, cz["N"])
    return _verdicts[key]


def sections(po, cz, multiopen):
    """name -> (byte offset of the section's first 32 bytes, "point" | "scalar") for every section a tampered proof is made from"""
    import plonk_oracle as PO
    sh, N = cz["c"]["key"]["shape"], cz["N"]
    A, L, S, H, pieces = sh.num_advice, len(sh.lookups), sh.num_sets, len(sh.shuffles), sh.degree - 1
    last = -(sh.blinding_factors + 1)
    out, at = {}, 0
    out["advice commitment"] = (0, "point")
    at += N * A
    if L:
        out["permuted lookup commitment"] = (32 * at, "point")
    at += 2 * L * N
    if S + L + H:
        out["product commitment"] = (32 * at, "point")
    at += N * (S + L + H)
    out["random commitment"] = (32 * at, "point")
    at += 1
    out["h piece"] = (32 * (at + pieces - 1), "point")
    at += pieces
    order = PO.evaluation_order(sh, N)
    first = lambda pred: next((i for i, (k, r) in enumerate(order) if pred(k, r)), None)
    wanted = {"advice evaluation": lambda k, r: k[0] == "advice", "fixed evaluation": lambda k, r: k[0] == "fixed", "random evaluation": lambda k, r: k[0] == "random",
              "sigma evaluation": lambda k, r: k[0] == "sigma", "permutation product at x": lambda k, r: k[0] == "perm_z" and r == 0,
              "permutation product at omega x": lambda k, r: k[0] == "perm_z" and r == 1, "permutation product at omega^last x": lambda k, r: k[0] == "perm_z" and r == last,
              "lookup evaluation": lambda k, r: k[0] == "lookup_a" and r == -1, "lookup product evaluation": lambda k, r: k[0] == "lookup_z" and r == 1,
              "shuffle evaluation": lambda k, r: k[0] == "shuffle_z" and r == 1}
    for label, pred in wanted.items():
        i = first(pred)
        if i is not None:
            out[label] = (32 * (at + i), "scalar")
    at += len(order)
    total = PO.proof_length(sh, N, multiopen)
    assert total > 32 * at
    out["last multiopen commitment"] = (total - 32, "point")
    out["first evaluation offset"] = (32 * at - 32 * len(order), "scalar")
    return out


def flip(data, offset):
    """the lowest bit of the byte at `offset` flipped"""
    bad = bytearray(data)
    bad[offset] ^= 1
    return bytes(bad)


def expected_reason(po, data, offset, kind):
    """what a reader makes of the 32 bytes at `offset`: MALFORMED where the oracle's ReadTranscript refuses them, else PAIRING"""
    from verifier import ReadTranscript
    T = ReadTranscript(po.BN254, data[offset:offset + 32])
    try:
        T.read_point() if kind == "point" else T.read_scalar()
    except ValueError:
        return MALFORMED
    return PAIRING


def g2_raw(c):
    import pairing as pr
    return pr.g2_to_raw(pr.G2), pr.g2_to_raw(c["s_g2"])


def host_verifier(pkg, cz, multiopen="gwc", format="raw-unchecked", vk=None, s_g2=None, ctx=None):
    """a verifier from the raw parts: g[0], g2, s_g2, the constraint system and the vk bytes; the oracle's transcript_repr set"""
    from dehalo2_amd import native
    c = cz["c"]
    g2, sg2 = g2_raw(c)
    return native.Verifier.from_vk(pkg.fields.BN254, c["k"], np.asarray(c["srs"]["g"][0]), g2, sg2 if s_g2 is None else s_g2, cz["cs"], cz["vk"] if vk is None else vk,
                                   num_selectors=len(cz["selectors"]), format=format, ctx=ctx, multiopen=multiopen, transcript_repr=c["rep"])


def verify(v, cz, data, instances=None):
    """-> (accept, reason) of a native verifier on one proof of the case"""
    inst = cz["instances"] if instances is None else instances
    ok = v.verify(data, inst, num_circuits=cz["N"])
    return ok, v.last_reject


def vk_in_format(pkg, cz, format):
    """the case's vk bytes in a SerdeFormat: both raw formats are the RawBytes vk, Processed compresses the commitments (the Python mirror's codec)"""
    from dehalo2_amd import keygen
    raw, key = cz["vk"], cz["c"]["key"]
    if format != "processed":
        return raw
    count = len(key["fixed_commitments"]) + len(key["perm_commitments"])
    pts = np.frombuffer(raw[8:8 + 64 * count], dtype=np.uint64).reshape(-1, 8)
    return raw[:8] + keygen.commitments_bytes(pkg.fields.BN254, pts, "processed") + raw[8 + 64 * count:]
