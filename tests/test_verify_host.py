"""CPU suite: verify_proof for KZG on the HOST verifier (ctx = None: csrc/verify_host.hpp behind dehalo_verifier_create_vk / dehalo_verify_proof(s)) against the
oracle's verifiers (oracle/verifier.py verify_proof, tests/shplonk_oracle.py verify_proof_shplonk).

Proofs come from the ORACLE prover (tests/verify_cases.py: one circuit, N = 3 circuits, a phased key with challenges, a shuffle, nine rotations, instance
values; GWC and SHPLONK).  Per case: the valid proof is accepted by both; one flipped bit in every section of the proof -- commitments of every kind, one
evaluation of every class, the last multiopen commitment -- is rejected by both, with reason PAIRING, or MALFORMED where the flipped bytes are no point (derived
from the oracle's ReadTranscript); truncation, a trailing byte and a scalar equal to r are MALFORMED; a wrong instance value, a wrong transcript_repr and the s_g2
of another secret are PAIRING.  A verifier from the vk in each SerdeFormat gives the same verdicts.  Batches: three valid proofs, each position tampered in turn, an
unreadable proof, count = 1, and the weight schedule pinned through DEHALO_RNG_CALLBACK.  tests/native_host/verify_host_check.cpp runs verify_host.hpp on one valid and
one tampered proof under ASan + UBSan, as a program of its own."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import verify_cases as VC
from conftest import ROOT

R_BN254 = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


@pytest.fixture(scope="module")
def get(pkg, po, co):
    """(case name, multiopen) -> (case, proof, host verifier), made once"""
    made = {}

    def fn(name, multiopen):
        if (name, multiopen) not in made:
            cz = VC.case(pkg, po, co, name)
            made[(name, multiopen)] = (cz, VC.proof(pkg, po, co, name, multiopen), VC.host_verifier(pkg, cz, multiopen))
        return made[(name, multiopen)]
    return fn


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
@pytest.mark.parametrize("name", VC.NAMES)
def test_valid_proof_is_accepted_by_both(po, get, name, multiopen):
    cz, proof, v = get(name, multiopen)
    assert VC.oracle_accepts(po, cz, proof, multiopen) is True
    assert VC.verify(v, cz, proof) == (True, 0)
    assert VC.verify(v, cz, proof) == (True, 0)      # and again: no state is kept between calls


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
@pytest.mark.parametrize("name", VC.NAMES)
def test_one_flipped_bit_in_every_section_is_rejected_by_both(po, get, name, multiopen):
    cz, proof, v = get(name, multiopen)
    secs = VC.sections(po, cz, multiopen)
    del secs["first evaluation offset"]
    sh = cz["c"]["key"]["shape"]
    must = {"advice commitment", "random commitment", "h piece", "advice evaluation", "random evaluation", "last multiopen commitment"}
    must |= {"fixed evaluation"} if sh.fixed_queries else set()
    must |= {"sigma evaluation", "product commitment", "permutation product at x", "permutation product at omega x"} if sh.perm_columns else set()
    must |= {"permutation product at omega^last x"} if sh.num_sets > 1 else set()
    must |= {"permuted lookup commitment", "lookup evaluation", "lookup product evaluation"} if sh.lookups else set()
    must |= {"shuffle evaluation"} if sh.shuffles else set()
    assert must <= set(secs), sorted(must - set(secs))
    for label, (off, kind) in secs.items():
        bad = VC.flip(proof, off)
        want = VC.expected_reason(po, bad, off, kind)
        assert VC.oracle_accepts(po, cz, bad, multiopen) is False, label
        assert VC.verify(v, cz, bad) == (False, want), (label, want)
    assert VC.verify(v, cz, proof) == (True, 0)


def test_the_cases_cover_every_section(po, get):
    """over all cases every section of a proof is tampered somewhere, and both reasons occur among the flipped commitments"""
    seen, reasons = set(), set()
    for name in VC.NAMES:
        cz, proof, _ = get(name, "gwc")
        for label, (off, kind) in VC.sections(po, cz, "gwc").items():
            seen.add(label)
            if kind == "point":
                reasons.add(VC.expected_reason(po, VC.flip(proof, off), off, kind))
    assert {"permuted lookup commitment", "product commitment", "shuffle evaluation", "lookup evaluation", "permutation product at omega^last x", "sigma evaluation",
            "fixed evaluation"} <= seen
    assert reasons == {VC.MALFORMED, VC.PAIRING}


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
@pytest.mark.parametrize("name", VC.NAMES)
def test_malformed_proofs(po, get, name, multiopen):
    cz, proof, v = get(name, multiopen)
    first_eval = VC.sections(po, cz, multiopen)["first evaluation offset"][0]
    r_scalar = proof[:first_eval] + R_BN254.to_bytes(32, "little") + proof[first_eval + 32:]
    for label, bad in (("truncated by 1", proof[:-1]), ("truncated by 32", proof[:-32]), ("one trailing byte", proof + b"\0"), ("a scalar replaced by r", r_scalar),
                       ("empty", b"")):
        assert VC.oracle_accepts(po, cz, bad, multiopen) is False, label
        assert VC.verify(v, cz, bad) == (False, VC.MALFORMED), label


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
def test_wrong_public_inputs_fail_the_pairing(pkg, po, co, get, multiopen):
    import pairing as pr
    cz, proof, v = get("instance", multiopen)
    wrong = [[list(cz["instances"][0][0])]]
    wrong[0][0][2] += 1
    assert VC.oracle_accepts(po, cz, proof, multiopen, wrong) is False
    assert VC.verify(v, cz, proof, wrong) == (False, VC.PAIRING)
    shorter = [[list(cz["instances"][0][0])[:-1]]]      # a missing value is a wrong value
    assert VC.verify(v, cz, proof, shorter) == (False, VC.PAIRING) and VC.oracle_accepts(po, cz, proof, multiopen, shorter) is False
    assert VC.verify(v, cz, proof) == (True, 0)
    # transcript_repr
    cz, proof, _ = get("one", multiopen)
    v2 = VC.host_verifier(pkg, cz, multiopen)
    assert VC.verify(v2, cz, proof) == (True, 0)
    v2.transcript_repr = cz["c"]["rep"] + 1
    assert VC.verify(v2, cz, proof) == (False, VC.PAIRING)
    v2.transcript_repr = cz["c"]["rep"]
    assert VC.verify(v2, cz, proof) == (True, 0)
    v2.release()
    # s_g2 of another secret
    v3 = VC.host_verifier(pkg, cz, multiopen, s_g2=pr.g2_to_raw(pr.g2_mul(VC.PC.S_TOXIC + 1, pr.G2)))
    assert VC.verify(v3, cz, proof) == (False, VC.PAIRING)
    v3.release()


def test_the_other_multiopens_proof_is_rejected(po, get):
    for name in ("one", "shuffle"):      # SHUF1's two proofs have the same length: the bytes are read, and fail the pairing
        cz, gwc, v_gwc = get(name, "gwc")
        _, shp, v_shp = get(name, "shplonk")
        assert VC.verify(v_gwc, cz, shp)[0] is False and VC.oracle_accepts(po, cz, shp, "gwc") is False
        assert VC.verify(v_shp, cz, gwc)[0] is False and VC.oracle_accepts(po, cz, gwc, "shplonk") is False


def test_callers_errors(pkg, po, co, get):
    from dehalo2_amd import native
    cz, proof, v = get("instance", "gwc")
    for bad in ([[]], [[[5, 7, 9, 11], [1]]]):                                  # no column, two columns
        with pytest.raises(pkg.DehaloError) as e:
            v.verify(proof, bad, num_circuits=1)
        assert e.value.code == -1
    usable = (1 << cz["c"]["k"]) - (cz["cs"].blinding_factors() + 1)
    with pytest.raises(pkg.DehaloError) as e:
        v.verify(proof, [[[1] * (usable + 1)]], num_circuits=1)
    assert e.value.code == -1
    # a column of exactly the usable rows is the caller's right; its values are absorbed one by one, so trailing zeros make another statement
    longest = [[[5, 7, 9, 11] + [0] * (usable - 4)]]
    assert VC.verify(v, cz, proof, longest) == (False, VC.PAIRING) and VC.oracle_accepts(po, cz, proof, "gwc", longest) is False
    cz1, proof1, v1 = get("one", "gwc")
    assert cz1["cs"].num_instance == 1
    with pytest.raises(pkg.DehaloError) as e:
        v1.verify(proof1, [[[], []]], num_circuits=1)
    assert e.value.code == -1
    lib = pkg.load_library()
    acc = C.c_int(7)
    assert lib.dehalo_verify_proof(None, None, None, 0, 1, proof, len(proof), C.byref(acc), None) == -1
    assert lib.dehalo_verify_proof(v.handle, None, None, 1, 0, proof, len(proof), C.byref(acc), None) == -1      # no circuit
    assert lib.dehalo_verifier_set_multiopen(v.handle, 2) == -1 and lib.dehalo_verifier_set_multiopen(None, 0) == -1
    assert lib.dehalo_verifier_release(None) == 0


def test_a_refused_call_draws_nothing_and_a_failed_constructor_says_why(pkg, po, co, get):
    """the caller's errors come before the weights are drawn: the generator of a refused batch is where it was; a host verifier's constructor, which has no
    context to leave its message with, reports it through dehalo_verifier_create_error"""
    cz, proof, v = get("instance", "gwc")
    w = Weights(pkg.fields.BN254.scalar, [5, 6])
    with pytest.raises(pkg.DehaloError) as e:
        v.verify_batch([proof, proof, proof], [[[]], [[]], [[]]], rng=w, num_circuits=1)      # no instance column
    assert e.value.code == -1 and w.drawn == 0 and "num_instance_columns" in str(e.value)
    assert v.verify_batch([proof, proof, proof], [cz["instances"]] * 3, rng=w, num_circuits=1) is True and w.drawn == 2
    g2, s_g2 = VC.g2_raw(cz["c"])
    for kw, text in ((dict(s_g2=bytes(128)), "s_g2"), (dict(vk=cz["vk"][:-1]), "length"), (dict(vk=b"\0" * 3), "length")):
        with pytest.raises(pkg.DehaloError) as e:
            VC.host_verifier(pkg, cz, **kw)
        assert e.value.code == -1 and text in str(e.value), str(e.value)
    from dehalo2_amd import native
    R = native.Blake2bRead(pkg.fields.BN254, proof)
    with pytest.raises(TypeError):
        R.write_scalar(1)


@pytest.mark.parametrize("curve", ["PALLAS", "VESTA"])
def test_pasta_is_unsupported(pkg, po, co, get, curve):
    from dehalo2_amd import native
    cz, _, _ = get("shuffle", "gwc")
    g2, s_g2 = VC.g2_raw(cz["c"])
    with pytest.raises(pkg.DehaloError) as e:
        native.Verifier.from_vk(getattr(pkg.fields, curve), cz["c"]["k"], np.zeros(8, dtype=np.uint64), g2, s_g2, cz["cs"], cz["vk"])
    assert e.value.code == -5


def test_constructor_checks_g2_and_the_vk(pkg, po, co, get):
    import pairing as pr
    cz, proof, _ = get("one", "gwc")
    g2, s_g2 = VC.g2_raw(cz["c"])
    off = bytearray(s_g2)
    off[64] ^= 1
    for bad in (bytes(off), bytes(128)):      # off the twist; the identity
        with pytest.raises(pkg.DehaloError) as e:
            VC.host_verifier(pkg, cz, s_g2=bad)
        assert e.value.code == -1
    for bad_vk in (cz["vk"][:-1], cz["vk"] + b"\0", struct.pack(">I", 6) + cz["vk"][4:], b""):
        with pytest.raises(pkg.DehaloError) as e:
            VC.host_verifier(pkg, cz, vk=bad_vk)
        assert e.value.code == -1
    broken = bytearray(cz["vk"])
    broken[8 + 32] ^= 1                        # fixed commitment 0's y: off the curve
    with pytest.raises(pkg.DehaloError):
        VC.host_verifier(pkg, cz, vk=bytes(broken), format="raw")
    v = VC.host_verifier(pkg, cz, vk=bytes(broken), format="raw-unchecked")      # copied in unseen: the proof then fails
    assert VC.verify(v, cz, proof)[0] is False
    v.release()


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
def test_every_serde_format_gives_the_same_verdicts(pkg, po, co, get, multiopen):
    from dehalo2_amd import keygen
    cz, proof, v_raw = get("one", multiopen)
    curve, key, c = pkg.fields.BN254, cz["c"]["key"], cz["c"]
    nf, npc = len(key["fixed_commitments"]), len(key["perm_commitments"])
    raw = cz["vk"]
    pts = np.frombuffer(raw[8:8 + 64 * (nf + npc)], dtype=np.uint64).reshape(-1, 8)
    processed = raw[:8] + keygen.commitments_bytes(curve, pts, "processed") + raw[8 + 64 * (nf + npc):]
    assert len(processed) == len(raw) - 32 * (nf + npc)
    # selectors ride behind the commitments, 2^k bits each: they lengthen the key and feed the substitute transcript_repr only
    sel = bytes(range(1, 1 + (1 << cz["c"]["k"]) // 8))
    v_sel = VC.host_verifier(pkg, dict(cz, selectors=[None, None]), multiopen, format="processed", vk=processed + sel + sel)
    assert VC.verify(v_sel, cz, proof) == (True, 0)
    v_sel.release()
    with pytest.raises(pkg.DehaloError):
        VC.host_verifier(pkg, dict(cz, selectors=[None, None]), multiopen, format="processed", vk=processed + sel)
    secs = VC.sections(po, cz, multiopen)
    probes = [proof, VC.flip(proof, secs["sigma evaluation"][0]), VC.flip(proof, secs["h piece"][0]), proof[:-32]]
    want = [VC.verify(v_raw, cz, p) for p in probes]
    assert want[0] == (True, 0) and not any(w[0] for w in want[1:])
    for fmt, data in (("processed", processed), ("raw", raw), ("raw-unchecked", raw)):
        v = VC.host_verifier(pkg, cz, multiopen, format=fmt, vk=data)
        assert [VC.verify(v, cz, p) for p in probes] == want, fmt
        v.release()
    with pytest.raises(pkg.DehaloError):      # the raw bytes are no Processed key
        VC.host_verifier(pkg, cz, multiopen, format="processed", vk=raw)


def test_default_transcript_repr_is_keygens_substitute(pkg, po, co, get):
    """until it is set, a from_vk verifier's transcript_repr is a function of the vk bytes and the circuit alone: the same for every format, another for another key"""
    from dehalo2_amd import native
    cz, proof, _ = get("one", "gwc")
    c = cz["c"]
    g2, s_g2 = VC.g2_raw(c)
    v = native.Verifier.from_vk(pkg.fields.BN254, c["k"], np.asarray(c["srs"]["g"][0]), g2, s_g2, cz["cs"], cz["vk"], num_selectors=len(cz["selectors"]))
    assert VC.verify(v, cz, proof) == (False, VC.PAIRING)      # the proof was made under the oracle's representation, not the substitute
    v.transcript_repr = c["rep"]
    assert VC.verify(v, cz, proof) == (True, 0)
    v.release()


# ------------------------------------------------------------------------------------------------------------------------------ batches
class Weights:
    """a DEHALO_RNG_CALLBACK generator that hands out the given scalars, in order"""

    def __init__(self, field, values):
        self.field, self.values, self.drawn = field, list(values), 0

    def scalars(self, count):
        out = self.field.encode_many(self.values[self.drawn:self.drawn + count])
        assert out.shape[0] == count, "the library drew more scalars than count - 1"
        self.drawn += count
        return out


@pytest.fixture(scope="module")
def batch(pkg, po, co, get):
    cz, _, _ = get("one", "gwc")
    return {mo: [VC.proof(pkg, po, co, "one", mo, seed) for seed in (7, 8, 9)] for mo in VC.MULTIOPENS}


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
def test_batch_accepts_and_rejects(pkg, po, get, batch, multiopen):
    cz, _, v = get("one", multiopen)
    proofs = batch[multiopen]
    assert len(set(proofs)) == 3 and all(VC.oracle_accepts(po, cz, p, multiopen) for p in proofs)
    inst = [cz["instances"]] * 3
    assert v.verify_batch(proofs, inst, num_circuits=1) is True and v.first_malformed == -1 and v.last_reject == 0
    off = VC.sections(po, cz, multiopen)["advice evaluation"][0]
    for i in range(3):
        bad = list(proofs)
        bad[i] = VC.flip(bad[i], off)
        assert v.verify_batch(bad, inst, num_circuits=1) is False and v.first_malformed == -1 and v.last_reject == VC.PAIRING, i
    bad = [proofs[0], proofs[1][:-1], proofs[2] + b"\0"]
    assert v.verify_batch(bad, inst, num_circuits=1) is False and v.first_malformed == 1 and v.last_reject == VC.MALFORMED
    # count = 1 is the single call
    for p in (proofs[0], VC.flip(proofs[0], off), proofs[0][:-32]):
        single = VC.verify(v, cz, p)
        assert v.verify_batch([p], [cz["instances"]], num_circuits=1) is single[0] and v.last_reject == single[1]
    assert v.verify_batch([], [], num_circuits=1) is True      # the empty product


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
def test_batch_weight_schedule(pkg, po, get, batch, multiopen):
    """w_0 = 1 and w_1 = the first scalar drawn: the same PAIRING-tampered proof twice under w_1 = r - 1 sums to the identity on both sides and passes -- which
    is why the weights must be unpredictable to whoever made the proofs -- and fails under w_1 = 1 and under the library's own entropy"""
    cz, _, v = get("one", multiopen)
    f = pkg.fields.BN254.scalar
    bad = VC.flip(batch[multiopen][0], VC.sections(po, cz, multiopen)["advice evaluation"][0])
    assert VC.verify(v, cz, bad) == (False, VC.PAIRING)
    inst = [cz["instances"]] * 2
    w = Weights(f, [R_BN254 - 1])
    assert v.verify_batch([bad, bad], inst, rng=w, num_circuits=1) is True and w.drawn == 1
    w = Weights(f, [1])
    assert v.verify_batch([bad, bad], inst, rng=w, num_circuits=1) is False and w.drawn == 1 and v.last_reject == VC.PAIRING
    assert v.verify_batch([bad, bad], inst, rng=None, num_circuits=1) is False
    # three proofs draw two scalars, in order: w_2 = r - 1 cancels proof 2 against proof 0 only when proof 1 is valid and w_1 is whatever comes first
    good = batch[multiopen][1]
    w = Weights(f, [12345, R_BN254 - 1])
    assert v.verify_batch([bad, good, bad], [cz["instances"]] * 3, rng=w, num_circuits=1) is True and w.drawn == 2
    w = Weights(f, [R_BN254 - 1, 12345])
    assert v.verify_batch([bad, good, bad], [cz["instances"]] * 3, rng=w, num_circuits=1) is False
    txt = open(os.path.join(ROOT, "include", "dehalo.h")).read()
    assert "UNPREDICTABLE TO WHOEVER MADE THE PROOFS" in txt


def test_batch_of_multi_circuit_proofs(pkg, po, co, get):
    cz, proof, v = get("three", "shplonk")
    other = VC.proof(pkg, po, co, "three", "shplonk", 11)
    assert other != proof
    assert v.verify_batch([proof, other], [cz["instances"]] * 2, num_circuits=3) is True
    bad = VC.flip(other, VC.sections(po, cz, "shplonk")["shuffle evaluation"][0])
    assert v.verify_batch([proof, bad], [cz["instances"]] * 2, num_circuits=3) is False and v.first_malformed == -1


# ------------------------------------------------------------------------------------------------------------------------------ verify_host.hpp alone, sanitized
def _descriptor_bytes(desc):
    """a dehalo_constraint_system as flat little-endian words, for the stand-alone program: counts, then every array"""
    d = desc.struct
    u32s = lambda ptr, n: [int(ptr[i]) for i in range(n)]
    total_l = sum(u32s(d.lookup_lens, d.num_lookups))
    total_s = sum(u32s(d.shuffle_lens, d.num_shuffles))
    out = struct.pack("<12I", d.num_advice, d.num_fixed, d.num_instance, d.minimum_degree, d.num_nodes, d.num_constants, d.num_gates, d.num_lookups,
                      d.num_permutation_columns, d.num_advice_queries, d.num_fixed_queries, d.num_instance_queries)
    out += struct.pack("<2I", d.num_challenges, d.num_shuffles)
    for i in range(d.num_nodes):
        e = d.nodes[i]
        out += struct.pack("<IIIi", e.kind, e.a, e.b, e.rotation)
    out += C.string_at(d.constants, 32 * d.num_constants) if d.num_constants else b""
    out += struct.pack("<%dI" % d.num_gates, *u32s(d.gates, d.num_gates))
    out += struct.pack("<%dI" % d.num_lookups, *u32s(d.lookup_lens, d.num_lookups))
    out += struct.pack("<%dI" % total_l, *u32s(d.lookup_inputs, total_l)) + struct.pack("<%dI" % total_l, *u32s(d.lookup_tables, total_l))
    for arr, n in ((d.permutation_columns, d.num_permutation_columns), (d.advice_queries, d.num_advice_queries), (d.fixed_queries, d.num_fixed_queries),
                   (d.instance_queries, d.num_instance_queries)):
        for i in range(n):
            out += struct.pack("<IIi", arr[i].kind, arr[i].index, arr[i].rotation)
    out += C.string_at(d.advice_phases, d.num_advice) if d.advice_phases else bytes(d.num_advice)
    out += C.string_at(d.challenge_phases, d.num_challenges) if d.num_challenges else b""
    out += struct.pack("<%dI" % d.num_shuffles, *u32s(d.shuffle_lens, d.num_shuffles))
    out += struct.pack("<%dI" % total_s, *u32s(d.shuffle_inputs, total_s)) + struct.pack("<%dI" % total_s, *u32s(d.shuffle_tables, total_s))
    return out


@pytest.mark.parametrize("name,multiopen", [("phased", "gwc"), ("three", "shplonk")])
def test_sanitized_program_gives_the_same_verdicts(pkg, po, co, get, tmp_path, name, multiopen):
    from dehalo2_amd import native
    out = subprocess.run(["make", "-C", ROOT, "verify_host_check"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    cz, proof, v = get(name, multiopen)
    c = cz["c"]
    g2, s_g2 = VC.g2_raw(c)
    desc = native.ConstraintSystemDescriptor(cz["cs"], pkg.fields.BN254.scalar)
    bad = VC.flip(proof, VC.sections(po, cz, multiopen)["advice evaluation"][0])
    blob = struct.pack("<5I", c["k"], len(cz["selectors"]), cz["N"], 1 if multiopen == "shplonk" else 0, len(cz["vk"]))
    blob += np.asarray(c["srs"]["g"][0], dtype=np.uint64).tobytes() + g2 + s_g2 + pkg.fields.BN254.scalar.encode(c["rep"]).tobytes() + cz["vk"] + _descriptor_bytes(desc)
    for p in (proof, bad, proof[:-1]):
        blob += struct.pack("<I", len(p)) + p
    path = tmp_path / "case.bin"
    path.write_bytes(blob)
    r = subprocess.run([os.path.join(ROOT, "tests", "native_host", "verify_host_check"), str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    want = [VC.verify(v, cz, p) for p in (proof, bad, proof[:-1])]
    assert want == [(True, 0), (False, VC.PAIRING), (False, VC.MALFORMED)]
    assert r.stdout.split() == ["%d:%d" % (int(a), b) for a, b in want]
