"""verify_proof for IPA on the HOST (dehalo_verifier_create_ipa_host: no context, no GPU): the native verifier against the oracle's (oracle/verifier.py
verify_proof_ipa) on the proofs of the ORACLE prover over Vesta -- maingate, RLC3 (phases), SHUF1, R9all, and a circuit with a committed instance column.

Every valid proof is accepted by both; one flipped bit in every section of a proof (each commitment phase, each kind of evaluation, the multiopen's f and q
evaluations, the opening's S, an L_j, an R_j, c and f) is rejected by both, with the reason the bytes dictate (MALFORMED exactly where a read fails -- decided
from the oracle's ReadTranscript -- else OPENING); truncation, a trailing byte and a scalar equal to r are MALFORMED; wrong public inputs, a wrong transcript_repr,
another key and another W are OPENING; the three vk formats give the same verdicts; batches: accepted, rejected, first_malformed, and the weight schedule pinned
through DEHALO_RNG_CALLBACK.  tests/native_host/verify_ipa_host_check.cpp runs verify_host.hpp on one valid, one tampered and one truncated proof under ASan + UBSan."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import verify_ipa_cases as VI
from conftest import ROOT
from test_verify_host import Weights, _descriptor_bytes

R_VESTA = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001      # the order of Vesta = the modulus of its scalar field (pasta Fp)


@pytest.fixture(scope="module")
def get(pkg, po, co):
    """case name -> (case, proof, host verifier), made once"""
    made = {}

    def fn(name):
        if name not in made:
            assert R_VESTA == po.VESTA.scalar.p
            cz = VI.case(pkg, po, co, name)
            made[name] = (cz, VI.proof(pkg, po, co, name), VI.host_verifier(pkg, cz))
        return made[name]
    return fn


@pytest.mark.parametrize("name", VI.NAMES)
def test_valid_proof_is_accepted_by_both(po, get, name):
    cz, proof, v = get(name)
    assert VI.oracle_accepts(po, cz, proof) is True
    assert VI.verify(v, cz, proof) == (True, 0)
    assert VI.verify(v, cz, proof) == (True, 0)      # and again: no state is kept between calls


@pytest.mark.parametrize("name", VI.NAMES)
def test_one_flipped_bit_in_every_section_is_rejected_by_both(po, get, name):
    cz, proof, v = get(name)
    secs = VI.sections(po, cz, len(proof))
    del secs["first evaluation offset"]
    sh = cz["c"]["key"]["shape"]
    must = {"advice commitment", "random commitment", "h piece", "advice evaluation", "random evaluation", "multiopen f commitment", "first q evaluation",
            "last q evaluation", "opening S", "opening L_1", "opening R_1", "opening L_k", "opening R_k", "opening c", "opening f"}
    must |= {"fixed evaluation"} if sh.fixed_queries else set()
    must |= {"instance evaluation"} if sh.instance_queries else set()
    must |= {"sigma evaluation", "product commitment", "permutation product at x", "permutation product at omega x"} if sh.perm_columns else set()
    must |= {"permutation product at omega^last x"} if sh.num_sets > 1 else set()
    must |= {"permuted lookup commitment", "lookup evaluation", "lookup product evaluation"} if sh.lookups else set()
    must |= {"shuffle evaluation"} if sh.shuffles else set()
    assert must <= set(secs), sorted(must - set(secs))
    for label, (off, kind) in secs.items():
        bad = VI.flip(proof, off)
        want = VI.expected_reason(po, bad, off, kind)
        assert VI.oracle_accepts(po, cz, bad) is False, label
        assert VI.verify(v, cz, bad) == (False, want), (label, want)
    assert VI.verify(v, cz, proof) == (True, 0)


def test_the_cases_cover_every_section(po, get):
    """over all cases every section of a proof is tampered somewhere, and both reasons occur among the flipped commitments"""
    seen, reasons = set(), set()
    for name in VI.NAMES:
        cz, proof, _ = get(name)
        for label, (off, kind) in VI.sections(po, cz, len(proof)).items():
            seen.add(label)
            if kind == "point":
                reasons.add(VI.expected_reason(po, VI.flip(proof, off), off, kind))
    assert {"permuted lookup commitment", "product commitment", "shuffle evaluation", "lookup evaluation", "permutation product at omega^last x", "sigma evaluation",
            "fixed evaluation", "instance evaluation", "multiopen f commitment", "first q evaluation", "opening S", "opening L_1", "opening R_k", "opening c",
            "opening f"} <= seen
    assert reasons == {VI.MALFORMED, VI.OPENING}


@pytest.mark.parametrize("name", VI.NAMES)
def test_malformed_proofs(po, get, name):
    cz, proof, v = get(name)
    secs = VI.sections(po, cz, len(proof))
    r = R_VESTA.to_bytes(32, "little")
    put = lambda off: proof[:off] + r + proof[off + 32:]
    for label, bad in (("truncated by 1", proof[:-1]), ("truncated by 32", proof[:-32]), ("one trailing byte", proof + b"\0"), ("32 trailing bytes", proof + proof[-32:]),
                       ("an evaluation replaced by r", put(secs["first evaluation offset"][0])), ("a q evaluation replaced by r", put(secs["last q evaluation"][0])),
                       ("c replaced by r", put(secs["opening c"][0])), ("empty", b"")):
        assert VI.oracle_accepts(po, cz, bad) is False, label
        assert VI.verify(v, cz, bad) == (False, VI.MALFORMED), label


def test_wrong_public_inputs_are_an_opening_failure(pkg, po, co, get):
    cz, proof, v = get("instance")
    wrong = [[list(cz["instances"][0][0])]]
    wrong[0][0][2] += 1
    assert VI.oracle_accepts(po, cz, proof, wrong) is False
    assert VI.verify(v, cz, proof, wrong) == (False, VI.OPENING)
    shorter = [[list(cz["instances"][0][0])[:-1]]]      # a missing value is a wrong value
    assert VI.verify(v, cz, proof, shorter) == (False, VI.OPENING) and VI.oracle_accepts(po, cz, proof, shorter) is False
    longer = [[list(cz["instances"][0][0]) + [0, 0]]]   # under IPA the column is committed: trailing zeros commit to the same column
    assert VI.verify(v, cz, proof, longer) == (True, 0) and VI.oracle_accepts(po, cz, proof, longer) is True
    assert VI.verify(v, cz, proof) == (True, 0)
    # transcript_repr
    cz, proof, _ = get("one")
    v2 = VI.host_verifier(pkg, cz)
    assert VI.verify(v2, cz, proof) == (True, 0)
    v2.transcript_repr = cz["c"]["rep"] + 1
    assert VI.verify(v2, cz, proof) == (False, VI.OPENING)
    v2.transcript_repr = cz["c"]["rep"]
    assert VI.verify(v2, cz, proof) == (True, 0)
    v2.release()
    # another W, another U: the opening no longer closes
    c = cz["c"]
    for kw in (dict(w=c["u"]), dict(u=c["w"])):
        v3 = VI.host_verifier(pkg, cz, **kw)
        assert VI.verify(v3, cz, proof) == (False, VI.OPENING)
        v3.release()


def test_a_proof_under_another_key_is_rejected(pkg, po, co, get):
    """SHUF1's key on maingate's proof and the reverse: the lengths differ (MALFORMED); the same circuit's key with one commitment swapped reads and fails"""
    cz1, proof1, v1 = get("one")
    cz2, proof2, v2 = get("shuffle")
    assert VI.verify(v1, cz1, proof2)[0] is False and VI.verify(v2, cz2, proof1)[0] is False
    key = cz1["c"]["ipa_key"]
    nf = len(key["fixed_commitments"])
    at = lambda i: slice(8 + 64 * i, 8 + 64 * i + 64)
    assert nf >= 1 and key["perm_commitments"] and cz1["vk"][at(0)] != cz1["vk"][at(nf)]
    vk = bytearray(cz1["vk"])
    vk[at(0)], vk[at(nf)] = cz1["vk"][at(nf)], cz1["vk"][at(0)]      # fixed commitment 0 and sigma commitment 0 exchanged
    v = VI.host_verifier(pkg, cz1, vk=bytes(vk))
    assert VI.verify(v, cz1, proof1) == (False, VI.OPENING)
    v.release()


def test_callers_errors(pkg, po, co, get):
    from dehalo2_amd import native
    cz, proof, v = get("instance")
    for bad in ([[]], [[[5, 7, 9, 11], [1]]]):                                  # no column, two columns
        with pytest.raises(pkg.DehaloError) as e:
            v.verify(proof, bad, num_circuits=1)
        assert e.value.code == -1
    usable = (1 << cz["c"]["k"]) - (cz["cs"].blinding_factors() + 1)
    with pytest.raises(pkg.DehaloError) as e:
        v.verify(proof, [[[1] * (usable + 1)]], num_circuits=1)
    assert e.value.code == -1
    with pytest.raises(pkg.DehaloError) as e:                                   # several circuits in one IPA proof: the opening plan's own refusal
        v.verify(proof, [cz["instances"][0], cz["instances"][0]], num_circuits=2)
    assert e.value.code == -5 and "KZG only" in str(e.value)
    lib = pkg.load_library()
    assert lib.dehalo_verifier_set_multiopen(v.handle, 0) == -1 and lib.dehalo_verifier_set_multiopen(v.handle, 1) == -1
    with pytest.raises(pkg.DehaloError) as e:
        v.set_multiopen("shplonk")
    assert e.value.code == -1
    assert VI.verify(v, cz, proof) == (True, 0)
    # BN254 has no IPA; an unknown curve; k out of range; points that are none
    c = cz["c"]
    args = lambda **kw: dict(dict(curve=pkg.fields.VESTA, k=c["k"], g=c["srs"]["g"], g_lagrange=c["srs"]["g_lagrange"], w=c["w"], u=c["u"]), **kw)
    make = lambda a: native.Verifier.from_ipa_host(a["curve"], a["k"], a["g"], a["g_lagrange"], a["w"], a["u"], cz["cs"], cz["vk"])
    with pytest.raises(pkg.DehaloError) as e:
        make(args(curve=pkg.fields.BN254))
    assert e.value.code == -5 and "Pallas / Vesta" in str(e.value)
    off_curve = np.array(c["w"], dtype=np.uint64).copy()
    off_curve[4] ^= np.uint64(1)
    for kw in (dict(w=off_curve), dict(u=np.zeros(8, dtype=np.uint64))):
        with pytest.raises(pkg.DehaloError) as e:
            make(args(**kw))
        assert e.value.code == -1 and "curve point" in str(e.value)
    g_bad = np.array(c["srs"]["g"], dtype=np.uint64).reshape(-1, 8).copy()
    g_bad[3] = 0
    with pytest.raises(pkg.DehaloError) as e:
        make(args(g=g_bad))
    assert e.value.code == -1
    with pytest.raises(ValueError):
        make(args(k=c["k"] + 1))
    for bad_vk in (cz["vk"][:-1], cz["vk"] + b"\0", b""):
        with pytest.raises(pkg.DehaloError) as e:
            VI.host_verifier(pkg, cz, vk=bad_vk)
        assert e.value.code == -1
    acc = C.c_int(7)
    assert lib.dehalo_ipa_verify(None, None, None, None, None, None, 0, C.byref(acc)) == -1
    assert lib.dehalo_verifier_create_ipa(None, None, None, None) == -1 and lib.dehalo_verifier_create_ipa_vk(None, None, None, None, 0, 0, 0, None) == -1


def test_kzg_constructors_still_refuse_pasta_and_name_the_new_ones(pkg, po, co, get):
    from dehalo2_amd import native
    cz, _, _ = get("shuffle")
    with pytest.raises(pkg.DehaloError) as e:
        native.Verifier.from_vk(pkg.fields.VESTA, cz["c"]["k"], np.zeros(8, dtype=np.uint64), bytes(128), bytes(128), cz["cs"], cz["vk"])
    assert e.value.code == -5 and "KZG over BN254 only" in str(e.value) and "dehalo_verifier_create_ipa" in str(e.value)


def test_every_serde_format_gives_the_same_verdicts(pkg, po, co, get):
    cz, proof, v_raw = get("one")
    raw, processed = cz["vk"], VI.vk_in_format(pkg, cz, "processed")
    key = cz["c"]["ipa_key"]
    assert len(processed) == len(raw) - 32 * (len(key["fixed_commitments"]) + len(key["perm_commitments"]))
    secs = VI.sections(po, cz, len(proof))
    probes = [proof, VI.flip(proof, secs["sigma evaluation"][0]), VI.flip(proof, secs["h piece"][0]), VI.flip(proof, secs["opening R_1"][0]), proof[:-32]]
    want = [VI.verify(v_raw, cz, p) for p in probes]
    assert want[0] == (True, 0) and not any(w[0] for w in want[1:])
    for fmt, data in (("processed", processed), ("raw", raw), ("raw-unchecked", raw)):
        v = VI.host_verifier(pkg, cz, format=fmt, vk=data)
        assert [VI.verify(v, cz, p) for p in probes] == want, fmt
        v.release()
    with pytest.raises(pkg.DehaloError):      # the raw bytes are no Processed key
        VI.host_verifier(pkg, cz, format="processed", vk=raw)


# ------------------------------------------------------------------------------------------------------------------------------ batches
@pytest.fixture(scope="module")
def batch(pkg, po, co, get):
    return [VI.proof(pkg, po, co, "one", seed) for seed in (7, 8, 9)]


def test_batch_accepts_and_rejects(pkg, po, get, batch):
    cz, _, v = get("one")
    proofs = batch
    assert len(set(proofs)) == 3 and all(VI.oracle_accepts(po, cz, p) for p in proofs)
    inst = [cz["instances"]] * 3
    assert v.verify_batch(proofs, inst, num_circuits=1) is True and v.first_malformed == -1 and v.last_reject == 0
    secs = VI.sections(po, cz, len(proofs[0]))
    for i in range(3):
        for label in ("advice evaluation", "opening c"):
            bad = list(proofs)
            bad[i] = VI.flip(bad[i], secs[label][0])
            assert v.verify_batch(bad, inst, num_circuits=1) is False and v.first_malformed == -1 and v.last_reject == VI.OPENING, (i, label)
    bad = [proofs[0], proofs[1][:-1], proofs[2] + b"\0"]
    assert v.verify_batch(bad, inst, num_circuits=1) is False and v.first_malformed == 1 and v.last_reject == VI.MALFORMED
    for p in (proofs[0], VI.flip(proofs[0], secs["advice evaluation"][0]), proofs[0][:-32]):      # count = 1 is the single call
        single = VI.verify(v, cz, p)
        assert v.verify_batch([p], [cz["instances"]], num_circuits=1) is single[0] and v.last_reject == single[1]
    assert v.verify_batch([], [], num_circuits=1) is True      # the empty sum


def test_batch_weight_schedule(pkg, po, get, batch):
    """w_0 = 1 and w_1 = the first scalar drawn.  Every term of a proof -- its list over the fresh bases, its init = -w c and its g[0] correction -w v -- carries
    the proof's weight, so the same OPENING-tampered proof twice under w_1 = r - 1 sums to the identity and passes (which is why the weights must be unpredictable
    to whoever made the proofs); it fails under w_1 = 1 and under the library's own entropy."""
    cz, _, v = get("one")
    f = pkg.fields.VESTA.scalar
    secs = VI.sections(po, cz, len(batch[0]))
    for label in ("advice evaluation", "opening c", "opening f"):
        bad = VI.flip(batch[0], secs[label][0])
        assert VI.verify(v, cz, bad) == (False, VI.OPENING)
        inst = [cz["instances"]] * 2
        w = Weights(f, [R_VESTA - 1])
        assert v.verify_batch([bad, bad], inst, rng=w, num_circuits=1) is True and w.drawn == 1, label
        w = Weights(f, [1])
        assert v.verify_batch([bad, bad], inst, rng=w, num_circuits=1) is False and w.drawn == 1 and v.last_reject == VI.OPENING
    assert v.verify_batch([bad, bad], inst, rng=None, num_circuits=1) is False
    # three proofs draw two scalars, in order: w_2 = r - 1 cancels proof 2 against proof 0 only when proof 1 is valid and w_1 is whatever comes first
    good = batch[1]
    w = Weights(f, [12345, R_VESTA - 1])
    assert v.verify_batch([bad, good, bad], [cz["instances"]] * 3, rng=w, num_circuits=1) is True and w.drawn == 2
    w = Weights(f, [R_VESTA - 1, 12345])
    assert v.verify_batch([bad, good, bad], [cz["instances"]] * 3, rng=w, num_circuits=1) is False
    # a refused call draws nothing
    w = Weights(f, [5, 6])
    with pytest.raises(pkg.DehaloError):
        v.verify_batch([good, good, good], [[[], []]] * 3, rng=w, num_circuits=1)
    assert w.drawn == 0


def _python_terms(po, cz, proof):
    """One readable proof as the terms of ipa.verify_opening's multi-exponentiation, from the oracle's own pieces (read_plonk, construct_intermediate_sets,
    lagrange_eval, compute_s, compute_b): -> (s: the 2^k scalars over g with v subtracted at s[0], [(fresh base as canonical (x, y), scalar)])"""
    import ipa
    import verifier as V
    c, curve = cz["c"], po.VESTA
    p, k = curve.scalar.p, c["k"]
    T = V.ReadTranscript(curve, proof)
    inst_cm = [ipa.commit_reference(curve, c["srs"]["g_lagrange"], c["w"], list(vals), ipa.DEFAULT_BLIND) for vals in cz["instances"][0]]
    Q, _ = V.read_plonk(T, curve, c["desc"], k, c["fc"], c["pc"], c["rep"], cz["instances"][0], inst_cm)
    x1, x2 = T.challenge(), T.challenge()
    commitments, point_sets = ipa.construct_intermediate_sets([(key, pt) for key, pt, _, _ in Q])
    item = {key: cm for key, _, cm, _ in Q}
    evals_of = {(key, pt): e for key, pt, _, e in Q}
    q_cm, q_sets = [None] * len(point_sets), [[0] * len(ps) for ps in point_sets]
    for key, si, _ in commitments:
        q_cm[si] = po.ec_add(curve, po.ec_mul(curve, x1, q_cm[si]) if q_cm[si] is not None else None, item[key])
        for j, pt in enumerate(point_sets[si]):
            q_sets[si][j] = (q_sets[si][j] * x1 + evals_of[(key, pt)]) % p
    P = T.read_point()
    x3 = T.challenge()
    q_evals = [T.read_scalar() for _ in point_sets]
    v = 0
    for pts, evs, u_i in zip(point_sets, q_sets, q_evals):
        e = (u_i - ipa.lagrange_eval(pts, evs, x3, p)) % p
        for pt in pts:
            e = e * pow((x3 - pt) % p, -1, p) % p
        v = (v * x2 + e) % p
    x4 = T.challenge()
    for qc, u_i in zip(q_cm, q_evals):
        P = po.ec_add(curve, po.ec_mul(curve, x4, P), qc)
        v = (v * x4 + u_i) % p
    S = T.read_point()
    xi, z = T.challenge(), T.challenge()
    rounds = []
    for _ in range(k):
        L, R = T.read_point(), T.read_point()
        rounds.append((L, R, T.challenge()))
    cc, fv = T.read_scalar(), T.read_scalar()
    assert T.pos == len(T.data)
    us = [u for _, _, u in rounds]
    s = ipa.compute_s(us, -cc, p)
    s[0] = (s[0] - v) % p
    b = ipa.compute_b(x3, us, p)
    fresh = [(P, 1), (S, xi)] + [(L, pow(u, -1, p)) for L, _, u in rounds] + [(R, u) for _, R, u in rounds]
    fresh += [(ipa.dec_point(curve, c["u"]), -cc * b * z % p), (ipa.dec_point(curve, c["w"]), -fv % p)]
    return s, fresh


def _python_batch_identity(po, co, cz, terms, weights):
    """sum_i w_i (<s_i, G> + the fresh-bases terms of proof i) = the identity?  One multi-exponentiation in the C restatement over [G | every proof's fresh bases]"""
    import ipa
    curve, c = po.VESTA, cz["c"]
    p = curve.scalar.p
    total = [0] * (1 << c["k"])
    bases, scalars = [], []
    for (s, fresh), w in zip(terms, weights):
        total = [(a + w * b) % p for a, b in zip(total, s)]
        bases += [ipa.enc_point(curve, P) for P, _ in fresh]
        scalars += [w * sc % p for _, sc in fresh]
    all_bases = np.concatenate([np.ascontiguousarray(c["srs"]["g"], dtype=np.uint64).reshape(-1, 8), np.stack(bases)])
    cid = po.CURVE_IDS[curve.name]
    return not co.to_affine(cid, co.best_multiexp(cid, ipa.enc(curve.scalar, total + scalars), all_bases, 4)).any()


def test_batch_identity_in_python_integers(pkg, po, co, get, batch):
    """The weight schedule against the batch identity recomputed in Python integers: with weights (1, w_1, w_2, ..) handed out through DEHALO_RNG_CALLBACK, the
    library accepts a batch exactly when  sum_i w_i (<compute_s(u_i, -c_i) - v_i e_0, G> + P_i + [xi_i] S_i + sum_j ([u_ij^-1] L_ij + [u_ij] R_ij) - [c_i b_i z_i] U
    - [f_i] W)  is the identity -- valid proofs under any weights, tampered ones under weights that cancel, and not under weights that do not, nor under the same
    weights in another order."""
    cz, _, v = get("one")
    f = pkg.fields.VESTA.scalar
    secs = VI.sections(po, cz, len(batch[0]))
    good = list(batch)
    bad_c = VI.flip(batch[0], secs["opening c"][0])
    bad_e = VI.flip(batch[1], secs["advice evaluation"][0])
    terms = {pr: _python_terms(po, cz, pr) for pr in good + [bad_c, bad_e]}
    for pr in good:
        assert _python_batch_identity(po, co, cz, [terms[pr]], [1]) is True
    for pr in (bad_c, bad_e):
        assert _python_batch_identity(po, co, cz, [terms[pr]], [1]) is False and VI.verify(v, cz, pr) == (False, VI.OPENING)
    a = 0x1234567890ABCDEF1234567890ABCDEF
    cases = [(good, [3, 5], True), ([good[0], good[1]], [R_VESTA - 1], True),
             ([bad_c, bad_c], [R_VESTA - 1], True), ([bad_c, bad_c], [12345], False), ([bad_e, bad_e], [R_VESTA - 1], True),
             ([bad_c, bad_c, bad_c], [a, R_VESTA - 1 - a], True), ([bad_c, bad_c, bad_c], [R_VESTA - 1 - a, a], True), ([bad_c, bad_c, bad_c], [a, R_VESTA - a], False),
             ([bad_c, good[1], bad_c], [a, R_VESTA - 1], True), ([bad_c, good[1], bad_c], [R_VESTA - 1, a], False),
             ([bad_c, bad_e], [R_VESTA - 1], False), ([bad_c, good[1], bad_e], [7, 9], False)]
    for proofs, ws, want in cases:
        python = _python_batch_identity(po, co, cz, [terms[pr] for pr in proofs], [1] + ws)
        w = Weights(f, ws)
        got = v.verify_batch(proofs, [cz["instances"]] * len(proofs), rng=w, num_circuits=1)
        assert w.drawn == len(ws)
        assert got is python is want, (ws, got, python, want)
        assert v.last_reject == (0 if got else VI.OPENING)


# ------------------------------------------------------------------------------------------------------------------------------ verify_host.hpp alone, sanitized
def test_sanitized_program_gives_the_same_verdicts(pkg, po, co, get, tmp_path):
    from dehalo2_amd import native
    out = subprocess.run(["make", "-C", ROOT, "verify_ipa_host_check"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    cz, proof, v = get("instance")
    c = cz["c"]
    desc = native.ConstraintSystemDescriptor(cz["cs"], pkg.fields.VESTA.scalar)
    bad = VI.flip(proof, VI.sections(po, cz, len(proof))["instance evaluation"][0])
    values = cz["instances"][0][0]
    words = lambda a: np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    blob = struct.pack("<5I", 2, c["k"], len(cz["selectors"]), len(cz["vk"]), len(values))      # curve id, k, selectors, vk length, instance values
    blob += words(c["srs"]["g"]) + words(c["srs"]["g_lagrange"]) + words(c["w"]) + words(c["u"]) + pkg.fields.VESTA.scalar.encode(c["rep"]).tobytes()
    blob += cz["vk"] + _descriptor_bytes(desc) + pkg.fields.VESTA.scalar.encode_many(values).tobytes()
    for p in (proof, bad, proof[:-1]):
        blob += struct.pack("<I", len(p)) + p
    path = tmp_path / "case.bin"
    path.write_bytes(blob)
    assert pkg.fields.VESTA.id == 2
    r = subprocess.run([os.path.join(ROOT, "tests", "native_host", "verify_ipa_host_check"), str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    want = [VI.verify(v, cz, p) for p in (proof, bad, proof[:-1])]
    assert want == [(True, 0), (False, VI.OPENING), (False, VI.MALFORMED)]
    assert r.stdout.split() == ["%d:%d" % (int(a), b) for a, b in want]
