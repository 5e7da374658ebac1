"""GPU suite: keys in every SerdeFormat -- the scalar codec (dehalo_scalars_from_repr_device, dehalo_scalars_check_device), dehalo_pk_read_custom /
_write_custom, dehalo_vk_write_custom and dehalo_keygen_pk.

The scalar kernels alone, on every field id, at 1, 255, 256, 257 and 1000 elements, against Python integers: 0, 1, p - 1, p, p + 1, 2^256 - 1 and random
values; no bad element (status 0, first_bad = count), bad elements at index 0, at the last index and at {257, 700} together (status 1, first_bad the
lowest, each written as 0 between neighbours converted correctly); in place equals out of place; a 4-byte aligned input that is not 16-byte aligned.
Whole keys of the maingate circuit (tests/proof_chains.py) at k = 6 without lookups and at k = 9 with range lookups, BN254 / KZG and Vesta / IPA: every format
round-trips to dehalo_pk_write's bytes, both raw formats ARE those bytes, Processed equals the Python mirror's, and a key read in each format makes the
proof the original key makes, byte for byte.  Every tampering of tests/test_key_format_host.py on real key bytes: the refusal names kind, section and the
lowest slice-local element index, and the context goes on reading and proving.  dehalo_keygen_pk under each vk format gives dehalo_keygen's key without
launching an MSM, takes a foreign commitment verbatim (the verifier then rejects), and refuses a vk that does not fit.
The whole-key tests call the _custom entry points through ctypes for all three format ids (c_write, c_vk, c_read): native.ProvingKey's wrappers send
"raw-unchecked" to the calls the library has always had."""
import struct

import numpy as np
import pytest

from test_ipa_proof import ipa_chain      # noqa: F401  (the IPA chains of the maingate circuit, with the circuit)
from test_key_format_host import elem_off, put

FIELD_NAMES = ["bn254_fr", "pasta_fq", "pasta_fp", "bn254_fq"]      # the three scalar fields and one base field: every field id
COUNTS = [1, 255, 256, 257, 1000]
FORMATS = ["processed", "raw", "raw-unchecked"]
INVALID = -1


def _values(f, count, seed):
    """canonical integers below p: 0, 1, p - 1 first, then random"""
    rng = np.random.default_rng(seed)
    vals = [0, 1, f.p - 1][:count]
    return vals + [int.from_bytes(rng.bytes(32), "little") % f.p for _ in range(count - len(vals))]


def _words(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)


def _bad_sets(count):
    """the index sets that hold a bad element, for this count"""
    sets = [[0], [count - 1]]
    if count > 700:
        sets.append([257, 700])
    return sets


# ------------------------------------------------------------------------------------------------------------------------------ the scalar kernels alone
@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("fname", FIELD_NAMES)
def test_scalars_from_repr_against_python_integers(pkg, ctx, fname, count):
    import torch
    f = pkg.fields.FIELDS[fname]
    R = (1 << 256) % f.p
    vals = _values(f, count, 100 + count)
    want = _words([v * R % f.p for v in vals])
    d_in = ctx.upload(_words(vals))
    d_out = torch.zeros((count, 4), dtype=torch.int64, device="cuda")
    assert ctx.scalars_from_repr(f.id, d_in.data_ptr(), count, d_out.data_ptr()) == (0, count)
    assert np.array_equal(ctx.download_tensor(d_out), want)
    assert np.array_equal(ctx.download_tensor(d_in), _words(vals))      # out of place: the input stays
    assert ctx.scalars_from_repr(f.id, d_in.data_ptr(), count, d_in.data_ptr()) == (0, count)      # in place
    assert np.array_equal(ctx.download_tensor(d_in), want)
    # a 4-byte aligned input that is not 16-byte aligned
    shifted = ctx.upload(np.frombuffer(bytes(4) + _words(vals).tobytes() + bytes(4), dtype=np.uint64))
    d_out.zero_()
    torch.cuda.synchronize()
    assert ctx.scalars_from_repr(f.id, shifted.data_ptr() + 4, count, d_out.data_ptr()) == (0, count)
    assert np.array_equal(ctx.download_tensor(d_out), want)
    # bad elements: p, p + 1, 2^256 - 1
    for bad_at in _bad_sets(count):
        for j, bad in enumerate((f.p, f.p + 1, (1 << 256) - 1)):
            v2, w2 = list(vals), want.copy()
            for i in bad_at:
                v2[i] = bad if i == bad_at[0] else (f.p, f.p + 1, (1 << 256) - 1)[(j + 1) % 3]
                w2[i] = 0
            for inplace in (False, True):
                d_in = ctx.upload(_words(v2))
                dst = d_in if inplace else d_out
                assert ctx.scalars_from_repr(f.id, d_in.data_ptr(), count, dst.data_ptr()) == (1, bad_at[0]), (bad_at, bad, inplace)
                assert np.array_equal(ctx.download_tensor(dst), w2), (bad_at, bad, inplace)      # the bad ones are 0, their neighbours converted


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("fname", FIELD_NAMES)
def test_scalars_check_against_python_integers(pkg, ctx, fname, count):
    f = pkg.fields.FIELDS[fname]
    words = _values(f, count, 200 + count)      # stored words below p, 0, 1 and p - 1 among them
    d = ctx.upload(_words(words))
    assert ctx.scalars_check(f.id, d.data_ptr(), count) == (0, count)
    assert np.array_equal(ctx.download_tensor(d), _words(words))      # reads only
    for bad_at in _bad_sets(count):
        for bad in (f.p, f.p + 1, (1 << 256) - 1):
            w2 = list(words)
            for i in bad_at:
                w2[i] = bad
            d = ctx.upload(_words(w2))
            assert ctx.scalars_check(f.id, d.data_ptr(), count) == (1, bad_at[0]), (bad_at, bad)
            assert np.array_equal(ctx.download_tensor(d), _words(w2))


@pytest.mark.gpu
def test_scalars_edge_arguments(pkg, ctx):
    import torch
    d = torch.zeros((8, 4), dtype=torch.int64, device="cuda")
    for f in pkg.fields.FIELDS.values():
        assert ctx.scalars_from_repr(f.id, 0, 0, 0) == (0, 0) and ctx.scalars_check(f.id, 0, 0) == (0, 0)      # count = 0: no launch, no pointer read
        assert ctx.scalars_from_repr(f.id, d.data_ptr(), 0, d.data_ptr()) == (0, 0)
    for call in (lambda: ctx.scalars_from_repr(4, d.data_ptr(), 8, d.data_ptr()), lambda: ctx.scalars_check(-1, d.data_ptr(), 8),
                 lambda: ctx.scalars_from_repr(4, 0, 0, 0), lambda: ctx.scalars_check(7, 0, 0),                      # an unknown field, at any count
                 lambda: ctx.scalars_from_repr(0, d.data_ptr(), 1 << 29, d.data_ptr()), lambda: ctx.scalars_check(0, d.data_ptr(), 1 << 29),
                 lambda: ctx.scalars_from_repr(0, d.data_ptr() + 32, 4, d.data_ptr()),                               # overlapping without being in place
                 lambda: ctx.scalars_from_repr(0, d.data_ptr() + 2, 1, d.data_ptr() + 128),                          # encodings not 4-byte aligned
                 lambda: ctx.scalars_from_repr(0, 0, 4, d.data_ptr()), lambda: ctx.scalars_check(0, 0, 4)):          # null with work to do
        with pytest.raises(pkg.DehaloError) as e:
            call()
        assert e.value.code == INVALID
    assert ctx.scalars_check(0, d.data_ptr(), 8) == (0, 8)      # the context is as usable as before


# ------------------------------------------------------------------------------------------------------------------------------ whole keys
@pytest.fixture(scope="module")
def kzg_chain(pkg, po, co):
    """(k, range_lookups) -> tests/proof_chains.py's KZG chain of circuits.synthesize(p, k, range_lookups, seed=3), with the circuit"""
    import proof_chains as PC
    import shapes
    from dehalo2_amd import circuits
    cache = {}

    def get(k, rl):
        if (k, rl) not in cache:
            circ = circuits.synthesize(po.BN254.scalar.p, k, rl, seed=3)
            desc = shapes.maingate_description(rl)
            assert desc == circ.cs.description()
            cache[(k, rl)] = dict(PC.kzg_chain(po, co, desc, k, circ.fixed, circ.assembly.mapping, circ.advice, circ.selectors), circ=circ)
        return cache[(k, rl)]
    return get


@pytest.fixture(scope="module")
def keys(pkg, po, ctx, kzg_chain, ipa_chain):      # noqa: F811
    """(scheme, k, range_lookups) -> the chain, the native params, dehalo_keygen's key with the chain's transcript_repr, its RawBytes and its proof"""
    import pairing as pr
    from dehalo2_amd import native, prover
    cache = {}

    def get(scheme, k, rl):
        if (scheme, k, rl) not in cache:
            if scheme == "ipa":
                c = ipa_chain(k, rl)
                curve = pkg.fields.VESTA
                params = native.ParamsIPA.create(ctx, curve, k, c["srs"]["g"], c["srs"]["g_lagrange"], c["w"], c["u"])
            else:
                c = kzg_chain(k, rl)
                curve = pkg.fields.BN254
                params = native.ParamsKZG.create(ctx, curve, k, c["srs"]["g"], c["srs"]["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(c["s_g2"]))
            circ = c["circ"]
            pk = native.ProvingKey.keygen(ctx, params, circ.cs, circ.fixed, circ.assembly, circ.selectors)
            default_repr = pk.transcript_repr
            pk.transcript_repr = c["rep"]
            d = dict(c=c, curve=curve, params=params, pk=pk, raw=pk.write(), vk=pk.vk_bytes(), nsel=len(circ.selectors), default_repr=default_repr)
            d["proof"] = prove(d, pk)
            cache[(scheme, k, rl)] = d
        return cache[(scheme, k, rl)]

    yield get
    for v in cache.values():
        v["pk"].release()
        v["params"].release()


def prove(d, pk):
    from dehalo2_amd import native, prover
    P = native.Prover(d["params"], pk)
    try:
        return P.create_proof(d["c"]["adv"], [[]], prover.SeededRng(7)).finalize()
    finally:
        P.release()


# The _custom entry points, called as they are for EVERY format id: native.ProvingKey's wrappers send "raw-unchecked" to dehalo_pk_read / dehalo_pk_write /
# dehalo_vk_write, so the tests of the new calls go past them.
FORMAT_IDS = {"processed": 0, "raw": 1, "raw-unchecked": 2}


def c_write(pkg, ctx, pk, fmt):
    """dehalo_pk_size_custom + dehalo_pk_write_custom"""
    from dehalo2_amd import native
    lib = pkg.load_library()
    out = np.full(lib.dehalo_pk_size_custom(pk.handle, FORMAT_IDS[fmt]), 0xA5, dtype=np.uint8)
    native._check(ctx, lib.dehalo_pk_write_custom(ctx.handle, pk.handle, FORMAT_IDS[fmt], out.ctypes.data, out.size))
    return out.tobytes()


def c_vk(pkg, ctx, pk, fmt):
    """dehalo_vk_size_custom + dehalo_vk_write_custom"""
    from dehalo2_amd import native
    lib = pkg.load_library()
    out = np.full(lib.dehalo_vk_size_custom(pk.handle, FORMAT_IDS[fmt]), 0xA5, dtype=np.uint8)
    native._check(ctx, lib.dehalo_vk_write_custom(ctx.handle, pk.handle, FORMAT_IDS[fmt], out.ctypes.data, out.size))
    return out.tobytes()


def c_read(pkg, ctx, d, data, fmt):
    """dehalo_pk_read_custom -> native.ProvingKey over the handle; DehaloError on refusal"""
    import ctypes as C
    from dehalo2_amd import native
    cs = d["c"]["circ"].cs
    desc = native.ConstraintSystemDescriptor(cs, d["curve"].scalar)
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    h = C.c_void_p()
    native._check(ctx, pkg.load_library().dehalo_pk_read_custom(ctx.handle, d["curve"].id, desc.ref(), buf.ctypes.data if buf.size else None, buf.size, FORMAT_IDS[fmt],
                                                                d["nsel"], C.byref(h)))
    assert h.value
    return native.ProvingKey(ctx, d["curve"], cs, h)


def key_layout(pkg, d, fmt):
    from dehalo2_amd import keygen
    from dehalo2_amd.domain import EvaluationDomain
    cs, k = d["c"]["circ"].cs, d["c"]["k"]
    ext = EvaluationDomain(None, d["curve"].scalar, cs.degree(), k).extended_k - k
    return keygen.key_layout(fmt, k, cs.num_fixed, len(cs.permutation_columns), d["nsel"], ext)


CASES = [("kzg", 6, False), ("kzg", 9, True), ("ipa", 6, False), ("ipa", 9, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,k,rl", CASES)
def test_whole_keys_in_every_format(pkg, po, ctx, keys, scheme, k, rl):
    import proof_chains as PC
    from dehalo2_amd import keygen, native
    d = keys(scheme, k, rl)
    cs, pk, raw = d["c"]["circ"].cs, d["pk"], d["raw"]
    assert PC.accepts(po, d["c"], d["proof"], [[]])
    nc = cs.num_fixed + len(cs.permutation_columns)
    mirror = keygen.HostProvingKey.from_bytes(d["curve"], cs, raw, d["nsel"], "raw-unchecked")
    for fmt in FORMATS:
        data, vk = c_write(pkg, ctx, pk, fmt), c_vk(pkg, ctx, pk, fmt)      # the _custom calls themselves, for all three format ids
        assert data == pk.write(fmt) and vk == pk.vk_bytes(fmt)             # ... and the Python wrappers give the same
        L = key_layout(pkg, d, fmt)
        assert len(data) == L["pk_size"] and len(vk) == L["vk_size"] and data.startswith(vk)
        if fmt == "processed":
            assert len(data) == len(raw) - 32 * nc and len(vk) == len(d["vk"]) - 32 * nc
            assert data == mirror.to_bytes("processed")
        else:
            assert data == raw and vk == d["vk"]      # both raw formats ARE dehalo_pk_write's / dehalo_vk_write's bytes
        for read in (lambda: c_read(pkg, ctx, d, data, fmt), lambda: native.ProvingKey.read(ctx, d["curve"], cs, data, d["nsel"], fmt)):
            back = read()
            try:
                assert back.write() == raw and back.vk_bytes() == d["vk"] and c_write(pkg, ctx, back, fmt) == data and c_vk(pkg, ctx, back, fmt) == vk
                assert back.transcript_repr == d["default_repr"]
                back.transcript_repr = d["c"]["rep"]
                assert prove(d, back) == d["proof"]
            finally:
                back.release()
    for call in (lambda: pk.write("compressed"), lambda: pk.vk_bytes("compressed"), lambda: native.ProvingKey.read(ctx, d["curve"], cs, raw, d["nsel"], "compressed")):
        with pytest.raises(ValueError):
            call()
    lib = pkg.load_library()
    assert lib.dehalo_pk_size_custom(pk.handle, 3) == 0 and lib.dehalo_vk_size_custom(pk.handle, -1) == 0
    buf = np.zeros(len(raw), dtype=np.uint8)
    assert lib.dehalo_pk_write_custom(ctx.handle, pk.handle, 3, buf.ctypes.data, buf.size) == INVALID
    assert lib.dehalo_vk_write_custom(ctx.handle, pk.handle, 3, buf.ctypes.data, buf.size) == INVALID
    assert lib.dehalo_pk_write_custom(ctx.handle, pk.handle, 0, buf.ctypes.data, 100) == INVALID      # buffer too small


@pytest.mark.gpu
def test_identity_commitment_survives_every_format(pkg, ctx, keys):
    """The maingate circuit without lookups leaves fixed columns all zero (KZG: their commitments are the identity, 64 zero bytes); one more is zeroed here."""
    from dehalo2_amd import native
    d = keys("kzg", 6, False)
    circ = d["c"]["circ"]
    nf = circ.cs.num_fixed
    fixed = np.array(circ.fixed, dtype=np.uint64, copy=True)
    live = next(j for j in range(nf) if any(d["raw"][8 + 64 * j:72 + 64 * j]))
    fixed[live] = 0      # an all-zero fixed column: its commitment is the identity
    pk = native.ProvingKey.keygen(ctx, d["params"], circ.cs, fixed, circ.assembly, circ.selectors)
    try:
        raw = pk.write()
        zero = [j for j in range(nf) if not any(raw[8 + 64 * j:72 + 64 * j])]
        assert live in zero and len(zero) < nf
        for fmt in FORMATS:
            data = c_write(pkg, ctx, pk, fmt)
            if fmt == "processed":
                assert [j for j in range(nf) if not any(data[8 + 32 * j:40 + 32 * j])] == zero
            back = c_read(pkg, ctx, d, data, fmt)
            try:
                assert back.write() == raw
            finally:
                back.release()
            under = native.ProvingKey.keygen_pk(ctx, d["params"], circ.cs, c_vk(pkg, ctx, pk, fmt), fixed, circ.assembly, d["nsel"], fmt)
            try:
                assert under.write() == raw
            finally:
                under.release()
    finally:
        pk.release()


# ------------------------------------------------------------------------------------------------------------------------------ rejections
def real_tamperings(pkg, ctx, d, fmt):
    """name -> (bytes, the words the refusal must hold, accepted?): tests/test_key_format_host.py's list on the real key's bytes in `fmt`"""
    cs, k = d["c"]["circ"].cs, d["c"]["k"]
    f, q, b = d["curve"].scalar, d["curve"].base.p, d["curve"].b
    data, L = c_write(pkg, ctx, d["pk"], fmt), key_layout(pkg, d, fmt)
    n, m, nf = L["n"], L["m"], cs.num_fixed
    le = lambda v: v.to_bytes(32, "little")
    kind = "an element is not below the modulus" if fmt == "processed" else "an element's stored word is not below the modulus"
    out = {}
    out["element = p"] = (put(data, elem_off(L, "fixed_polys", 1, 2), le(f.p)), [kind, "fixed_polys", "element %d" % (n + 2)], False)
    out["element = p - 1"] = (put(data, elem_off(L, "permutation cosets", 0, 3), le(f.p - 1)), [], True)
    # two bad elements in different polynomials of one slice: the slice-local index of the lower one
    two = put(put(data, elem_off(L, "fixed_cosets", nf - 1, 5), le(f.p + 1)), elem_off(L, "fixed_cosets", 1, m - 1), le((1 << 256) - 1))
    out["two bad elements in one slice"] = (two, [kind, "fixed_cosets", "element %d" % (2 * m - 1)], False)
    two = put(put(data, elem_off(L, "permutation values", 2, 0), le(f.p)), elem_off(L, "permutation values", 0, n - 1), le(f.p))
    out["two bad elements in one slice, the first polynomial's last"] = (two, [kind, "permutation values", "element %d" % (n - 1)], False)
    out["l_active_row"] = (put(data, elem_off(L, "l_active_row", 0, m - 1), le(f.p)), [kind, "l_active_row", "element %d" % (m - 1)], False)
    out["l0"] = (put(data, elem_off(L, "l0", 0, 0), le(f.p)), [kind, "l0", "element 0"], False)
    if fmt == "raw":
        o = L["off_fixed_c"] + 32
        y1 = (int.from_bytes(data[o:o + 32], "little") + 1) % q
        out["(x, y + 1)"] = (put(data, o, le(y1)), ["neither on the curve", "fixed commitments"], False)
        out["coordinate word = q"] = (put(data, L["off_perm_c"] + 64, le(q)), ["stored word is not below the modulus", "permutation commitments"], False)
    else:
        x = next(x for x in range(1, 200) if pow((x ** 3 + b) % q, (q - 1) // 2, q) == q - 1)
        out["x without a square root"] = (put(data, L["off_perm_c"], le(x)), ["not on the curve", "permutation commitments"], False)
        out["x = 0 with the sign bit"] = (put(data, L["off_fixed_c"] + 32, bytes(31) + b"\x80"), ["x = 0 with the sign bit", "fixed commitments"], False)
        out["x = q"] = (put(data, L["off_fixed_c"], le(q)), ["x coordinate is not below the modulus", "fixed commitments"], False)
    out["truncated"] = (data[:-1], ["length"], False)
    out["trailing byte"] = (data + b"\0", ["length"], False)
    out["wrong k"] = (struct.pack(">I", k + 1) + data[4:], ["length"], False)      # (a read has no k to compare with: the length no longer fits)
    out["k out of range"] = (struct.pack(">I", 29) + data[4:], ["k out of range"], False)
    out["wrong fixed-column count"] = (data[:4] + struct.pack(">I", nf + 1) + data[8:], ["fixed-column count"], False)
    out["seven bytes"] = (data[:7], ["length"], False)
    o = L["polys"]["fixed_polys"][0]
    out["polynomial count"] = (put(data, o, struct.pack(">I", nf - 1)), ["polynomial count", "fixed_polys"], False)
    out["polynomial length"] = (put(data, o + 4, struct.pack(">I", n - 1)), ["polynomial length", "fixed_polys"], False)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["processed", "raw"])
@pytest.mark.parametrize("scheme", ["kzg", "ipa"])
def test_rejections_name_kind_section_and_index(pkg, ctx, keys, scheme, fmt):
    from dehalo2_amd import native
    d = keys(scheme, 6, False)
    cs, good = d["c"]["circ"].cs, c_write(pkg, ctx, d["pk"], fmt)
    read = lambda data, f=fmt: c_read(pkg, ctx, d, data, f)      # dehalo_pk_read_custom itself
    for name, (bad, words, ok) in real_tamperings(pkg, ctx, d, fmt).items():
        if ok:
            pk = read(bad)
            assert c_write(pkg, ctx, pk, fmt) == bad, name
            pk.release()
            continue
        with pytest.raises(pkg.DehaloError) as e:
            read(bad)
        assert e.value.code == INVALID and all(w in str(e.value) for w in words), (name, str(e.value))
        pk = read(good)      # the same context reads the good bytes and proves
        try:
            pk.transcript_repr = d["c"]["rep"]
            assert prove(d, pk) == d["proof"], name
        finally:
            pk.release()
        if fmt == "raw" and name in ("element = p", "two bad elements in one slice", "l0", "(x, y + 1)", "coordinate word = q"):
            took, old = read(bad, "raw-unchecked"), native.ProvingKey.read(ctx, d["curve"], cs, bad, d["nsel"])      # unseen, as dehalo_pk_read takes them ...
            try:
                assert c_write(pkg, ctx, took, "raw-unchecked") == old.write()      # ... giving an equal key
            finally:
                took.release(); old.release()


# ------------------------------------------------------------------------------------------------------------------------------ keygen_pk
@pytest.mark.gpu
@pytest.mark.parametrize("scheme,k,rl", [("kzg", 6, False), ("ipa", 6, False), ("kzg", 9, True), ("ipa", 9, True)])
def test_keygen_pk_under_an_existing_vk(pkg, po, ctx, keys, scheme, k, rl):
    from dehalo2_amd import native
    from dehalo2_amd._lib import K_MSM_ACCUMULATE
    d = keys(scheme, k, rl)
    circ = d["c"]["circ"]
    ctx.timing_enable(True)
    try:
        ctx.timing_reset()
        again = native.ProvingKey.keygen(ctx, d["params"], circ.cs, circ.fixed, circ.assembly, circ.selectors)
        again.release()
        msms = ctx.timing_get(K_MSM_ACCUMULATE)[1]
        assert msms > 0      # dehalo_keygen's commitments are timed MSM regions ...
        for fmt in FORMATS:
            vk = c_vk(pkg, ctx, d["pk"], fmt)
            before = ctx.timing_get(K_MSM_ACCUMULATE)[1]      # (the proofs below run MSMs of their own)
            pk = native.ProvingKey.keygen_pk(ctx, d["params"], circ.cs, vk, circ.fixed, circ.assembly, d["nsel"], fmt)
            try:
                assert ctx.timing_get(K_MSM_ACCUMULATE)[1] == before, fmt      # ... and dehalo_keygen_pk launches none
                assert pk.write() == d["raw"] and pk.vk_bytes() == d["vk"] and pk.transcript_repr == d["default_repr"]
                if k == 6:
                    pk.transcript_repr = d["c"]["rep"]
                    assert prove(d, pk) == d["proof"]
            finally:
                pk.release()
    finally:
        ctx.timing_enable(False)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["kzg", "ipa"])
def test_keygen_pk_takes_the_vk_at_its_word(pkg, po, ctx, keys, scheme):
    """A vk whose first fixed commitment is another valid point: the key carries it verbatim -- nothing compares it with the columns, so the proof is the one the
    right key makes -- and a verifier that holds this vk rejects the proof."""
    import proof_chains as PC
    from dehalo2_amd import native
    d = keys(scheme, 6, False)
    c, circ, vk = d["c"], d["c"]["circ"], d["vk"]
    at = lambda j: vk[8 + 64 * j:72 + 64 * j]
    j = next(j for j in range(1, circ.cs.num_fixed) if at(j) != at(0) and any(at(j)))      # another valid point, not the identity
    foreign = vk[:8] + at(j) + vk[72:]
    theirs = dict(c, fc=[c["fc"][j]] + c["fc"][1:]) if scheme == "ipa" else dict(c, key=dict(c["key"], fixed_commitments=[c["key"]["fixed_commitments"][j]] + c["key"]["fixed_commitments"][1:]))
    for fmt in FORMATS:
        pk = native.ProvingKey.keygen_pk(ctx, d["params"], circ.cs, foreign if fmt != "processed" else _processed_vk(pkg, d, foreign), circ.fixed, circ.assembly, d["nsel"], fmt)
        try:
            assert pk.vk_bytes() == foreign and pk.write()[len(vk):] == d["raw"][len(vk):]
            assert pk.transcript_repr != d["default_repr"]      # the substitute representation is taken over the vk's bytes
            pk.transcript_repr = c["rep"]
            proof = prove(d, pk)
            assert PC.accepts(po, c, proof, [[]]) and not PC.accepts(po, theirs, proof, [[]])
        finally:
            pk.release()


def _processed_vk(pkg, d, vk_raw):
    """the mirror's Processed form of RawBytes vk bytes"""
    import io
    from dehalo2_amd import keygen
    out = io.BytesIO()
    keygen.VerifyingKey.read(d["curve"], d["c"]["circ"].cs, io.BytesIO(vk_raw), d["nsel"], "raw").write(out, "processed")
    return out.getvalue()


@pytest.mark.gpu
def test_keygen_pk_refusals(pkg, ctx, keys):
    from dehalo2_amd import native
    d, d9 = keys("kzg", 6, False), keys("kzg", 9, True)
    circ = d["c"]["circ"]
    q = d["curve"].base.p
    under = lambda vk, fmt: native.ProvingKey.keygen_pk(ctx, d["params"], circ.cs, vk, circ.fixed, circ.assembly, d["nsel"], fmt)
    for fmt in FORMATS:
        vk = c_vk(pkg, ctx, d["pk"], fmt)
        cases = {"wrong k": (struct.pack(">I", 7) + vk[4:], "k differs"), "k out of range": (struct.pack(">I", 29) + vk[4:], "k out of range"),
                 "wrong num_fixed": (vk[:4] + struct.pack(">I", circ.cs.num_fixed - 1) + vk[8:], "fixed-column count"), "truncated": (vk[:-1], "length"),
                 "trailing byte": (vk + b"\0", "length"), "a pk": (c_write(pkg, ctx, d["pk"], fmt), "length"), "seven bytes": (vk[:7], "length")}
        if fmt == "raw":
            cases["word = q"] = (put(vk, 8, q.to_bytes(32, "little")), "fixed commitments")
        if fmt == "processed":
            cases["x = 0 with the sign bit"] = (put(vk, 8, bytes(31) + b"\x80"), "fixed commitments")
        for name, (bad, word) in cases.items():
            with pytest.raises(pkg.DehaloError) as e:
                under(bad, fmt)
            assert e.value.code == INVALID and word in str(e.value), (fmt, name, str(e.value))
    with pytest.raises(pkg.DehaloError) as e:      # a vk of another k under these params
        native.ProvingKey.keygen_pk(ctx, d["params"], circ.cs, d9["vk"], circ.fixed, circ.assembly, d["nsel"], "raw")
    assert e.value.code == INVALID and "k differs" in str(e.value)
    with pytest.raises(ValueError):
        under(d["vk"], "compressed")
    pk = under(d["vk"], "raw")      # the context is as usable as before
    assert pk.write() == d["raw"]
    pk.release()
