"""The ChaCha20 generator kinds' draws, host and device, pinned to RFC 8439 through the keyed kind (DEHALO_RNG_CHACHA20, prover.KeyedRng): from the key on it is
the code path of the default generator (DEHALO_RNG_OS), so what is pinned here is what a production proof draws.

The judge is tests/chacha_reference.py -- the block function, the host's serial stream, the kernel's indexed draw and a scalar source for the oracle prover, on
plain integers -- and it is itself judged first, by four vectors of RFC 8439 (2.3.2; A.1 #1, #3, #5).

CPU: the vectors; dehalo_rng_scalars under the keyed kind against the serial stream for the four fields and two keys, with what `skip` does; the condition that
the reference's own indexed draws reach rejection attempts 1, 2 and 3; the acceptance step on crafted candidates (tests/native_host/hostrng_check.cpp, ASan +
UBSan); the refusals.
GPU: dehalo_rng_scalars_device against the indexed draw element for element at the block's edges, three streams, four fields, with a guarded tail; streams 1 and
2 disjoint; whole proofs under KeyedRng byte for byte against the oracle prover driven by ReferenceRng (KZG GWC with and without a side context, SHPLONK, IPA
over Vesta and Pallas, two circuits in one proof, a stand-alone opening); one key twice, two keys."""
import collections
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import chacha_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("bn254_fr", "bn254_fq", "pasta_fp", "pasta_fq")
KEY_A = bytes(range(32))                      # RFC 8439's 00 01 .. 1f
KEY_B = KEY_A[:31] + b"\x20"                  # differs in the last byte
ZERO_KEY, ONE_KEY = bytes(32), bytes(31) + b"\x01"
STREAM_W15 = 0x02000000 << 32                 # sets word 15 (RFC 8439 A.1 #5's nonce)
STREAMS = (1, 2, STREAM_W15)
SIZES = (1, 255, 256, 257, 4099)              # the block is 256 threads: one short, full, one over, many blocks with a ragged tail
N_MAX = max(SIZES)
INVALID = -1

# (key, w12 w13 w14 w15, the block): RFC 8439 2.3.2 is the second (its counter 1 and nonce 00 00 00 09 | 00 00 00 4a | 00 00 00 00 as words 12 .. 15); A.1 #1, #3, #5.
# w13 = 0x0900 << 16 would be rejection attempt 0x900 of the indexed draw: no entry point reaches it, it pins the restatement alone.
VECTORS = [
    (ZERO_KEY, (0, 0, 0, 0),
     "76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7da41597c5157488d7724e03fb8d84a376a43b8f41518a11cc387b669b2ee6586"),
    (KEY_A, (1, 0x09000000, 0x4A000000, 0),
     "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4ed2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e"),
    (ONE_KEY, (1, 0, 0, 0),
     "3aeb5224ecf849929b9d828db1ced4dd832025e8018b8160b82284f3c949aa5a8eca00bbb4a73bdad192b5c42f73f2fd4e273644c8b36125a64addeb006c13a0"),
    (ZERO_KEY, (0, 0, 0, 0x02000000),
     "c2c64d378cd536374ae204b9ef933fcd1a8b2288b3dfa49672ab765b54ee27c78a970e0e955c14f3a88e741b97c286f75f8fc299e8148362fa198a39531bed6d"),
]


def keyed(pkg, key):
    """the dehalo_rng struct of prover.KeyedRng(key)"""
    from dehalo2_amd import native, prover
    r = native.rng_struct(prover.KeyedRng(key))
    assert r.kind == native.RNG_CHACHA20 == 3
    return r


def masked(half_block: bytes, f) -> int:
    return int.from_bytes(half_block, "little") & ((1 << f.p.bit_length()) - 1)


_INDEXED = {}


def indexed_draws(f, key, stream):
    """the reference's first N_MAX indexed draws [(scalar, attempt)], made once; a smaller n is a prefix"""
    k = (f.name, key, stream)
    if k not in _INDEXED:
        _INDEXED[k] = [CR.indexed(key, stream, i, f.p, f.p.bit_length()) for i in range(N_MAX)]
    return _INDEXED[k]


def reaches_attempts(draws):
    seen = collections.Counter(a for _, a in draws)
    return all(seen[a] >= 1 for a in (1, 2, 3)), dict(seen)


# ------------------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("case", range(len(VECTORS)))
def test_reference_block_function_is_rfc8439(case):
    key, words, want = VECTORS[case]
    assert len(want) == 128
    assert CR.block(key, *words).hex() == want


@pytest.mark.parametrize("key", (KEY_A, KEY_B), ids=("key_a", "key_b"))
@pytest.mark.parametrize("fname", FIELDS)
def test_host_serial_stream_equals_the_reference(pkg, fname, key):
    """dehalo_rng_scalars under the keyed kind = stream 0: consecutive blocks, two candidates each, a rejected one gone with its half block.  `skip` moves no
    ChaCha20 stream (include/dehalo.h): skip = 30 returns the scalars of skip = 0.  The caller's key is left as it is."""
    f = pkg.fields.FIELDS[fname]
    lib = pkg.load_library()
    r = keyed(pkg, key)
    out = np.zeros((4096, 4), dtype=np.uint64)
    assert lib.dehalo_rng_scalars(C.byref(r), f.id, 0, out.ctypes.data, 4096) == 0
    want = list(itertools.islice(CR.serial(key, f.p, f.p.bit_length()), 4096))
    assert all(v < f.p for v in want)
    got = [int(v[0]) | int(v[1]) << 64 | int(v[2]) << 128 | int(v[3]) << 192 for v in out]
    assert got == want, "first difference at scalar %d" % next(i for i in range(4096) if got[i] != want[i])
    assert bytes(r.pcg_state) + bytes(r.pcg_inc) == key and r.kind == 3
    again, skipped = np.zeros((64, 4), dtype=np.uint64), np.zeros((64, 4), dtype=np.uint64)
    assert lib.dehalo_rng_scalars(C.byref(r), f.id, 0, again.ctypes.data, 64) == 0
    assert lib.dehalo_rng_scalars(C.byref(r), f.id, 30, skipped.ctypes.data, 64) == 0
    assert np.array_equal(again, out[:64]) and np.array_equal(skipped, out[:64])


def test_host_serial_stream_starts_with_the_rfcs_blocks(pkg):
    """Without the restatement in between: under the zero key the first block of stream 0 is A.1 #1 -- both its halves are below BN254 Fr's modulus once
    masked, so they are the first two scalars; under the key 00 .. 00 01 the second block is A.1 #3, and both its masked halves are scalars too."""
    f = pkg.fields.FIELDS["bn254_fr"]
    lib = pkg.load_library()
    for key, _, hexblock in (VECTORS[0], VECTORS[2]):
        halves = [masked(bytes.fromhex(hexblock)[:32], f), masked(bytes.fromhex(hexblock)[32:], f)]
        assert all(h < f.p for h in halves)
        out = np.zeros((4, 4), dtype=np.uint64)
        assert lib.dehalo_rng_scalars(C.byref(keyed(pkg, key)), f.id, 0, out.ctypes.data, 4) == 0
        got = [int(v[0]) | int(v[1]) << 64 | int(v[2]) << 128 | int(v[3]) << 192 for v in out]
        if key == ZERO_KEY:
            assert got[:2] == halves
        else:
            at = got.index(halves[0])
            assert got[at:at + 2] == halves


@pytest.mark.parametrize("fname", FIELDS)
def test_reference_draws_reach_rejection_attempts_1_2_3(pkg, fname):
    """A condition on the INPUTS of the device tests, asserted so that it cannot go soft: for each field the reference's own indexed draws contain scalars
    produced at attempts 1, 2 and 3 (BN254 rejects about a quarter of all candidates: ~48 of 4096 draws at attempt 3; Pasta about half: hundreds) -- on
    stream 1 within the first 4096, and on every stream of the device test within its 4099."""
    f = pkg.fields.FIELDS[fname]
    for key in (KEY_A, KEY_B):
        ok, seen = reaches_attempts(indexed_draws(f, key, 1)[:4096])
        assert ok, seen
    for stream in STREAMS:
        ok, seen = reaches_attempts(indexed_draws(f, KEY_A, stream))
        assert ok, (stream, seen)


def test_acceptance_step_on_crafted_candidates():
    """chacha_accept (csrc/hostrng.hpp), the one function the host's draw and the kernel share, at the boundaries no keystream reaches"""
    out = subprocess.run(["make", "-C", ROOT, "hostrng_check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    run = subprocess.run([os.path.join(ROOT, "tests", "native_host", "hostrng_check")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("286 checks passed"), run.stdout


def test_unknown_kinds_are_refused_without_a_device(pkg):
    """dehalo_rng_scalars takes kinds 0 .. 3 and refuses the rest (HostRng::init, the gate of every export that takes a dehalo_rng: hostrng_check.cpp calls it
    directly); the device entry point refuses a NULL context before anything else."""
    from dehalo2_amd._lib import CRng
    lib = pkg.load_library()
    out = np.zeros((2, 4), dtype=np.uint64)
    for kind in (4, 5, 255, -1, 1 << 30):
        r = keyed(pkg, KEY_A)
        r.kind = kind
        assert lib.dehalo_rng_scalars(C.byref(r), 0, 0, out.ctypes.data, 2) == INVALID
        assert not out.any()
    assert lib.dehalo_rng_scalars(C.byref(keyed(pkg, KEY_A)), 4, 0, out.ctypes.data, 2) == INVALID      # an unknown field
    assert lib.dehalo_rng_scalars_device(None, C.byref(keyed(pkg, KEY_A)), 0, 1, None, 0, None) == INVALID
    assert C.sizeof(CRng) == 56                                                                          # the struct of the three earlier kinds, unchanged
    from dehalo2_amd import prover
    with pytest.raises(ValueError):
        prover.KeyedRng(b"short")


# ------------------------------------------------------------------------------------------------------------------------------ GPU: the kernel
PATTERN = 0xA5A5A5A55A5A5A5A


def device_draw(ctx, f, r, stream, n):
    """-> (the n scalars as integers, the four guard elements behind them) of dehalo_rng_scalars_device into a buffer pre-filled with PATTERN"""
    buf = ctx.upload(np.full((n + 4, 4), PATTERN, dtype=np.uint64))
    ctx.rng_scalars_device(r, f.id, stream, buf.data_ptr(), n)
    out = ctx.download_tensor(buf)
    return [int(v[0]) | int(v[1]) << 64 | int(v[2]) << 128 | int(v[3]) << 192 for v in out[:n]], out[n:]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("stream", STREAMS, ids=("stream1", "stream2", "word15"))
@pytest.mark.parametrize("fname", FIELDS)
def test_device_draw_equals_the_indexed_reference(pkg, ctx, fname, stream, n):
    f = pkg.fields.FIELDS[fname]
    ref = indexed_draws(f, KEY_A, stream)[:n]
    if n == N_MAX:
        ok, seen = reaches_attempts(ref)
        assert ok, seen
    got, tail = device_draw(ctx, f, keyed(pkg, KEY_A), stream, n)
    want = [v for v, _ in ref]
    assert got == want, "first difference at scalar %d (reference attempt %d)" % next((i, ref[i][1]) for i in range(n) if got[i] != want[i])
    assert (tail == np.uint64(PATTERN)).all(), "the kernel wrote behind its n scalars"


@pytest.mark.gpu
@pytest.mark.parametrize("fname", FIELDS)
def test_device_streams_1_and_2_share_no_element(pkg, ctx, fname):
    f = pkg.fields.FIELDS[fname]
    one, _ = device_draw(ctx, f, keyed(pkg, KEY_A), 1, N_MAX)
    two, _ = device_draw(ctx, f, keyed(pkg, KEY_A), 2, N_MAX)
    assert len(set(one)) == len(set(two)) == N_MAX and not set(one) & set(two)
    other, _ = device_draw(ctx, f, keyed(pkg, KEY_B), 1, N_MAX)
    assert not set(one) & set(other)


@pytest.mark.gpu
def test_device_draw_starts_with_the_rfcs_blocks(pkg, ctx):
    """Without the restatement in between (BN254 Fr, where the masked first halves are below p): zero key, stream 0, scalar 0 = A.1 #1; key 00 .. 01, stream 0,
    scalar 1 = A.1 #3; zero key, the stream that sets word 15, scalar 0 = A.1 #5."""
    f = pkg.fields.FIELDS["bn254_fr"]
    for (key, words, hexblock), stream, index in ((VECTORS[0], 0, 0), (VECTORS[2], 0, 1), (VECTORS[3], STREAM_W15, 0)):
        assert words == (index, 0, stream & 0xFFFFFFFF, stream >> 32)
        want = masked(bytes.fromhex(hexblock)[:32], f)
        assert want < f.p
        got, _ = device_draw(ctx, f, keyed(pkg, key), stream, 2)
        assert got[index] == want


@pytest.mark.gpu
def test_device_entry_point_refusals(pkg, ctx):
    """Every kind but 3 is refused (the default kind too: its output could not be checked), and what is refused writes nothing; n = 0 does nothing."""
    from dehalo2_amd import native, prover
    lib, f = pkg.load_library(), pkg.fields.FIELDS["pasta_fp"]
    buf = ctx.upload(np.full((8, 4), PATTERN, dtype=np.uint64))
    call = lambda r, field=f.id, n=4, out=True: lib.dehalo_rng_scalars_device(ctx.handle, C.byref(r) if r is not None else None, field, 1, buf.data_ptr() if out else None, n, None)
    good = keyed(pkg, KEY_A)
    os_kind = keyed(pkg, KEY_A)
    os_kind.kind = native.RNG_OS
    unknown = keyed(pkg, KEY_A)
    unknown.kind = 4
    assert call(None) == INVALID
    assert call(native.rng_struct(prover.SeededRng(7))) == INVALID
    assert call(native.rng_struct(_Callback())) == INVALID
    assert call(os_kind) == INVALID and call(unknown) == INVALID
    assert call(good, field=4) == INVALID and call(good, field=-1) == INVALID
    assert call(good, n=1 << 29) == INVALID
    assert call(good, out=False) == INVALID
    assert call(good, n=0) == 0 and call(good, n=0, out=False) == 0
    assert (ctx.download_tensor(buf) == np.uint64(PATTERN)).all()
    assert call(good) == 0
    out = ctx.download_tensor(buf)
    assert (out[4:] == np.uint64(PATTERN)).all() and not (out[:4] == np.uint64(PATTERN)).any()


class _Callback:
    """an object with .scalars and no PCG64 inside: native.rng_struct makes a DEHALO_RNG_CALLBACK of it"""

    def scalars(self, count):
        return np.zeros((count, 4), dtype=np.uint64)


# ------------------------------------------------------------------------------------------------------------------------------ GPU: whole proofs
def first_difference(got, want):
    return [i // 32 for i in range(0, max(len(got), len(want)), 32) if got[i:i + 32] != want[i:i + 32]][:8]


@pytest.fixture(scope="module")
def kzg(pkg, po, co, ctx):
    """tests/test_multi_circuit.py's Rlast_k6 case (chain, witnesses) with its key on the device"""
    import pairing as pr
    import plonk_oracle as PO
    import test_multi_circuit as MC
    from dehalo2_amd import native
    cs = MC.case_of(pkg, po, co, "Rlast_k6")
    c = cs["chain"]
    ccs, fixed, asm, selectors = MC.native_circuit(pkg, po, "Rlast_k6")
    params = native.ParamsKZG.create(ctx, pkg.fields.BN254, c["k"], c["srs"]["g"], c["srs"]["g_lagrange"], pr.g2_to_raw(pr.G2), pr.g2_to_raw(c["s_g2"]))
    pk = native.ProvingKey.keygen(ctx, params, ccs, fixed, asm, selectors)
    assert pk.vk_bytes() == PO.vk_bytes(po.BN254, c["key"], selectors)
    pk.transcript_repr = c["rep"]
    yield dict(case=cs, params=params, pk=pk)
    pk.release(); params.release()


@pytest.fixture(scope="module")
def side_ctx(pkg, ctx):
    c = pkg.Context(0)
    yield c
    c.close()


def kzg_reference(po, cs, N, scheme, key):
    """the oracle prover's proof over the first N witnesses under ReferenceRng(key); KZG has one n-scalar draw, the random polynomial's"""
    import plonk_oracle as PO
    import proof_chains as PC
    c = cs["chain"]
    rng = CR.ReferenceRng(key, po.BN254.scalar.p, 1 << c["k"])
    proof = PO.create_proof_multi(po.BN254, c["srs"], c["key"], cs["advs"][:N], cs["insts"][:N], rng, c["rep"], PC.THREADS, scheme)[0]
    assert rng.large == 1
    return proof


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,with_side", (("gwc", False), ("gwc", True), ("shplonk", True)), ids=("gwc_one_context", "gwc_side_context", "shplonk_side_context"))
def test_kzg_proof_under_a_key_equals_the_oracle(pkg, po, ctx, side_ctx, kzg, scheme, with_side):
    """Blinding rows and blinds from the host's stream 0, the random polynomial from the kernel on stream 1 -- queued by the proving thread (one context) or
    by the helper thread on the side context's stream"""
    import test_multi_circuit as MC
    from dehalo2_amd import native, prover
    cs = kzg["case"]
    want = kzg_reference(po, cs, 1, scheme, KEY_A)
    P = native.Prover(kzg["params"], kzg["pk"], side_ctx=side_ctx if with_side else None, multiopen=scheme)
    try:
        proof = P.create_proof(cs["advs"][0], cs["insts"][0], prover.KeyedRng(KEY_A)).finalize()
        assert len(proof) == len(want) and not first_difference(proof, want), "proof items differ from the oracle's: %r" % first_difference(proof, want)
        assert MC.accepts(po, cs["chain"], proof, cs["insts"][:1], scheme)
    finally:
        P.release()


@pytest.mark.gpu
def test_kzg_proof_over_two_circuits_under_a_key_equals_the_oracle(pkg, po, ctx, kzg):
    from dehalo2_amd import native, prover
    cs = kzg["case"]
    want = kzg_reference(po, cs, 2, "gwc", KEY_A)
    P = native.Prover(kzg["params"], kzg["pk"], num_circuits=2)
    try:
        proof = P.create_proof_multi(cs["advs"][:2], cs["insts"][:2], prover.KeyedRng(KEY_A)).finalize()
        assert len(proof) == len(want) and not first_difference(proof, want), "proof items differ from the oracle's: %r" % first_difference(proof, want)
    finally:
        P.release()


@pytest.mark.gpu
def test_one_key_twice_and_two_keys(pkg, po, ctx, kzg):
    """A key is not written back: the same key gives the same bytes.  Keys that differ in the last byte differ from the first advice commitment on -- the
    first point a blinding row touches."""
    import test_multi_circuit as MC
    from dehalo2_amd import native, prover
    cs = kzg["case"]
    P = native.Prover(kzg["params"], kzg["pk"])
    try:
        rng = prover.KeyedRng(KEY_A)
        a = P.create_proof(cs["advs"][0], cs["insts"][0], rng).finalize()
        assert rng.key == KEY_A
        assert P.create_proof(cs["advs"][0], cs["insts"][0], rng).finalize() == a
        b = P.create_proof(cs["advs"][0], cs["insts"][0], prover.KeyedRng(KEY_B)).finalize()
        assert len(b) == len(a) and b[:32] != a[:32]
        assert MC.accepts(po, cs["chain"], b, cs["insts"][:1], "gwc")
    finally:
        P.release()


def ipa_case(pkg, po, co, curve, k=6):
    """tests/proof_chains.py's IPA chain of circuits.synthesize(p, k, no range lookups, seed=3) over `curve` (ipa_chain itself is Vesta's)"""
    import ipa
    import plonk_oracle as PO
    import proof_chains as PC
    import shapes
    from dehalo2_amd import circuits
    circ = circuits.synthesize(curve.scalar.p, k, False, seed=3)
    desc = shapes.maingate_description(False)
    assert desc == circ.cs.description()
    c = PC._chain(curve, co, desc, k, circ.fixed, circ.assembly.mapping, circ.advice)
    uw = co.fixed_base_mul(po.CURVE_IDS[curve.name], co.fill_scalars(po.FIELD_IDS[curve.scalar.name], "uniform", 2, 7))
    fc, pc = ipa.blinded_key_commitments(curve, c["key"], uw[1])
    ipa_key = dict(c["key"], fixed_commitments=fc, perm_commitments=pc)
    return dict(c, u=uw[0], w=uw[1], fc=fc, pc=pc, circ=circ, rep=PO.transcript_repr(curve, ipa_key, circ.selectors))


@pytest.mark.gpu
@pytest.mark.parametrize("curve_name,with_side", (("vesta", True), ("pallas", False)), ids=("vesta_side_context", "pallas_one_context"))
def test_ipa_proof_under_a_key_equals_the_oracle(pkg, po, co, ctx, side_ctx, curve_name, with_side):
    """Streams 1 (the random polynomial) and 2 (s_poly of the opening) are both live in one proof, with the serial stream on either side of each"""
    import plonk_oracle as PO
    import proof_chains as PC
    import verifier as V
    from dehalo2_amd import native, prover
    curve, spec, k = po.CURVES[curve_name], pkg.fields.CURVES[curve_name], 6
    c = ipa_case(pkg, po, co, curve, k)
    rng = CR.ReferenceRng(KEY_A, curve.scalar.p, 1 << k)
    want = PO.create_proof_ipa(curve, c["srs"], c["u"], c["w"], c["key"], c["adv"], [[]], rng, c["rep"], PC.THREADS)[0]
    assert rng.large == 2
    assert V.verify_proof_ipa(curve, c["desc"], k, c["fc"], c["pc"], c["rep"], c["srs"]["g"], c["srs"]["g_lagrange"], c["u"], c["w"], [[]], want)
    params = native.ParamsIPA.create(ctx, spec, k, c["srs"]["g"], c["srs"]["g_lagrange"], c["w"], c["u"])
    pk = native.ProvingKey.keygen(ctx, params, c["circ"].cs, c["circ"].fixed, c["circ"].assembly, c["circ"].selectors)
    pk.transcript_repr = c["rep"]
    P = native.Prover(params, pk, ctx, side_ctx if with_side else None)
    try:
        proof = P.create_proof(c["adv"], [[]], prover.KeyedRng(KEY_A)).finalize()
        assert len(proof) == len(want) and not first_difference(proof, want), "proof items differ from the oracle's: %r" % first_difference(proof, want)
    finally:
        P.release(); pk.release(); params.release()


@pytest.mark.gpu
def test_stand_alone_opening_under_a_key_equals_the_oracle(pkg, po, co, ctx):
    """dehalo_ipa_open at k = 4: s_poly from the kernel on stream 1, s_poly_blind and the rounds' l_rand / r_rand from stream 0"""
    import test_ipa as TI
    from dehalo2_amd import native, prover
    cs, curve, k = pkg.fields.VESTA, po.VESTA, 4
    prm, g, u, w = TI._params(pkg, ctx, co, pkg.fields, cs, k)
    try:
        poly = TI._poly(pkg.fields, cs, 1 << k, 4)
        blind, x3 = 4242, 0x55AA55
        d_poly = ctx.upload(cs.scalar.encode_many(poly))
        got = prm.open(d_poly.data_ptr(), blind, x3, rng=prover.KeyedRng(KEY_A)).finalize()
        rng = CR.ReferenceRng(KEY_A, curve.scalar.p, 1 << k)
        want = TI.reference_opening(curve, g, u, w, poly, blind, x3, rng.scalars)
        assert rng.large == 1
        assert got == want, first_difference(got, want)
        assert prm.open(d_poly.data_ptr(), blind, x3, rng=prover.KeyedRng(KEY_B)).finalize()[:32] != got[:32]      # S = commit(s_poly, s_poly_blind)
    finally:
        prm.release()


@pytest.mark.gpu
def test_proving_calls_refuse_unknown_kinds(pkg, po, co, ctx, kzg):
    """dehalo_create_proof, dehalo_create_proof_multi and dehalo_ipa_open with kinds >= 4: DEHALO_ERR_INVALID, and the prover proves again afterwards"""
    import test_ipa as TI
    from dehalo2_amd import native, prover
    lib, cs = pkg.load_library(), kzg["case"]
    adv = np.ascontiguousarray(cs["advs"][0], dtype=np.uint64)
    none, zero = (C.c_void_p * 1)(None), (C.c_size_t * 1)(0)
    P = native.Prover(kzg["params"], kzg["pk"])
    try:
        want = P.create_proof(cs["advs"][0], cs["insts"][0], prover.KeyedRng(KEY_A)).finalize()
        for kind in (4, 7, -1):
            r = keyed(pkg, KEY_A)
            r.kind = kind
            tr = native.Blake2bWrite(kzg["pk"].curve)
            assert lib.dehalo_create_proof(P.handle, adv.ctypes.data, none, zero, 0, C.byref(r), tr.handle, 0) == INVALID
            assert lib.dehalo_create_proof_multi(P.handle, (C.c_void_p * 1)(adv.ctypes.data), none, zero, 0, 1, C.byref(r), tr.handle, 0) == INVALID
        assert P.create_proof(cs["advs"][0], cs["insts"][0], prover.KeyedRng(KEY_A)).finalize() == want
    finally:
        P.release()
    vs = pkg.fields.VESTA
    prm, g, u, w = TI._params(pkg, ctx, co, pkg.fields, vs, 4)
    try:
        d_poly = ctx.upload(vs.scalar.encode_many(TI._poly(pkg.fields, vs, 16, 4)))
        b, x = vs.scalar.encode(5), vs.scalar.encode(6)
        r = keyed(pkg, KEY_A)
        r.kind = 4
        tr = native.Blake2bWrite(vs)
        assert lib.dehalo_ipa_open(ctx.handle, prm.handle, d_poly.data_ptr(), b.ctypes.data, x.ctypes.data, C.byref(r), tr.handle) == INVALID
    finally:
        prm.release()
