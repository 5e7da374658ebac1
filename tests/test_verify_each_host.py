"""CPU suite: dehalo_verify_proofs_each -- a verdict per proof from one batch verification -- on the HOST verifiers (ctx = None: csrc/verify_host.hpp
verify_proofs_each_host over the host backend's per-segment double-and-add, csrc/blame_search.hpp) against dehalo_verify_proof of every proof alone and the
oracle's verifiers.

Proofs come from the ORACLE prover (tests/verify_cases.py "one", "three", "instance" under GWC and SHPLONK; tests/verify_ipa_cases.py "one", "instance"), two valid
proofs a case, repeated to fill a batch.  Batches of 8 and 9 (a power of two, and one more: the search's halves are then unequal) with the bad set none, {5},
{0, last} and all -- a bad proof has one evaluation flipped --, and one with a truncated proof (MALFORMED) next to a flipped one.  Per batch: reasons[i] is what
verify gives for proof i alone, the accept bit is the oracle's, and the subset checks stay within 1 (nothing bad) / 1 + 2 b ceil(log2 n) over the n proofs the
walk leaves.  Then count = 0 and 1, two copies of one invalid proof, the weights' draw (w_1 = r - 1 lets the two copies cancel, as in verify_batch: why the weights
must be unpredictable), and the argument errors, which are verify_batch's."""
import ctypes as C

import pytest

import verify_cases as VC
import verify_ipa_cases as VI

R_BN254 = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SEEDS = (7, 8)
KZG = [(name, mo) for name in ("one", "three", "instance") for mo in VC.MULTIOPENS]
IPA = ["one", "instance"]


def bound(n, bad):
    """the subset checks n proofs with `bad` invalid ones may cost (csrc/blame_search.hpp)"""
    if n == 0:
        return 0
    return 1 if bad == 0 else 1 + 2 * bad * (n - 1).bit_length()


def bad_sets(size):
    return {"none": set(), "{5}": {5}, "{0, last}": {0, size - 1}, "all": set(range(size))}


class Weights:
    """a DEHALO_RNG_CALLBACK generator that hands out the given scalars, in order"""

    def __init__(self, field, values):
        self.field, self.values, self.drawn = field, list(values), 0

    def scalars(self, count):
        out = self.field.encode_many(self.values[self.drawn:self.drawn + count])
        assert out.shape[0] == count, "the library drew more scalars than count - 1"
        self.drawn += count
        return out


class Kzg:
    """one KZG case under one multiopen: its host verifier, two valid proofs and the same with an evaluation flipped"""
    PROVEN_BAD = VC.PAIRING

    def __init__(self, pkg, po, co, name, multiopen, ctx=None, verifier=None):
        self.po, self.mo = po, multiopen
        self.cz = VC.case(pkg, po, co, name)
        self.v = verifier if verifier is not None else VC.host_verifier(pkg, self.cz, multiopen, ctx=ctx)
        self.valid = [VC.proof(pkg, po, co, name, multiopen, s) for s in SEEDS]
        self.off = VC.sections(po, self.cz, multiopen)["advice evaluation"][0]
        self.N, self.instances = self.cz["N"], self.cz["instances"]

    def flipped(self, p):
        return VC.flip(p, self.off)

    def single(self, p):
        return VC.verify(self.v, self.cz, p)

    def oracle(self, p):
        return VC.oracle_accepts(self.po, self.cz, p, self.mo)


class Ipa:
    PROVEN_BAD = VI.OPENING

    def __init__(self, pkg, po, co, name, verifier=None):
        self.po = po
        self.cz = VI.case(pkg, po, co, name)
        self.v = verifier if verifier is not None else VI.host_verifier(pkg, self.cz)
        self.valid = [VI.proof(pkg, po, co, name, s) for s in SEEDS]
        self.off = VI.sections(po, self.cz, len(self.valid[0]))["advice evaluation"][0]
        self.N, self.instances = 1, self.cz["instances"]

    def flipped(self, p):
        return VI.flip(p, self.off)

    def single(self, p):
        return VI.verify(self.v, self.cz, p)

    def oracle(self, p):
        return VI.oracle_accepts(self.po, self.cz, p)


def each(s, proofs, rng=None):
    """-> (reasons, checks) of verify_each on the case's verifier"""
    reasons = s.v.verify_each(proofs, [s.instances] * len(proofs), rng=rng, num_circuits=s.N)
    return reasons, s.v.last_checks


def check_batch(s, proofs, label=""):
    """verify_each on `proofs` against verify on each alone, the oracle's accept bit and the bound on the checks"""
    reasons, checks = each(s, proofs)
    singles = {p: s.single(p) for p in set(proofs)}
    assert reasons == [singles[p][1] for p in proofs], label
    for p in set(proofs):
        assert s.oracle(p) is singles[p][0], label
    live = [r for r in reasons if r in (0, s.PROVEN_BAD)]      # (the walk rejects MALFORMED proofs: they take no part in the search)
    assert checks <= bound(len(live), sum(1 for r in live if r)), (label, checks)
    if not any(live):
        assert checks == (1 if live else 0), label
    return reasons, checks


def batches_of(s, size):
    base = [s.valid[i % len(s.valid)] for i in range(size)]
    for label, bad in bad_sets(size).items():
        yield "%d proofs, bad %s" % (size, label), [s.flipped(p) if i in bad else p for i, p in enumerate(base)], bad
    mixed = list(base)
    mixed[2] = mixed[2][:-1]
    mixed[6] = s.flipped(mixed[6])
    yield "%d proofs, one truncated and one flipped" % size, mixed, None


def run_case(s):
    assert len(set(s.valid)) == len(SEEDS) and all(s.single(p) == (True, 0) for p in s.valid)
    assert all(s.single(s.flipped(p)) == (False, s.PROVEN_BAD) for p in s.valid)
    for size in (8, 9):
        for label, proofs, bad in batches_of(s, size):
            reasons, checks = check_batch(s, proofs, label)
            if bad is not None:
                assert [i for i, r in enumerate(reasons) if r] == sorted(bad), label
                assert all(r == s.PROVEN_BAD for r in reasons if r), label
            else:
                assert reasons == [0, 0, VC.MALFORMED, 0, 0, 0, s.PROVEN_BAD] + [0] * (size - 7), label
    # the figures of the search: one bad proof among 8 costs 1 + 2 * 3 checks at the most, all 8 bad 15
    assert each(s, [s.flipped(p) for p in (s.valid * 4)])[1] == 15


@pytest.fixture(scope="module")
def kzg(pkg, po, co):
    made = {}

    def fn(name, multiopen):
        if (name, multiopen) not in made:
            made[(name, multiopen)] = Kzg(pkg, po, co, name, multiopen)
        return made[(name, multiopen)]
    return fn


@pytest.fixture(scope="module")
def ipa(pkg, po, co):
    made = {}

    def fn(name):
        if name not in made:
            made[name] = Ipa(pkg, po, co, name)
        return made[name]
    return fn


@pytest.mark.parametrize("name,multiopen", KZG)
def test_kzg_reasons_are_the_single_verdicts(kzg, name, multiopen):
    run_case(kzg(name, multiopen))


@pytest.mark.parametrize("name", IPA)
def test_ipa_reasons_are_the_single_verdicts(ipa, name):
    run_case(ipa(name))


def edge_counts(s):
    assert each(s, []) == ([], 0)
    good, bad = s.valid[0], s.flipped(s.valid[0])
    assert each(s, [good]) == ([0], 1)
    assert each(s, [bad]) == ([s.PROVEN_BAD], 1)          # the one check fails, and a set of one needs no second
    assert each(s, [good[:-32]]) == ([VC.MALFORMED], 0)   # nothing is left to check
    assert each(s, [good + b"\0", b""]) == ([VC.MALFORMED, VC.MALFORMED], 0)
    # two copies of one invalid proof are both named
    assert each(s, [bad, bad])[0] == [s.PROVEN_BAD] * 2
    assert each(s, [good, bad, bad, good])[0] == [0, s.PROVEN_BAD, s.PROVEN_BAD, 0]


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
def test_kzg_count_zero_one_and_copies(kzg, multiopen):
    edge_counts(kzg("one", multiopen))


def test_ipa_count_zero_one_and_copies(ipa):
    edge_counts(ipa("one"))


@pytest.mark.parametrize("multiopen", VC.MULTIOPENS)
def test_the_weights_are_verify_batchs(pkg, kzg, multiopen):
    """w_0 = 1 and w_1 .. the generator's first count - 1 scalars: under w_1 = r - 1 two copies of one invalid proof cancel in every subset that holds both and
    are reported valid -- by verify_batch and by verify_each alike -- which is why the weights must be unpredictable; under w_1 = 1 both are named"""
    s = kzg("one", multiopen)
    f = pkg.fields.BN254.scalar
    bad, good = s.flipped(s.valid[0]), s.valid[1]
    inst = [s.instances] * 2
    w = Weights(f, [R_BN254 - 1])
    assert each(s, [bad, bad], rng=w) == ([0, 0], 1) and w.drawn == 1
    w = Weights(f, [R_BN254 - 1])
    assert s.v.verify_batch([bad, bad], inst, rng=w, num_circuits=1) is True
    w = Weights(f, [1])
    assert each(s, [bad, bad], rng=w)[0] == [VC.PAIRING] * 2 and w.drawn == 1
    w = Weights(f, [12345, 678])      # three proofs draw two scalars
    assert each(s, [good, bad, good], rng=w)[0] == [0, VC.PAIRING, 0] and w.drawn == 2


def test_argument_errors_are_verify_batchs(pkg, kzg, ipa):
    for s, f in ((kzg("instance", "gwc"), pkg.fields.BN254.scalar), (ipa("instance"), pkg.fields.VESTA.scalar)):
        p = s.valid[0]
        usable = (1 << s.cz["c"]["k"]) - (s.cz["cs"].blinding_factors() + 1)
        for bad in ([[]], [[[5, 7, 9, 11], [1]]], [[[1] * (usable + 1)]]):      # no column, two columns, a column longer than the usable rows
            errors = []
            for call in (s.v.verify_batch, s.v.verify_each):
                w = Weights(f, [5, 6])
                with pytest.raises(pkg.DehaloError) as e:
                    call([p, p, p], [bad] * 3, rng=w, num_circuits=1)
                assert w.drawn == 0      # a refused call has drawn nothing
                errors.append((e.value.code, str(e.value)))
            assert errors[0] == errors[1] and errors[0][0] == -1, errors
        assert each(s, [p, p, p])[0] == [0, 0, 0]
    s = kzg("one", "gwc")
    with pytest.raises(pkg.DehaloError) as e:
        s.v.verify_each([s.valid[0]], [[[]]], num_circuits=0)      # no circuit
    assert e.value.code == -1
    lib = pkg.load_library()
    reasons, checks = (C.c_int * 2)(7, 7), C.c_uint32(9)
    one = (C.c_void_p * 1)(None)
    lens = (C.c_size_t * 1)(0)
    assert lib.dehalo_verify_proofs_each(None, one, lens, 1, one, lens, 1, 1, None, reasons, C.byref(checks)) == -1
    assert lib.dehalo_verify_proofs_each(s.v.handle, one, lens, 1, one, lens, 1, 1, None, None, C.byref(checks)) == -1      # nowhere to write the reasons
    assert lib.dehalo_verify_proofs_each(s.v.handle, None, None, 1, one, lens, 1, 1, None, reasons, C.byref(checks)) == -1
    assert list(reasons) == [7, 7] and checks.value == 9      # a call in error writes neither
    assert lib.dehalo_verify_proofs_each(s.v.handle, one, lens, 1, one, lens, 1, 1, None, reasons, None) == 0 and reasons[0] == VC.MALFORMED      # checks is optional


def test_timings_keep_their_four_slots(kzg):
    s = kzg("one", "gwc")
    each(s, [s.valid[0], s.flipped(s.valid[1])])
    t = s.v.last_timings()
    assert list(t) == ["decompress", "walk", "msm", "pairing"] and all(v >= 0 for v in t.values()) and t["pairing"] > 0 and t["msm"] > 0
