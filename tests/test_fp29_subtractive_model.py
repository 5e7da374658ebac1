"""The subtractive Montgomery columns of the Pasta primes (csrc/fp29.cuh: f29_montgomery_columns, columns2, f29_mul_pair) in the bit-accurate model
tools/fp29_model.py, against Python integers.  The model itself asserts, on every call, that each signed column value stays in [-2^63, 2^63), that every
emitted limb is in [0, 2^29) and the top limb non-negative, and that the result equals the additive form's limb for limb -- except for a product that is
0 mod 2^261, where it is the additive value + p.  No GPU."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import fp29_model as M

FIELDS = ["pasta_fp", "pasta_fq"]
R = 1 << M.RBITS


@pytest.fixture(scope="module", params=FIELDS)
def F(request):
    return M.F29(M.po.FIELDS[request.param])


def check(F, a, b):
    """mont / sqr on limb vectors against integers: the residue, the bound, the relation to the additive columns"""
    va, vb = M.value(a), M.value(b)
    out = F.mont(a, b)
    T = va * vb
    assert M.value(out) * R % F.p == T % F.p and M.value(out) <= T // R + F.p
    add = M.value(F.mont_additive(a, b))
    assert M.value(out) == add + (F.p if T % R == 0 else 0)
    if a == b and all(2 * x < M.U32 for x in a):
        assert F.sqr(a) == out
    return out


def edge_values(F):
    p = F.p
    return [0, 1, 2, p - 1, p - 2, (p - 1) // 2, F.R, (1 << 232), (1 << 254) % p, M.MASK, M.MASK << 29]


def test_edge_operands(F):
    """0, 1, p - 1, all-ones limbs, top-limb-only operands, each against each: a zero operand returns p (T = 0 mod 2^261), everything else the additive limbs"""
    vecs = [M.limbs(v) for v in edge_values(F)] + [[M.MASK] * 8 + [(F.p >> 232)], [0] * 8 + [1 << 22], [0] * 8 + [M.MASK >> 4], [1] + [0] * 8]
    for a in vecs:
        for b in vecs:
            out = check(F, a, b)
            if M.value(a) == 0 or M.value(b) == 0:
                assert M.value(out) == F.p
    # a product that is 0 mod 2^261 without a zero operand: 2^232 * 2^29
    out = check(F, [0] * 8 + [1], [0, 1] + [0] * 7)
    assert M.value(out) == 1 + F.p


def solve_m(F, rnd, k, target):
    """operands whose multiplier m_k is `target`: column k holds a_0 b_k, a_0 odd, and no earlier column reads b_k"""
    a = [rnd.randrange(M.MASK + 1) | (i == 0) for i in range(8)] + [rnd.randrange(1 << 20)]
    b = [rnd.randrange(M.MASK + 1) for i in range(8)] + [rnd.randrange(1 << 20)]
    b[k] = 0
    F.mont(a, b)
    seen = F.m_seen[k] + ((1 << M.B) if k == 8 else 0)          # m_8 is stored biased by -2^29
    b[k] = (target - seen) * pow(a[0], -1, 1 << M.B) % (1 << M.B)
    F.mont(a, b)
    assert F.m_seen[k] + ((1 << M.B) if k == 8 else 0) == target
    return a, b


def test_single_multipliers_zero_and_all_ones(F):
    rnd = random.Random(29)
    for k in range(9):
        for target in (0, M.MASK):
            a, b = solve_m(F, rnd, k, target)
            check(F, a, b)
    # the low eight multipliers all 0 (b = 2^232: the low eight columns are empty), and all-ones limbs against 1
    check(F, M.limbs(rnd.randrange(F.p)), [0] * 8 + [1])
    assert F.m_seen[:8] == [0] * 8
    check(F, [M.MASK] * 8 + [1 << 20], [1] + [0] * 8)


def test_call_site_bounds(F):
    """operand limbs at the largest bounds each call site admits (tools/fp29_model.py call_site_operands): the sites the HIP code runs on the subtractive
    columns fit with more than a carry to spare, the two it keeps additive do not"""
    refused = M.call_site_bounds(F, random.Random(5))
    assert len(refused) == 2 and all("U" in r for r in refused)
    for name, kind, ops, fits in M.call_site_operands(F):
        if fits and kind == "mul":
            check(F, ops[0], ops[1])
    assert -(1 << 63) <= F.col_min and F.col_max < (1 << 63)


def test_random_pairs(F):
    """a few thousand seeded pairs: canonical values, and lazily reduced ones with 29-bit x 30-bit limbs"""
    rnd = random.Random(2024)
    F.col_min = F.col_max = 0
    for _ in range(1500):
        check(F, M.limbs(rnd.randrange(F.p)), M.limbs(rnd.randrange(F.p)))
    for _ in range(1500):
        a = [rnd.randrange(1 << 29) for _ in range(8)] + [rnd.randrange(1 << 26)]
        b = [rnd.randrange(1 << 30) for _ in range(8)] + [rnd.randrange(1 << 26)]
        check(F, a, b)
    for _ in range(500):
        a = [rnd.randrange(1 << 29) for _ in range(8)] + [rnd.randrange(1 << 26)]
        assert F.sqr(a) == check(F, a, a)
    assert -(1 << 59) < F.col_min and F.col_max < (1 << 63)


def test_bn254_keeps_the_additive_columns():
    F = M.F29(M.po.FIELDS["bn254_fr"])
    assert not F.subtractive
    a, b = M.limbs(F.p - 1), M.limbs(0)
    assert M.value(F.mont(a, b)) == 0 and F.mont(a, a) == F.mont_additive(a, a)


# ---- caller words that are not below p (include/dehalo.h "Non-canonical words") ----
ALL_FIELDS = ["pasta_fp", "pasta_fq", "bn254_fr", "bn254_fq"]      # the Pasta primes on the subtractive columns, BN254 on the additive ones
W256 = 1 << 256


def caller_words(F, rnd, count=200):
    """the stored words a caller may hand over: 2^256 - 1, every multiple of p below 2^256 (and its neighbours), R + p, and random words >= p"""
    p = F.p
    ws = [W256 - 1, W256 - 2, W256 % p + p]
    j = 1
    while j * p < W256:
        ws += [j * p, j * p + 1, j * p - 1]
        j += 1
    assert j - 1 == (W256 - 1) // p and j - 1 >= 3
    ws += [rnd.randrange(p, W256) for _ in range(count)]
    assert all(p - 1 <= w < W256 for w in ws)
    return ws


@pytest.fixture(scope="module", params=ALL_FIELDS)
def G(request):
    return M.F29(M.po.FIELDS[request.param])


def test_from_std_of_words_not_below_p(G):
    """f29_from_std (every poly_load, the points and factors of the poly kernels, the quotient kernels' columns): one multiplication by a canonical constant
    takes any 256-bit word below 2p, with every column and limb assertion of the model on"""
    F, rnd = G, random.Random(77)
    assert F.subtractive == (F.p >> 253 == 2)
    for w in caller_words(F, rnd):
        out = F.from_std(w)
        assert M.value(out) * R % F.p == w * F.TO29 % F.p and M.value(out) < 2 * F.p
        assert all(0 <= v <= M.MASK for v in out[:8])
        assert F.to_std(out) == w % F.p                       # and back: the canonical word it stands for


def test_sites_that_take_a_caller_word_as_a_plain_integer(G):
    """The call sites that unpack a caller's word without a multiplication of its own: a column of k_lincomb against a converted coefficient, a coefficient
    added into a Horner chain (eval_polynomial, kate_division, the vanishing quotient) and multiplied by the point, k_scale's element against its factor, and
    a coset transform's element against zeta: normalized limbs whose top limb has 24 bits, not 22"""
    F, rnd = G, random.Random(78)
    p = F.p
    ws = caller_words(F, rnd, 60)
    for w in ws:
        lw = M.limbs(w)
        assert lw[8] < (1 << 24)
        c = F.from_std(rnd.choice(ws))                        # a converted coefficient / point / factor: < 2p, itself from a lifted word
        prod = F.mont(c, lw)
        assert M.value(prod) * R % p == M.value(c) * w % p and M.value(prod) < 2 * p
        acc = F.add(F.mont(F.from_std(rnd.choice(ws)), c), lw)      # acc x + c_j with a raw coefficient: below 2p + 2^256
        nxt = F.mont(acc, c)
        assert M.value(nxt) < 2 * p and M.value(nxt) * R % p == M.value(acc) * M.value(c) % p
        chain = F.norm(acc)
        for _ in range(8):                                    # eight raw coefficients a thread, then the tree's additions: far below 2^261
            chain = F.norm(F.add(F.mont(chain, c), lw))
        assert M.value(chain) < 2 * p + W256
    # lincomb's sub0: the library reduces the word before the subtraction (f29_canon), because KM dominates a value below 3p only
    for w in ws:
        a = F.mont(F.from_std(rnd.choice(ws)), M.limbs(rnd.choice(ws)))
        d = F.norm(F.sub(a, F.cond_sub(F.cond_sub(F.cond_sub(M.limbs(w), 4 * p), 2 * p), p), F.KM))
        assert M.value(d) % p == (M.value(a) - w) % p
    if W256 > F.KM[1] + 2 * p:      # BN254: 2^256 > 5p > KM = 4p: without the reduction the constant does not dominate the word
        with pytest.raises(AssertionError, match="does not dominate"):
            F.sub(M.limbs(0), M.limbs(W256 - 1), F.KM)


def test_ntt_first_round_on_words_not_below_p(G):
    """k_ntt_pass loads the caller's words as plain integers and its first butterflies do not multiply: u - v + K with v a whole 256-bit word (stage 0) or the
    sum of two (stage 1, twiddle one).  KW dominates both; KM (4p) does not dominate a word above 4p, which BN254 has (2^256 > 5p)."""
    F, rnd = G, random.Random(79)
    p = F.p
    ws = caller_words(F, rnd, 40)
    w1 = F.enc(rnd.randrange(p))
    assert F.KW[0][8] >= (1 << 25) and F.KW[1] % p == 0
    quads = [[W256 - 1] * 4, [0, W256 - 1, 0, W256 - 1], [0, 0, W256 - 1, W256 - 1], [W256 - 1, 0, W256 - 1, 0]] + [[rnd.choice(ws) for _ in range(4)] for _ in range(300)]
    for q in quads:
        out = F.ntt_first_round([M.limbs(w) for w in q], w1, F.KW)
        a, b, c, d = q
        t = M.value(w1) * pow(R, -1, p)
        want = [a + b + c + d, a - b + (c - d) * t, a + b - c - d, a - b - (c - d) * t]
        assert [M.value(o) % p for o in out] == [v % p for v in want]
        assert max(M.value(o) for o in out) < 30 * p          # what the later stages' bounds start from
        F.mont(out[3], w1); F.mont(out[1], w1)                # and the next round multiplies them
    if W256 > F.KM[1] + p:
        with pytest.raises(AssertionError, match="does not dominate"):
            F.ntt_first_round([M.limbs(w) for w in (0, W256 - 1, 0, 0)], w1, F.KM)
    else:                                                     # the Pasta primes: 4p > 2^256 covers one word; two words need KW as well
        F.bfly(M.limbs(0), M.limbs(W256 - 1), None, False, F.KM)
        with pytest.raises(AssertionError, match="does not dominate"):
            F.ntt_first_round([M.limbs(w) for w in (0, 0, W256 - 1, W256 - 1)], w1, F.KM)
