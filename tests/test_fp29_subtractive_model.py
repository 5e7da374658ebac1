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
