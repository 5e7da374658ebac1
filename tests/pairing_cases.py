"""Inputs of the pairing-table tests (tests/test_pairing_lines_host.py on the CPU, tests/test_pairing_device.py on the GPU): G1 points as the words
dehalo_pairing_checks reads, checks that cancel or do not over fixed G2 points [b_j] G2, and the change of basis between the library's GT words and the
oracle's degree-12 coefficient lists."""
import numpy as np

B_BIG = 0xFEDCBA0987654321FEDCBA0987654321FEDCBA09      # tests/test_pairing_host.py's large b
BS = (1, 7, B_BIG)                                        # the tables' Q_j = [BS[j]] G2

_g1 = {}


def g1_mul(po, pr, k):
    """[k] G1 as (x, y) canonical ints, None for the identity; remembered"""
    k %= pr.R
    if k not in _g1:
        _g1[k] = po.ec_mul(po.BN254, k, pr.G1) if k else None
    return _g1[k]


def words(pkg, P):
    """(x, y) | None -> the 8 Montgomery words of dehalo_pairing_checks"""
    f = pkg.fields.BN254.base
    out = np.zeros(8, dtype=np.uint64)
    if P is not None:
        out[:4], out[4:] = f.encode(P[0]), f.encode(P[1])
    return out


def g2_raws(pr, pairs):
    return [pr.g2_to_raw(pr.g2_mul(b, pr.G2)) for b in BS[:pairs]]


def check_scalars(pr, pairs, c, cancels):
    """the scalars a_j of check c's points P_j = [a_j] G1 against Q_j = [b_j] G2: sum a_j b_j = 0 mod r iff `cancels` (one pair: the identity cancels, alone)"""
    r = pr.R
    a = [(1000003 * (c + 1) + 17 * j + 5) % r for j in range(pairs - 1)]
    last = -sum(x * b for x, b in zip(a, BS)) * pow(BS[pairs - 1], -1, r) % r
    if not cancels:
        last = (last + c + 1) % r
        assert sum(x * b for x, b in zip(a + [last], BS)) % r != 0
    return a + [last]


def interleaved(pkg, po, pr, pairs, checks):
    """-> (g1 words (checks, pairs, 8), expected statuses): check c cancels iff c % 3 != 1, every check's points its own, so that a mixed-up index shows"""
    g1 = np.zeros((checks, pairs, 8), dtype=np.uint64)
    want = np.zeros(checks, dtype=np.uint8)
    for c in range(checks):
        want[c] = 1 if c % 3 != 1 else 0
        for j, a in enumerate(check_scalars(pr, pairs, c, bool(want[c]))):
            g1[c, j] = words(pkg, g1_mul(po, pr, a))
    return g1, want


def gt_to_f12(pkg, pr, gt):
    """12 x 4 words -- the Fq2 coefficients a_j + b_j i of w^0 .. w^5 -- -> the oracle's 12 coefficients: with i = w^6 - 9, a_j - 9 b_j at w^j and b_j at w^(j + 6)"""
    f = pkg.fields.BN254.base
    v = [f.decode(np.asarray(row, dtype=np.uint64)) for row in np.asarray(gt).reshape(12, 4)]
    return [(v[2 * j] - 9 * v[2 * j + 1]) % pr.Q for j in range(6)] + [v[2 * j + 1] for j in range(6)]
