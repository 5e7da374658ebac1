"""Structured keys for the lookup-permutation kernels (csrc/lookup_permute.hip), their crafted misses, and the reference in Python integers.

The parity tests draw tables from the uniform distribution: every comparison of two such keys is decided by word 7.  The families here decide it in a chosen
32-bit word (with the words below it ordered the other way round), at word and limb boundaries, at both ends of the field, and in the production shape
theta * tag + value.  All keys are canonical integers below p of every field (asserted); the word families keep word 7 below 0x30000000, so one recipe serves
BN254 and Pasta.  The reference is oracle/pyoracle.py permute_expression_pair on these integers; encoding and decoding is structured_inputs.StructuredField's.
A plain helper, imported like tests/proof_chains.py.

    F = field(po, "pasta_fq")                 keys(po, F, "word_3", 600) -> 600 distinct ints
    crafted_misses(F, table_keys)             -> [(label, int)], none of them in the table
    reference(po, F, inputs, table, n)        -> (A', S') as ints, or None
"""
import numpy as np

import structured_inputs as SI
from structured_inputs import constant_c, field  # noqa: F401  (field: re-exported)

FIELDS4 = ["bn254_fr", "bn254_fq", "pasta_fp", "pasta_fq"]
FIELDS2 = ["bn254_fr", "pasta_fq"]
WORD_FAMILIES = ["word_%d" % w for w in range(8)]
FAMILIES = WORD_FAMILIES + ["carry", "theta_tag", "small", "uniform"]
TOP_WORD_BOUND = 0x30000000          # below the top word of every field's modulus
M32 = 0xFFFFFFFF


def words(v):
    return [(v >> (32 * w)) & M32 for w in range(8)]


def from_words(ws):
    return sum(x << (32 * w) for w, x in enumerate(ws))


def _word_values(w, count):
    """count distinct values of the deciding word, ascending: 0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF and their neighbours; at 0x80000000 upwards in steps of two
    (so that v and v + 2 are keys and v + 1 is not).  Word 7: small values."""
    if w == 7:
        assert count < TOP_WORD_BOUND
        return list(range(count))
    out, j = set(), 0
    while len(out) < count:
        for v in (j, 0x7FFFFFFF - j, 0x80000000 + 2 * j, M32 - j, 0x40000000 + j * 0x10001):
            if len(out) < count:
                out.add(v & M32)
        j += 1
    return sorted(out)


def word_family(F, w, count):
    """keys equal in every word above w, different in word w, and ANTI-ordered in every word below it: a comparison that skips word w sees the reverse order"""
    top = words(constant_c(F))
    assert top[7] < TOP_WORD_BOUND
    out = []
    for r, v in enumerate(_word_values(w, count)):
        ws = list(top)
        ws[w] = v
        for x in range(w):
            ws[x] = (M32 - r) if (w - x) % 2 else (0x80000000 + (count - 1 - r))
        out.append(from_words(ws))
    return out


def carry_family(F, count):
    """neighbours of word and limb boundaries and both ends of the field; beyond the 22 named ones, the neighbours of every other power of two"""
    p = F.p
    vs = [0, 1, 2]
    for k in (32, 64, 128, 192, 224):
        vs += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    vs += [p - 2, p - 1, (p - 1) // 2, (p + 1) // 2]
    for k in range(2, 254):
        vs += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    j = 3
    while len(set(vs)) < count:
        vs += [p - j, ((p - 1) // 2) - j + 2, (1 << 128) + j]
        j += 1
    seen, out = set(), []
    for v in vs:
        if v not in seen and len(out) < count:
            seen.add(v)
            out.append(v)
    return out


THETA_TAGS = [0, 1, 2, 5, 339]


def theta_tag_family(F, count):
    """theta * tag + value mod p (what the prover compresses a (tag, value) range table to): a few tags, the values filling a range from zero"""
    theta, per = constant_c(F), -(-count // len(THETA_TAGS))
    return [(theta * tag + v) % F.p for tag in THETA_TAGS for v in range(per)][:count]


def keys(po, F, family, count):
    """count distinct canonical keys of the family, in the family's own (not sorted) order"""
    if family.startswith("word_"):
        ks = word_family(F, int(family[5:]), count)
        ks = ks[1::2] + ks[0::2]                        # not handed over sorted
    elif family == "carry":
        ks = carry_family(F, count)
    elif family == "theta_tag":
        ks = theta_tag_family(F, count)
    elif family == "small":
        assert count <= 65521
        ks = [(j * 13 + 5) % 65521 for j in range(count)]
    elif family == "uniform":
        ks = SI.uniform_ints(po, F, count, 4242)
    else:
        raise KeyError(family)
    assert len(ks) == count and len(set(ks)) == count, (family, count)
    bound = F.p if family in ("carry", "theta_tag", "uniform") else min(po.FIELDS[name].p for name in FIELDS4)      # (those three are built from F.p)
    assert 0 <= min(ks) and max(ks) < bound <= F.p
    return ks


def crafted_misses(F, table_keys):
    """[(label, value)]: values that are NOT in the table but sit as close to it as a value can -- one bit of one word of a key flipped (a low and a high bit of
    every word), v + 1 between adjacent keys (first those with v + 2 a key), min - 1, max + 1, p - 1"""
    p, have = F.p, set(table_keys)
    srt = sorted(have)
    out, seen = [], set()

    def add(label, v):
        if 0 <= v < p and v not in have and v not in seen:
            seen.add(v)
            out.append((label, v))
            return True
        return False

    probes = [srt[len(srt) // 2], srt[0], srt[-1], srt[len(srt) // 3]] + srt      # the first of them whose flipped value is below p and no key
    for w in range(8):
        for bit in ((0, 27) if w == 7 else (0, 31)):
            ok = any(add("word%d_bit%d" % (w, bit), k ^ (1 << (32 * w + bit))) for k in probes)
            assert ok or len(srt) < 3, (w, bit)
    gaps = [i for i in range(len(srt) - 1) if srt[i + 1] - srt[i] == 2] or [i for i in range(len(srt) - 1) if srt[i + 1] - srt[i] > 2]
    for i in ([gaps[0], gaps[len(gaps) // 2], gaps[-1]] if gaps else []):
        add("between_%d" % i, srt[i] + 1)
    if srt[0] > 0:
        add("min_minus_1", srt[0] - 1)
    add("max_plus_1", srt[-1] + 1)
    add("p_minus_1", p - 1)
    assert out and all(v not in have and 0 <= v < p for _, v in out)
    return out


def reference(po, F, inputs, table, n):
    """oracle/pyoracle.py permute_expression_pair on canonical ints -> (A', S') or None"""
    return po.permute_expression_pair(F.of, inputs, table, n)


def check_invariants(inputs, table, n, res):
    """the lookup argument's own conditions on (A', S'), checked without either restatement"""
    a, s = res
    assert len(a) == n and len(s) == n
    assert a == sorted(inputs[:n])                                          # A' is the sorted input
    assert sorted(s) == sorted(table[:n])                                   # S' is a permutation of the table
    assert all(a[i] == s[i] or (i > 0 and a[i] == a[i - 1]) for i in range(n))


def draw(n, below, seed):
    return np.random.default_rng(seed).integers(0, max(1, below), size=n).tolist()


# ---- general path -----------------------------------------------------------------------------------------------------------------------------------------
GENERAL_KEYS = 600


def general_case(po, F, family, n, seed=1):
    """-> (inputs, table, keys): the table is the family's keys repeated cyclically, the inputs a fixed-seed draw over a prefix of them (so leftovers exist).  At
    n that is no multiple of the 2048-key tile the table also holds p - 1 (three times from six rows on) and the inputs look it up: the largest value there is
    sits against the sort's +infinity padding."""
    top = (3 if n >= 6 else 1) if n % 2048 else 0
    ks = keys(po, F, family, max(1, min(GENERAL_KEYS, n - top)))
    table = [ks[i % len(ks)] for i in range(n - top)] + [F.p - 1] * top
    table = [table[i] for i in np.random.default_rng(seed + n).permutation(n).tolist()]      # (p - 1 is not only in the last rows)
    prefix = ks[:max(1, len(ks) // 3)]
    inputs = [prefix[i] for i in draw(n, len(prefix), 77 * seed + n)]
    if top:
        inputs[0] = inputs[n - 1] = inputs[n // 2] = F.p - 1
    return inputs, table, ks


PLATEAU_RUNS = [(0, 511), (17, 2049), (40, 513), (41, 4097), (87, 2047)]      # (rank of the key among the sorted keys, run length)
PLATEAU_KEYS = 88


def plateau_table(po, F):
    """-> (table, sorted keys): runs of equal keys that straddle the 512-output merge block and the 2048-key tile, plus singles, rows shuffled"""
    srt = sorted(keys(po, F, "word_0", PLATEAU_KEYS))
    runs = dict(PLATEAU_RUNS)
    table = [k for r, k in enumerate(srt) for _ in range(runs.get(r, 1))]
    order = np.random.default_rng(5).permutation(len(table)).tolist()
    return [table[i] for i in order], srt


def plateau_inputs(srt, n):
    big = srt[41]
    return {"all_one_key": [big] * n,
            "every_key_once_rest_one": srt + [srt[17]] * (n - len(srt)),
            "only_smallest": [srt[0]] * n,
            "only_largest": [srt[-1]] * n}


def input_tile_cases(po, F, n=2049):
    """one input in the second tile: inputs all equal, all distinct, two alternating keys (the table holds every key once)"""
    ks = keys(po, F, "word_3", n)
    table = ks[::-1]
    return table, {"all_equal": [ks[5]] * n, "all_distinct": ks[7:] + ks[:7], "alternating": [ks[3] if i % 2 else ks[n - 2] for i in range(n)]}


# ---- distinct-rows path -----------------------------------------------------------------------------------------------------------------------------------
def distinct_table(entries, seed):
    """entries: [(key, multiplicity)], keys may coincide.  -> (table: every key as often as its entries say, rows shuffled; representative row of every entry and
    its multiplicity as uint32 arrays, the entries in shuffled order)"""
    rng = np.random.default_rng(seed)
    flat, reps, start = [], [], 0
    for key, m in entries:
        assert m >= 1
        flat += [key] * m
        reps.append(start + (m // 2))                                       # some copy of the entry, not always its first
        start += m
    n = len(flat)
    perm = rng.permutation(n)                                               # table[i] = flat[perm[i]]
    where = np.empty(n, dtype=np.int64)
    where[perm] = np.arange(n)
    table = [flat[i] for i in perm.tolist()]
    order = rng.permutation(len(entries))
    rep = np.array([where[reps[e]] for e in order], dtype=np.uint32)
    mult = np.array([entries[e][1] for e in order], dtype=np.uint32)
    assert all(table[int(r)] == entries[e][0] for r, e in zip(rep, order)) and int(mult.sum()) == n
    return table, rep, mult


def spread_multiplicities(d, n, seed):
    """d multiplicities >= 1 that sum to n: half of the spare rows on entry 0 (a range table's padding row), the rest drawn"""
    m = [1] * d
    spare = n - d
    assert spare >= 0
    m[0] += spare - spare // 2
    for i in draw(spare // 2, d, seed):
        m[i] += 1
    return m


def distinct_case(po, F, family, d, n, seed=3):
    """-> (inputs, table, rep, mult): d distinct keys among n rows; the inputs draw over two thirds of the keys (entry 0 and single-copy keys among them)"""
    ks = keys(po, F, family, d)
    table, rep, mult = distinct_table(list(zip(ks, spread_multiplicities(d, n, seed + d))), seed + 1)
    prefix = ks[:max(1, (2 * d) // 3)]
    inputs = [prefix[i] for i in draw(n, len(prefix), seed + 2 + d)]
    return inputs, table, rep, mult


WAVE_SHAPES = ["all_equal", "but_lane_0", "but_lane_31", "but_lane_63", "alternating", "last_wave_cut"]


def wave_inputs(ks, shape, n):
    """inputs in groups of 64 rows (one wave of the rank kernel; the groups start at multiples of 64, so they are aligned to the 2048-row tile): every group its
    own key, with the odd lane out where the shape says so.  last_wave_cut: as all_equal, with an n that cuts the last wave"""
    out = []
    for i in range(n):
        g, lane = divmod(i, 64)
        a, b = ks[(7 * g) % len(ks)], ks[(7 * g + 3) % len(ks)]
        odd = {"all_equal": False, "last_wave_cut": False, "but_lane_0": lane == 0, "but_lane_31": lane == 31, "but_lane_63": lane == 63, "alternating": lane % 2 == 1}[shape]
        out.append(b if odd else a)
    return out
