"""Non-canonical operands for the C ABI: 256-bit words that are not below the modulus, with the canonical words they stand for, in Python integers.

include/dehalo.h ("Non-canonical words"): a field element or scalar read from caller memory is any 256-bit word w and stands for w mod p; what the library computes
and writes is below p; the entry points that only move elements copy the words.  halo2curves never produces a word >= p, so no parity test feeds one.  This module
makes them: `lift` adds a multiple of p to stored words, `families` plants the lifted words where a kernel can treat them differently from their neighbours, and
`canon` takes everything back below p -- with Python integers, never with the library -- so that the truth of a test is the oracle on the canonical input.
A plain helper, imported like tests/structured_inputs.py; words are (n, 4) u64, little-endian limbs, as the ABI takes them.
"""
import random

import numpy as np

W = 1 << 256
ALL_FIELDS = ["bn254_fr", "bn254_fq", "pasta_fp", "pasta_fq"]
FAMILY_LIFTS = {"bn254_fr": (1, 2, 3, 4), "bn254_fq": (1, 2, 3, 4), "pasta_fp": (1, 2), "pasta_fq": (1, 2)}      # the j with x + j p < 2^256 for EVERY x < p
BLOCK_EDGES = (64, 256, 512, 1024, 2048)      # a wave, the blocks of the element-wise and poly kernels, a poly tile (4 x 256), an NTT tile


def to_ints(words):
    b = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def to_words(ints):
    out = bytearray()
    for v in ints:
        out += v.to_bytes(32, "little")          # (raises for a value of more than 256 bits: nothing is truncated)
    return np.frombuffer(bytes(out), dtype=np.uint64).reshape(-1, 4).copy()


def max_lift(w, p):
    """the largest j with w + j p < 2^256"""
    return (W - 1 - w) // p


def lift(words, j, p):
    """stored words + j p (j: one multiple for all, or one per element; 0 leaves an element as it is).  Every lifted element must land in [p, 2^256): a j that
    does not fit is an error, never a case dropped."""
    ints = to_ints(words)
    js = [j] * len(ints) if isinstance(j, int) else list(j)
    assert len(js) == len(ints)
    out = []
    for v, m in zip(ints, js):
        assert m >= 0
        u = v + m * p
        assert u < W and (m == 0 or u >= p), "lift by %d does not fit" % m
        out.append(u)
    return to_words(out)


def canon(words, p):
    return to_words([v % p for v in to_ints(words)])


def all_below(words, p):
    return all(v < p for v in to_ints(words))


def positions(n, edges=BLOCK_EDGES):
    """index 0, the last index, and both sides of every block edge inside the vector"""
    out = {0, n - 1}
    for e in edges:
        if 0 < e < n:
            out |= {e - 1, e}
    return sorted(out)


def special_words(p):
    """name -> (stored word, the canonical word it stands for).  R = 2^256 mod p is the memory form of the field's one."""
    R = W % p
    top = (W - 1) // p * p
    return {"zero_as_p": (p, 0), "zero_as_top_multiple": (top, 0), "one_as_R_plus_p": (R + p, R), "all_ones_word": (W - 1, (W - 1) % p)}


def families(words, p, edges=BLOCK_EDGES, seed=1, singles=True):
    """-> [(name, stored words, canonical words)] for canonical `words`.  The first families keep every residue (canonical words = `words`): every element lifted
    by the largest multiple that fits it, a uniform mix of 0 / 1 / that largest multiple, and one lifted element at each of positions().  The last four overwrite
    the elements at positions() with one of special_words() -- the canonical vector changes with them."""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4)
    ints = to_ints(words)
    n = len(ints)
    assert n and max(ints) < p
    top = [max_lift(v, p) for v in ints]
    assert min(top) >= 1
    rnd = random.Random(seed)
    mix = [rnd.choice((0, 1, t)) for t in top]
    if not any(mix):
        mix[0] = 1                                            # (a vector of one or two elements: the draw may leave all of them alone)
    out = [("all_max", lift(words, top, p), words), ("mix", lift(words, mix, p), words)]
    pos = positions(n, edges)
    if singles:
        for i in pos:
            one = words.copy()
            one[i] = lift(words[i:i + 1], top[i], p)[0]
            out.append(("one@%d" % i, one, words))
    for name, (stored, stands_for) in special_words(p).items():
        s, c = words.copy(), words.copy()
        for i in pos:
            s[i], c[i] = to_words([stored])[0], to_words([stands_for])[0]
        out.append((name, s, c))
    for name, s, c in out:
        assert s.shape == words.shape and not np.array_equal(s, c), name
    return out


def lift_word(word, p, j=None):
    """one element (4 u64) lifted by j (default: the largest that fits)"""
    v = to_ints(word)[0]
    return lift(np.asarray(word).reshape(1, 4), max_lift(v, p) if j is None else j, p)[0]


def uniform_words(po, field, n, seed):
    """n uniform canonical elements in memory form (the integer itself is what is stored: uniform below p either way)"""
    return to_words(po.scalars_uniform(field, n, po.Xoshiro(seed)))
