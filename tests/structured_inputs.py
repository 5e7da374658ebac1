"""Structured operands for the field-vector kernels, and what the kernels must make of them, in Python integers.

The parity tests draw their operands from the uniform distribution, which never produces an output congruent to zero, an intermediate equal to one, a root of
unity of a tile's order, or an extreme starting integer for the inversion's divstep loop.  This module generates the values that do -- canonical (all < p), in
the memory form the ABI takes (4 x u64, x * 2^256 mod p) -- with their expected outputs in closed form.  tests/test_structured_values.py first checks every
closed form against the C restatement (no GPU) and then judges the kernels by them.  A plain helper, imported like tests/proof_chains.py.

    F = field(po, "bn254_fr")        F.p, F.fid, F.omega(log_n), F.enc(list of ints) -> (n, 4) u64, F.dec(array) -> list of ints
"""
import numpy as np

FIELDS3 = ["bn254_fr", "pasta_fp", "pasta_fq"]
FIELDS2 = ["bn254_fr", "pasta_fp"]


class StructuredField:
    def __init__(self, po, name):
        self.of = po.FIELDS[name]
        self.name, self.fid, self.p = name, po.FIELD_IDS[name], self.of.p
        self._rinv = pow(1 << 256, -1, self.p)

    def omega(self, log_n):
        """a primitive 2^log_n-th root of unity (the one EvaluationDomain takes)"""
        return self.of.omega(log_n) if log_n else 1

    def enc1(self, v):
        assert 0 <= v < self.p
        return np.frombuffer(((v << 256) % self.p).to_bytes(32, "little"), dtype=np.uint64).copy()

    def enc(self, vals):
        """canonical ints -> (n, 4) u64 Montgomery limbs (every distinct value is converted once: the structured vectors hold few)"""
        if not len(vals):
            return np.zeros((0, 4), dtype=np.uint64)
        distinct = list(set(vals))
        assert 0 <= min(distinct) and max(distinct) < self.p
        p = self.p
        table = np.frombuffer(b"".join(((v << 256) % p).to_bytes(32, "little") for v in distinct), dtype=np.uint64).reshape(-1, 4)
        row = {v: i for i, v in enumerate(distinct)}
        return table[np.fromiter(map(row.__getitem__, vals), dtype=np.int64, count=len(vals))]

    def dec(self, arr):
        p, ri = self.p, self._rinv
        return [int.from_bytes(r.tobytes(), "little") * ri % p for r in np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)]

    def inv(self, x):
        return pow(x, -1, self.p)


_FIELDS = {}


def field(po, name):
    if name not in _FIELDS:
        _FIELDS[name] = StructuredField(po, name)
    return _FIELDS[name]


def constant_c(F):
    """the constant the families are built on: full width, no structure of its own"""
    return 0x1234567890ABCDEF0FEDCBA9876543210123456789ABCDEF0FEDCBA987654321 % F.p


def log2_ceil(n):
    return max(0, (n - 1).bit_length())


# ---- vectors ------------------------------------------------------------------------------------------------------------------------------------------------
def delta_positions(n):
    return sorted({0, min(1, n - 1), n // 2, n - 1})


def vectors(F, n, w=None):
    """name -> list of n canonical ints.  w: the root of unity the single-frequency inputs are written in (the transform's own root for an NTT test), of order
    2^log2_ceil(n) by default.  The frequencies and delta positions are {0, 1, n/2, n-1} (fewer where they coincide)."""
    p, c = F.p, constant_c(F)
    if w is None:
        w = F.omega(log2_ceil(n))
    out = {"zero": [0] * n, "one": [1] * n, "pm1": [p - 1] * n, "const": [c] * n, "alt": [c if i % 2 == 0 else p - c for i in range(n)]}
    for j in delta_positions(n):
        out["delta%d" % j] = [c if i == j else 0 for i in range(n)]
    wi = pow(w, -1, p)
    for m in delta_positions(n):
        step, v, a = pow(wi, m, p), c, []
        for _ in range(n):
            a.append(v)
            v = v * step % p
        out["freq%d" % m] = a
    out["sparse"] = [(c + i) % p if i % 64 == 0 else 0 for i in range(n)]
    out["selector"] = [((i * 2654435761) >> 7) & 1 for i in range(n)]
    return out


def ntt_closed_form(F, name, n, w):
    """best_fft(vectors(F, n, w)[name], w) in closed form, or None where there is none (sparse, selector)"""
    p, c = F.p, constant_c(F)
    at = lambda idx, v: [v % p if i == idx else 0 for i in range(n)]
    if name == "zero":
        return [0] * n
    if name in ("one", "pm1", "const"):
        return at(0, n * {"one": 1, "pm1": p - 1, "const": c}[name])
    if name == "alt":
        return at(n // 2, n * c) if n > 1 else [c]
    if name.startswith("freq"):
        return at(int(name[4:]) % n, n * c)
    if name.startswith("delta"):
        step, v, a = pow(w, int(name[5:]), p), c, []
        for _ in range(n):
            a.append(v)
            v = v * step % p
        return a
    return None


# ---- points and polynomials ------------------------------------------------------------------------------------------------------------------------------
def points(F, n):
    """name -> point: 0, 1, -1, 2, 1/2, primitive 8th and 2048th roots of unity, w_n and its inverse (w_n of order 2^log2_ceil(n))"""
    p = F.p
    wn = F.omega(log2_ceil(n))
    return {"0": 0, "1": 1, "-1": p - 1, "2": 2, "half": (p + 1) // 2, "w8": F.omega(3), "w2048": F.omega(11), "wn": wn, "wn_inv": pow(wn, -1, p)}


def horner(a, x, p):
    acc = 0
    for c in reversed(a):
        acc = (acc * x + c) % p
    return acc


def eval_closed_form(F, name, n, zname):
    """eval_polynomial(vectors(F, n)[name], points(F, n)[zname]) where a closed form exists, else None"""
    p, c = F.p, constant_c(F)
    first = {"zero": 0, "one": 1, "pm1": p - 1, "const": c, "alt": c, "sparse": c, "selector": 0}
    if zname == "0":
        if name in first:
            return first[name]
        if name.startswith("delta"):
            return c if name == "delta0" else 0
        return c                                              # every single-frequency input starts with c
    order = {"1": 1, "-1": 2, "w8": 8, "w2048": 2048, "wn": 1 << log2_ceil(n), "wn_inv": 1 << log2_ceil(n)}.get(zname)
    scale = {"zero": 0, "one": 1, "pm1": p - 1, "const": c}.get(name)
    if scale is not None and order is not None and n % order == 0:
        return scale * n % p if order == 1 else 0            # a geometric sum over whole periods of a root of unity
    return None


def kate_recurrence(a, z, p):
    """arithmetic::kate_division: q[i] = a[i + 1] + z q[i + 1], len(a) - 1 coefficients"""
    q, acc = [0] * (len(a) - 1), 0
    for i in range(len(a) - 1, 0, -1):
        acc = (a[i] + z * acc) % p
        q[i - 1] = acc
    return q


def mul_linear(b, z, p):
    """b(X) (X - z)"""
    out = [0] * (len(b) + 1)
    for i, c in enumerate(b):
        out[i] = (out[i] - z * c) % p
        out[i + 1] = (out[i + 1] + c) % p
    return out


def uniform_ints(po, F, n, seed):
    return po.scalars_uniform(F.of, n, po.Xoshiro(seed))


def kate_polys(po, F, n, z):
    """name -> coefficients, for the division by (X - z): monomial X^(n-1), all-ones, all-zero, all p-1, sparse, and (X - z) b for a uniform b"""
    v = vectors(F, n)
    out = {"monomial": [0] * (n - 1) + [1], "one": v["one"], "zero": v["zero"], "pm1": v["pm1"], "sparse": v["sparse"]}
    out["multiple"] = mul_linear(uniform_ints(po, F, n - 1, 7000 + n), z, F.p)
    return out


def kate_closed_form(po, F, name, n, z):
    """kate_division(kate_polys(po, F, n, z)[name], z) in closed form, or None"""
    p = F.p
    if name == "zero":
        return [0] * (n - 1)
    if name == "monomial":
        return [pow(z, n - 2 - i, p) for i in range(n - 1)]
    if name == "multiple":
        return uniform_ints(po, F, n - 1, 7000 + n)
    if z == 0 and name in ("one", "pm1", "sparse"):
        return kate_polys(po, F, n, z)[name][1:]             # a shift
    if name in ("one", "pm1"):
        s = 1 if name == "one" else p - 1
        if z == 1:
            return [s * (n - 1 - i) % p for i in range(n - 1)]
        if z == p - 1:
            return [s if (n - 1 - i) % 2 == 1 else 0 for i in range(n - 1)]      # 1 - 1 + 1 ...: an odd number of terms above i gives 1
    return None


# ---- inversion operands ------------------------------------------------------------------------------------------------------------------------------------
INTERNAL_SHIFT = 261         # a kernel's element is x * 2^261 mod p; the batch inversion hands that integer to f29_inv_safegcd


def divstep_starts(p):
    """the integers the divstep loop is to start from (and, taken as field elements themselves, a second operand list)"""
    vs = [1, 2, 3, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    vs += [1 << k for k in range(254)] + [(1 << k) - 1 for k in range(1, 254)]
    vs += [p - (1 << k) for k in (1, 29, 30, 60, 253)]
    vs.append((((p >> 240) - 1) << 240) | ((1 << 240) - 1))      # the largest value below p whose eight low 30-bit limbs are all ones
    seen, out = set(), []
    for v in vs:
        assert 0 < v < p
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def inversion_operands(F):
    """-> (xs whose internal form x * 2^261 mod p is each chosen V, the Vs themselves)"""
    vs = divstep_starts(F.p)
    back = pow(1 << INTERNAL_SHIFT, -1, F.p)
    return [v * back % F.p for v in vs], vs


def padded_with_zeros(xs, n):
    """xs with a zero after every third element, repeated from the start up to n elements"""
    out = []
    i = 0
    while len(out) < n:
        out.append(xs[i % len(xs)])
        i += 1
        if i % 3 == 0 and len(out) < n:
            out.append(0)
    return out


# ---- products, combinations ----------------------------------------------------------------------------------------------------------------------------------
def grand_product_ints(num, den, p):
    z, acc = [], 1
    for a, b in zip(num, den):
        z.append(acc)
        acc = acc * a % p * pow(b, -1, p) % p
    return z


def grand_product_cases(po, F, n):
    """name -> (num, den, closed form or None); the denominators are nonzero"""
    p = F.p
    u = uniform_ints(po, F, n, 8000 + n)
    assert all(u)
    zero_at = min(1500, n // 2)
    hit = list(u)
    hit[zero_at] = 0
    den2 = uniform_ints(po, F, n, 8100 + n)
    return {"num_eq_den": (u, u, [1] * n),
            "ones": ([1] * n, [1] * n, [1] * n),
            "pm1": ([p - 1] * n, [1] * n, [1 if i % 2 == 0 else p - 1 for i in range(n)]),
            "pm1_both": ([p - 1] * n, [p - 1] * n, [1] * n),
            "zero_in_num": (hit, den2, None)}, zero_at


def lincomb_ints(cols, coefs, sub0, p):
    out = [sum(c * col[i] for c, col in zip(coefs, cols)) % p for i in range(len(cols[0]))]
    if sub0 is not None:
        out[0] = (out[0] - sub0) % p
    return out


def scale_ints(a, pattern, p):
    return [v * pattern[i % len(pattern)] % p for i, v in enumerate(a)]
