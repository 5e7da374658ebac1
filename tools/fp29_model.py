#!/usr/bin/env python3
"""Bit-accurate Python model of csrc/fp29.cuh: 9 x 29-bit limb, carry-free, lazily reduced
Montgomery arithmetic (R' = 2^261) and the XYZZ formulas built on it.

Every u32 limb and u64 accumulator is range-asserted, so running the group formulas on random
and adversarial inputs proves the absence of overflow for the bounds the kernels rely on, and
the results are checked against oracle/pyoracle.py.  Also emits the per-field constants
(csrc/fp29_constants.h).  Dev-time tool; not part of the product path.

    python tools/fp29_model.py            # self-test
    python tools/fp29_model.py --emit     # write csrc/fp29_constants.h
"""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import pyoracle as po

B = 29
L = 9
MASK = (1 << B) - 1
RBITS = B * L  # 261
U32 = 1 << 32
U64 = 1 << 64
I63 = 1 << 63


def limbs(x):
    assert 0 <= x < (1 << RBITS)
    return [(x >> (B * i)) & MASK for i in range(L)]


def value(l):
    return sum(v << (B * i) for i, v in enumerate(l))


class F29:
    def __init__(self, f: po.Field):
        self.f = f
        self.p = f.p
        self.P = limbs(f.p)
        self.INV = (-pow(f.p, -1, 1 << B)) % (1 << B)
        self.subtractive = self.INV == MASK           # p = 1 mod 2^29 (Pasta): the product-scanning schedule subtracts m p (sub_columns)
        assert not self.subtractive or self.P[0] == 1
        self.col_min = self.col_max = 0                # extremes of the signed column accumulator seen so far
        self.R = (1 << RBITS) % f.p            # Montgomery one
        self.R2 = pow(1 << RBITS, 2, f.p)
        # converts: standard form (x * 2^256) <-> internal (x * 2^261)
        self.TO29 = (1 << (RBITS + (RBITS - 256))) % f.p      # mont(m, TO29) = m * 2^5
        self.FROM29 = (1 << 256) % f.p                          # mont(x, FROM29) = x * 2^-5
        # subtraction constants: multiples of p whose limb representation dominates the subtrahend
        # (value bounds, in units of p, are the fixpoint of the XYZZ formulas: see DESIGN.md)
        self.KM = self.sub_const(3.0, 29)    # subtrahend: a product (normalized limbs, value < 3 p)
        self.KA = self.sub_const(9.5, 29)    # subtrahend: a stored coordinate (normalized limbs, value < 9.5 p)
        self.KB = self.sub_const(4.5, 31)    # subtrahend: PPP + 2Q (limbs < 3 * 2^29, value < 4.5 p)
        self.KN = self.sub_const(1.0, 29)    # negation of a canonical value (< p)
        # subtrahend: a caller's 256-bit word, or the sum of two (the NTT's butterflies without a multiplication: normalized limbs, value < 2^257)
        self.KW = self.sub_const(None, 29, vmax=(1 << 257) - 1)

    def sub_const(self, vbound, s, vmax=None):
        """limbs K'_i of a multiple K of p such that K'_i >= (max subtrahend limb_i) for i < 8 and
        K'_8 >= (max subtrahend top limb); offsets 2^s borrowed from the next limb.  The subtrahend's value is below vbound p, or at most vmax."""
        top_need = ((int(vbound * self.p) if vmax is None else vmax) >> (B * 8)) + 1
        borrow = 1 << (s - B)
        k = 1
        while True:
            K = k * self.p
            kl = limbs(K) if K < (1 << RBITS) else None
            if kl is not None and kl[8] - borrow >= top_need:
                break
            k += 1
        out = [kl[0] + (1 << s)] + [kl[i] + (1 << s) - borrow for i in range(1, 8)] + [kl[8] - borrow]
        assert value(out) == K and all(0 <= v < U32 for v in out)
        return out, K

    # ---- primitives (mirroring the HIP code) ----
    def sub_columns(self, prod):
        """The subtractive product-scanning reduction of f29_montgomery_columns / columns2 / f29_mul_pair for p = 1 mod 2^29: prod[k] is the list of the
        products of column k in issue order.  ONE signed 64-bit accumulator; m_k = acc & MASK, the carry is the arithmetic shift, the later columns get
        -m_i P[k - i]; m_8 is biased by -2^29 and keeps its multiply-add by -P[0] = -1.  Asserts every intermediate accumulator in [-2^63, 2^63), every emitted
        limb in [0, 2^29) and the top limb non-negative."""
        assert self.subtractive
        NP = [-x for x in self.P]
        m, out, acc = [0] * L, [], 0

        def step(term):
            nonlocal acc
            acc += term
            assert -I63 <= acc < I63, "signed column overflow"
            self.col_min, self.col_max = min(self.col_min, acc), max(self.col_max, acc)

        for k in range(2 * L - 1):
            for t in prod[k]:
                assert 0 <= t < U64
                step(t)                                   # v_mad_u64_u32
            for i in range(L):
                if i < k and k - i < L and self.P[k - i] != 0:
                    assert -(1 << 31) <= m[i] < (1 << 31) and -(1 << 31) <= NP[k - i] < (1 << 31)
                    step(m[i] * NP[k - i])                # v_mad_i64_i32
            if k < L - 1:
                m[k] = acc & MASK
            elif k == L - 1:
                m[k] = (acc & MASK) - (1 << B)           # (u32)acc | ~MASK as an int32
                step(m[k] * NP[0])
                assert acc & MASK == 0
            else:
                out.append(acc & MASK)
            acc >>= B                                     # arithmetic shift (floor), the low limb is m_k or the emitted limb
        assert 0 <= acc < (1 << B), "top limb negative or result exceeds 2^261"
        out.append(acc)
        self.m_seen = m
        return out

    def os_sub(self, a, b=None):
        """The subtractive rows of the operand-scanning schedule (f29_mul_os, or f29_sqr_os for b = None: all products first): 18 signed accumulators, each a
        partial sum of one column in the order the HIP code adds to it -- products of the rows so far, minus the reduction terms so far, plus the carry."""
        assert self.subtractive
        acc = [0] * (2 * L)

        def add(k, term):
            acc[k] += term
            assert -I63 <= acc[k] < I63, "signed column overflow"
            self.col_min, self.col_max = min(self.col_min, acc[k]), max(self.col_max, acc[k])

        def reduce_row(i):
            m = (acc[i] & MASK) - ((1 << B) if i == L - 1 else 0)
            for j in range(L):
                if self.P[j] != 0 and (j > 0 or i == L - 1):
                    add(i + j, -m * self.P[j])
            if i == L - 1:
                assert acc[i] & MASK == 0
            add(i + 1, acc[i] >> B)

        if b is None:
            for i in range(L):
                add(2 * i, a[i] * a[i])
                for j in range(i + 1, L):
                    add(i + j, 2 * a[i] * a[j])
            for i in range(L):
                reduce_row(i)
        else:
            for i in range(L):
                for j in range(L):
                    add(i + j, a[i] * b[j])
                reduce_row(i)
        out, c = [], 0
        for j in range(L - 1):
            t = acc[L + j] + c
            assert -I63 <= t < I63
            out.append(t & MASK)
            c = t >> B
        assert 0 <= acc[2 * L - 1] + c < (1 << B), "top limb negative or result exceeds 2^261"
        return out + [acc[2 * L - 1] + c]

    def sub_check(self, out_add, out_sub, T):
        """the subtractive form against the additive one: identical limbs unless T = 0 mod 2^261, then exactly + p"""
        if T % (1 << RBITS) != 0:
            assert out_sub == out_add, "subtractive reduction differs from the additive one"
        else:
            assert value(out_sub) == value(out_add) + self.p and all(0 <= v <= MASK for v in out_sub[:8])
        assert value(out_sub) * (1 << RBITS) % self.p == T % self.p and value(out_sub) <= T // (1 << RBITS) + self.p
        return out_sub

    def mont(self, a, b, sub=True):
        """a * b * 2^-261 mod p, not fully reduced.  Result limbs normalized (< 2^29), value < a*b/2^261 + p.  The additive columns (every field's operand
        scanning, BN254's product scanning); for the Pasta primes also the subtractive columns of the product-scanning schedule, whose result is returned
        (sub=False: a call site that keeps the additive form)."""
        out = self.mont_additive(a, b)
        if sub and self.subtractive:
            prod = [[a[i] * b[k - i] for i in range(L) if 0 <= k - i < L] for k in range(2 * L - 1)]
            res = self.sub_check(out, self.sub_columns(prod), value(a) * value(b))
            assert self.os_sub(a, b) == res            # the operand-scanning schedule (f29_lat<F>): same limbs
            return res
        return out

    def mont_additive(self, a, b):
        assert len(a) == L and len(b) == L
        assert all(0 <= x < U32 for x in a) and all(0 <= x < U32 for x in b)
        acc = [0] * (2 * L)
        for i in range(L):
            for j in range(L):
                acc[i + j] += a[i] * b[j]
                assert acc[i + j] < U64, "product column overflow"
            m = ((acc[i] & 0xFFFFFFFF) * self.INV) & MASK
            for j in range(L):
                acc[i + j] += m * self.P[j]
                assert acc[i + j] < U64, "reduction column overflow"
            assert acc[i] & MASK == 0
            acc[i + 1] += acc[i] >> B
            assert acc[i + 1] < U64
        out = []
        carry = 0
        for j in range(L):
            v = acc[L + j] + carry
            assert v < U64
            if j < L - 1:
                out.append(v & MASK)
                carry = v >> B
            else:
                assert v < (1 << B), "result exceeds 2^261"
                out.append(v)
        return out

    def mont2(self, a, b, c, d):
        """(a * b + c * d) * 2^-261 mod p with ONE reduction (f29_mul2): both products go into the same columns."""
        for x in (a, b, c, d):
            assert len(x) == L and all(0 <= v < U32 for v in x)
        acc = [0] * (2 * L)
        for i in range(L):
            for j in range(L):
                acc[i + j] += a[i] * b[j] + c[i] * d[j]
        # column totals including every reduction term and carry must fit 64 bits (product scanning keeps ONE accumulator per column)
        carry = 0
        m = [0] * L
        tot = list(acc)
        out = []
        for k in range(2 * L - 1):
            col = tot[k] + carry
            for i in range(L):
                if i < k and k - i < L and i < L:
                    col += m[i] * self.P[k - i] if i < L and k - i >= 1 else 0
            if k < L:
                m[k] = ((col & 0xFFFFFFFF) * self.INV) & MASK
                col += m[k] * self.P[0]
                assert col & MASK == 0
            assert col < U64, "fused column overflow"
            if k >= L:
                out.append(col & MASK)
            carry = col >> B
        assert carry < (1 << B), "result exceeds 2^261"
        out.append(carry)
        want = (value(a) * value(b) + value(c) * value(d)) * pow(1 << RBITS, -1, self.p) % self.p
        assert value(out) % self.p == want
        assert value(out) < (value(a) * value(b) + value(c) * value(d)) // (1 << RBITS) + self.p + 1
        return out

    def sqr(self, a, sub=True):
        """a^2 * 2^-261 with cross products taken once against the doubled operand (f29_sqr); sub as in mont."""
        out = self.sqr_additive(a)
        if sub and self.subtractive:
            d = [2 * x for x in a]
            prod = [[d[i] * a[k - i] for i in range(L) if i < k - i < L] + ([a[k // 2] * a[k // 2]] if k % 2 == 0 else []) for k in range(2 * L - 1)]
            res = self.sub_check(out, self.sub_columns(prod), value(a) * value(a))
            assert self.os_sub(a) == res
            return res
        return out

    def mont_pair(self, a, b, c, d):
        """f29_mul_pair: two multiplications in lockstep -- the columns of each are mont's"""
        return self.mont(a, b), self.mont(c, d)

    def sqr_pair(self, a, c):
        """f29_sqr_pair (f29_montgomery_columns2): the columns of each are sqr's"""
        return self.sqr(a), self.sqr(c)

    def sqr_additive(self, a):
        assert all(0 <= x < U32 for x in a)
        d = [2 * x for x in a]
        assert all(x < U32 for x in d)
        acc = [0] * (2 * L)
        for i in range(L):
            acc[2 * i] += a[i] * a[i]
            assert acc[2 * i] < U64
            for j in range(i + 1, L):
                acc[i + j] += d[i] * a[j]
                assert acc[i + j] < U64, "square column overflow"
        for i in range(L):
            m = ((acc[i] & 0xFFFFFFFF) * self.INV) & MASK
            for j in range(L):
                acc[i + j] += m * self.P[j]
                assert acc[i + j] < U64, "reduction column overflow"
            assert acc[i] & MASK == 0
            acc[i + 1] += acc[i] >> B
            assert acc[i + 1] < U64
        out, carry = [], 0
        for j in range(L):
            v = acc[L + j] + carry
            if j < L - 1:
                out.append(v & MASK)
                carry = v >> B
            else:
                assert v < (1 << B)
                out.append(v)
        assert out == self.mont_additive(a, a)
        return out

    def norm(self, a):
        assert all(x + 8 < U32 for x in a), "normalize: u32 limb + carry overflow"
        out, carry = [], 0
        for j in range(L):
            v = a[j] + carry
            assert v < U64
            if j < L - 1:
                out.append(v & MASK)
                carry = v >> B
            else:
                assert v < (1 << B), "normalize: value exceeds 2^261"
                out.append(v)
        return out

    def add(self, a, b):
        out = [x + y for x, y in zip(a, b)]
        assert all(v < U32 for v in out)
        return out

    def dbl(self, a):
        return self.add(a, a)

    def sub(self, a, b, kc):
        K, _ = kc
        out = []
        for x, y, k in zip(a, b, K):
            assert k >= y, "subtraction constant does not dominate the subtrahend limb"
            v = x + k - y
            assert v < U32
            out.append(v)
        return out

    def bfly(self, u, v, w, mul, kc):
        """bfly29 of csrc/ntt.cuh: t = v w (or v itself, normalized, where the twiddle is one); -> (u + t, u - t + K)"""
        t = self.mont(v, w) if mul else self.norm(v)
        return self.add(u, t), self.sub(u, t, kc)

    def ntt_first_round(self, e, w1, kc):
        """the first radix-4 round of k_ntt_pass on four loaded words e (limbs of plain 256-bit integers): stage 0 without a multiplication, stage 1 with the
        twiddles 1 and w1; kc: the constant of the butterflies that do not multiply.  -> the four values as stored (normalized)"""
        e0, e1, e2, e3 = e
        e0, e1 = self.bfly(e0, e1, None, False, kc)
        e2, e3 = self.bfly(e2, e3, None, False, kc)
        e0, e2 = self.bfly(e0, e2, None, False, kc)
        e1, e3 = self.bfly(e1, e3, w1, True, self.KM)
        return [self.norm(x) for x in (e0, e1, e2, e3)]

    def canon(self, a):
        """fully reduced value in [0, p), normalized limbs"""
        v = value(self.norm(a)) % self.p
        return limbs(v)

    def is_zero_mod_p(self, a_norm, max_mult):
        v = value(a_norm)
        assert v < (max_mult + 1) * self.p, "zero-test candidate set too small"
        return any(v == k * self.p for k in range(max_mult + 1))

    # ---- the quotient kernels' lazily reduced helpers (csrc/evalh.cuh) ----
    def cond_sub(self, a, c):
        """f29_cond_sub: v >= c ? v - c : v on normalized limbs, with its 32-bit signed borrow chain"""
        assert all(0 <= x <= MASK for x in a[:8]) and 0 <= a[8] < (1 << 31), "cond_sub: limbs not normalized"
        cl = limbs(c)
        d, borrow = [], 0
        for i in range(8):
            t = a[i] - cl[i] + borrow
            assert -(1 << 31) <= t < (1 << 31)
            d.append(t & MASK)
            borrow = t >> 31
        top = a[8] - cl[8] + borrow
        assert -(1 << 31) <= top < (1 << 31)
        out = d + [top] if top >= 0 else list(a)
        assert value(out) == (value(a) - c if value(a) >= c else value(a))
        return out

    def evh_add(self, a, b):
        return self.cond_sub(self.norm(self.add(a, b)), 2 * self.p)

    def evh_sub(self, a, b):
        t = self.norm(self.sub(a, b, self.KM))
        return self.cond_sub(self.cond_sub(t, 4 * self.p), 2 * self.p)

    def evh_neg(self, a):
        return self.cond_sub(self.norm(self.sub([0] * L, a, self.KM)), 2 * self.p)

    def evh_bounds(self, rnd):
        """The stored-value invariant of evalh.cuh is <= 2p, with 2p itself produced by evh_neg(0) alone: every helper and every consumer on the representatives
        0, p and 2p of zero, on the largest values below them and on random values <= 2p -- all stay <= 2p (the products and evh_sub strictly below), and the two
        stores come out canonical."""
        p = self.p
        assert self.KM[1] == 4 * p
        edge = [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p]
        vals = edge + [rnd.randrange(2 * p + 1) for _ in range(40)]
        assert value(self.evh_neg(limbs(0))) == 2 * p
        for x in vals:
            a = limbs(x)
            n = value(self.evh_neg(a))
            assert n % p == -x % p and n <= 2 * p and (n < 2 * p or x == 0)
            assert value(self.canon(a)) == x % p and value(self.cond_sub(self.cond_sub(self.cond_sub(self.cond_sub(a, 8 * p), 4 * p), 2 * p), p)) == x % p       # f29_canon
            t = self.mont(a, limbs(self.FROM29))                                                 # f29_to_std
            assert value(t) < 2 * p and value(self.cond_sub(t, p)) == x * pow(1 << (RBITS - 256), -1, p) % p
            assert value(self.sqr(a)) < 2 * p
            for y in vals:
                b = limbs(y)
                s, d, m = value(self.evh_add(a, b)), value(self.evh_sub(a, b)), value(self.mont(a, b))
                assert s % p == (x + y) % p and s <= 2 * p and (s < 2 * p or x == y == 2 * p)
                assert d % p == (x - y) % p and d < 2 * p
                assert m < 2 * p
                assert value(self.mont2(a, b, b, a)) < 2 * p
        # k_shuffle_h_batch: v = v y + l0 (1 - z); v = v y + l_last (z^2 - z); v = v y + l_active (z(wX) sv - z iv) -- every operand a stored value <= 2p, every
        # result the next term's v: z, z(wX) over the representatives of zero and their neighbours, the two side values over all pairs of them
        one = limbs((1 << RBITS) % p)
        inv = pow(1 << RBITS, -1, p)
        for z_ in edge:
            for zn_ in edge:
                for iv_ in edge:
                    for sv_ in (edge[(edge.index(iv_) + 3) % len(edge)], iv_):
                        v_, y_, l_ = (vals[(z_ + zn_ + iv_ + sv_ + i) % len(vals)] for i in range(3))
                        z, zn, iv, sv, v, y, l = (limbs(t) for t in (z_, zn_, iv_, sv_, v_, y_, l_))
                        t1, t2 = self.evh_sub(one, z), self.evh_sub(self.sqr(z), z)
                        lhs, rhs = self.mont(zn, sv), self.mont(z, iv)
                        t3 = self.evh_sub(lhs, rhs)
                        assert max(value(t) for t in (t1, t2, lhs, rhs, t3)) < 2 * p
                        assert value(t3) % p == (zn_ * sv_ - z_ * iv_) * inv % p and value(t2) % p == (z_ * z_ * inv - z_) % p
                        for t in (t1, t2, t3):
                            v = self.mont2(v, y, t, l)
                            assert value(v) < 2 * p
                        assert value(self.canon(v)) < p

    # ---- codecs ----
    def enc(self, x):       # integer -> internal Montgomery limbs (canonical)
        return limbs(x * (1 << RBITS) % self.p)

    def dec(self, l):
        return value(l) * pow(1 << RBITS, -1, self.p) % self.p

    def from_std(self, m256):   # standard-form packed value (x * 2^256 mod p) -> internal
        return self.mont(limbs(m256), limbs(self.TO29))

    def to_std(self, l):        # internal -> standard-form canonical integer
        return value(self.canon(self.mont(self.norm(l), limbs(self.FROM29))))


class XYZZ29:
    """Group formulas exactly as csrc/ec29.cuh evaluates them (value bounds tracked as maxima)."""

    def __init__(self, curve: po.Curve):
        self.c = curve
        self.F = F29(curve.base)
        self.maxv = {}

    def track(self, name, l):
        v = value(l)
        self.maxv[name] = max(self.maxv.get(name, 0), v)

    def identity(self):
        z = [0] * L
        return (z, z, z, z)

    def from_affine(self, P):
        F = self.F
        if P is None:
            return self.identity()
        one = limbs(F.R)
        return (F.enc(P[0]), F.enc(P[1]), one, one)

    def to_affine(self, A):
        F = self.F
        zz = F.dec(A[2])
        if zz == 0:
            return None
        p = F.p
        return (F.dec(A[0]) * pow(zz, -1, p) % p, F.dec(A[1]) * pow(F.dec(A[3]), -1, p) % p)

    def madd(self, A, q, neg=False):
        """A + q (q affine canonical internal limbs, or None)."""
        F = self.F
        if q is None:
            return A
        X1, Y1, ZZ1, ZZZ1 = A
        x2, y2 = q
        if neg:
            y2 = F.sub([0] * L, y2, F.KN)          # p' - y, loose
        U2 = F.mont(x2, ZZ1)
        S2 = F.mont(y2, ZZZ1)
        P = F.norm(F.sub(U2, X1, F.KA))
        Rr = F.norm(F.sub(S2, Y1, F.KA))
        PP = F.sqr(P)
        PPP = F.mont(P, PP)
        Q = F.mont(X1, PP)
        RR = F.sqr(Rr)
        X3 = F.norm(F.sub(RR, F.add(PPP, F.dbl(Q)), F.KB))
        T = F.sub(Q, X3, F.KA)
        NY = F.norm(F.sub([0] * L, Y1, F.KA))           # -Y1 + 10p
        Y3 = F.mont2(Rr, T, NY, PPP)                     # R (Q - X3) - Y1 PPP, one reduction
        ZZ3 = F.mont(ZZ1, PP)
        ZZZ3 = F.mont(ZZZ1, PPP)
        for n, v in (("P", P), ("X3", X3), ("Y3", Y3), ("ZZ3", ZZ3), ("ZZZ3", ZZZ3), ("T", T), ("PPP", PPP)):
            self.track(n, v)
        if F.is_zero_mod_p(ZZ3, 1):
            # slow path: decide exactly
            a_id = value(F.canon(ZZ1)) == 0
            if a_id:
                one = limbs(F.R)
                return (x2, F.canon(y2), one, one)
            if value(F.canon(Rr)) == 0:
                return self.dbl_affine((x2, F.canon(y2)))
            return self.identity()
        return (X3, Y3, ZZ3, ZZZ3)

    def dbl_affine(self, q):
        one = limbs(self.F.R)
        return self.dbl((q[0], q[1], one, one))

    def dbl(self, A):
        F = self.F
        X1, Y1, ZZ1, ZZZ1 = A
        U = F.dbl(Y1)                       # limbs < 2^30
        V = F.sqr(U, sub=False)             # additive columns: see call_site_bounds
        W = F.mont(U, V)
        S = F.mont(X1, V)
        XX = F.sqr(X1)
        M = F.norm(F.add(F.dbl(XX), XX))
        MM = F.sqr(M)
        X3 = F.norm(F.sub(MM, F.dbl(S), F.KB))
        T = F.sub(S, X3, F.KA)
        Y3 = F.norm(F.sub(F.mont(M, T), F.mont(W, Y1), F.KM))
        ZZ3 = F.mont(V, ZZ1)
        ZZZ3 = F.mont(W, ZZZ1)
        for n, v in (("dX3", X3), ("dY3", Y3), ("dZZ3", ZZ3)):
            self.track(n, v)
        return (X3, Y3, ZZ3, ZZZ3)

    def add(self, A, Bp):
        F = self.F
        X1, Y1, ZZ1, ZZZ1 = A
        X2, Y2, ZZ2, ZZZ2 = Bp
        U1 = F.mont(X1, ZZ2)
        U2 = F.mont(X2, ZZ1)
        S1 = F.mont(Y1, ZZZ2)
        S2 = F.mont(Y2, ZZZ1)
        P = F.norm(F.sub(U2, U1, F.KM))
        Rr = F.norm(F.sub(S2, S1, F.KM))
        PP = F.sqr(P)
        PPP = F.mont(P, PP)
        Q = F.mont(U1, PP)
        RR = F.sqr(Rr)
        X3 = F.norm(F.sub(RR, F.add(PPP, F.dbl(Q)), F.KB))
        T = F.sub(Q, X3, F.KA)
        Y3 = F.norm(F.sub(F.mont(Rr, T), F.mont(S1, PPP), F.KM))
        ZZ3 = F.mont(F.mont(ZZ1, ZZ2), PP)
        ZZZ3 = F.mont(F.mont(ZZZ1, ZZZ2), PPP)
        for n, v in (("aX3", X3), ("aY3", Y3), ("aZZ3", ZZ3)):
            self.track(n, v)
        if F.is_zero_mod_p(ZZ3, 1):
            if value(F.canon(ZZ1)) == 0:
                return Bp
            if value(F.canon(ZZ2)) == 0:
                return A
            if value(F.canon(Rr)) == 0:
                return self.dbl(A)
            return self.identity()
        return (X3, Y3, ZZ3, ZZZ3)


def call_site_operands(F):
    """The largest operands each class of call site of the product-scanning multiplications admits (csrc/ec29.cuh, ntt.cuh, poly.cuh, evalh.cuh), as
    (name, kind, operands, fits): limbs at their bound, the top limb from the value bound.  fits says whether the subtractive columns (< 2^63) hold them;
    the call sites that do not fit keep the additive columns in the HIP code (SUB = false)."""
    p = F.p
    top = lambda mult: (int(mult * p) >> (B * 8)) + 1
    norm = lambda mult: [MASK] * 8 + [top(mult)]                       # normalized limbs, value < mult p
    loose = lambda K, mult: [MASK + K[0][i] for i in range(8)] + [top(mult)]      # x - y + K, un-normalized: x normalized, y = 0
    two = lambda mult: [2 * MASK] * 8 + [top(mult)]                    # a sum of two normalized values / a doubled one
    return [
        ("normalized x normalized (poly, evalh, conversions, zero tests)", "mul", (norm(16), norm(3)), True),
        ("add_mixed: x2 ZZ1, (p' - y2) ZZZ1", "pair", (norm(1), norm(1.1), list(F.KN[0]), norm(1.1)), True),
        ("add_mixed: P^2, R^2 (P, R = product - coordinate + KA, normalized)", "sqr_pair", (norm(F.KA[1] // p + 3), norm(F.KA[1] // p + 3)), True),
        ("add_mixed: P PP, X1 PP; ZZ1 PP, ZZZ1 PPP", "pair", (norm(F.KA[1] // p + 3), norm(3), norm(9.5), norm(3)), True),
        ("add / double: R T, M T with T = Q - X3 + KA un-normalized", "mul", (norm(F.KA[1] // p + 3), loose(F.KA, F.KA[1] // p + 3)), True),
        ("double: U V with U = 2 Y1", "mul", (two(19), norm(3)), True),
        ("double: U^2 with U = 2 Y1 (4 cross products of 2^31 * 2^30 in column 7)", "sqr", (two(19),), False),
        ("double_quad: U U as a multiplication (8 products of 2^30 * 2^30 in column 7)", "mul", (two(19), two(19)), False),
        ("NTT butterfly, second stage of a round: v = u - t + KM un-normalized, canonical twiddle", "mul", (loose(F.KM, 30), norm(1)), True),
        ("Horner step: (acc x + c) x, acc x + c a sum of two normalized values", "mul", (two(3), norm(2)), True),
    ]


def call_site_bounds(F, rnd):
    """every call-site class on its largest operands and on random ones under them: the subtractive columns stay signed 64-bit where the HIP code uses
    them; a refused class either overflows or comes closer to 2^63 than 2^35 (one carry): no margin to rely on"""
    refused = []
    for name, kind, ops, fits in call_site_operands(F):
        run = {"mul": lambda o: F.mont(*o), "sqr": lambda o: F.sqr(*o), "pair": lambda o: F.mont_pair(*o), "sqr_pair": lambda o: F.sqr_pair(*o)}[kind]
        F.col_min = F.col_max = 0
        try:
            run(ops)
            ok = F.col_max < I63 - (1 << 35)
        except AssertionError as e:
            assert "signed column overflow" in str(e), (name, e)
            ok = False
        assert ok == fits, (name, ok, F.col_max.bit_length())
        if not ok:
            refused.append(name)
            continue
        for _ in range(40):
            run(tuple([rnd.randrange(v + 1) for v in o] for o in ops))
        assert -I63 <= F.col_min and F.col_max < I63
    return refused


def self_test():
    rnd = random.Random(1)
    for fname in ("pasta_fp", "pasta_fq", "bn254_fq", "bn254_fr"):
        F = F29(po.FIELDS[fname])
        p = F.p
        # mont on canonical and on maximally loose inputs
        for _ in range(300):
            a, b = rnd.randrange(p), rnd.randrange(p)
            assert F.dec(F.mont(F.enc(a), F.enc(b))) == a * b % p
        worst_a = [(1 << 31) + (1 << 30) - 1] * 8 + [(1 << 26)]     # loose-31 limbs, ~2^258
        worst_b = [MASK] * 8 + [1 << 26]
        F.mont_additive(worst_a, worst_b)          # the additive columns' contract (60 bits); the subtractive ones': call_site_bounds
        loose30 = [(1 << 30) - 1] * 8 + [1 << 27]
        F.mont_additive(loose30, loose30)
        if F.subtractive:
            refused = call_site_bounds(F, rnd)
            print(fname, "subtractive columns: refused call sites (additive in the HIP code):", refused)
        # conversions
        for _ in range(50):
            x = rnd.randrange(p)
            std = x * (1 << 256) % p
            assert F.dec(F.from_std(std)) == x
            assert F.to_std(F.enc(x)) == std
        F.evh_bounds(random.Random(2))
        print(fname, "mont ok; KM mult", F.KM[1] // p, "KA mult", F.KA[1] // p, "KB mult", F.KB[1] // p, "KN mult", F.KN[1] // p, "INV", hex(F.INV), "P limbs", [hex(v) for v in F.P])
    for cname in ("pallas", "vesta", "bn254"):
        c = po.CURVES[cname]
        G = XYZZ29(c)
        F = G.F
        pts = po.synth_bases(c, 40)
        enc = lambda P: None if P is None else (F.enc(P[0]), F.enc(P[1]))
        # long random accumulation chains incl. negations, duplicates, identities, cancellations
        for trial in range(6):
            acc = G.identity()
            ref = None
            seq = [rnd.choice(pts) for _ in range(120)]
            seq[5] = seq[4]            # P + P  (doubling branch)
            seq[10] = None             # identity point
            for i, P in enumerate(seq):
                neg = rnd.random() < 0.3
                acc = G.madd(acc, enc(P), neg)
                ref = po.ec_add(c, ref, po.ec_neg(c, P) if neg else P)
                if i % 17 == 0:
                    assert G.to_affine(acc) == ref
            assert G.to_affine(acc) == ref
            # cancel: acc + (-acc_affine) = identity, then continue
            a_aff = G.to_affine(acc)
            acc2 = G.madd(acc, enc(a_aff), True)
            assert G.to_affine(acc2) is None
            acc2 = G.madd(acc2, enc(pts[3]), False)
            assert G.to_affine(acc2) == pts[3]
            # full adds and doublings
            other = G.identity()
            oref = None
            for P in seq[:30]:
                other = G.madd(other, enc(P))
                oref = po.ec_add(c, oref, P)
            s = G.add(acc, other)
            assert G.to_affine(s) == po.ec_add(c, ref, oref)
            assert G.to_affine(G.add(acc, acc)) == po.ec_add(c, ref, ref)
            assert G.to_affine(G.add(acc, G.identity())) == ref
            assert G.to_affine(G.add(G.identity(), acc)) == ref
            d = acc
            dref = ref
            for _ in range(20):
                d = G.dbl(d)
                dref = po.ec_add(c, dref, dref)
            assert G.to_affine(d) == dref
            assert G.to_affine(G.dbl(G.identity())) is None
        print(cname, "xyzz ok; max value / p:", {k: round(v / c.base.p, 2) for k, v in sorted(G.maxv.items())})


def emit():
    out = ["// GENERATED by tools/fp29_model.py --emit -- do not edit.",
           "// 9 x 29-bit limb constants (R' = 2^261) for csrc/fp29.cuh.", "#pragma once", "#include <stdint.h>", ""]
    names = {"bn254_fr": "Bn254Fr", "bn254_fq": "Bn254Fq", "pasta_fp": "PastaFp", "pasta_fq": "PastaFq"}
    w = lambda l: ", ".join("0x%08xu" % v for v in l)
    for fname, sn in names.items():
        F = F29(po.FIELDS[fname])
        out += ["struct %s29 {" % sn,
                "  typedef %s Std;" % sn,
                "  static constexpr uint32_t INV = 0x%08xu;          // -p^-1 mod 2^29" % F.INV,
                "  static constexpr uint32_t P[9] = {%s};" % w(F.P),
                "  static constexpr uint32_t ONE[9] = {%s};   // 2^261 mod p" % w(limbs(F.R)),
                "  static constexpr uint32_t TO29[9] = {%s};  // mont(std, TO29) = std * 2^5" % w(limbs(F.TO29)),
                "  static constexpr uint32_t FROM29[9] = {%s}; // mont(x, FROM29) = x * 2^-5" % w(limbs(F.FROM29)),
                "  static constexpr uint32_t KM[9] = {%s};  // %d p, dominates normalized limbs of a value < 3 p" % (w(F.KM[0]), F.KM[1] // F.p),
                "  static constexpr uint32_t KA[9] = {%s};  // %d p, dominates normalized limbs of a value < 9.5 p" % (w(F.KA[0]), F.KA[1] // F.p),
                "  static constexpr uint32_t KB[9] = {%s};  // %d p, dominates limbs < 3 * 2^29" % (w(F.KB[0]), F.KB[1] // F.p),
                "  static constexpr uint32_t KN[9] = {%s};  // %d p, negation of a canonical value" % (w(F.KN[0]), F.KN[1] // F.p),
                "  static constexpr uint32_t KW[9] = {%s};  // %d p, dominates normalized limbs of a value < 2^257 (one or two 256-bit words of a caller)" % (w(F.KW[0]), F.KW[1] // F.p),
                "  static constexpr uint32_t P2[9] = {%s};  // 2p" % w(limbs(2 * F.p)),
                "  static constexpr uint32_t P4[9] = {%s};  // 4p" % w(limbs(4 * F.p)),
                "  static constexpr uint32_t P8[9] = {%s};  // 8p" % w(limbs(8 * F.p)),
                "  static constexpr uint32_t R3[9] = {%s};  // 2^783 mod p: mont(v, R3) = v * 2^522 (integer inverse -> internal form)" % w(limbs(pow(2, 783, F.p))),
                "  static constexpr uint32_t PINV30 = 0x%08xu;       // p^-1 mod 2^30 (safegcd inversion, 30-bit signed limbs)" % pow(F.p, -1, 1 << 30),
                "};", ""]
    out += ["template <class F> struct f29_of;"]
    for fname, sn in names.items():
        out += ["template <> struct f29_of<%s> { typedef %s29 type; };" % (sn, sn)]
    out += [""]
    path = os.path.join(HERE, "..", "delay-encryption-in-halo2_amd", "csrc", "fp29_constants.h")
    open(path, "w").write("\n".join(out))
    print("wrote", os.path.normpath(path))


if __name__ == "__main__":
    if "--emit" in sys.argv:
        emit()
    else:
        self_test()
