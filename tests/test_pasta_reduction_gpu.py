"""GPU: the subtractive Montgomery reduction of the Pasta primes (csrc/fp29.cuh) where it runs -- the 9 x 29-bit multiplier behind field_op "mul29", the
bucket accumulation of an MSM over a registered table, the NTT butterflies -- on structured operands: zeros (the one case whose internal value differs
from the additive reduction's, by + p), single reduction multipliers 0 / 2^29 - 1, internal forms with zero low limbs, scalars with 0, 1, -1, all-equal
and alternating-sign digits.  Truth: Python integers, and the C restatement of best_multiexp / best_fft.  Bit-exact."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import fp29_model as M

pytestmark = pytest.mark.gpu

R = 1 << M.RBITS


def structured_values(f, rnd):
    """integers x whose internal form x * 2^261 mod p is structured: edge values, zero low limbs, and pairs solved so that one multiplier m_k is 0 or all ones"""
    p = f.p
    F = M.F29(f)
    rinv = pow(R, -1, p)
    a = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (1 << 255) % p, rinv, (p - 1) * rinv % p]
    a += [(t << (29 * k)) * rinv % p for k in range(1, 9) for t in (1, 3, (1 << 21) - 1) if (t << (29 * k)) < p]       # internal form t * 2^(29 k)
    a += [(((1 << 29) - 1) << (29 * k)) * rinv % p for k in range(8)]                                                     # one all-ones limb
    b = list(reversed(a))
    for k in range(8):                       # (m_8 needs a free top limb: covered by the model test, not by canonical values)
        for target in (0, M.MASK):
            while True:
                x = [rnd.randrange(M.MASK + 1) | (i == 0) for i in range(8)] + [rnd.randrange(1 << 21)]
                y = [rnd.randrange(M.MASK + 1) for i in range(8)] + [rnd.randrange(1 << 21)]
                y[k] = 0
                F.mont(x, y)
                y[k] = (target - F.m_seen[k]) * pow(x[0], -1, 1 << M.B) % (1 << M.B)
                if M.value(x) < p and M.value(y) < p:
                    break
            a.append(M.value(x) * rinv % p)
            b.append(M.value(y) * rinv % p)
    return a, b


@pytest.mark.parametrize("fname", ["pasta_fp", "pasta_fq"])
def test_mul29_structured_and_random(pkg, po, ctx, fname):
    f = po.FIELDS[fname]
    spec = pkg.fields.FIELDS[fname]
    p = f.p
    rnd = random.Random(77 + spec.id)
    a, b = structured_values(f, rnd)
    a += [0] * 4 + [rnd.randrange(p) for _ in range(4096)]
    b += [0, 1, p - 1, rnd.randrange(p)] + [rnd.randrange(p) for _ in range(4096)]
    ea, eb = spec.encode_many(a), spec.encode_many(b)
    assert spec.decode_many(ctx.field_op(spec.id, "mul29", ea, eb)) == [x * y % p for x, y in zip(a, b)]
    assert spec.decode_many(ctx.field_op(spec.id, "mul29", ea, ea)) == [x * x % p for x in a]
    assert spec.decode_many(ctx.field_op(spec.id, "mul29", eb, eb)) == [y * y % p for y in b]


def test_mul29_bn254_fr_untouched_path(pkg, po, ctx):
    f = po.FIELDS["bn254_fr"]
    spec = pkg.fields.FIELDS["bn254_fr"]
    p = f.p
    rnd = random.Random(78)
    a = [0, 1, p - 1, (p - 1) // 2, pow(R, -1, p)] + [rnd.randrange(p) for _ in range(1024)]
    b = list(reversed(a))
    ea, eb = spec.encode_many(a), spec.encode_many(b)
    assert spec.decode_many(ctx.field_op(spec.id, "mul29", ea, eb)) == [x * y % p for x, y in zip(a, b)]
    assert spec.decode_many(ctx.field_op(spec.id, "mul29", ea, ea)) == [x * x % p for x in a]


def alternating_digit_scalars(r):
    """sum_i (-1)^i d 2^(c i): signed window digits +d, -d, +d, ... for every window width the MSM may choose, the top digit positive"""
    out = []
    for c in range(4, 18):
        for d in (1, (1 << (c - 1)) - 1):
            terms = (253 // c - 1) | 1                     # odd: the top digit is +d; c * terms <= 253 bits
            s = sum((-1) ** i * d << (c * i) for i in range(terms))
            assert 0 < s < r
            out.append(s)
    return out


@pytest.mark.parametrize("cname", ["pallas", "vesta"])
@pytest.mark.parametrize("log_n", [10, 12])
def test_msm_structured_scalars(pkg, co, ctx, cname, log_n):
    spec = pkg.fields.CURVES[cname]
    r = spec.scalar.p
    n = 1 << log_n
    bases = co.synth_bases(spec.id, n)
    mixed = co.fill_scalars(spec.scalar.id, "uniform", n, 3100 + log_n)
    special = [0, 1, r - 1, 0, 1, r - 1, 2, r - 2] + alternating_digit_scalars(r)
    mixed[8:8 + len(special)] = spec.scalar.encode_many(special)
    mixed[n - len(special):] = spec.scalar.encode_many(special)
    cases = {"mixed": mixed}
    for name, v in (("all_zero", 0), ("all_one", 1), ("all_minus_one", r - 1), ("all_equal", alternating_digit_scalars(r)[5])):
        cases[name] = np.repeat(spec.scalar.encode_many([v]), n, axis=0)
    h = ctx.register_bases(spec.id, bases, 0, True)
    try:
        for name, scalars in cases.items():
            got = ctx.to_affine(spec.id, ctx.msm(h, scalars))[0]
            want = co.to_affine(spec.id, co.best_multiexp(spec.id, scalars, bases, 4))
            assert np.array_equal(got, want), (cname, log_n, name)
    finally:
        h.release()


@pytest.mark.parametrize("log_n", [11, 12])
def test_ntt_pasta_fp_zero_delta_random(pkg, po, co, ctx, log_n):
    """2^11: one pass; 2^12: two.  An all-zero input makes every butterfly product p instead of 0."""
    spec = pkg.fields.FIELDS["pasta_fp"]
    f = po.FIELDS["pasta_fp"]
    n = 1 << log_n
    omega = spec.encode(f.omega(log_n))
    zero = spec.encode_many([0] * n)
    delta0, delta_mid = zero.copy(), zero.copy()
    delta0[0] = spec.encode(1)
    delta_mid[n // 2 + 3] = spec.encode(f.p - 1)
    for name, a in (("zero", zero), ("delta0", delta0), ("delta_mid", delta_mid), ("random", co.fill_scalars(spec.id, "uniform", n, 4200 + log_n))):
        got = pkg.best_fft(ctx, spec, a, omega, log_n)
        assert np.array_equal(got, co.best_fft(spec.id, a, omega, log_n, 4)), (log_n, name)
    assert not pkg.best_fft(ctx, spec, zero, omega, log_n).any()
