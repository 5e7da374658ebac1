"""The judge of the generated points (include/dehalo.h, "Generated points"; dehalo_points_generate_device, dehalo_params_ipa_generate): the rule restated
on plain Python integers over chacha_reference.block, with a square root of its own.  It imports nothing from the package or from oracle/ -- the curves'
constants are written out below -- so that what the device computes is compared with the rule, not with itself.

    point(curve, key, stream, index) -> (x, y, attempt)      curve: "bn254" | "pallas" | "vesta"; key: 32 bytes or None (the default key)

Not covered anywhere: an index that uses up its 256 attempts.  Under a real key that has probability (3/4)^256 (Pasta), no key that reaches it is known, and
the library has no hook to force it."""
from chacha_reference import block

DEFAULT_KEY = b"dehalo ParamsIPA generators v1" + bytes(2)
MAX_ATTEMPTS = 256

# base-field modulus p and the b of y^2 = x^3 + b; `id` is the library's dehalo_curve
CURVES = {
    "bn254": {"id": 0, "p": 21888242871839275222246405745257275088696311157297823662689037894645226208583, "b": 3},
    "pallas": {"id": 1, "p": 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001, "b": 5},
    "vesta": {"id": 2, "p": 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001, "b": 5},
}

ACCEPTED, X_ZERO, X_NOT_BELOW_P, NOT_A_NONZERO_SQUARE = "accepted", "x = 0", "x >= p", "x^3 + b is not a non-zero square"


def sqrt_mod(a: int, p: int):
    """a square root of a modulo the odd prime p, or None for a non-residue (Tonelli-Shanks); sqrt(0) = 0"""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    s, t = 0, p - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, tt, r = s, pow(z, t, p), pow(a, t, p), pow(a, (t + 1) // 2, p)
    while tt != 1:
        i, t2 = 0, tt
        while t2 != 1:
            t2, i = t2 * t2 % p, i + 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, tt, r = i, b * b % p, tt * b * b % p, r * b % p
    assert r * r % p == a
    return r


def candidate(key: bytes, stream: int, index: int, attempt: int) -> bytes:
    """the 32 candidate bytes of one attempt: the first half of the block over sigma | key | index mod 2^32 | (index >> 32 & 0xffff) | attempt << 16 | stream"""
    assert 0 <= index < 1 << 48 and 0 <= attempt < 1 << 16
    return block(key, index & 0xFFFFFFFF, ((index >> 32) & 0xFFFF) | (attempt << 16), stream & 0xFFFFFFFF, stream >> 32)[:32]


def judge(curve: str, enc: bytes):
    """one candidate -> (verdict, x, s, y): y is the root with parity s when the verdict is ACCEPTED, else None"""
    c = CURVES[curve]
    p = c["p"]
    v = int.from_bytes(enc, "little")
    x, s = v & ((1 << 255) - 1), v >> 255
    if x == 0:
        return X_ZERO, x, s, None
    if x >= p:
        return X_NOT_BELOW_P, x, s, None
    y = sqrt_mod((x * x * x + c["b"]) % p, p)
    if y is None or y == 0:
        return NOT_A_NONZERO_SQUARE, x, s, None
    return ACCEPTED, x, s, (y if y & 1 == s else p - y)


def attempts(curve: str, key, stream: int, index: int):
    """every attempt of one index up to and including the accepted one: [(candidate bytes, verdict, x, s, y)]"""
    key = DEFAULT_KEY if key is None else bytes(key)
    out = []
    for attempt in range(MAX_ATTEMPTS):
        enc = candidate(key, stream, index, attempt)
        out.append((enc,) + judge(curve, enc))
        if out[-1][1] == ACCEPTED:
            return out
    raise AssertionError("no point in %d attempts" % MAX_ATTEMPTS)


def point(curve: str, key, stream: int, index: int):
    """-> (x, y, attempt): the point named (curve, key, stream, index), canonical integers, and the attempt that produced it"""
    tries = attempts(curve, key, stream, index)
    _, _, x, _, y = tries[-1]
    return x, y, len(tries) - 1


def params_ipa(curve: str, key, k: int):
    """-> (g, w, u): g[i] = (stream 0, index i), i < 2^k; W = (stream 1, index 0); U = (stream 1, index 1); points as (x, y)"""
    g = [point(curve, key, 0, i)[:2] for i in range(1 << k)]
    return g, point(curve, key, 1, 0)[:2], point(curve, key, 1, 1)[:2]
