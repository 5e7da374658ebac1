"""An independent restatement of the ChaCha20 generator kinds' draws (include/dehalo.h, dehalo_rng_kind) on plain Python integers: RFC 8439's block function
over the raw state words, the host's serial stream, the kernel's indexed draw, and a scalar source in the form the oracle prover reads.  It imports nothing from
the package or from oracle/ -- a modulus is passed in as an integer -- so that what it says is judged by the RFC's vectors alone (tests/test_rng_chacha.py)."""
import struct

import numpy as np

SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
M32 = 0xFFFFFFFF


def _rotl(x, n):
    return ((x << n) & M32) | (x >> (32 - n))


def _quarter(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 7)


def block(key: bytes, w12: int, w13: int, w14: int, w15: int) -> bytes:
    """The ChaCha20 block function (RFC 8439 2.3) over the state sigma | key | w12 w13 w14 w15 -> 64 bytes"""
    assert len(key) == 32
    st = list(SIGMA) + list(struct.unpack("<8I", key)) + [w12 & M32, w13 & M32, w14 & M32, w15 & M32]
    x = list(st)
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
    return struct.pack("<16I", *[(a + b) & M32 for a, b in zip(x, st)])


def _candidate(half_block: bytes, bits: int) -> int:
    """eight 32-bit words, least significant first, masked to `bits`"""
    return int.from_bytes(half_block, "little") & ((1 << bits) - 1)


def serial(key: bytes, field_p: int, bits: int, stream: int = 0):
    """The host's serial stream (stream 0): a generator of scalars.  Consecutive blocks, a 64-bit block counter in words 12-13 and the stream id in words
    14-15; every block is two candidates of eight words, and a candidate >= p is skipped -- with the half block it took."""
    counter = 0
    while True:
        b = block(key, counter, counter >> 32, stream, stream >> 32)
        counter += 1
        for half in (b[:32], b[32:]):
            v = _candidate(half, bits)
            if v < field_p:
                yield v


def indexed(key: bytes, stream: int, i: int, field_p: int, bits: int):
    """The kernel's draw of scalar i on `stream` -> (scalar, the attempt that produced it)"""
    attempt = 0
    while True:
        v = _candidate(block(key, i, ((i >> 32) & 0xFFFF) | (attempt << 16), stream, stream >> 32)[:32], bits)
        if v < field_p:
            return v, attempt
        attempt += 1


def limbs(values) -> np.ndarray:
    """integers -> (len, 4) u64, least significant word first"""
    return np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for v in values], dtype=np.uint64).reshape(-1, 4)


class ReferenceRng:
    """.scalars(count) -> (count, 4) u64, what a proof over 2^k = n rows draws under `key`, in upstream's order: every draw from the serial stream, except a
    draw of exactly n scalars -- the j-th of those (j = 0: the random polynomial, or a stand-alone opening's s_poly; j = 1: s_poly inside an IPA proof) is the
    indexed draw of stream j + 1 from index 0 and takes nothing from the serial stream.  No other draw of a proof has n scalars (blinding rows: n - usable;
    grand products: blinding_factors).  field_p: the modulus; the values are raw representations, as the library hands them over."""

    def __init__(self, key: bytes, field_p: int, n: int):
        self.key, self.p, self.bits, self.n = bytes(key), field_p, field_p.bit_length(), n
        self.stream = serial(self.key, self.p, self.bits)
        self.large = 0            # n-scalar draws so far
        self.attempts = []        # of every indexed scalar, in order

    def scalars(self, count: int) -> np.ndarray:
        if count == self.n:
            self.large += 1
            assert self.large <= 2, "a proof has at most two n-scalar draws"
            drawn = [indexed(self.key, self.large, i, self.p, self.bits) for i in range(count)]
            self.attempts += [a for _, a in drawn]
            return limbs([v for v, _ in drawn])
        return limbs([next(self.stream) for _ in range(count)])
