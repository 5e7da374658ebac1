"""The whole call through the C ABI: ParamsKZG, keygen, ProvingKey / VerifyingKey, Blake2bWrite and `create_proof` as ONE
library call each (include/dehalo.h, "the whole call"; csrc/params.hip, keygen.hip, prover.hip) -- the objects and the call of the reference's benches
(benches/delay_enc.rs:41-54 params, :84-115 keys, :120-134 create_proof into a Blake2bWrite transcript).  Python is a caller
here: it serialises the ConstraintSystem into the C descriptor and passes pointers; phases, transcript hashing and every
launch run in C++.  (tests/fine_grained_prover.py -- test infrastructure -- drives the same proof from Python through the fine-grained entry points.)"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import plonk
from ._lib import (CCheckFailure, CCheckReport, CCircuitInputs, CColumnQuery, CConstraintSystem, CExprNode, CRng, CSynthesisInfo, Context, DehaloError, FixedBase, PairingTable, RNG_FILL_FN, load_library)
from .fields import CurveSpec, FieldSpec

EXPR_KIND = {"const": 0, plonk.FIXED: 1, plonk.ADVICE: 2, plonk.INSTANCE: 3, "neg": 4, "sum": 5, "product": 6, "scaled": 7, "challenge": 8}
COLUMN_KIND = {plonk.ADVICE: 0, plonk.FIXED: 1, plonk.INSTANCE: 2}
RNG_OS, RNG_PCG64, RNG_CALLBACK, RNG_CHACHA20 = 0, 1, 2, 3
KEYGEN_FIXED_CANONICAL = 1
PROOF_ADVICE_ON_DEVICE, PROOF_ADVICE_CANONICAL = 1, 2
CIRCUIT_DELAY_ENC, CIRCUIT_MOD_POW, CIRCUIT_POSE_ENC = 0, 1, 2
SERDE_FORMATS = {"processed": 0, "raw": 1, "raw-unchecked": 2}      # dehalo_serde_format
KEEP_K = 0xFFFFFFFF                                                # DEHALO_KEEP_K
CHECK_GATE, CHECK_LOOKUP, CHECK_COPY, CHECK_SHUFFLE = 0, 1, 2, 3
PHASES = ("advice", "lookups", "products", "random", "quotient", "evaluations", "openings", "total")


def _instance_words(f, v) -> np.ndarray:
    """one instance column as (len, 4) u64 Montgomery words: a list of ints is encoded (canonical words); a (len, 4) uint64 array is taken as the words
    themselves, as a C caller would hand them over -- any 256-bit word, standing for its residue (dehalo.h "Non-canonical words")"""
    if isinstance(v, np.ndarray) and v.dtype == np.uint64 and v.ndim == 2 and v.shape[1] == 4:
        return np.ascontiguousarray(v)
    return f.encode_many(list(v)) if len(v) else np.zeros((0, 4), dtype=np.uint64)


class ConstraintSystemDescriptor:
    """dehalo_constraint_system built from a plonk.ConstraintSystem; owns the arrays the C struct points into."""

    def __init__(self, cs: plonk.ConstraintSystem, field: FieldSpec):
        nodes: List[tuple] = []
        consts: List[int] = []
        memo: Dict[tuple, int] = {}

        def const(c: int) -> int:
            c %= field.p
            if c not in consts:
                consts.append(c)
            return consts.index(c)

        def emit(e) -> int:
            if e in memo:
                return memo[e]
            k = e[0]
            if k == "const":
                node = (0, const(e[1]), 0, 0)
            elif k in (plonk.FIXED, plonk.ADVICE, plonk.INSTANCE):
                node = (EXPR_KIND[k], e[1], 0, e[2])
            elif k == "neg":
                node = (4, emit(e[1]), 0, 0)
            elif k in ("sum", "product"):
                a = emit(e[1])
                node = (EXPR_KIND[k], a, emit(e[2]), 0)
            elif k == "scaled":
                node = (7, emit(e[1]), const(e[2]), 0)
            elif k == "challenge":
                node = (8, e[1], 0, 0)
            else:
                raise ValueError("unknown expression node %r" % (k,))
            nodes.append(node)
            memo[e] = len(nodes) - 1
            return memo[e]

        gates = [emit(g) for g in cs.gates]
        lens, lin, ltab = [], [], []
        for inputs, tables in cs.lookups:
            if len(inputs) != len(tables):
                raise ValueError("lookup: input and table expression counts differ")
            lens.append(len(inputs))
            lin += [emit(e) for e in inputs]
            ltab += [emit(e) for e in tables]
        slens, sin, stab = [], [], []
        for inputs, sides in cs.shuffles:
            if len(inputs) != len(sides):
                raise ValueError("shuffle: input and shuffle expression counts differ")
            slens.append(len(inputs))
            sin += [emit(e) for e in inputs]
            stab += [emit(e) for e in sides]
        self._nodes = (CExprNode * max(1, len(nodes)))(*[CExprNode(*nd) for nd in nodes])
        self._consts = field.encode_many(consts) if consts else np.zeros((1, 4), dtype=np.uint64)
        u32 = lambda xs: (C.c_uint32 * max(1, len(xs)))(*xs)
        self._gates, self._lens, self._lin, self._ltab = u32(gates), u32(lens), u32(lin), u32(ltab)
        self._perm = (CColumnQuery * max(1, len(cs.permutation_columns)))(*[CColumnQuery(COLUMN_KIND[k], i, 0) for k, i in cs.permutation_columns])
        mk = lambda lst, kind: (CColumnQuery * max(1, len(lst)))(*[CColumnQuery(COLUMN_KIND[kind], c, r) for c, r in lst])
        self._aq, self._fq, self._iq = mk(cs.advice_queries, plonk.ADVICE), mk(cs.fixed_queries, plonk.FIXED), mk(cs.instance_queries, plonk.INSTANCE)
        d = CConstraintSystem()
        d.num_advice, d.num_fixed, d.num_instance, d.minimum_degree = cs.num_advice, cs.num_fixed, cs.num_instance, cs.minimum_degree
        d.nodes, d.num_nodes = self._nodes, len(nodes)
        d.constants, d.num_constants = self._consts.ctypes.data, len(consts)
        d.gates, d.num_gates = self._gates, len(gates)
        d.lookup_lens, d.num_lookups, d.lookup_inputs, d.lookup_tables = self._lens, len(lens), self._lin, self._ltab
        d.permutation_columns, d.num_permutation_columns = self._perm, len(cs.permutation_columns)
        d.advice_queries, d.num_advice_queries = self._aq, len(cs.advice_queries)
        d.fixed_queries, d.num_fixed_queries = self._fq, len(cs.fixed_queries)
        d.instance_queries, d.num_instance_queries = self._iq, len(cs.instance_queries)
        # the Challenge API: NULL / 0 for a circuit without later phases and challenges -- the descriptor of before
        self._aph = np.asarray(cs.phases(), dtype=np.uint8) if any(cs.phases()) else None
        self._cph = np.asarray(cs.challenge_phases, dtype=np.uint8) if cs.challenge_phases else None
        d.advice_phases = self._aph.ctypes.data if self._aph is not None else None
        d.challenge_phases, d.num_challenges = self._cph.ctypes.data if self._cph is not None else None, len(cs.challenge_phases)
        # shuffle arguments: NULL / 0 for a circuit without one -- the descriptor of before
        if slens:
            self._slens, self._sin, self._stab = u32(slens), u32(sin), u32(stab)
            d.shuffle_lens, d.shuffle_inputs, d.shuffle_tables, d.num_shuffles = self._slens, self._sin, self._stab, len(slens)
        self.struct = d

    def ref(self):
        return C.byref(self.struct)


def _check(ctx: Context, rc: int):
    if rc != 0:
        raise DehaloError(rc, load_library().dehalo_last_error(ctx.handle).decode())


def _serde(format: str) -> int:
    if format not in SERDE_FORMATS:
        raise ValueError("unknown format %r" % (format,))
    return SERDE_FORMATS[format]


def _bytes_ptr(b):
    return C.cast(C.c_char_p(bytes(b)), C.c_void_p)


class ParamsKZG:
    """dehalo_params: ParamsKZG<Bn256> resident on the device."""

    def __init__(self, ctx: Context, curve: CurveSpec, handle):
        self.ctx, self.curve, self.handle = ctx, curve, handle

    @classmethod
    def create(cls, ctx: Context, curve: CurveSpec, k: int, g, g_lagrange, g2: bytes = b"", s_g2: bytes = b"") -> "ParamsKZG":
        g = np.ascontiguousarray(g, dtype=np.uint64).reshape(-1, 8)
        gl = np.ascontiguousarray(g_lagrange, dtype=np.uint64).reshape(-1, 8)
        if g.shape[0] != 1 << k or gl.shape[0] != 1 << k:
            raise ValueError("g and g_lagrange must hold 2^k points")
        h = C.c_void_p()
        b2, bs = bytes(g2).ljust(128, b"\0"), bytes(s_g2).ljust(128, b"\0")
        _check(ctx, load_library().dehalo_params_create(ctx.handle, curve.id, k, g.ctypes.data, gl.ctypes.data, _bytes_ptr(b2), _bytes_ptr(bs), C.byref(h)))
        return cls(ctx, curve, h)

    @classmethod
    def setup(cls, ctx: Context, curve: CurveSpec, k: int, s: Optional[int] = None) -> "ParamsKZG":
        """ParamsKZG::setup(k, rng) (benches/delay_enc.rs:43): the SRS for the secret `s` (a field element; None = drawn from OS entropy, as the reference's OsRng
        does), generated on the device -- dehalo_params_setup."""
        if s is None:
            import secrets
            s = secrets.randbelow(curve.scalar.p - 2) + 2
        h = C.c_void_p()
        sm = curve.scalar.encode(s % curve.scalar.p)
        _check(ctx, load_library().dehalo_params_setup(ctx.handle, curve.id, k, sm.ctypes.data, C.byref(h)))
        return cls(ctx, curve, h)

    @classmethod
    def from_g(cls, ctx: Context, curve: CurveSpec, k: int, g, g2: bytes = b"", s_g2: bytes = b"") -> "ParamsKZG":
        """ParamsKZG from g, g2 and s_g2 alone: g_lagrange = g_to_lagrange(g), a group FFT on the device (dehalo_params_from_g)."""
        g = np.ascontiguousarray(g, dtype=np.uint64).reshape(-1, 8)
        if g.shape[0] != 1 << k:
            raise ValueError("g must hold 2^k points")
        h = C.c_void_p()
        b2, bs = bytes(g2).ljust(128, b"\0"), bytes(s_g2).ljust(128, b"\0")
        _check(ctx, load_library().dehalo_params_from_g(ctx.handle, curve.id, k, g.ctypes.data, _bytes_ptr(b2), _bytes_ptr(bs), C.byref(h)))
        return cls(ctx, curve, h)

    @classmethod
    def read(cls, ctx: Context, curve: CurveSpec, data: bytes, format: str = "raw-unchecked", downsize: Optional[int] = None) -> "ParamsKZG":
        """ParamsKZG::read_custom: `format` one of SERDE_FORMATS ("processed": compressed points, decompressed on the device; "raw": Montgomery limbs, every point
        checked; "raw-unchecked": the same bytes copied in unseen).  downsize = k': read + downsize(k') in one step -- only g[0 .. 2^k') is taken from the file,
        g_lagrange is the group FFT of it (dehalo_params_read_custom).  The defaults are dehalo_params_read."""
        h = C.c_void_p()
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        lib = load_library()
        if format == "raw-unchecked" and downsize is None:
            _check(ctx, lib.dehalo_params_read(ctx.handle, curve.id, buf.ctypes.data if buf.size else None, buf.size, C.byref(h)))
        else:
            _check(ctx, lib.dehalo_params_read_custom(ctx.handle, curve.id, buf.ctypes.data if buf.size else None, buf.size, SERDE_FORMATS[format],
                                                      KEEP_K if downsize is None else downsize, C.byref(h)))
        return cls(ctx, curve, h)

    def write(self, format: str = "raw-unchecked") -> bytes:
        """ParamsKZG::write_custom (dehalo_params_write_custom); the default is dehalo_params_write, whose bytes both raw formats are."""
        lib = load_library()
        if format == "raw-unchecked":
            out = np.empty(lib.dehalo_params_size(self.handle), dtype=np.uint8)
            _check(self.ctx, lib.dehalo_params_write(self.handle, out.ctypes.data, out.size))
        else:
            out = np.empty(lib.dehalo_params_size_custom(self.handle, SERDE_FORMATS[format]), dtype=np.uint8)
            _check(self.ctx, lib.dehalo_params_write_custom(self.handle, SERDE_FORMATS[format], out.ctypes.data, out.size))
        return out.tobytes()

    def downsize(self, k: int):
        """Params::downsize(k) as a new object of the same scheme: the first 2^k of g, g_lagrange by the group FFT on the device (dehalo_params_downsize).  This
        object stays as it is and is released on its own."""
        h = C.c_void_p()
        _check(self.ctx, load_library().dehalo_params_downsize(self.ctx.handle, self.handle, k, C.byref(h)))
        return type(self)(self.ctx, self.curve, h)

    def release(self):
        if self.handle is not None:
            load_library().dehalo_params_release(self.ctx.handle, self.handle)
            self.handle = None


class ParamsIPA(ParamsKZG):
    """dehalo_params over IPACommitmentScheme<C> (Pallas / Vesta): g, g_lagrange, w, u handed over as the caller's ParamsIPA holds them
    (dehalo_params_ipa_create), built from g, w, u alone (from_g), read from ParamsIPA::write's bytes (read) or derived with nothing handed over (generate).  ProvingKey.keygen and Prover take it as they take ParamsKZG: Prover(params, pk).create_proof then writes a ProverIPA
    proof (blinded commitments, committed instance columns, the multiopen and the opening argument).  `open` opens one polynomial."""

    @classmethod
    def create(cls, ctx: Context, curve: CurveSpec, k: int, g, g_lagrange, w, u) -> "ParamsIPA":
        g = np.ascontiguousarray(g, dtype=np.uint64).reshape(-1, 8)
        gl = np.ascontiguousarray(g_lagrange, dtype=np.uint64).reshape(-1, 8)
        w = np.ascontiguousarray(w, dtype=np.uint64).reshape(8)
        u = np.ascontiguousarray(u, dtype=np.uint64).reshape(8)
        if g.shape[0] != 1 << k or gl.shape[0] != 1 << k:
            raise ValueError("g and g_lagrange must hold 2^k points")
        h = C.c_void_p()
        _check(ctx, load_library().dehalo_params_ipa_create(ctx.handle, curve.id, k, g.ctypes.data, gl.ctypes.data, w.ctypes.data, u.ctypes.data, C.byref(h)))
        return cls(ctx, curve, h)

    @classmethod
    def from_g(cls, ctx: Context, curve: CurveSpec, k: int, g, w, u) -> "ParamsIPA":
        """ParamsIPA from g alone, as upstream builds it: g_lagrange = g_to_lagrange(g), a group FFT on the device (dehalo_params_ipa_from_g)."""
        g = np.ascontiguousarray(g, dtype=np.uint64).reshape(-1, 8)
        w = np.ascontiguousarray(w, dtype=np.uint64).reshape(8)
        u = np.ascontiguousarray(u, dtype=np.uint64).reshape(8)
        if g.shape[0] != 1 << k:
            raise ValueError("g must hold 2^k points")
        h = C.c_void_p()
        _check(ctx, load_library().dehalo_params_ipa_from_g(ctx.handle, curve.id, k, g.ctypes.data, w.ctypes.data, u.ctypes.data, C.byref(h)))
        return cls(ctx, curve, h)

    @classmethod
    def generate(cls, ctx: Context, curve: CurveSpec, k: int, key: Optional[bytes] = None) -> "ParamsIPA":
        """ParamsIPA at any k without a file: g, W, U derived on the device by the library's public rule (include/dehalo.h, "Generated points": ChaCha20 under
        `key`, 32 bytes, None = the default key; try-and-increment onto the curve), g_lagrange by the group FFT (dehalo_params_ipa_generate).  Not upstream's
        generators: an upstream verifier takes them from write()'s bytes through ParamsIPA::read."""
        if key is not None and len(key) != 32:
            raise ValueError("key must be 32 bytes")
        h = C.c_void_p()
        _check(ctx, load_library().dehalo_params_ipa_generate(ctx.handle, curve.id, k, _bytes_ptr(bytes(key)) if key is not None else None, C.byref(h)))
        return cls(ctx, curve, h)

    @classmethod
    def setup(cls, *a, **kw):
        raise NotImplementedError("ParamsIPA::new (hash-to-curve generators) is not provided: pass g, w, u to ParamsIPA.from_g, or g, g_lagrange, w, u to ParamsIPA.create")

    @classmethod
    def read(cls, ctx: Context, curve: CurveSpec, data: bytes) -> "ParamsIPA":
        """ParamsIPA::read: k | g | g_lagrange | w | u with 32-byte compressed points, decompressed on the device (dehalo_params_ipa_read)."""
        h = C.c_void_p()
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        _check(ctx, load_library().dehalo_params_ipa_read(ctx.handle, curve.id, buf.ctypes.data if buf.size else None, buf.size, C.byref(h)))
        return cls(ctx, curve, h)

    def write(self) -> bytes:
        """ParamsIPA::write (dehalo_params_ipa_write)."""
        lib = load_library()
        out = np.empty(lib.dehalo_params_ipa_size(self.handle), dtype=np.uint8)
        _check(self.ctx, lib.dehalo_params_ipa_write(self.handle, out.ctypes.data, out.size))
        return out.tobytes()

    @property
    def fixed_base(self) -> FixedBase:
        """W's window table (dehalo_params_fixed_base): what every commit / commit_lagrange adds [blind] W from.  It belongs to the params and goes with them."""
        return FixedBase(self.ctx, C.c_void_p(load_library().dehalo_params_fixed_base(self.handle)), self.curve.id, owned=False)

    def open(self, d_poly: int, blind: int, x3: int, transcript: Optional["Blake2bWrite"] = None, rng=None) -> "Blake2bWrite":
        """commitment::create_proof of the 2^k coefficients at d_poly (device, Montgomery) with blind `blind` at x3 (dehalo_ipa_open)."""
        t = transcript if transcript is not None else Blake2bWrite(self.curve)
        r = rng_struct(rng)
        f = self.curve.scalar
        b, x = f.encode(blind % f.p), f.encode(x3 % f.p)
        _check(self.ctx, load_library().dehalo_ipa_open(self.ctx.handle, self.handle, d_poly, b.ctypes.data, x.ctypes.data, C.byref(r) if r is not None else None, t.handle))
        rng_writeback(rng, r)
        return t


class CheckReport:
    """dehalo_check_report and the stored failures of one ProvingKey.check_witness: `failures` = tuples (kind, index, row) in (kind, index, row) order -- kind
    CHECK_GATE: index into cs.gates' polynomials; CHECK_LOOKUP: index into cs.lookups; CHECK_COPY: index into cs.permutation_columns; CHECK_SHUFFLE:
    index into cs.shuffles -- at most `cap` of them; the counters are exact whatever `cap` was."""

    def __init__(self, rep: CCheckReport, failures):
        self.failures = failures
        self.gate_failures, self.lookup_failures, self.copy_failures = int(rep.gate_failures), int(rep.lookup_failures), int(rep.copy_failures)
        self.rows, self.lookup_inputs, self.cells_in_cycles = int(rep.rows), int(rep.lookup_inputs), int(rep.cells_in_cycles)
        self.written = int(rep.written)
        self.shuffle_failures, self.shuffle_inputs = int(rep.shuffle_failures), int(rep.shuffle_inputs)

    @property
    def ok(self) -> bool:
        return self.gate_failures == 0 and self.lookup_failures == 0 and self.copy_failures == 0 and self.shuffle_failures == 0

    def __repr__(self):
        return "CheckReport(ok=%s, gate_failures=%d, lookup_failures=%d, copy_failures=%d, rows=%d, lookup_inputs=%d, cells_in_cycles=%d, failures=%r)" % (
            self.ok, self.gate_failures, self.lookup_failures, self.copy_failures, self.rows, self.lookup_inputs, self.cells_in_cycles, self.failures)


class ProvingKey:
    """dehalo_pk: ProvingKey (with its VerifyingKey and compiled programs) resident on the device."""

    def __init__(self, ctx: Context, curve: CurveSpec, cs: plonk.ConstraintSystem, handle):
        self.ctx, self.curve, self.cs, self.handle = ctx, curve, cs, handle

    @classmethod
    def keygen(cls, ctx: Context, params: ParamsKZG, cs: plonk.ConstraintSystem, fixed_canonical, assembly: plonk.Assembly, selectors: Sequence = ()) -> "ProvingKey":
        """keygen_vk + keygen_pk (benches/delay_enc.rs:86,103): fixed_canonical = (num_fixed, n, 4) u64 canonical values."""
        f = params.curve.scalar
        desc = ConstraintSystemDescriptor(cs, f)
        fixed = np.ascontiguousarray(fixed_canonical, dtype=np.uint64)
        mapping = np.ascontiguousarray(assembly.mapping, dtype=np.uint64)
        sels = [np.ascontiguousarray(np.asarray(s, dtype=np.uint8)) for s in selectors]
        sel_ptrs = (C.c_void_p * max(1, len(sels)))(*[s.ctypes.data for s in sels])
        h = C.c_void_p()
        _check(ctx, load_library().dehalo_keygen(ctx.handle, params.handle, desc.ref(), fixed.ctypes.data, mapping.ctypes.data, sel_ptrs, len(sels), KEYGEN_FIXED_CANONICAL,
                                                 C.byref(h)))
        return cls(ctx, params.curve, cs, h)

    @classmethod
    def keygen_pk(cls, ctx: Context, params: ParamsKZG, cs: plonk.ConstraintSystem, vk_bytes: bytes, fixed_canonical, assembly: plonk.Assembly, num_selectors: int = 0,
                  format: str = "raw-unchecked") -> "ProvingKey":
        """VerifyingKey::read + keygen_pk(params, vk, circuit) (benches/delay_enc.rs:96-103): the proving key of the columns UNDER the verifying key `vk_bytes` (in
        `format`, one of SERDE_FORMATS) -- its commitments are taken, not recomputed and not compared with the columns; no MSM runs (dehalo_keygen_pk)."""
        f = params.curve.scalar
        desc = ConstraintSystemDescriptor(cs, f)
        fixed = np.ascontiguousarray(fixed_canonical, dtype=np.uint64)
        mapping = np.ascontiguousarray(assembly.mapping, dtype=np.uint64)
        buf = np.frombuffer(bytes(vk_bytes), dtype=np.uint8)
        h = C.c_void_p()
        _check(ctx, load_library().dehalo_keygen_pk(ctx.handle, params.handle, desc.ref(), buf.ctypes.data if buf.size else None, buf.size, _serde(format), num_selectors,
                                                    fixed.ctypes.data, mapping.ctypes.data, KEYGEN_FIXED_CANONICAL, C.byref(h)))
        return cls(ctx, params.curve, cs, h)

    @classmethod
    def read(cls, ctx: Context, curve: CurveSpec, cs: plonk.ConstraintSystem, data: bytes, num_selectors: int = 0, format: str = "raw-unchecked") -> "ProvingKey":
        """ProvingKey::read(.., SerdeFormat): `format` one of SERDE_FORMATS ("processed": compressed commitments and canonical elements, decompressed / converted on the
        device; "raw": Montgomery limbs, every point and every element checked; "raw-unchecked": the same bytes copied in unseen).  The default is dehalo_pk_read."""
        desc = ConstraintSystemDescriptor(cs, curve.scalar)
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        h = C.c_void_p()
        lib = load_library()
        if format == "raw-unchecked":
            _check(ctx, lib.dehalo_pk_read(ctx.handle, curve.id, desc.ref(), buf.ctypes.data if buf.size else None, buf.size, num_selectors, C.byref(h)))
        else:
            _check(ctx, lib.dehalo_pk_read_custom(ctx.handle, curve.id, desc.ref(), buf.ctypes.data if buf.size else None, buf.size, _serde(format), num_selectors, C.byref(h)))
        return cls(ctx, curve, cs, h)

    def write(self, format: str = "raw-unchecked") -> bytes:
        """ProvingKey::write(.., SerdeFormat) (dehalo_pk_write_custom); the default is dehalo_pk_write, whose bytes both raw formats are."""
        lib = load_library()
        if format == "raw-unchecked":
            out = np.empty(lib.dehalo_pk_size(self.handle), dtype=np.uint8)
            _check(self.ctx, lib.dehalo_pk_write(self.ctx.handle, self.handle, out.ctypes.data, out.size))
        else:
            out = np.empty(lib.dehalo_pk_size_custom(self.handle, _serde(format)), dtype=np.uint8)
            _check(self.ctx, lib.dehalo_pk_write_custom(self.ctx.handle, self.handle, _serde(format), out.ctypes.data, out.size))
        return out.tobytes()

    def vk_bytes(self, format: str = "raw-unchecked") -> bytes:
        """VerifyingKey::write(.., SerdeFormat) (dehalo_vk_write_custom); the default is dehalo_vk_write, whose bytes both raw formats are."""
        lib = load_library()
        if format == "raw-unchecked":
            out = np.empty(lib.dehalo_vk_size(self.handle), dtype=np.uint8)
            _check(self.ctx, lib.dehalo_vk_write(self.handle, out.ctypes.data, out.size))
        else:
            out = np.empty(lib.dehalo_vk_size_custom(self.handle, _serde(format)), dtype=np.uint8)
            _check(self.ctx, lib.dehalo_vk_write_custom(self.ctx.handle, self.handle, _serde(format), out.ctypes.data, out.size))
        return out.tobytes()

    @property
    def transcript_repr(self) -> int:
        out = np.zeros(4, dtype=np.uint64)
        _check(self.ctx, load_library().dehalo_pk_get_transcript_repr(self.handle, out.ctypes.data))
        return self.curve.scalar.decode(out)

    @transcript_repr.setter
    def transcript_repr(self, value: int):
        _check(self.ctx, load_library().dehalo_pk_set_transcript_repr(self.handle, self.curve.scalar.encode(value).ctypes.data))

    def check_witness(self, advice, instances: Sequence[Sequence[int]] = ((),), assembly=None, canonical: bool = False, cap: int = 64, ctx: Optional[Context] = None,
                      challenges: Optional[Sequence[int]] = None) -> CheckReport:
        """dehalo_check_witness -- MockProver::verify on the device: which gate polynomials, lookup inputs and copy constraints the witness breaks, and where.
        advice / instances / canonical as Prover.create_proof takes them; assembly: the plonk.Assembly (or its mapping array) keygen was given, None = the copy
        constraints are not checked; cap: how many failures are stored (the totals are exact regardless); challenges: one canonical int per challenge of the
        constraint system (dehalo_check_witness_challenges) -- required, DehaloError(-1) otherwise, when an expression of the circuit reads a challenge."""
        lib = load_library()
        ctx = ctx if ctx is not None else self.ctx
        f = self.curve.scalar
        flags = PROOF_ADVICE_CANONICAL if canonical else 0
        if hasattr(advice, "data_ptr"):
            adv_ptr, flags = advice.data_ptr(), flags | PROOF_ADVICE_ON_DEVICE
            if hasattr(advice, "is_cuda") and advice.is_cuda:
                import torch
                torch.cuda.current_stream().synchronize()      # the library reads the tensor on its own stream
        else:
            adv = np.ascontiguousarray(advice, dtype=np.uint64)
            adv_ptr = adv.ctypes.data
        cols = [_instance_words(f, v) for v in instances]
        ptrs = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data if c.size else None for c in cols])
        lens = (C.c_size_t * max(1, len(cols)))(*[c.shape[0] for c in cols])
        mapping = None
        if assembly is not None:
            mapping = np.ascontiguousarray(getattr(assembly, "mapping", assembly), dtype=np.uint64).reshape(-1)
        fails = (CCheckFailure * cap)() if cap else None
        rep = CCheckReport()
        if challenges is None:
            _check(ctx, lib.dehalo_check_witness(ctx.handle, self.handle, adv_ptr, ptrs, lens, len(cols), mapping.ctypes.data if mapping is not None else None, flags, fails, cap,
                                                 C.byref(rep)))
        else:
            ch = f.encode_many([c % f.p for c in challenges]) if len(challenges) else np.zeros((1, 4), dtype=np.uint64)
            _check(ctx, lib.dehalo_check_witness_challenges(ctx.handle, self.handle, adv_ptr, ptrs, lens, len(cols), mapping.ctypes.data if mapping is not None else None, flags,
                                                            ch.ctypes.data, len(challenges), fails, cap, C.byref(rep)))
        return CheckReport(rep, [(int(fails[i].kind), int(fails[i].index), int(fails[i].row)) for i in range(int(rep.written))])

    def phases(self) -> tuple:
        """dehalo_pk_phases: (advice phases in use, challenges)."""
        out = (C.c_uint32 * 2)()
        _check(self.ctx, load_library().dehalo_pk_phases(self.handle, out))
        return int(out[0]), int(out[1])

    def info(self) -> dict:
        out = (C.c_uint32 * 8)()
        _check(self.ctx, load_library().dehalo_pk_info(self.handle, out))
        return dict(zip(("k", "extended_k", "blinding_factors", "degree", "permutation_sets", "commitments_before_evaluations", "evaluations", "opening_points"), out))

    def release(self):
        if self.handle is not None:
            load_library().dehalo_pk_release(self.ctx.handle, self.handle)
            self.handle = None


class Blake2bWrite:
    """dehalo_transcript: Blake2bWrite<Vec<u8>, C, Challenge255<C>> held by the library."""

    def __init__(self, curve: CurveSpec):
        self.curve = curve
        self.handle = C.c_void_p()
        rc = load_library().dehalo_transcript_create(curve.id, C.byref(self.handle))
        if rc:
            raise DehaloError(rc, "transcript_create")

    def _s(self, v: int):
        return self.curve.scalar.encode(v).ctypes.data

    def common_scalar(self, s: int):
        load_library().dehalo_transcript_common_scalar(self.handle, self._s(s))

    def write_scalar(self, s: int):
        load_library().dehalo_transcript_write_scalar(self.handle, self._s(s))

    def write_point(self, P):
        if P is None:
            raise ValueError("cannot write points at infinity to the transcript")
        xy = np.concatenate([self.curve.base.encode(P[0]), self.curve.base.encode(P[1])])
        if load_library().dehalo_transcript_write_point(self.handle, xy.ctypes.data):
            raise ValueError("cannot write points at infinity to the transcript")

    def squeeze_challenge_scalar(self) -> int:
        out = np.zeros(4, dtype=np.uint64)
        load_library().dehalo_transcript_squeeze_challenge(self.handle, out.ctypes.data)
        return self.curve.scalar.decode(out)

    def finalize(self) -> bytes:
        lib = load_library()
        out = np.empty(max(1, lib.dehalo_transcript_len(self.handle)), dtype=np.uint8)
        n = lib.dehalo_transcript_len(self.handle)
        if lib.dehalo_transcript_finalize(self.handle, out.ctypes.data, out.size):
            raise DehaloError(-1, "transcript_finalize")
        return out[:n].tobytes()

    def __del__(self):
        try:
            if self.handle:
                load_library().dehalo_transcript_release(self.handle)
                self.handle = None
        except Exception:      # noqa: BLE001 -- interpreter shutdown
            pass


class Blake2bRead(Blake2bWrite):
    """dehalo_transcript over a proof's bytes: Blake2bRead<_, C, Challenge255<C>>.  common_scalar and squeeze_challenge_scalar are the writer's; a read that
    the library refuses (bytes missing, a scalar not below r, an x not below p or not on the curve, the all-zero identity) raises ValueError and consumes nothing."""

    def __init__(self, curve: CurveSpec, proof: bytes):
        self.curve = curve
        self.handle = C.c_void_p()
        data = np.frombuffer(bytes(proof), dtype=np.uint8)
        rc = load_library().dehalo_transcript_create_read(curve.id, data.ctypes.data if data.size else None, data.size, C.byref(self.handle))
        if rc:
            raise DehaloError(rc, "transcript_create_read")

    def write_scalar(self, s: int):
        raise TypeError("Blake2bRead: a reading transcript writes nothing")

    def write_point(self, P):
        raise TypeError("Blake2bRead: a reading transcript writes nothing")

    def read_scalar(self) -> int:
        out = np.zeros(4, dtype=np.uint64)
        if load_library().dehalo_transcript_read_scalar(self.handle, out.ctypes.data):
            raise ValueError("read_scalar: no canonical scalar at this position")
        return self.curve.scalar.decode(out)

    def read_point(self):
        out = np.zeros(8, dtype=np.uint64)
        if load_library().dehalo_transcript_read_point(self.handle, out.ctypes.data):
            raise ValueError("read_point: no curve point at this position")
        return (self.curve.base.decode(out[:4]), self.curve.base.decode(out[4:]))

    @property
    def remaining(self) -> int:
        return load_library().dehalo_transcript_remaining(self.handle)


def pairing_check(curve: CurveSpec, pairs) -> bool:
    """dehalo_pairing_check: prod e(P_i, Q_i) == 1 for [(P in G1, Q in G2)] on the host.  P = (x, y) canonical integers or None (the identity); Q = the 128 raw
    bytes ParamsKZG keeps for g2 / s_g2 (all zero: the identity).  DehaloError for a point off its curve or subgroup (-1) and for a curve without a pairing (-5)."""
    g1 = np.zeros((max(1, len(pairs)), 8), dtype=np.uint64)
    g2 = bytearray()
    for i, (P1, Q2) in enumerate(pairs):
        if P1 is not None:
            g1[i, :4], g1[i, 4:] = curve.base.encode(P1[0]), curve.base.encode(P1[1])
        if len(Q2) != 128:
            raise ValueError("pairing_check: a G2 point is 128 raw bytes")
        g2 += bytes(Q2)
    raw = np.frombuffer(bytes(g2) or bytes(1), dtype=np.uint8)
    is_one = C.c_int(-1)
    rc = load_library().dehalo_pairing_check(curve.id, g1.ctypes.data, raw.ctypes.data, len(pairs), C.byref(is_one))
    if rc:
        raise DehaloError(rc, "pairing_check")
    return bool(is_one.value)


def rng_struct(rng) -> Optional[CRng]:
    """None / prover.OsRng -> NULL (operating-system entropy inside the library); prover.KeyedRng -> its ChaCha20 key; prover.SeededRng -> its PCG64
    state; any other object with .scalars(count) -> a callback."""
    if rng is None or type(rng).__name__ == "OsRng":
        return None
    r = CRng()
    if type(rng).__name__ == "KeyedRng":
        r.kind = RNG_CHACHA20
        C.memmove(r.pcg_state, rng.key, 16)
        C.memmove(r.pcg_inc, rng.key[16:], 16)
        return r
    gen = getattr(rng, "gen", None)
    if gen is not None and type(gen.bit_generator).__name__ == "PCG64":
        st = gen.bit_generator.state["state"]
        r.kind = RNG_PCG64
        r.pcg_state[0], r.pcg_state[1] = st["state"] & ((1 << 64) - 1), st["state"] >> 64
        r.pcg_inc[0], r.pcg_inc[1] = st["inc"] & ((1 << 64) - 1), st["inc"] >> 64
        return r
    r.kind = RNG_CALLBACK

    def fill(_user, out, count, _position):
        a = np.ascontiguousarray(rng.scalars(count), dtype=np.uint64).reshape(-1)
        C.memmove(out, a.ctypes.data, 32 * count)
        return 0
    r._keep = RNG_FILL_FN(fill)
    r.fill = r._keep
    return r


REJECT_NONE, REJECT_MALFORMED, REJECT_PAIRING, REJECT_OPENING = 0, 1, 2, 3      # dehalo_reject_reason


def _create_error() -> str:
    """dehalo_verifier_create_error: why this thread's last verifier constructor failed (a host verifier has no context to ask)"""
    buf = C.create_string_buffer(512)
    load_library().dehalo_verifier_create_error(buf, len(buf))
    return buf.value.decode()


class Verifier:
    """dehalo_verifier: verify_proof for KZG (GWC and SHPLONK) and for IPA over Pallas / Vesta (from_ipa, from_ipa_vk, from_ipa_host), one proof or a batch.  It holds the verifying half of the params and of the key only.
    With a Context the proofs' points are decompressed and the two sums of the reduction are formed on the device; with ctx=None it is a HOST verifier -- a mode
    the caller chooses (machines without a GPU), never a fallback.  The pairing check runs on the host in both, unless a verifier with a Context is switched to
    pairing="device" (set_pairing): the checks then go through the device kernel, verify_each's all in one launch."""

    MULTIOPEN = {"gwc": 0, "shplonk": 1}      # dehalo_multiopen
    PAIRING = {"host": 0, "device": 1}        # dehalo_verifier_set_pairing

    def __init__(self, ctx: Optional[Context], curve: CurveSpec, handle, multiopen: Optional[str] = "gwc", pairing: str = "host"):
        self.ctx, self.curve, self.handle = ctx, curve, handle
        self.last_reject = REJECT_NONE          # why the last verify / verify_batch said no
        self.first_malformed = -1               # verify_batch: the first unreadable proof
        self.last_checks = 0                    # verify_each: the subset checks of the last call
        self.ipa = multiopen is None            # an IPA verifier has one multiopen: nothing to set
        self._params = None                     # IPA with a context: the borrowed ParamsIPA, kept alive
        if not self.ipa:
            self.set_multiopen(multiopen)
        if pairing != "host":
            self.set_pairing(pairing)

    def _check(self, rc: int):
        if rc != 0:
            raise DehaloError(rc, load_library().dehalo_verifier_last_error(self.handle).decode() if self.handle else "verifier")

    @classmethod
    def from_pk(cls, params: ParamsKZG, pk: "ProvingKey", multiopen: str = "gwc", pairing: str = "host") -> "Verifier":
        """from objects the caller already has (dehalo_verifier_create): g[0], g2, s_g2, k of the params; the commitments, constraint system and transcript_repr of the key"""
        h = C.c_void_p()
        rc = load_library().dehalo_verifier_create(params.ctx.handle, params.handle, pk.handle, C.byref(h))
        if rc:
            raise DehaloError(rc, _create_error())
        return cls(params.ctx, params.curve, h, multiopen, pairing)

    @classmethod
    def from_vk(cls, curve: CurveSpec, k: int, g0, g2: bytes, s_g2: bytes, cs: plonk.ConstraintSystem, vk_bytes: bytes, num_selectors: int = 0,
                format: str = "raw-unchecked", ctx: Optional[Context] = None, multiopen: str = "gwc", transcript_repr: Optional[int] = None, pairing: str = "host") -> "Verifier":
        """ParamsVerifierKZG + VerifyingKey::read (dehalo_verifier_create_vk): g0 = g[0] as (x, y) canonical ints or 8 Montgomery words; g2, s_g2 the 128 raw bytes
        ParamsKZG keeps; vk_bytes in `format` (one of SERDE_FORMATS).  transcript_repr: None = the substitute keygen gives the same vk bytes."""
        if isinstance(g0, tuple):
            g0 = np.concatenate([curve.base.encode(g0[0]), curve.base.encode(g0[1])])
        g0 = np.ascontiguousarray(g0, dtype=np.uint64).reshape(8)
        desc = ConstraintSystemDescriptor(cs, curve.scalar)
        buf = np.frombuffer(bytes(vk_bytes), dtype=np.uint8)
        h = C.c_void_p()
        lib = load_library()
        rc = lib.dehalo_verifier_create_vk(ctx.handle if ctx is not None else None, curve.id, k, g0.ctypes.data, _bytes_ptr(bytes(g2).ljust(128, b"\0")),
                                           _bytes_ptr(bytes(s_g2).ljust(128, b"\0")), desc.ref(), buf.ctypes.data if buf.size else None, buf.size, _serde(format), num_selectors,
                                           C.byref(h))
        if rc:
            raise DehaloError(rc, _create_error())
        v = cls(ctx, curve, h, multiopen, pairing)
        if transcript_repr is not None:
            v.transcript_repr = transcript_repr
        return v

    @classmethod
    def from_ipa(cls, params: "ParamsIPA", pk: "ProvingKey") -> "Verifier":
        """verify_proof for IPA from a ParamsIPA and a key made under it (dehalo_verifier_create_ipa).  The params are borrowed: this object keeps them referenced."""
        h = C.c_void_p()
        rc = load_library().dehalo_verifier_create_ipa(params.ctx.handle, params.handle, pk.handle, C.byref(h))
        if rc:
            raise DehaloError(rc, _create_error())
        v = cls(params.ctx, params.curve, h, None)
        v._params = params
        return v

    @classmethod
    def from_ipa_vk(cls, params: "ParamsIPA", cs: plonk.ConstraintSystem, vk_bytes: bytes, num_selectors: int = 0, format: str = "raw-unchecked",
                    transcript_repr: Optional[int] = None) -> "Verifier":
        """the verifier's side under IPA: ParamsIPA::read + VerifyingKey::read, no proving key (dehalo_verifier_create_ipa_vk); vk_bytes in `format`"""
        desc = ConstraintSystemDescriptor(cs, params.curve.scalar)
        buf = np.frombuffer(bytes(vk_bytes), dtype=np.uint8)
        h = C.c_void_p()
        rc = load_library().dehalo_verifier_create_ipa_vk(params.ctx.handle, params.handle, desc.ref(), buf.ctypes.data if buf.size else None, buf.size, _serde(format),
                                                         num_selectors, C.byref(h))
        if rc:
            raise DehaloError(rc, _create_error())
        v = cls(params.ctx, params.curve, h, None)
        v._params = params
        if transcript_repr is not None:
            v.transcript_repr = transcript_repr
        return v

    @classmethod
    def from_ipa_host(cls, curve: CurveSpec, k: int, g, g_lagrange, w, u, cs: plonk.ConstraintSystem, vk_bytes: bytes, num_selectors: int = 0,
                      format: str = "raw-unchecked", transcript_repr: Optional[int] = None) -> "Verifier":
        """a HOST verifier for IPA over points the caller holds (dehalo_verifier_create_ipa_host): g, g_lagrange 2^k rows of 8 Montgomery words, w, u one row each.
        About 380 x 2^k group operations a call on one thread: for small k and machines without a GPU.  A mode, never a fallback."""
        g = np.ascontiguousarray(g, dtype=np.uint64).reshape(-1, 8)
        gl = np.ascontiguousarray(g_lagrange, dtype=np.uint64).reshape(-1, 8)
        w = np.ascontiguousarray(w, dtype=np.uint64).reshape(8)
        u = np.ascontiguousarray(u, dtype=np.uint64).reshape(8)
        if not 0 <= k < 64 or g.shape[0] != 1 << k or gl.shape[0] != 1 << k:
            raise ValueError("g and g_lagrange must hold 2^k points")
        desc = ConstraintSystemDescriptor(cs, curve.scalar)
        buf = np.frombuffer(bytes(vk_bytes), dtype=np.uint8)
        h = C.c_void_p()
        rc = load_library().dehalo_verifier_create_ipa_host(curve.id, k, g.ctypes.data, gl.ctypes.data, w.ctypes.data, u.ctypes.data, desc.ref(),
                                                           buf.ctypes.data if buf.size else None, buf.size, _serde(format), num_selectors, C.byref(h))
        if rc:
            raise DehaloError(rc, _create_error())
        v = cls(None, curve, h, None)
        if transcript_repr is not None:
            v.transcript_repr = transcript_repr
        return v

    def set_multiopen(self, multiopen: str):
        if multiopen not in self.MULTIOPEN:
            raise ValueError("multiopen: 'gwc' or 'shplonk'")
        self._check(load_library().dehalo_verifier_set_multiopen(self.handle, self.MULTIOPEN[multiopen]))

    def set_pairing(self, where: str):
        """dehalo_verifier_set_pairing: "host" (the default) or "device" -- the pairing checks through the kernel: verify and verify_batch one check, verify_each
        every live proof its own check in ONE launch, no search (last_checks = the live proofs).  DehaloError(-1) on a host or an IPA verifier."""
        if where not in self.PAIRING:
            raise ValueError("pairing: 'host' or 'device'")
        self._check(load_library().dehalo_verifier_set_pairing(self.handle, self.PAIRING[where]))

    def _set_repr(self, value: int):
        self._check(load_library().dehalo_verifier_set_transcript_repr(self.handle, self.curve.scalar.encode(value).ctypes.data))

    transcript_repr = property(None, _set_repr)

    def _instances(self, per_proof):
        """[proof][circuit][column] -> the pointer and length tables of dehalo_verify_proofs, the arrays they point into, columns per circuit, circuits"""
        f = self.curve.scalar
        circuits = len(per_proof[0]) if per_proof else 1
        ncols = len(per_proof[0][0]) if per_proof and circuits else 0
        cols = []
        for inst in per_proof:
            if len(inst) != circuits or any(len(c) != ncols for c in inst):
                raise ValueError("every proof needs the same number of circuits and instance columns")
            cols += [_instance_words(f, v) for c in inst for v in c]
        ptrs = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data if c.size else None for c in cols])
        lens = (C.c_size_t * max(1, len(cols)))(*[c.shape[0] for c in cols])
        return ptrs, lens, cols, ncols, circuits

    def verify(self, proof: bytes, instances: Sequence = ((),), num_circuits: Optional[int] = None) -> bool:
        """dehalo_verify_proof.  instances: one list of canonical ints per instance column; with num_circuits = N, instances[c] circuit c's columns.  False: see
        last_reject (REJECT_MALFORMED: a read failed, bytes missing or trailing; REJECT_PAIRING).  DehaloError(-1): a wrong number of instance columns or a column
        longer than the usable rows."""
        per_circuit = [list(instances)] if num_circuits is None else [list(c) for c in instances]
        ptrs, lens, keep, ncols, circuits = self._instances([per_circuit])
        buf = np.frombuffer(bytes(proof), dtype=np.uint8)
        accept, reason = C.c_int(0), C.c_int(0)
        self._check(load_library().dehalo_verify_proof(self.handle, ptrs, lens, ncols, circuits, buf.ctypes.data if buf.size else None, buf.size, C.byref(accept), C.byref(reason)))
        self.last_reject = int(reason.value)
        return bool(accept.value)

    def verify_batch(self, proofs: Sequence[bytes], instances: Optional[Sequence] = None, rng=None, num_circuits: Optional[int] = None) -> bool:
        """dehalo_verify_proofs: every proof read, then ONE pairing check over the weighted sums (w_0 = 1, the others the first len(proofs) - 1 scalars of rng;
        None = OS entropy -- the weights must be unpredictable to whoever made the proofs).  instances[i]: proof i's, as verify takes them (None: no instance
        values anywhere).  False: first_malformed names the first unreadable proof, or is -1 (the pairing failed: verify singly to find which)."""
        bufs = [np.frombuffer(bytes(p), dtype=np.uint8) for p in proofs]
        if instances is None:
            instances = [((),) if num_circuits is None else [((),)] * num_circuits] * len(bufs)
        per_proof = [[list(i)] if num_circuits is None else [list(c) for c in i] for i in instances]
        if len(per_proof) != len(bufs):
            raise ValueError("one instance list per proof")
        ptrs, lens, keep, ncols, circuits = self._instances(per_proof)
        pp = (C.c_void_p * max(1, len(bufs)))(*[b.ctypes.data if b.size else None for b in bufs])
        pl = (C.c_size_t * max(1, len(bufs)))(*[b.size for b in bufs])
        r = rng_struct(rng)
        accept, first = C.c_int(0), C.c_int64(-1)
        self._check(load_library().dehalo_verify_proofs(self.handle, pp, pl, len(bufs), ptrs, lens, ncols, circuits if bufs else (num_circuits or 1),
                                                       C.byref(r) if r is not None else None, C.byref(accept), C.byref(first)))
        rng_writeback(rng, r)
        self.first_malformed = int(first.value)
        self.last_reject = REJECT_NONE if accept.value else (REJECT_MALFORMED if first.value >= 0 else REJECT_OPENING if self.ipa else REJECT_PAIRING)
        return bool(accept.value)

    def verify_each(self, proofs: Sequence[bytes], instances: Optional[Sequence] = None, rng=None, num_circuits: Optional[int] = None) -> List[int]:
        """dehalo_verify_proofs_each: a verdict per proof from one batch verification -- REJECT_NONE for a valid proof, otherwise what verify says of that proof
        alone (REJECT_MALFORMED, REJECT_PAIRING, IPA: REJECT_OPENING).  Arguments as verify_batch takes them, the weights' draw and the warning about it too.
        last_checks: the subset checks the call made (1 when every readable proof is valid, 13 for one invalid proof among 64)."""
        bufs = [np.frombuffer(bytes(p), dtype=np.uint8) for p in proofs]
        if instances is None:
            instances = [((),) if num_circuits is None else [((),)] * num_circuits] * len(bufs)
        per_proof = [[list(i)] if num_circuits is None else [list(c) for c in i] for i in instances]
        if len(per_proof) != len(bufs):
            raise ValueError("one instance list per proof")
        ptrs, lens, keep, ncols, circuits = self._instances(per_proof)
        pp = (C.c_void_p * max(1, len(bufs)))(*[b.ctypes.data if b.size else None for b in bufs])
        pl = (C.c_size_t * max(1, len(bufs)))(*[b.size for b in bufs])
        r = rng_struct(rng)
        reasons, checks = (C.c_int * max(1, len(bufs)))(), C.c_uint32(0)
        self._check(load_library().dehalo_verify_proofs_each(self.handle, pp, pl, len(bufs), ptrs, lens, ncols, circuits if bufs else (num_circuits or 1),
                                                            C.byref(r) if r is not None else None, reasons, C.byref(checks)))
        rng_writeback(rng, r)
        self.last_checks = int(checks.value)
        return [int(reasons[i]) for i in range(len(bufs))]

    def last_timings(self) -> dict:
        """milliseconds of the last call: point decompression, the transcript walks, the two MSMs (verify_each: the per-proof sums), the pairing check (verify_each:
        the total of the subset checks)"""
        out = (C.c_double * 4)()
        self._check(load_library().dehalo_verifier_last_timings(self.handle, out))
        return dict(zip(("decompress", "walk", "msm", "g_sum" if self.ipa else "pairing"), out))

    def release(self):
        if self.handle is not None:
            load_library().dehalo_verifier_release(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.release()
        except Exception:      # noqa: BLE001 -- interpreter shutdown
            pass


def rng_writeback(rng, r: Optional[CRng]):
    """The library advanced the PCG64 state past the proof's draws (upstream's `&mut rng`): mirror it in the Python generator."""
    if r is not None and r.kind == RNG_PCG64:
        st = rng.gen.bit_generator.state
        st["state"]["state"] = int(r.pcg_state[0]) | (int(r.pcg_state[1]) << 64)
        rng.gen.bit_generator.state = st


def ipa_verify(params: "ParamsIPA", commitment, x3: int, v: int, proof: bytes) -> bool:
    """dehalo_ipa_verify: does `proof` (a stand-alone opening, ParamsIPA.open's bytes) open `commitment` -- (x, y) canonical ints or 8 Montgomery words -- to v at x3?"""
    curve = params.curve
    if isinstance(commitment, tuple):
        commitment = np.concatenate([curve.base.encode(commitment[0]), curve.base.encode(commitment[1])])
    cm = np.ascontiguousarray(commitment, dtype=np.uint64).reshape(8)
    f = curve.scalar
    xe, ve = f.encode(x3 % f.p), f.encode(v % f.p)
    buf = np.frombuffer(bytes(proof), dtype=np.uint8)
    accept = C.c_int(0)
    _check(params.ctx, load_library().dehalo_ipa_verify(params.ctx.handle, params.handle, cm.ctypes.data, xe.ctypes.data, ve.ctypes.data, buf.ctypes.data if buf.size else None,
                                                       buf.size, C.byref(accept)))
    return bool(accept.value)


class Prover:
    """dehalo_prover: the device buffers of one proof in flight; create_proof is ONE library call."""

    MULTIOPEN = {"gwc": 0, "shplonk": 1}      # dehalo_multiopen

    def __init__(self, params: ParamsKZG, pk: ProvingKey, ctx: Optional[Context] = None, side_ctx: Optional[Context] = None, multiopen: str = "gwc",
                 num_circuits: int = 1):
        """multiopen: which KZG multiopen the proofs carry, "gwc" (ProverGWC, the default) or "shplonk" (ProverSHPLONK); ParamsIPA takes "gwc" (unset) only.
        num_circuits: how many witnesses of the key one proof is over (dehalo_prover_create_multi; create_proof_multi); 1: create_proof and the rest."""
        self.params, self.pk, self.num_circuits = params, pk, num_circuits
        self.ctx = ctx if ctx is not None else pk.ctx
        self.side = side_ctx
        self.handle = C.c_void_p()
        if multiopen not in self.MULTIOPEN:
            raise ValueError("multiopen: 'gwc' or 'shplonk'")
        _check(self.ctx, load_library().dehalo_prover_create_multi(self.ctx.handle, side_ctx.handle if side_ctx is not None else None, params.handle, pk.handle, num_circuits,
                                                                   C.byref(self.handle)))
        if multiopen != "gwc":
            try:
                self.set_multiopen(multiopen)
            except Exception:
                self.release()
                raise

    def set_multiopen(self, multiopen):
        """dehalo_prover_set_multiopen: "gwc" | "shplonk" (or the enum's value); DehaloError(-5) on a prover over ParamsIPA, (-1) for anything else."""
        _check(self.ctx, load_library().dehalo_prover_set_multiopen(self.handle, self.MULTIOPEN.get(multiopen, multiopen)))

    def set_shard(self, rank: int, world: int, gather=None):
        """dehalo_prover_set_shard: this process runs the MSMs of its share of every multi-column commitment phase only; `gather(points, first, num)` --
        points a (count, 8) uint64 array whose rows [first[rank], first[rank] + num[rank]) are filled -- must fill in the other rows in place (an all-gather:
        sharding.gather_points).  Every process must prove with the same inputs and the same seeded rng.  world = 1 switches it off."""
        from ._lib import GATHER_FN

        def thunk(_user, pts, count, first, num, w):
            try:
                arr = np.ctypeslib.as_array(pts, shape=(count, 8))
                gather(arr, [first[i] for i in range(w)], [num[i] for i in range(w)])
                return 0
            except Exception:      # noqa: BLE001  (an exception must not unwind through the C frames)
                import traceback
                traceback.print_exc()
                return -1

        self._gather_cb = GATHER_FN(thunk) if world > 1 else GATHER_FN()      # kept alive as long as the prover may call it
        _check(self.ctx, load_library().dehalo_prover_set_shard(self.handle, rank, world, self._gather_cb, None))

    def create_proof(self, advice, instances: Sequence[Sequence[int]] = ((),), rng=None, transcript: Optional[Blake2bWrite] = None, canonical: bool = False) -> Blake2bWrite:
        """advice: (num_advice, n, 4) u64 Montgomery (or plain integers < p with canonical=True: what native.synthesize returns) -- a host
        array or a device tensor (anything with .data_ptr()).  instances: one list of canonical ints per instance column.  rng: None = OS
        entropy; prover.SeededRng for reproducible test proofs."""
        lib = load_library()
        tr = transcript if transcript is not None else Blake2bWrite(self.pk.curve)
        f = self.pk.curve.scalar
        flags = PROOF_ADVICE_CANONICAL if canonical else 0
        if hasattr(advice, "data_ptr"):
            adv_ptr, flags = advice.data_ptr(), flags | PROOF_ADVICE_ON_DEVICE
            if hasattr(advice, "is_cuda") and advice.is_cuda:
                import torch
                torch.cuda.current_stream().synchronize()      # the library reads the tensor on its own stream
        else:
            adv = np.ascontiguousarray(advice, dtype=np.uint64)
            adv_ptr = adv.ctypes.data
        cols = [_instance_words(f, v) for v in instances]
        ptrs = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data if c.size else None for c in cols])
        lens = (C.c_size_t * max(1, len(cols)))(*[c.shape[0] for c in cols])
        r = rng_struct(rng)
        rc = lib.dehalo_create_proof(self.handle, adv_ptr, ptrs, lens, len(cols), C.byref(r) if r is not None else None, tr.handle, flags)
        if rc != 0:
            msg = lib.dehalo_last_error(self.ctx.handle).decode()
            if rc == -1 and ("instance" in msg or "infinity" in msg):
                raise ValueError(msg)
            raise DehaloError(rc, msg)
        rng_writeback(rng, r)
        return tr

    def create_proof_multi(self, advices, instances: Sequence[Sequence[Sequence[int]]], rng=None, transcript: Optional[Blake2bWrite] = None, canonical: bool = False,
                           num_circuits: Optional[int] = None) -> Blake2bWrite:
        """dehalo_create_proof_multi: ONE proof over len(advices) witnesses of the key.  advices: create_proof's `advice`, one per circuit (all host arrays or all
        device tensors); instances[c]: circuit c's instance columns, each a list of canonical ints (every circuit the same number of columns)."""
        lib = load_library()
        tr = transcript if transcript is not None else Blake2bWrite(self.pk.curve)
        f = self.pk.curve.scalar
        flags = PROOF_ADVICE_CANONICAL if canonical else 0
        on_device = [hasattr(a, "data_ptr") for a in advices]
        if any(on_device) and not all(on_device):
            raise ValueError("create_proof_multi: the witnesses are all host arrays or all device tensors")
        if advices and all(on_device):
            flags |= PROOF_ADVICE_ON_DEVICE
            if any(getattr(a, "is_cuda", False) for a in advices):
                import torch
                torch.cuda.current_stream().synchronize()      # the library reads the tensors on its own stream
            keep, adv_ptrs = list(advices), [a.data_ptr() for a in advices]
        else:
            keep = [np.ascontiguousarray(a, dtype=np.uint64) for a in advices]
            adv_ptrs = [a.ctypes.data for a in keep]
        per_circuit = {len(inst) for inst in instances}
        if len(instances) != len(advices) or len(per_circuit) > 1:
            raise ValueError("create_proof_multi: one list of instance columns per circuit, every circuit the same number of columns")
        ncols = per_circuit.pop() if per_circuit else 0
        cols = [_instance_words(f, v) for inst in instances for v in inst]
        ptrs = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data if c.size else None for c in cols])
        lens = (C.c_size_t * max(1, len(cols)))(*[c.shape[0] for c in cols])
        r = rng_struct(rng)
        rc = lib.dehalo_create_proof_multi(self.handle, (C.c_void_p * max(1, len(adv_ptrs)))(*adv_ptrs), ptrs, lens, ncols, len(advices) if num_circuits is None else num_circuits,
                                           C.byref(r) if r is not None else None, tr.handle, flags)
        del keep
        if rc != 0:
            msg = lib.dehalo_last_error(self.ctx.handle).decode()
            if rc == -1 and ("instance" in msg or "infinity" in msg):
                raise ValueError(msg)
            raise DehaloError(rc, msg)
        rng_writeback(rng, r)
        return tr

    def create_proof_phased(self, witness_fn, instances: Sequence[Sequence[int]] = ((),), rng=None, transcript: Optional[Blake2bWrite] = None, canonical: bool = False) -> Blake2bWrite:
        """dehalo_create_proof_phased: witness_fn(phase, challenges) -> advice is called once per advice phase, in order, with the circuit's challenges as
        canonical ints (those not yet squeezed are 0); it returns the advice as create_proof takes it -- every call a host array or every call a device tensor -- of
        which the columns of `phase` are read.  An exception in witness_fn ends the proof (DehaloError(-1), the exception chained); the prover stays usable."""
        from ._lib import ADVICE_FN
        lib = load_library()
        tr = transcript if transcript is not None else Blake2bWrite(self.pk.curve)
        f = self.pk.curve.scalar
        # whether the advice lives on the device is one of the call's flags, which exist before the first callback: phase 0's witness depends on no
        # challenge, so it is asked for here and handed over when the library's turn comes
        first = witness_fn(0, [0] * self.pk.phases()[1])
        state = {"keep": None, "device": hasattr(first, "data_ptr"), "error": None}

        def thunk(_user, phase, chal, count, out):
            try:
                values = [f.decode(np.ctypeslib.as_array(chal, shape=(count, 4))[j]) for j in range(count)] if count else []
                advice = first if phase == 0 else witness_fn(int(phase), values)
                if hasattr(advice, "data_ptr") != state["device"]:
                    raise TypeError("witness_fn must return host arrays in every phase or device tensors in every phase")
                if state["device"]:
                    if hasattr(advice, "is_cuda") and advice.is_cuda:
                        import torch
                        torch.cuda.current_stream().synchronize()      # the library reads the tensor on its own stream
                    state["keep"], ptr = advice, advice.data_ptr()
                else:
                    state["keep"] = np.ascontiguousarray(advice, dtype=np.uint64)      # (alive until the next callback or the return)
                    ptr = state["keep"].ctypes.data
                out[0] = ptr
                return 0
            except Exception as e:      # noqa: BLE001  (an exception must not unwind through the C frames)
                state["error"] = e
                return 1

        flags = (PROOF_ADVICE_CANONICAL if canonical else 0) | (PROOF_ADVICE_ON_DEVICE if state["device"] else 0)
        cols = [_instance_words(f, v) for v in instances]
        ptrs = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data if c.size else None for c in cols])
        lens = (C.c_size_t * max(1, len(cols)))(*[c.shape[0] for c in cols])
        r = rng_struct(rng)
        cb = ADVICE_FN(thunk)
        rc = lib.dehalo_create_proof_phased(self.handle, cb, None, ptrs, lens, len(cols), C.byref(r) if r is not None else None, tr.handle, flags)
        if rc != 0:
            msg = lib.dehalo_last_error(self.ctx.handle).decode()
            if state["error"] is not None:
                raise DehaloError(rc, msg) from state["error"]
            if rc == -1 and ("instance" in msg or "infinity" in msg):
                raise ValueError(msg)
            raise DehaloError(rc, msg)
        rng_writeback(rng, r)
        return tr

    def create_proof_circuit(self, circuit: int, instances: Sequence[Sequence[int]] = ((),), rng=None, transcript: Optional[Blake2bWrite] = None, **inputs):
        """create_proof(&params, &pk, &[circuit], instances, rng, &mut transcript) as the reference calls it (benches/delay_enc.rs:123-131): the circuit is
        synthesized inside the call (dehalo_create_proof_circuit).  `inputs`: n_big, e, x, exp_bits, message, key, bits_len as for synthesize().
        -> (transcript, {"rows", "rsa_rows", "rsa_result", "cipher"})"""
        lib = load_library()
        tr = transcript if transcript is not None else Blake2bWrite(self.pk.curve)
        f = self.pk.curve.scalar
        inp, keep = circuit_inputs(circuit, self.pk.info()["k"], **inputs)
        cols = [_instance_words(f, v) for v in instances]
        ptrs = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data if c.size else None for c in cols])
        lens = (C.c_size_t * max(1, len(cols)))(*[c.shape[0] for c in cols])
        r = rng_struct(rng)
        info = CSynthesisInfo()
        rc = lib.dehalo_create_proof_circuit(self.handle, C.byref(inp), C.byref(info), ptrs, lens, len(cols), C.byref(r) if r is not None else None, tr.handle)
        if rc != 0:
            raise DehaloError(rc, lib.dehalo_last_error(self.ctx.handle).decode())
        rng_writeback(rng, r)
        return tr, _info_dict(info)

    def proof_size(self) -> int:
        """Byte length of one proof for this prover's params (KZG / GWC or IPA), instance commitments and evaluations included."""
        return int(load_library().dehalo_prover_proof_size(self.handle))

    def last_timings(self) -> dict:
        out = (C.c_double * 8)()
        load_library().dehalo_prover_last_timings(self.handle, out)
        return dict(zip(PHASES, out))

    def release(self):
        if self.handle:
            load_library().dehalo_prover_release(self.handle)
            self.handle = C.c_void_p()


def create_proofs(provers: Sequence[Prover], advice, rngs: Sequence, count: Optional[int] = None) -> List[bytes]:
    """Batch / throughput mode (BASELINE configs[4]): proof i on prover i mod len(provers), one library thread per prover, no interpreter
    in the loop.  `advice`: one device tensor / host array used for every proof, or a list of them."""
    lib = load_library()
    count = len(rngs) if count is None else count
    advs = list(advice) if isinstance(advice, (list, tuple)) else [advice] * count
    on_device = hasattr(advs[0], "data_ptr")
    if on_device:
        import torch
        torch.cuda.current_stream().synchronize()
        adv_ptrs = [a.data_ptr() for a in advs]
    else:
        keep = [np.ascontiguousarray(a, dtype=np.uint64) for a in advs]
        adv_ptrs = [a.ctypes.data for a in keep]
    info = provers[0].pk.info()
    cap = 32 * (info["commitments_before_evaluations"] + info["evaluations"] + info["opening_points"])
    bufs = [np.empty(cap, dtype=np.uint8) for _ in range(count)]
    lens = (C.c_size_t * max(1, count))()
    rs = (CRng * max(1, count))()
    keepalive = []
    for i, g in enumerate(rngs):
        r = rng_struct(g)
        if r is None:
            rs[i].kind = RNG_OS
        else:
            keepalive.append(r)
            rs[i] = r
    ph = (C.c_void_p * len(provers))(*[p.handle.value for p in provers])
    rc = lib.dehalo_create_proofs(ph, len(provers), (C.c_void_p * max(1, count))(*adv_ptrs), count, rs, PROOF_ADVICE_ON_DEVICE if on_device else 0,
                                  (C.c_void_p * max(1, count))(*[b.ctypes.data for b in bufs]), cap, lens)
    if rc != 0:
        raise DehaloError(rc, "; ".join(lib.dehalo_last_error(p.ctx.handle).decode() for p in provers))
    return [bufs[i][:lens[i]].tobytes() for i in range(count)]


def create_proofs_circuit(provers: Sequence[Prover], circuit: int, inputs: Sequence[dict], rngs: Sequence) -> List[bytes]:
    """Batch mode with every proof's circuit synthesized inside its call (dehalo_create_proofs_circuit): inputs[i] = the keyword arguments of
    synthesize() for proof i (n_big, e, x, exp_bits, message, key, bits_len)."""
    lib = load_library()
    count = len(inputs)
    k = provers[0].pk.info()["k"]
    arr = (CCircuitInputs * max(1, count))()
    keep = []
    for i, kw in enumerate(inputs):
        inp, arrays = circuit_inputs(circuit, k, **kw)
        arr[i] = inp
        keep.append(arrays)
    info = provers[0].pk.info()
    cap = 32 * (info["commitments_before_evaluations"] + info["evaluations"] + info["opening_points"])
    bufs = [np.empty(cap, dtype=np.uint8) for _ in range(count)]
    lens = (C.c_size_t * max(1, count))()
    rs = (CRng * max(1, count))()
    keepalive = []
    for i, g in enumerate(rngs):
        r = rng_struct(g)
        if r is None:
            rs[i].kind = RNG_OS
        else:
            keepalive.append(r)
            rs[i] = r
    ph = (C.c_void_p * len(provers))(*[p.handle.value for p in provers])
    rc = lib.dehalo_create_proofs_circuit(ph, len(provers), arr, count, rs, (C.c_void_p * max(1, count))(*[b.ctypes.data for b in bufs]), cap, lens)
    if rc != 0:
        raise DehaloError(rc, "; ".join(lib.dehalo_last_error(p.ctx.handle).decode() for p in provers))
    return [bufs[i][:lens[i]].tobytes() for i in range(count)]


def _limbs(x: int, count: int) -> np.ndarray:
    return np.frombuffer(int(x).to_bytes(8 * count, "little"), dtype=np.uint64).copy()


def circuit_inputs(circuit: int, k: int, *, n_big: int = 0, e: int = 0, x: int = 0, exp_bits: int = 0, message: Sequence[int] = (), key: Sequence[int] = (), bits_len: int = 2048):
    """-> (dehalo_circuit_inputs, the arrays it points into): the reference's circuit structs as values (DelayEncryptCircuit { n, e, x, spec, enc_key... },
    RSACircuit, PoseidonEncCircuit)."""
    nl = bits_len // 64
    inp = CCircuitInputs()
    inp.circuit, inp.k, inp.bits_len, inp.exp_bits, inp.e = circuit, k, bits_len, exp_bits, e
    keep = [_limbs(n_big, nl), _limbs(x, nl), np.ascontiguousarray(np.frombuffer(b"".join(int(m).to_bytes(32, "little") for m in message) or bytes(32), dtype=np.uint64)),
            np.ascontiguousarray(np.frombuffer(b"".join(int(m).to_bytes(32, "little") for m in key) or bytes(64), dtype=np.uint64))]
    inp.n, inp.x, inp.message, inp.message_len, inp.key = keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, len(message), keep[3].ctypes.data
    return inp, keep


def _info_dict(info) -> dict:
    return {"rows": int(info.total_rows), "rsa_rows": int(info.rsa_rows), "rsa_result": sum(int(v) << (64 * i) for i, v in enumerate(info.rsa_result)),
            "cipher": [sum(int(info.cipher[4 * i + j]) << (64 * j) for j in range(4)) for i in range(info.cipher_len)]}


def synthesize(circuit: int, k: int, *, n_big: int = 0, e: int = 0, x: int = 0, exp_bits: int = 0, message: Sequence[int] = (), key: Sequence[int] = (), bits_len: int = 2048,
               keygen: bool = False, out=None) -> dict:
    """dehalo_synthesize: Circuit::synthesize of the reference's circuits as values, in C++ (csrc/witness.hip; src/lib.rs:164-318,
    benches/mod_pow.rs:63-110, src/encryption/chip.rs:114-204).  -> {"advice": (5, n, 4) u64 CANONICAL, "rows", "rsa_rows", "rsa_result",
    "cipher"} and, with keygen=True, "fixed" (canonical), "mapping", "selectors".  `out`: a C-contiguous (5, n, 4) uint64 array the advice columns
    are written into (the library writes them in place: a caller that proves repeatedly hands over one page-locked buffer and uploads from it)."""
    lib = load_library()
    inp, keep = circuit_inputs(circuit, k, n_big=n_big, e=e, x=x, exp_bits=exp_bits, message=message, key=key, bits_len=bits_len)
    n = 1 << k
    nfix = 9 if circuit == CIRCUIT_POSE_ENC else 15
    if out is not None:
        if out.shape != (5, n, 4) or out.dtype != np.uint64 or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("synthesize: `out` must be a C-contiguous (5, %d, 4) uint64 array" % n)
        advice = out
    else:
        advice = np.empty((5, n, 4), dtype=np.uint64)
    fixed = np.empty((nfix, n, 4), dtype=np.uint64) if keygen else None
    mapping = np.empty(6 * n, dtype=np.uint64) if keygen else None
    sels = [np.zeros(n, dtype=np.uint8) for _ in range(2)] if keygen and circuit != CIRCUIT_POSE_ENC else []
    sel_ptrs = (C.c_void_p * 2)(*[s.ctypes.data for s in sels]) if sels else None
    info = CSynthesisInfo()
    rc = lib.dehalo_synthesize(C.byref(inp), advice.ctypes.data, fixed.ctypes.data if keygen else None, mapping.ctypes.data if keygen else None, sel_ptrs, C.byref(info))
    if rc != 0:
        raise ValueError("dehalo_synthesize failed (%d): bad inputs or not enough rows available" % rc)
    out = dict(_info_dict(info), advice=advice)
    if keygen:
        out.update(fixed=fixed, mapping=mapping, selectors=[s.astype(bool) for s in sels])
    return out
