//! `ParamsKZG<Bn256>` with `g` / `g_lagrange` resident in HBM [UPSTREAM halo2_proofs/src/poly/kzg/commitment.rs @ v2023_04_20; reference call sites
//! benches/delay_enc.rs:41-54 -- `ParamsKZG::<Bn256>::setup(K, OsRng)`, `params.write(..)`, `ParamsKZG::read(..)`].
//!
//! The patched `ParamsKZG` keeps upstream's public interface and holds one of these next to (or instead of) its `Vec<G1Affine>` fields:
//!
//! ```ignore
//! impl<'params> Params<'params, G1Affine> for ParamsKZG<Bn256> {
//!     fn commit_lagrange(&self, poly: &Polynomial<Fr, LagrangeCoeff>, _: Blind<Fr>) -> G1 { self.dehalo.commit_lagrange(&poly.values) }
//! }
//! impl<'params> ParamsProver<'params, G1Affine> for ParamsKZG<Bn256> {
//!     fn commit(&self, poly: &Polynomial<Fr, Coeff>, _: Blind<Fr>) -> G1 { self.dehalo.commit(&poly.values) }
//! }
//! ```
//! (KZG ignores the blind, exactly as upstream.)
use crate::{Context, DehaloError};
use dehalo_sys as sys;
use ff::Field;
use halo2curves::bn256::{Fr, G1};
use rand_core::RngCore;
use std::cell::Cell;

/// halo2curves' `SerdeFormat` as the library numbers it (`dehalo_serde_format`): `Processed` = compressed points, `RawBytes` = Montgomery limbs with every
/// point checked when read, `RawBytesUnchecked` = the same bytes copied in unseen (what `read` / `write` below have always taken).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum SerdeFormat {
    Processed,
    RawBytes,
    RawBytesUnchecked,
}

impl From<SerdeFormat> for sys::dehalo_serde_format {
    fn from(f: SerdeFormat) -> Self {
        match f {
            SerdeFormat::Processed => sys::DEHALO_SERDE_PROCESSED,
            SerdeFormat::RawBytes => sys::DEHALO_SERDE_RAW_BYTES,
            SerdeFormat::RawBytesUnchecked => sys::DEHALO_SERDE_RAW_BYTES_UNCHECKED,
        }
    }
}

/// `DEHALO_KEEP_K`: `read_custom` keeps the file's `k`.
const KEEP_K: u32 = 0xffff_ffff;

/// `dehalo_params`: the SRS with its precomputed window tables on the device and the RawBytes image on the host.
pub struct DehaloParamsKZG<'c> {
    pub(crate) ctx: &'c Context,
    pub(crate) raw: *mut sys::dehalo_params,
    pub k: u32,
    bases_g: Cell<*mut sys::dehalo_bases>,
    bases_gl: Cell<*mut sys::dehalo_bases>,
}

impl<'c> DehaloParamsKZG<'c> {
    /// `ParamsKZG::<Bn256>::setup(k, rng)` (benches/delay_enc.rs:43): draws `s` exactly as upstream does (`<Fr>::random(rng)`) and hands it over; `g[i] = [s^i] G` and
    /// `g_lagrange[i] = [L_i(s)] G` are made on the device.  k <= 25 (include/dehalo.h).
    pub fn setup<R: RngCore>(ctx: &'c Context, k: u32, mut rng: R) -> Result<Self, DehaloError> {
        let s = Fr::random(&mut rng);
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe { sys::dehalo_params_setup(ctx.as_ptr(), sys::DEHALO_CURVE_BN254_G1, k, &s as *const Fr as *const u64, &mut raw) })?;
        Self::finish(ctx, raw, k)
    }

    /// `ParamsKZG::read(&mut reader)` of the RawBytes file the bench caches (`:54`): `k: u32 LE | g | g_lagrange | g2 | s_g2`.
    pub fn read(ctx: &'c Context, bytes: &[u8]) -> Result<Self, DehaloError> {
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe { sys::dehalo_params_read(ctx.as_ptr(), sys::DEHALO_CURVE_BN254_G1, bytes.as_ptr(), bytes.len(), &mut raw) })?;
        let k = u32::from_le_bytes([bytes[0], bytes[1], bytes[2], bytes[3]]);
        Self::finish(ctx, raw, k)
    }

    /// From vectors upstream already holds (`params.get_g()`, `g_lagrange`, the two G2 points as 128 raw bytes each).
    pub fn from_vectors(ctx: &'c Context, k: u32, g: &[halo2curves::bn256::G1Affine], g_lagrange: &[halo2curves::bn256::G1Affine], g2: &[u8; 128], s_g2: &[u8; 128]) -> Result<Self, DehaloError> {
        assert_eq!(g.len(), 1usize << k);
        assert_eq!(g_lagrange.len(), 1usize << k);
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe {
            sys::dehalo_params_create(ctx.as_ptr(), sys::DEHALO_CURVE_BN254_G1, k, g.as_ptr() as *const u64, g_lagrange.as_ptr() as *const u64, g2.as_ptr(), s_g2.as_ptr(), &mut raw)
        })?;
        Self::finish(ctx, raw, k)
    }

    /// `ParamsKZG::read_custom(&mut reader, format)`, and with `downsize = Some(k')` the same followed by `Params::downsize(k')` in one step: only
    /// `g[0 .. 2^k')` is taken from the file and `g_lagrange` is the group FFT of it on the device -- a large SRS, a small circuit (`dehalo_params_read_custom`).
    pub fn read_custom(ctx: &'c Context, bytes: &[u8], format: SerdeFormat, downsize: Option<u32>) -> Result<Self, DehaloError> {
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe {
            sys::dehalo_params_read_custom(ctx.as_ptr(), sys::DEHALO_CURVE_BN254_G1, bytes.as_ptr(), bytes.len(), format.into(), downsize.unwrap_or(KEEP_K), &mut raw)
        })?;
        let k = downsize.unwrap_or_else(|| u32::from_le_bytes([bytes[0], bytes[1], bytes[2], bytes[3]]));
        Self::finish(ctx, raw, k)
    }

    /// From `g`, `g2` and `s_g2` alone: `g_lagrange = g_to_lagrange(g, k)` on the device (`dehalo_params_from_g`), as upstream's `from_parts` with `g_lagrange: None`.
    pub fn from_g(ctx: &'c Context, k: u32, g: &[halo2curves::bn256::G1Affine], g2: &[u8; 128], s_g2: &[u8; 128]) -> Result<Self, DehaloError> {
        assert_eq!(g.len(), 1usize << k);
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe { sys::dehalo_params_from_g(ctx.as_ptr(), sys::DEHALO_CURVE_BN254_G1, k, g.as_ptr() as *const u64, g2.as_ptr(), s_g2.as_ptr(), &mut raw) })?;
        Self::finish(ctx, raw, k)
    }

    /// `Params::downsize(k)` as a new object; `self` stays as it is (`dehalo_params_downsize`).
    pub fn downsize(&self, k: u32) -> Result<Self, DehaloError> {
        let mut raw = core::ptr::null_mut();
        self.ctx.check(unsafe { sys::dehalo_params_downsize(self.ctx.as_ptr(), self.raw, k, &mut raw) })?;
        Self::finish(self.ctx, raw, k)
    }

    /// `params.write_custom(&mut writer, format)` (`dehalo_params_write_custom`); `Processed` compresses the points on the device.
    pub fn write_custom(&self, format: SerdeFormat) -> Result<Vec<u8>, DehaloError> {
        let mut out = vec![0u8; unsafe { sys::dehalo_params_size_custom(self.raw, format.into()) }];
        self.ctx.check(unsafe { sys::dehalo_params_write_custom(self.raw, format.into(), out.as_mut_ptr(), out.len()) })?;
        Ok(out)
    }

    fn finish(ctx: &'c Context, raw: *mut sys::dehalo_params, k: u32) -> Result<Self, DehaloError> {
        Ok(DehaloParamsKZG { ctx, raw, k, bases_g: Cell::new(core::ptr::null_mut()), bases_gl: Cell::new(core::ptr::null_mut()) })
    }

    /// `params.write(&mut writer)` (RawBytes; benches/delay_enc.rs:45)
    pub fn write(&self) -> Result<Vec<u8>, DehaloError> {
        let mut out = vec![0u8; unsafe { sys::dehalo_params_size(self.raw) }];
        self.ctx.check(unsafe { sys::dehalo_params_write(self.raw, out.as_mut_ptr(), out.len()) })?;
        Ok(out)
    }

    /// `ParamsProver::commit(poly, _)`: `best_multiexp(&poly.values, &self.g[..len])` over the resident table; `len` may be shorter than n (a prefix).
    pub fn commit(&self, coeffs: &[Fr]) -> G1 {
        self.msm(coeffs, false)
    }

    /// `Params::commit_lagrange(poly, _)`: the same over `g_lagrange`.
    pub fn commit_lagrange(&self, values: &[Fr]) -> G1 {
        self.msm(values, true)
    }

    fn msm(&self, scalars: &[Fr], lagrange: bool) -> G1 {
        assert!(scalars.len() <= 1usize << self.k);
        // dehalo_params_commit_device is the prover's path (polynomials already in HBM); for a host slice the entry is dehalo_msm over registered bases.  Same group element.
        let n = scalars.len();
        let mut out = [0u64; 12];
        let bases = self.bases(lagrange).expect("dehalo: registering the SRS");
        self.ctx.check(unsafe { sys::dehalo_msm(self.ctx.as_ptr(), bases, scalars.as_ptr() as *const u64, n, out.as_mut_ptr()) }).expect("dehalo_msm");
        unsafe { core::mem::transmute_copy::<[u64; 12], G1>(&out) }
    }

    /// The bases handle of `g` / `g_lagrange` for `dehalo_msm` on host scalars.  `dehalo_params` keeps its own tables for the prover; a host-slice commit registers
    /// the same points once more on first use (the RawBytes image holds them) and keeps the handle.  (`Cell`: the struct is not `Sync`; one per proving thread.)
    fn bases(&self, lagrange: bool) -> Result<*const sys::dehalo_bases, DehaloError> {
        let slot = if lagrange { &self.bases_gl } else { &self.bases_g };
        if slot.get().is_null() {
            let raw = self.write()?;
            let n = 1usize << self.k;
            let off = 4 + if lagrange { 64 * n } else { 0 };
            // the file's points are 64-byte {x, y} Montgomery records: the layout dehalo_bases_register takes (stride 64); copied to an aligned buffer first
            let mut pts = vec![0u64; 8 * n];
            unsafe { core::ptr::copy_nonoverlapping(raw.as_ptr().add(off), pts.as_mut_ptr() as *mut u8, 64 * n) };
            let mut h = core::ptr::null_mut();
            self.ctx.check(unsafe { sys::dehalo_bases_register(self.ctx.as_ptr(), sys::DEHALO_CURVE_BN254_G1, pts.as_ptr(), n, 64, 0, 1, &mut h) })?;
            slot.set(h);
        }
        Ok(slot.get() as *const sys::dehalo_bases)
    }

    pub fn as_ptr(&self) -> *const sys::dehalo_params {
        self.raw
    }
}

impl Drop for DehaloParamsKZG<'_> {
    fn drop(&mut self) {
        unsafe {
            for h in [self.bases_g.get(), self.bases_gl.get()] {
                if !h.is_null() {
                    sys::dehalo_bases_release(self.ctx.as_ptr(), h);
                }
            }
            sys::dehalo_params_release(self.ctx.as_ptr(), self.raw);
        }
    }
}

/// `ParamsIPA<EqAffine>` (Vesta) from the vectors upstream's `ParamsIPA` holds (`params.g`, `params.g_lagrange`, `params.w`, `params.u`):
/// `dehalo_params_ipa_create`; from `params.g`, `params.w`, `params.u` alone (`from_g`: `g_to_lagrange` runs on the device); or from `ParamsIPA::write`'s
/// bytes (`read` / `write`).  `ParamsIPA::new` (the hash-to-curve generators) is not provided by the library; `generate` derives generators of the library's
/// own public rule instead.  What it provides over these params is
/// keygen (`commit_lagrange` with `Blind::default()`), whole `ProverIPA` proofs (`prover::create_proof_ipa`) and the opening argument of one
/// polynomial (`dehalo_ipa_open`, upstream's `poly::ipa::commitment::create_proof`).
pub struct DehaloParamsIPA<'c> {
    pub(crate) ctx: &'c Context,
    pub(crate) raw: *mut sys::dehalo_params,
    pub k: u32,
}

impl<'c> DehaloParamsIPA<'c> {
    pub fn from_vectors(ctx: &'c Context, k: u32, g: &[halo2curves::pasta::EqAffine], g_lagrange: &[halo2curves::pasta::EqAffine], w: &halo2curves::pasta::EqAffine,
                        u: &halo2curves::pasta::EqAffine) -> Result<Self, DehaloError> {
        assert_eq!(g.len(), 1usize << k);
        assert_eq!(g_lagrange.len(), 1usize << k);
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe {
            sys::dehalo_params_ipa_create(ctx.as_ptr(), sys::DEHALO_CURVE_VESTA, k, g.as_ptr() as *const u64, g_lagrange.as_ptr() as *const u64,
                                          w as *const _ as *const u64, u as *const _ as *const u64, &mut raw)
        })?;
        Ok(Self { ctx, raw, k })
    }

    /// `ParamsIPA` from `g` alone: `g_lagrange = g_to_lagrange(g, k)` on the device, then as `from_vectors` (`dehalo_params_ipa_from_g`)
    pub fn from_g(ctx: &'c Context, k: u32, g: &[halo2curves::pasta::EqAffine], w: &halo2curves::pasta::EqAffine, u: &halo2curves::pasta::EqAffine) -> Result<Self, DehaloError> {
        assert_eq!(g.len(), 1usize << k);
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe {
            sys::dehalo_params_ipa_from_g(ctx.as_ptr(), sys::DEHALO_CURVE_VESTA, k, g.as_ptr() as *const u64, w as *const _ as *const u64, u as *const _ as *const u64, &mut raw)
        })?;
        Ok(Self { ctx, raw, k })
    }

    /// `ParamsIPA` at any `k` without a file: `g`, `W`, `U` derived on the device by the library's public rule (include/dehalo.h, "Generated points":
    /// ChaCha20 under `key`, `None` = the default key), `g_lagrange` by the group FFT (`dehalo_params_ipa_generate`).  These are NOT the generators of
    /// upstream's `ParamsIPA::new`: an upstream verifier gets them through `write` and `ParamsIPA::read`.
    pub fn generate(ctx: &'c Context, k: u32, key: Option<&[u8; 32]>) -> Result<Self, DehaloError> {
        let mut raw = core::ptr::null_mut();
        let key_ptr = key.map_or(core::ptr::null(), |b| b.as_ptr());
        ctx.check(unsafe { sys::dehalo_params_ipa_generate(ctx.as_ptr(), sys::DEHALO_CURVE_VESTA, k, key_ptr, &mut raw) })?;
        Ok(Self { ctx, raw, k })
    }

    /// `ParamsIPA::read(&mut reader)`: k | g | g_lagrange | w | u, compressed points (`dehalo_params_ipa_read`)
    pub fn read(ctx: &'c Context, bytes: &[u8]) -> Result<Self, DehaloError> {
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe { sys::dehalo_params_ipa_read(ctx.as_ptr(), sys::DEHALO_CURVE_VESTA, bytes.as_ptr(), bytes.len(), &mut raw) })?;
        let k = if bytes.len() >= 4 { u32::from_le_bytes([bytes[0], bytes[1], bytes[2], bytes[3]]) } else { 0 };
        Ok(Self { ctx, raw, k })
    }

    /// `Params::downsize(k)` as a new object with its own table of `W`; `self` stays as it is (`dehalo_params_downsize`)
    pub fn downsize(&self, k: u32) -> Result<Self, DehaloError> {
        let mut raw = core::ptr::null_mut();
        self.ctx.check(unsafe { sys::dehalo_params_downsize(self.ctx.as_ptr(), self.raw, k, &mut raw) })?;
        Ok(Self { ctx: self.ctx, raw, k })
    }

    /// `params.write(&mut writer)` (`dehalo_params_ipa_write`)
    pub fn write(&self) -> Result<Vec<u8>, DehaloError> {
        let mut out = vec![0u8; unsafe { sys::dehalo_params_ipa_size(self.raw) }];
        self.ctx.check(unsafe { sys::dehalo_params_ipa_write(self.raw, out.as_mut_ptr(), out.len()) })?;
        Ok(out)
    }
}

impl Drop for DehaloParamsIPA<'_> {
    fn drop(&mut self) {
        unsafe { sys::dehalo_params_release(self.ctx.as_ptr(), self.raw) };
    }
}

/// `dehalo_fixed_base`: the window table of one point `P`, resident on the device -- `[s] P` without a doubling chain, for a few dozen scalars at a time.
/// Device pointers in and out (the scalars are a proof's blinds, already in HBM); one launch per call, asynchronous on the stream.
pub struct FixedBase<'c> {
    ctx: &'c Context,
    raw: *const sys::dehalo_fixed_base,
    owned: bool,
}

impl<'c> FixedBase<'c> {
    /// The table of `affine_xy` (`{x, y}`, Montgomery limbs as halo2curves holds them; all zero = the identity) on `curve` (`sys::DEHALO_CURVE_*`).
    pub fn new(ctx: &'c Context, curve: i32, affine_xy: &[u64; 8]) -> Result<Self, DehaloError> {
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe { sys::dehalo_fixed_base_create(ctx.as_ptr(), curve, affine_xy.as_ptr(), &mut raw) })?;
        Ok(Self { ctx, raw, owned: true })
    }

    /// `d_out_affine_xy[i] = [d_scalars[i]] P` for `i < count`: affine, `(0, 0)` for the identity.
    ///
    /// # Safety
    /// `d_scalars` (32 B each) and `d_out_affine_xy` (64 B each) are device memory for `count` elements; `stream` is a `hipStream_t` or null.
    pub unsafe fn mul_device(&self, d_scalars: *const u64, count: usize, d_out_affine_xy: *mut u64, stream: *mut core::ffi::c_void) -> Result<(), DehaloError> {
        self.ctx.check(sys::dehalo_fixed_base_mul_device(self.ctx.as_ptr(), self.raw, d_scalars, count, d_out_affine_xy, stream))
    }

    /// `d_jacobian[i] += [d_blinds[i]] P` in place: the blinding term of `ParamsIPA::commit` over the results of one batched MSM.
    ///
    /// # Safety
    /// `d_jacobian` (96 B each, as `dehalo_msm_device` leaves them) and `d_blinds` (32 B each) are device memory for `count` elements.
    pub unsafe fn blind_device(&self, d_jacobian: *mut u64, d_blinds: *const u64, count: usize, stream: *mut core::ffi::c_void) -> Result<(), DehaloError> {
        self.ctx.check(sys::dehalo_fixed_base_blind_device(self.ctx.as_ptr(), self.raw, d_jacobian, d_blinds, count, stream))
    }
}

impl Drop for FixedBase<'_> {
    fn drop(&mut self) {
        if self.owned {
            unsafe { sys::dehalo_fixed_base_release(self.ctx.as_ptr(), self.raw as *mut sys::dehalo_fixed_base) };
        }
    }
}

impl<'c> DehaloParamsIPA<'c> {
    /// `W`'s table, which the params own (`dehalo_params_fixed_base`): borrowed, so it cannot outlive them.
    pub fn fixed_base(&self) -> FixedBase<'_> {
        FixedBase { ctx: self.ctx, raw: unsafe { sys::dehalo_params_fixed_base(self.raw) }, owned: false }
    }
}
