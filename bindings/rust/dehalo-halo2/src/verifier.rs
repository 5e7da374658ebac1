//! `plonk::verify_proof::<KZGCommitmentScheme<Bn256>, VerifierGWC<_> | VerifierSHPLONK<_>, Challenge255<_>, Blake2bRead<_, _, _>, SingleStrategy<_>>` behind the
//! C ABI [UPSTREAM halo2_proofs/src/plonk/verifier.rs @ v2023_04_20; the reference's check of every proof: benches/delay_enc.rs:147-165], and upstream's
//! `BatchVerifier` / `AccumulatorStrategy` as one call.  The verifier holds the verifying half of the params and of the key; made with a context it decompresses
//! the proofs' points and forms the two sums of the reduction on the device, made without one it runs on the host (`dehalo_verifier_create_vk` with a null
//! context: a mode the caller chooses, never a fallback).  The pairing check runs on the host in both.
//!
//! `plonk::verify_proof::<IPACommitmentScheme<EqAffine>, VerifierIPA<_>, Challenge255<_>, Blake2bRead<_, _, _>, SingleStrategy<_>>` is the same verifier type
//! made by `DehaloVerifierIPA::from_vk` (`dehalo_verifier_create_ipa_vk`: `ParamsIPA::read` + `VerifyingKey::read`) and `verify_proof_ipa` below: the instance
//! columns enter as commitments, and acceptance is one multi-scalar multiplication over the params' generators whose scalars are built on the device.
use crate::constraint_system::Descriptor;
use crate::params::{DehaloParamsKZG, SerdeFormat};
use crate::prover::DehaloProvingKey;
use crate::{Context, DehaloError};
use core::ffi::c_void;
use dehalo_sys as sys;
use ff::Field;
use halo2_proofs::plonk::ConstraintSystem;
use halo2curves::bn256::{Fr, G1Affine};
use rand_core::RngCore;
use std::ffi::CStr;

/// Why a proof was not accepted (`dehalo_reject_reason`).
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum Reject {
    /// a read failed, bytes are missing or trail
    Malformed,
    /// the proof was read and the pairing check failed
    Pairing,
    /// IPA: the proof was read and the final sum is not the identity (or `x_3` hit an opening point, or a round challenge was zero)
    Opening,
}

pub struct DehaloVerifier {
    raw: *mut sys::dehalo_verifier,
}

unsafe extern "C" fn fill_from<R: RngCore + Send>(user: *mut c_void, out: *mut u64, count: usize, _position: u64) -> i32 {
    let rng = &mut *(user as *mut R);
    for i in 0..count {
        let s = Fr::random(&mut *rng);
        core::ptr::copy_nonoverlapping(&s as *const Fr as *const u64, out.add(4 * i), 4);
    }
    0
}

impl DehaloVerifier {
    fn check(&self, rc: i32) -> Result<(), DehaloError> {
        if rc == 0 {
            return Ok(());
        }
        let message = unsafe { CStr::from_ptr(sys::dehalo_verifier_last_error(self.raw)) }.to_string_lossy().into_owned();
        Err(DehaloError { code: rc, message })
    }

    /// from the objects a prover holds (`dehalo_verifier_create`): `g[0]`, `g2`, `s_g2`, `k` of the params; the commitments, constraint system and
    /// `transcript_repr` of the key
    pub fn from_pk<'c>(ctx: &'c Context, params: &DehaloParamsKZG<'c>, pk: &DehaloProvingKey<'c>) -> Result<Self, DehaloError> {
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe { sys::dehalo_verifier_create(ctx.as_ptr(), params.as_ptr(), pk.as_ptr(), &mut raw) })?;
        Ok(DehaloVerifier { raw })
    }

    /// `ParamsVerifierKZG` + `VerifyingKey::read(&mut reader, vk_format)`: `g0` = `params.get_g()[0]`, `g2` / `s_g2` = the 128 RawBytes of `params.g2()` /
    /// `params.s_g2()`.  `ctx == None`: a host verifier.  `transcript_repr` starts as the library's substitute: set upstream's with `set_transcript_repr`.
    pub fn from_vk(ctx: Option<&Context>, k: u32, g0: &G1Affine, g2: &[u8; 128], s_g2: &[u8; 128], cs: &ConstraintSystem<Fr>, vk_bytes: &[u8], vk_format: SerdeFormat,
                   num_selectors: u32) -> Result<Self, DehaloError> {
        let d = Descriptor::from_constraint_system(cs);
        let c = d.as_c();
        let mut raw = core::ptr::null_mut();
        let rc = unsafe {
            sys::dehalo_verifier_create_vk(ctx.map_or(core::ptr::null_mut(), |c| c.as_ptr()), sys::DEHALO_CURVE_BN254_G1, k, g0 as *const G1Affine as *const u64, g2.as_ptr(),
                                           s_g2.as_ptr(), &c, vk_bytes.as_ptr(), vk_bytes.len(), vk_format.into(), num_selectors, &mut raw)
        };
        match (rc, ctx) {
            (0, _) => Ok(DehaloVerifier { raw }),
            (_, Some(c)) => c.check(rc).map(|_| unreachable!()),
            (_, None) => {
                // no context to ask: the constructor's own text
                let mut why = [0 as core::ffi::c_char; 512];
                unsafe { sys::dehalo_verifier_create_error(why.as_mut_ptr(), why.len()) };
                Err(DehaloError { code: rc, message: unsafe { CStr::from_ptr(why.as_ptr()) }.to_string_lossy().into_owned() })
            }
        }
    }

    pub fn set_transcript_repr(&mut self, repr: &Fr) -> Result<(), DehaloError> {
        self.check(unsafe { sys::dehalo_verifier_set_transcript_repr(self.raw, repr as *const Fr as *const u64) })
    }

    /// `sys::DEHALO_MULTIOPEN_GWC` (`VerifierGWC`, the default) or `sys::DEHALO_MULTIOPEN_SHPLONK` (`VerifierSHPLONK`)
    pub fn set_multiopen(&mut self, multiopen: i32) -> Result<(), DehaloError> {
        self.check(unsafe { sys::dehalo_verifier_set_multiopen(self.raw, multiopen) })
    }

    /// Where the pairing checks run: `sys::DEHALO_PAIRING_ON_HOST` (the default) or `sys::DEHALO_PAIRING_ON_DEVICE` -- `verify` and `verify_batch` then make their
    /// one check through the kernel, and `verify_each` gives every live proof its own check in ONE launch, without a search (`checks` = the live proofs).
    /// `Err` on a verifier without a context and on an IPA verifier.
    pub fn set_pairing(&mut self, mode: u32) -> Result<(), DehaloError> {
        self.check(unsafe { sys::dehalo_verifier_set_pairing(self.raw, mode as i32) })
    }

    /// `verify_proof(&params, &vk, strategy, &[instances_0, .., instances_{N-1}], &mut transcript)` with `SingleStrategy`: `Ok(Ok(()))` accepted, `Ok(Err(why))`
    /// rejected, `Err(_)` the caller's error (a wrong number of instance columns, a column longer than the usable rows) or the device's.
    pub fn verify(&self, instances: &[&[&[Fr]]], proof: &[u8]) -> Result<Result<(), Reject>, DehaloError> {
        let columns = instances.first().map_or(0, |c| c.len());
        let ptrs: Vec<*const u64> = instances.iter().flat_map(|c| c.iter().map(|col| col.as_ptr() as *const u64)).collect();
        let lens: Vec<usize> = instances.iter().flat_map(|c| c.iter().map(|col| col.len())).collect();
        let (mut accept, mut reason) = (0, 0);
        self.check(unsafe {
            sys::dehalo_verify_proof(self.raw, ptrs.as_ptr(), lens.as_ptr(), columns as u32, instances.len().max(1) as u32, proof.as_ptr(), proof.len(), &mut accept, &mut reason)
        })?;
        Ok(if accept != 0 { Ok(()) } else if reason == sys::DEHALO_REJECT_MALFORMED { Err(Reject::Malformed) } else { Err(Reject::Pairing) })
    }

    /// `BatchVerifier::finalize` / `AccumulatorStrategy`: every proof read, ONE pairing check over the sums weighted by scalars drawn from `rng` -- which must be
    /// unpredictable to whoever made the proofs (`OsRng`).  `instances[i]`: proof i's, as `verify` takes them, every proof over the same number of circuits.
    /// `Ok(Err((why, first_malformed)))`: the index of the first unreadable proof, or -1 when the pairing failed (verify singly to find which).
    pub fn verify_batch<R: RngCore + Send>(&self, instances: &[&[&[&[Fr]]]], proofs: &[&[u8]], rng: &mut R) -> Result<Result<(), (Reject, i64)>, DehaloError> {
        let circuits = instances.first().map_or(1, |p| p.len().max(1));
        let columns = instances.first().and_then(|p| p.first()).map_or(0, |c| c.len());
        let ptrs: Vec<*const u64> = instances.iter().flat_map(|p| p.iter().flat_map(|c| c.iter().map(|col| col.as_ptr() as *const u64))).collect();
        let lens: Vec<usize> = instances.iter().flat_map(|p| p.iter().flat_map(|c| c.iter().map(|col| col.len()))).collect();
        let pp: Vec<*const u8> = proofs.iter().map(|p| p.as_ptr()).collect();
        let pl: Vec<usize> = proofs.iter().map(|p| p.len()).collect();
        let mut r = sys::dehalo_rng { kind: sys::DEHALO_RNG_CALLBACK, pcg_state: [0; 2], pcg_inc: [0; 2], fill: Some(fill_from::<R>), user: rng as *mut R as *mut c_void };
        let (mut accept, mut first) = (0, -1i64);
        self.check(unsafe {
            sys::dehalo_verify_proofs(self.raw, pp.as_ptr(), pl.as_ptr(), pp.len() as u32, ptrs.as_ptr(), lens.as_ptr(), columns as u32, circuits as u32, &mut r, &mut accept, &mut first)
        })?;
        Ok(if accept != 0 { Ok(()) } else if first >= 0 { Err((Reject::Malformed, first)) } else { Err((Reject::Pairing, -1)) })
    }

    /// A verdict per proof from one batch verification (`dehalo_verify_proofs_each`): entry i is `Ok(())` for a valid proof and otherwise what `verify` says of
    /// proof i alone.  Arguments and the warning about `rng` as for `verify_batch`.  The second value is the number of pairing checks made: 1 when every
    /// readable proof is valid, at most `1 + 2 b ceil(log2 n)` for b invalid proofs among n.
    pub fn verify_each<R: RngCore + Send>(&self, instances: &[&[&[&[Fr]]]], proofs: &[&[u8]], rng: &mut R) -> Result<(Vec<Result<(), Reject>>, u32), DehaloError> {
        let circuits = instances.first().map_or(1, |p| p.len().max(1));
        let columns = instances.first().and_then(|p| p.first()).map_or(0, |c| c.len());
        let ptrs: Vec<*const u64> = instances.iter().flat_map(|p| p.iter().flat_map(|c| c.iter().map(|col| col.as_ptr() as *const u64))).collect();
        let lens: Vec<usize> = instances.iter().flat_map(|p| p.iter().flat_map(|c| c.iter().map(|col| col.len()))).collect();
        let pp: Vec<*const u8> = proofs.iter().map(|p| p.as_ptr()).collect();
        let pl: Vec<usize> = proofs.iter().map(|p| p.len()).collect();
        let mut r = sys::dehalo_rng { kind: sys::DEHALO_RNG_CALLBACK, pcg_state: [0; 2], pcg_inc: [0; 2], fill: Some(fill_from::<R>), user: rng as *mut R as *mut c_void };
        let mut reasons = vec![sys::DEHALO_REJECT_NONE; pp.len().max(1)];
        let mut checks = 0u32;
        self.check(unsafe {
            sys::dehalo_verify_proofs_each(self.raw, pp.as_ptr(), pl.as_ptr(), pp.len() as u32, ptrs.as_ptr(), lens.as_ptr(), columns as u32, circuits as u32, &mut r,
                                           reasons.as_mut_ptr(), &mut checks)
        })?;
        let verdicts = reasons[..pp.len()].iter().map(|&why| {
            if why == sys::DEHALO_REJECT_NONE { Ok(()) } else if why == sys::DEHALO_REJECT_MALFORMED { Err(Reject::Malformed) } else { Err(Reject::Pairing) }
        }).collect();
        Ok((verdicts, checks))
    }
}

impl Drop for DehaloVerifier {
    fn drop(&mut self) {
        unsafe { sys::dehalo_verifier_release(self.raw) };
    }
}

/// `verify_proof::<KZGCommitmentScheme<Bn256>, VerifierGWC<_>, ..>` of one proof over one circuit (benches/delay_enc.rs:147-165): `accept`
pub fn verify_proof(verifier: &mut DehaloVerifier, instances: &[&[Fr]], proof: &[u8]) -> Result<bool, DehaloError> {
    verifier.set_multiopen(sys::DEHALO_MULTIOPEN_GWC)?;
    Ok(verifier.verify(&[instances], proof)?.is_ok())
}

/// the same with `VerifierSHPLONK<_>`
pub fn verify_proof_shplonk(verifier: &mut DehaloVerifier, instances: &[&[Fr]], proof: &[u8]) -> Result<bool, DehaloError> {
    verifier.set_multiopen(sys::DEHALO_MULTIOPEN_SHPLONK)?;
    Ok(verifier.verify(&[instances], proof)?.is_ok())
}

/// Many clients prove, one party verifies: a verdict per proof from ONE batch verification (`dehalo_verify_proofs_each`).  `instances[i]`: proof i's instance
/// columns (one circuit a proof); entry i of the result is `true` iff proof i is valid.  `rng` draws the batch weights and must be unpredictable to whoever made
/// the proofs (`OsRng`).  One pairing check when every proof is valid, 13 for one invalid proof among 64 -- against 64 for verifying them singly.
pub fn verify_proofs_each<R: RngCore + Send>(verifier: &DehaloVerifier, instances: &[&[&[Fr]]], proofs: &[&[u8]], rng: &mut R) -> Result<Vec<bool>, DehaloError> {
    let circuits: Vec<[&[&[Fr]]; 1]> = instances.iter().map(|columns| [*columns]).collect();
    let per_proof: Vec<&[&[&[Fr]]]> = circuits.iter().map(|c| &c[..]).collect();
    let (verdicts, _checks) = verifier.verify_each(&per_proof, proofs, rng)?;
    Ok(verdicts.iter().map(|v| v.is_ok()).collect())
}

/// The IPA verifier over Vesta (scalars in `pasta::Fp`): `dehalo_verifier` made by `dehalo_verifier_create_ipa_vk`.  It borrows the params.
pub struct DehaloVerifierIPA<'p, 'c> {
    raw: *mut sys::dehalo_verifier,
    _params: &'p crate::params::DehaloParamsIPA<'c>,
}

impl<'p, 'c> DehaloVerifierIPA<'p, 'c> {
    /// `ParamsIPA::read` + `VerifyingKey::read(&mut reader, vk_format)`: the key's commitments are the blinded ones a key made under `ParamsIPA` holds.
    /// `transcript_repr` starts as the library's substitute: set upstream's with `set_transcript_repr`.
    pub fn from_vk(ctx: &Context, params: &'p crate::params::DehaloParamsIPA<'c>, cs: &ConstraintSystem<halo2curves::pasta::Fp>, vk_bytes: &[u8], vk_format: SerdeFormat,
                   num_selectors: u32) -> Result<Self, DehaloError> {
        let d = Descriptor::from_constraint_system(cs);
        let c = d.as_c();
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe { sys::dehalo_verifier_create_ipa_vk(ctx.as_ptr(), params.raw, &c, vk_bytes.as_ptr(), vk_bytes.len(), vk_format.into(), num_selectors, &mut raw) })?;
        Ok(DehaloVerifierIPA { raw, _params: params })
    }

    fn check(&self, rc: i32) -> Result<(), DehaloError> {
        if rc == 0 {
            return Ok(());
        }
        let message = unsafe { CStr::from_ptr(sys::dehalo_verifier_last_error(self.raw)) }.to_string_lossy().into_owned();
        Err(DehaloError { code: rc, message })
    }

    pub fn set_transcript_repr(&mut self, repr: &halo2curves::pasta::Fp) -> Result<(), DehaloError> {
        self.check(unsafe { sys::dehalo_verifier_set_transcript_repr(self.raw, repr as *const _ as *const u64) })
    }

    /// one proof over one circuit; `instances`: one slice per instance column
    pub fn verify(&self, instances: &[&[halo2curves::pasta::Fp]], proof: &[u8]) -> Result<Result<(), Reject>, DehaloError> {
        let ptrs: Vec<*const u64> = instances.iter().map(|col| col.as_ptr() as *const u64).collect();
        let lens: Vec<usize> = instances.iter().map(|col| col.len()).collect();
        let (mut accept, mut reason) = (0, 0);
        self.check(unsafe { sys::dehalo_verify_proof(self.raw, ptrs.as_ptr(), lens.as_ptr(), ptrs.len() as u32, 1, proof.as_ptr(), proof.len(), &mut accept, &mut reason) })?;
        Ok(if accept != 0 { Ok(()) } else if reason == sys::DEHALO_REJECT_MALFORMED { Err(Reject::Malformed) } else { Err(Reject::Opening) })
    }
}

impl Drop for DehaloVerifierIPA<'_, '_> {
    fn drop(&mut self) {
        unsafe { sys::dehalo_verifier_release(self.raw) };
    }
}

/// `verify_proof::<IPACommitmentScheme<EqAffine>, VerifierIPA<_>, ..>` of one proof over one circuit: `accept`
pub fn verify_proof_ipa(verifier: &DehaloVerifierIPA<'_, '_>, instances: &[&[halo2curves::pasta::Fp]], proof: &[u8]) -> Result<bool, DehaloError> {
    Ok(verifier.verify(instances, proof)?.is_ok())
}
