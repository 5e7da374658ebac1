//! The one-call integration: `plonk::create_proof::<KZGCommitmentScheme<Bn256>, ProverGWC<_>, Challenge255<_>, _, Blake2bWrite<_, _, _>, _>` behind the C ABI
//! [UPSTREAM halo2_proofs/src/plonk/prover.rs @ v2023_04_20; the reference's timed call: benches/delay_enc.rs:123-131, benches/mod_pow.rs:201-209,
//! benches/pose_enc.rs:127-135].  From the first advice commitment to the last opening -- phases, Blake2b transcript, blinding, every launch -- in C++
//! (csrc/params.hip, keygen.hip, prover.hip); this module builds the objects and passes pointers, the sequence of `host/example.cpp` (which `tests/test_native.py` runs).
//!
//! The patched `plonk/prover.rs` keeps its signature; its body becomes
//!
//! ```ignore
//! let advice = synthesize_advice(params, pk, circuits, instances)?;          // upstream's own first step, unchanged: WitnessCollection + batch_invert_assigned
//! let proof = DEHALO.with(|h| h.prover.create_proof(&advice, instances[0], &mut rng))?;
//! transcript.write_raw(&proof)                                                // same wire format: 32-byte compressed points, 32-byte LE scalars
//! ```
use crate::constraint_system::Descriptor;
use crate::params::{DehaloParamsKZG, SerdeFormat};
use crate::{Context, DehaloError};
use core::ffi::{c_int, c_void};
use dehalo_sys as sys;
use ff::Field;
use halo2_proofs::plonk::ConstraintSystem;
use halo2curves::bn256::Fr;
use rand_core::RngCore;

/// `ProvingKey<G1Affine>` (with its `VerifyingKey`) on the device.
pub struct DehaloProvingKey<'c> {
    ctx: &'c Context,
    raw: *mut sys::dehalo_pk,
}

impl<'c> DehaloProvingKey<'c> {
    /// `keygen_vk` + `keygen_pk` (benches/delay_enc.rs:86,103): `fixed` = the circuit's fixed columns after selector compression, `num_fixed x 2^k` Montgomery
    /// elements, column after column; `mapping` = the permutation assembly, `columns x 2^k` cells as `column * 2^k + row`; `selectors` only feed `transcript_repr`.
    pub fn keygen(ctx: &'c Context, params: &DehaloParamsKZG<'c>, cs: &ConstraintSystem<Fr>, fixed: &[Fr], mapping: &[u64], selectors: &[Vec<u8>]) -> Result<Self, DehaloError> {
        let d = Descriptor::from_constraint_system(cs);
        let c = d.as_c();
        let sel: Vec<*const u8> = selectors.iter().map(|s| s.as_ptr()).collect();
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe {
            sys::dehalo_keygen(ctx.as_ptr(), params.as_ptr(), &c, fixed.as_ptr() as *const u64, mapping.as_ptr(), sel.as_ptr(), sel.len() as u32, 0, &mut raw)
        })?;
        Ok(DehaloProvingKey { ctx, raw })
    }

    /// `VerifyingKey::read(&mut reader, vk_format)` + `keygen_pk(&params, vk, &circuit)` (benches/delay_enc.rs:96-103): the proving key of these columns UNDER the
    /// verifying key `vk_bytes`.  Its commitments are taken as they are -- not recomputed (no MSM runs) and, as upstream, not compared with the columns; a checked
    /// format validates them (`dehalo_keygen_pk`).
    pub fn keygen_pk(ctx: &'c Context, params: &DehaloParamsKZG<'c>, cs: &ConstraintSystem<Fr>, vk_bytes: &[u8], vk_format: SerdeFormat, num_selectors: u32, fixed: &[Fr],
                     mapping: &[u64]) -> Result<Self, DehaloError> {
        let d = Descriptor::from_constraint_system(cs);
        let c = d.as_c();
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe {
            sys::dehalo_keygen_pk(ctx.as_ptr(), params.as_ptr(), &c, vk_bytes.as_ptr(), vk_bytes.len(), vk_format.into(), num_selectors, fixed.as_ptr() as *const u64,
                                  mapping.as_ptr(), 0, &mut raw)
        })?;
        Ok(DehaloProvingKey { ctx, raw })
    }

    /// `ProvingKey::read::<_, Circuit>(&mut reader, format)` of the file the bench caches (benches/delay_enc.rs:111-115, which passes `SerdeFormat::RawBytes`):
    /// `Processed` decompresses the commitments and converts every element on the device, `RawBytes` checks every point and every element there, and
    /// `RawBytesUnchecked` copies the bytes in unseen (`dehalo_pk_read_custom`).
    pub fn read(ctx: &'c Context, cs: &ConstraintSystem<Fr>, bytes: &[u8], format: SerdeFormat, num_selectors: u32) -> Result<Self, DehaloError> {
        let d = Descriptor::from_constraint_system(cs);
        let c = d.as_c();
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe {
            sys::dehalo_pk_read_custom(ctx.as_ptr(), sys::DEHALO_CURVE_BN254_G1, &c, bytes.as_ptr(), bytes.len(), format.into(), num_selectors, &mut raw)
        })?;
        Ok(DehaloProvingKey { ctx, raw })
    }

    /// `pk.write(&mut writer, format)` (`:105`); both raw formats write the same bytes (`dehalo_pk_write_custom`)
    pub fn write(&self, format: SerdeFormat) -> Result<Vec<u8>, DehaloError> {
        let mut out = vec![0u8; unsafe { sys::dehalo_pk_size_custom(self.raw, format.into()) }];
        self.ctx.check(unsafe { sys::dehalo_pk_write_custom(self.ctx.as_ptr(), self.raw, format.into(), out.as_mut_ptr(), out.len()) })?;
        Ok(out)
    }

    /// `vk.write(&mut writer, format)` (`:88`) (`dehalo_vk_write_custom`)
    pub fn vk_write(&self, format: SerdeFormat) -> Result<Vec<u8>, DehaloError> {
        let mut out = vec![0u8; unsafe { sys::dehalo_vk_size_custom(self.raw, format.into()) }];
        self.ctx.check(unsafe { sys::dehalo_vk_write_custom(self.ctx.as_ptr(), self.raw, format.into(), out.as_mut_ptr(), out.len()) })?;
        Ok(out)
    }

    pub fn as_ptr(&self) -> *const sys::dehalo_pk {
        self.raw
    }

    /// upstream derives `vk.transcript_repr` from Rust `Debug` text, so it is passed in: with upstream's value set, the first absorbed scalar is upstream's
    pub fn set_transcript_repr(&mut self, repr: &Fr) -> Result<(), DehaloError> {
        self.ctx.check(unsafe { sys::dehalo_pk_set_transcript_repr(self.raw, repr as *const Fr as *const u64) })
    }

    /// `MockProver::run(k, &circuit, instances)?.verify()` over this key, on the device (`dehalo_check_witness`): `advice` and `instances` as `create_proof` takes
    /// them, `mapping` = keygen's permutation assembly (`None`: the copy constraints are not checked).  Returns the exact totals and the first `cap` failures in
    /// `(kind, index, row)` order: `DEHALO_CHECK_GATE` indexes `cs.gates().flat_map(polynomials)`, `DEHALO_CHECK_LOOKUP` `cs.lookups()`, `DEHALO_CHECK_COPY`
    /// `cs.permutation().get_columns()`; the witness satisfies the circuit when the three totals are zero.  Naming a failure (gate name, region, offset) is the
    /// caller's, from its own `ConstraintSystem` and layouter.
    pub fn mock_verify(&self, advice: &[Fr], instances: &[&[Fr]], mapping: Option<&[u64]>, cap: usize) -> Result<(sys::dehalo_check_report, Vec<sys::dehalo_check_failure>), DehaloError> {
        let inst_ptrs: Vec<*const u64> = instances.iter().map(|c| c.as_ptr() as *const u64).collect();
        let inst_lens: Vec<usize> = instances.iter().map(|c| c.len()).collect();
        let mut report: sys::dehalo_check_report = unsafe { core::mem::zeroed() };
        let mut failures: Vec<sys::dehalo_check_failure> = Vec::with_capacity(cap);
        self.ctx.check(unsafe {
            sys::dehalo_check_witness(self.ctx.as_ptr(), self.raw, advice.as_ptr() as *const u64, inst_ptrs.as_ptr(), inst_lens.as_ptr(), inst_ptrs.len() as u32,
                                      mapping.map_or(core::ptr::null(), |m| m.as_ptr()), 0, if cap == 0 { core::ptr::null_mut() } else { failures.as_mut_ptr() }, cap, &mut report)
        })?;
        unsafe { failures.set_len(report.written as usize) };
        Ok((report, failures))
    }
}

impl Drop for DehaloProvingKey<'_> {
    fn drop(&mut self) {
        unsafe { sys::dehalo_pk_release(self.ctx.as_ptr(), self.raw) };
    }
}

/// `dehalo_rng` with `DEHALO_RNG_CALLBACK`: blinding scalars are drawn from the caller's `RngCore` in upstream's order.  (The random polynomial's `n` scalars are
/// requested early, from a helper thread, with their `position` in that order: a generator that cannot seek sees them out of order -- the proof is equally valid;
/// byte identity with a CPU run of the same seeded generator needs a seekable one, which `DEHALO_RNG_PCG64` is.)
/// `R: Send`: include/dehalo.h lets the library call `fill` from a helper thread of its own, so the generator crosses threads (`ThreadRng` is refused at compile time).
unsafe extern "C" fn fill_from<R: RngCore + Send>(user: *mut c_void, out: *mut u64, count: usize, _position: u64) -> i32 {
    let rng = &mut *(user as *mut R);
    for i in 0..count {
        let s = Fr::random(&mut *rng);
        core::ptr::copy_nonoverlapping(&s as *const Fr as *const u64, out.add(4 * i), 4);
    }
    0
}

/// Device buffers of ONE proof in flight, reused by every `create_proof` on it; `side` = a second context whose stream runs the NTTs and the random
/// polynomial's commitment beside the commitment phases.
pub struct DehaloProver<'c> {
    ctx: &'c Context,
    raw: *mut sys::dehalo_prover,
}

impl<'c> DehaloProver<'c> {
    pub fn new(ctx: &'c Context, side: Option<&'c Context>, params: &DehaloParamsKZG<'c>, pk: &DehaloProvingKey<'c>) -> Result<Self, DehaloError> {
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe { sys::dehalo_prover_create(ctx.as_ptr(), side.map_or(core::ptr::null_mut(), |s| s.as_ptr()), params.as_ptr(), pk.raw, &mut raw) })?;
        Ok(DehaloProver { ctx, raw })
    }

    /// A prover whose proofs are over `num_circuits` circuits of the key (`dehalo_prover_create_multi`): what `create_proof`'s `&[circuit_0, .., circuit_{N-1}]`
    /// needs.  KZG, one advice phase; `new` is its `num_circuits == 1` case.  With more than one circuit only `create_proof_multi` proves on it.
    pub fn new_multi(ctx: &'c Context, side: Option<&'c Context>, params: &DehaloParamsKZG<'c>, pk: &DehaloProvingKey<'c>, num_circuits: u32) -> Result<Self, DehaloError> {
        let mut raw = core::ptr::null_mut();
        ctx.check(unsafe {
            sys::dehalo_prover_create_multi(ctx.as_ptr(), side.map_or(core::ptr::null_mut(), |s| s.as_ptr()), params.as_ptr(), pk.raw, num_circuits, &mut raw)
        })?;
        Ok(DehaloProver { ctx, raw })
    }

    /// ONE proof on several GPUs (`dehalo_prover_set_shard`): of every multi-column commitment phase this process runs the MSMs of its share of the columns only and
    /// `gather` (an all-gather of at most ten affine points over RCCL / xGMI, see include/dehalo.h) fills in the rest; every process must then call `create_proof`
    /// with the same advice, instances and the same seeded generator.  `world == 1` switches it off.
    ///
    /// # Safety
    /// `gather` is called on the proving thread with `user`; both must stay valid for as long as the prover may prove.
    pub unsafe fn set_shard(&self, rank: u32, world: u32, gather: sys::dehalo_gather_fn, user: *mut c_void) -> Result<(), DehaloError> {
        self.ctx.check(sys::dehalo_prover_set_shard(self.raw, rank, world, gather, user))
    }

    /// Which KZG multiopen the proofs carry (`dehalo_prover_set_multiopen`): `sys::DEHALO_MULTIOPEN_GWC` (`ProverGWC`, the default) or
    /// `sys::DEHALO_MULTIOPEN_SHPLONK` (`ProverSHPLONK`: two commitments whatever the circuit's rotations are).  Everything up to the evaluations is the same proof.
    pub fn set_multiopen(&self, multiopen: i32) -> Result<(), DehaloError> {
        self.ctx.check(unsafe { sys::dehalo_prover_set_multiopen(self.raw, multiopen) })
    }

    /// `create_proof(&params, &pk, &[circuit], &[instances], rng, &mut transcript)` for ONE circuit: `advice` = what `circuit.synthesize` assigned
    /// (`num_advice x 2^k` Montgomery elements, column after column, host memory); returns the transcript bytes (`transcript.finalize()`).
    pub fn create_proof<R: RngCore + Send>(&self, advice: &[Fr], instances: &[&[Fr]], rng: &mut R) -> Result<Vec<u8>, DehaloError> {
        let inst_ptrs: Vec<*const u64> = instances.iter().map(|c| c.as_ptr() as *const u64).collect();
        let inst_lens: Vec<usize> = instances.iter().map(|c| c.len()).collect();
        let mut r = sys::dehalo_rng { kind: sys::DEHALO_RNG_CALLBACK, pcg_state: [0; 2], pcg_inc: [0; 2], fill: Some(fill_from::<R>), user: rng as *mut R as *mut c_void };
        let mut t = core::ptr::null_mut();
        self.ctx.check(unsafe { sys::dehalo_transcript_create(sys::DEHALO_CURVE_BN254_G1, &mut t) })?;
        let rc = unsafe {
            sys::dehalo_create_proof(self.raw, advice.as_ptr() as *const u64, inst_ptrs.as_ptr(), inst_lens.as_ptr(), inst_ptrs.len() as u32, &mut r, t, 0)
        };
        let out = if rc == 0 {
            let mut bytes = vec![0u8; unsafe { sys::dehalo_transcript_len(t) }];
            let rc2 = unsafe { sys::dehalo_transcript_finalize(t, bytes.as_mut_ptr(), bytes.len()) };
            if rc2 == 0 { Ok(bytes) } else { self.ctx.check(rc2).map(|_| vec![]) }
        } else {
            self.ctx.check(rc).map(|_| vec![])
        };
        unsafe { sys::dehalo_transcript_release(t) };
        out
    }

    /// `create_proof(&params, &pk, &[circuit_0, .., circuit_{N-1}], &[instances_0, ..], rng, &mut transcript)`: ONE proof over `advice.len()` circuits of the key
    /// (`dehalo_create_proof_multi`) on a prover of `new_multi` with that many.  `advice[c]` / `instances[c]`: circuit c's, as `create_proof` takes them; every
    /// circuit brings the key's number of instance columns.  Returns the transcript bytes.
    pub fn create_proof_multi<R: RngCore + Send>(&self, advice: &[&[Fr]], instances: &[&[&[Fr]]], rng: &mut R) -> Result<Vec<u8>, DehaloError> {
        let columns = instances.first().map_or(0, |c| c.len());
        if instances.len() != advice.len() || instances.iter().any(|c| c.len() != columns) {
            return self.ctx.check(sys::DEHALO_ERR_INVALID).map(|_| vec![]);
        }
        let adv_ptrs: Vec<*const u64> = advice.iter().map(|a| a.as_ptr() as *const u64).collect();
        let inst_ptrs: Vec<*const u64> = instances.iter().flat_map(|c| c.iter().map(|col| col.as_ptr() as *const u64)).collect();
        let inst_lens: Vec<usize> = instances.iter().flat_map(|c| c.iter().map(|col| col.len())).collect();
        let mut r = sys::dehalo_rng { kind: sys::DEHALO_RNG_CALLBACK, pcg_state: [0; 2], pcg_inc: [0; 2], fill: Some(fill_from::<R>), user: rng as *mut R as *mut c_void };
        let mut t = core::ptr::null_mut();
        self.ctx.check(unsafe { sys::dehalo_transcript_create(sys::DEHALO_CURVE_BN254_G1, &mut t) })?;
        let rc = unsafe {
            sys::dehalo_create_proof_multi(self.raw, adv_ptrs.as_ptr(), inst_ptrs.as_ptr(), inst_lens.as_ptr(), columns as u32, adv_ptrs.len() as u32, &mut r, t, 0)
        };
        let out = if rc == 0 {
            let mut bytes = vec![0u8; unsafe { sys::dehalo_transcript_len(t) }];
            let rc2 = unsafe { sys::dehalo_transcript_finalize(t, bytes.as_mut_ptr(), bytes.len()) };
            if rc2 == 0 { Ok(bytes) } else { self.ctx.check(rc2).map(|_| vec![]) }
        } else {
            self.ctx.check(rc).map(|_| vec![])
        };
        unsafe { sys::dehalo_transcript_release(t) };
        out
    }

    /// `create_proof` for a circuit with later-phase advice columns (`advice_column_in(SecondPhase)`, `challenge_usable_after`): upstream synthesizes the circuit once
    /// per phase, each time with the challenges squeezed so far; here `witness(phase, challenges)` plays that part (`dehalo_create_proof_phased`).  It is called
    /// once per phase on this thread -- for phase p > 0 after the commitments of phase p - 1 are in the transcript -- with every challenge of the circuit by index
    /// (those not squeezed yet are zero) and returns all `num_advice x 2^k` elements, of which the columns of `phase` are read.  The returned slice must stay valid
    /// and unchanged until the next call of `witness` or the return of this function; `witness` must not use this prover.  `Err(code)` from `witness` (code != 0)
    /// ends the proof with `DEHALO_ERR_INVALID`; the prover is usable afterwards.  On a one-phase key this writes `create_proof`'s bytes.
    pub fn create_proof_phased<'a, R: RngCore + Send, W: FnMut(u32, &[Fr]) -> Result<&'a [Fr], i32>>(&self, mut witness: W, instances: &[&[Fr]], rng: &mut R) -> Result<Vec<u8>, DehaloError> {
        unsafe extern "C" fn thunk<'a, W: FnMut(u32, &[Fr]) -> Result<&'a [Fr], i32>>(user: *mut c_void, phase: u32, challenges: *const u64, count: u32, advice: *mut *const u64) -> c_int {
            let w = &mut *(user as *mut W);
            let ch: &[Fr] = if count == 0 { &[] } else { core::slice::from_raw_parts(challenges as *const Fr, count as usize) };
            // (a panic must not unwind through the C frames)
            match std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| w(phase, ch))) {
                Ok(Ok(adv)) => { *advice = adv.as_ptr() as *const u64; 0 }
                Ok(Err(code)) => if code != 0 { code } else { 1 },
                Err(_) => 1,
            }
        }
        let inst_ptrs: Vec<*const u64> = instances.iter().map(|c| c.as_ptr() as *const u64).collect();
        let inst_lens: Vec<usize> = instances.iter().map(|c| c.len()).collect();
        let mut r = sys::dehalo_rng { kind: sys::DEHALO_RNG_CALLBACK, pcg_state: [0; 2], pcg_inc: [0; 2], fill: Some(fill_from::<R>), user: rng as *mut R as *mut c_void };
        let mut t = core::ptr::null_mut();
        self.ctx.check(unsafe { sys::dehalo_transcript_create(sys::DEHALO_CURVE_BN254_G1, &mut t) })?;
        let rc = unsafe {
            sys::dehalo_create_proof_phased(self.raw, Some(thunk::<W>), &mut witness as *mut W as *mut c_void, inst_ptrs.as_ptr(), inst_lens.as_ptr(), inst_ptrs.len() as u32, &mut r, t, 0)
        };
        let out = if rc == 0 {
            let mut bytes = vec![0u8; unsafe { sys::dehalo_transcript_len(t) }];
            let rc2 = unsafe { sys::dehalo_transcript_finalize(t, bytes.as_mut_ptr(), bytes.len()) };
            if rc2 == 0 { Ok(bytes) } else { self.ctx.check(rc2).map(|_| vec![]) }
        } else {
            self.ctx.check(rc).map(|_| vec![])
        };
        unsafe { sys::dehalo_transcript_release(t) };
        out
    }

    /// The reference's call shape in one entry point: the circuit's own inputs instead of its advice columns -- synthesized inside the call by the library's restatement
    /// of the three circuits (csrc/witness.hip: halo2wrong's layout instruction by instruction, unverified cell for cell against the crates -- pair it with a key from `keygen` over ITS fixed columns: `dehalo_synthesize`).
    pub fn create_proof_circuit<R: RngCore + Send>(&self, inputs: &sys::dehalo_circuit_inputs, rng: &mut R) -> Result<(Vec<u8>, sys::dehalo_synthesis_info), DehaloError> {
        let mut r = sys::dehalo_rng { kind: sys::DEHALO_RNG_CALLBACK, pcg_state: [0; 2], pcg_inc: [0; 2], fill: Some(fill_from::<R>), user: rng as *mut R as *mut c_void };
        let mut info: sys::dehalo_synthesis_info = unsafe { core::mem::zeroed() };
        let mut t = core::ptr::null_mut();
        self.ctx.check(unsafe { sys::dehalo_transcript_create(sys::DEHALO_CURVE_BN254_G1, &mut t) })?;
        let empty: [*const u64; 1] = [core::ptr::null()];
        let lens: [usize; 1] = [0];
        let rc = unsafe { sys::dehalo_create_proof_circuit(self.raw, inputs, &mut info, empty.as_ptr(), lens.as_ptr(), 1, &mut r, t) };
        let out = if rc == 0 {
            let mut bytes = vec![0u8; unsafe { sys::dehalo_transcript_len(t) }];
            let rc2 = unsafe { sys::dehalo_transcript_finalize(t, bytes.as_mut_ptr(), bytes.len()) };
            if rc2 == 0 { Ok((bytes, info)) } else { self.ctx.check(rc2).map(|_| (vec![], info)) }
        } else {
            self.ctx.check(rc).map(|_| (vec![], info))
        };
        unsafe { sys::dehalo_transcript_release(t) };
        out
    }

    /// milliseconds of the last proof by phase: advice, lookups, products, random, quotient, evaluations, openings, total
    pub fn last_timings(&self) -> Result<[f64; 8], DehaloError> {
        let mut t = [0f64; 8];
        self.ctx.check(unsafe { sys::dehalo_prover_last_timings(self.raw, t.as_mut_ptr()) })?;
        Ok(t)
    }
}

impl Drop for DehaloProver<'_> {
    fn drop(&mut self) {
        unsafe { sys::dehalo_prover_release(self.raw) };
    }
}

/// The bench's flow end to end (benches/delay_enc.rs:41-54, 84-131) for a caller that holds upstream's objects: SRS file bytes, the circuit's constraint system, its
/// fixed columns / permutation mapping, the advice columns of one proof.  One-time objects are built once and reused by the caller; shown as one function for the reader.
pub fn create_proof<R: RngCore + Send>(device: i32, params_raw_bytes: &[u8], cs: &ConstraintSystem<Fr>, fixed: &[Fr], mapping: &[u64], selectors: &[Vec<u8>],
                                transcript_repr: &Fr, advice: &[Fr], instances: &[&[Fr]], rng: &mut R) -> Result<Vec<u8>, DehaloError> {
    let ctx = Context::new(device)?;
    let side = Context::with_priority(device, 1)?;
    let params = DehaloParamsKZG::read(&ctx, params_raw_bytes)?;
    let mut pk = DehaloProvingKey::keygen(&ctx, &params, cs, fixed, mapping, selectors)?;
    pk.set_transcript_repr(transcript_repr)?;
    let prover = DehaloProver::new(&ctx, Some(&side), &params, &pk)?;
    prover.create_proof(advice, instances, rng)
}

/// The same flow for `plonk::create_proof::<KZGCommitmentScheme<Bn256>, ProverSHPLONK<_>, Challenge255<_>, _, Blake2bWrite<_, _, _>, _>`: one more call on the
/// prover; verify with `VerifierSHPLONK`.
pub fn create_proof_shplonk<R: RngCore + Send>(device: i32, params_raw_bytes: &[u8], cs: &ConstraintSystem<Fr>, fixed: &[Fr], mapping: &[u64], selectors: &[Vec<u8>],
                                        transcript_repr: &Fr, advice: &[Fr], instances: &[&[Fr]], rng: &mut R) -> Result<Vec<u8>, DehaloError> {
    let ctx = Context::new(device)?;
    let side = Context::with_priority(device, 1)?;
    let params = DehaloParamsKZG::read(&ctx, params_raw_bytes)?;
    let mut pk = DehaloProvingKey::keygen(&ctx, &params, cs, fixed, mapping, selectors)?;
    pk.set_transcript_repr(transcript_repr)?;
    let prover = DehaloProver::new(&ctx, Some(&side), &params, &pk)?;
    prover.set_multiopen(sys::DEHALO_MULTIOPEN_SHPLONK as i32)?;
    prover.create_proof(advice, instances, rng)
}

unsafe extern "C" fn fill_from_fp<R: RngCore + Send>(user: *mut c_void, out: *mut u64, count: usize, _position: u64) -> i32 {
    let rng = &mut *(user as *mut R);
    for i in 0..count {
        let s = halo2curves::pasta::Fp::random(&mut *rng);
        core::ptr::copy_nonoverlapping(&s as *const _ as *const u64, out.add(4 * i), 4);
    }
    0
}

/// `plonk::create_proof::<IPACommitmentScheme<EqAffine>, ProverIPA<_>, Challenge255<_>, _, Blake2bWrite<_, _, _>, _>` for ONE circuit over
/// `DehaloParamsIPA` (Vesta; scalars in `pasta::Fp`): keygen, prover and proof through the same three C calls as the KZG flow above -- the params'
/// scheme selects ProverIPA inside `dehalo_create_proof` (blinded commitments, committed instance columns, the multiopen, the opening argument).
/// The verifying key this keygen makes commits the fixed and permutation columns with `Blind::default()` taken as `Blind(F::ONE)` (INTEGRATION.md
/// section 7: parity with upstream unpinned).  Returns the transcript bytes; their length is `dehalo_prover_proof_size`.
pub fn create_proof_ipa<R: RngCore + Send>(ctx: &Context, side: Option<&Context>, params: &crate::params::DehaloParamsIPA<'_>,
                                           cs: &ConstraintSystem<halo2curves::pasta::Fp>, fixed: &[halo2curves::pasta::Fp], mapping: &[u64], selectors: &[Vec<u8>],
                                           transcript_repr: &halo2curves::pasta::Fp, advice: &[halo2curves::pasta::Fp], instances: &[&[halo2curves::pasta::Fp]],
                                           rng: &mut R) -> Result<Vec<u8>, DehaloError> {
    let d = Descriptor::from_constraint_system(cs);
    let c = d.as_c();
    let sel: Vec<*const u8> = selectors.iter().map(|s| s.as_ptr()).collect();
    let mut pk = core::ptr::null_mut();
    ctx.check(unsafe { sys::dehalo_keygen(ctx.as_ptr(), params.raw, &c, fixed.as_ptr() as *const u64, mapping.as_ptr(), sel.as_ptr(), sel.len() as u32, 0, &mut pk) })?;
    let mut prover = core::ptr::null_mut();
    let mut t = core::ptr::null_mut();
    let inst_ptrs: Vec<*const u64> = instances.iter().map(|c| c.as_ptr() as *const u64).collect();
    let inst_lens: Vec<usize> = instances.iter().map(|c| c.len()).collect();
    let mut r = sys::dehalo_rng { kind: sys::DEHALO_RNG_CALLBACK, pcg_state: [0; 2], pcg_inc: [0; 2], fill: Some(fill_from_fp::<R>), user: rng as *mut R as *mut c_void };
    let run = (|| {
        ctx.check(unsafe { sys::dehalo_pk_set_transcript_repr(pk, transcript_repr as *const _ as *const u64) })?;
        ctx.check(unsafe { sys::dehalo_prover_create(ctx.as_ptr(), side.map_or(core::ptr::null_mut(), |s| s.as_ptr()), params.raw, pk, &mut prover) })?;
        ctx.check(unsafe { sys::dehalo_transcript_create(sys::DEHALO_CURVE_VESTA, &mut t) })?;
        ctx.check(unsafe {
            sys::dehalo_create_proof(prover, advice.as_ptr() as *const u64, inst_ptrs.as_ptr(), inst_lens.as_ptr(), inst_ptrs.len() as u32, &mut r, t, 0)
        })?;
        let mut bytes = vec![0u8; unsafe { sys::dehalo_transcript_len(t) }];
        debug_assert_eq!(bytes.len(), unsafe { sys::dehalo_prover_proof_size(prover) });
        ctx.check(unsafe { sys::dehalo_transcript_finalize(t, bytes.as_mut_ptr(), bytes.len()) })?;
        Ok(bytes)
    })();
    unsafe {
        if !t.is_null() { sys::dehalo_transcript_release(t); }
        if !prover.is_null() { sys::dehalo_prover_release(prover); }
        sys::dehalo_pk_release(ctx.as_ptr(), pk);
    }
    run
}
