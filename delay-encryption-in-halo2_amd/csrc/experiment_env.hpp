// experiment_env.hpp -- DH_EXPERIMENT_ENV, for internal.hpp and for the host-only headers that compile without it (msm_plan.hpp).
#pragma once
#include <cstdlib>

// Experiment switches.  The default build reads NO tuning from the environment: DH_EXPERIMENT_ENV("DEHALO_...") is a null pointer there and the name is not even in
// the binary, so an environment variable cannot change which kernels a drop-in library runs (per-context tuning goes through dehalo_ctx_set_tuning, validated).
// A measurement build (`make EXPERIMENTS=1`: -DDEHALO_EXPERIMENTS, what tools/ab_*.sh build) turns them back into getenv and compiles the wall-clock phase stamps in.
// The default build reads three diagnostics, host side only: DEHALO_PROVER_TRACE, DEHALO_SYNTH_TRACE (timelines on stderr), DEHALO_SYNTH_THREADS (witness threads).
#ifdef DEHALO_EXPERIMENTS
#define DH_EXPERIMENT_ENV(name) getenv(name)
#else
#define DH_EXPERIMENT_ENV(name) ((const char*)nullptr)
#endif
