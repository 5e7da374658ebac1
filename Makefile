# Builds libdehalo.so (HIP, gfx950 only; one translation unit per curve / field so that
# `make -j` compiles them in parallel) and the oracle (test infrastructure).
HIPCC ?= /opt/rocm/bin/hipcc
PKG := delay-encryption-in-halo2_amd
CSRC := $(PKG)/csrc
# make EXPERIMENTS=1 builds into its own object directory and library file: objects do not depend on the flags, so sharing a directory would let a later plain
# `make` link stale -DDEHALO_EXPERIMENTS objects into the shipped library (and the reverse)
ifdef EXPERIMENTS
OBJDIR ?= gpurun_out/ab/exp/obj
LIB ?= gpurun_out/ab/exp/libdehalo.so
endif
OBJDIR ?= $(CSRC)/obj
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-function -Werror=unused-variable -Werror=pass-failed -ffp-contract=off
# make EXPERIMENTS=1: the measurement build (tools/ab_*.sh) -- A/B switches read from the environment and wall-clock phase stamps in the kernels (csrc/internal.hpp)
ifdef EXPERIMENTS
HIPFLAGS += -DDEHALO_EXPERIMENTS
endif
LIB ?= $(PKG)/libdehalo.so
UNITS := capi params transcript ipa_open keygen prover verify pairing check witness lookup_permute msm_bn254 msm_pallas msm_vesta ntt_bn254_fr ntt_bn254_fq ntt_pasta_fp ntt_pasta_fq
OBJS := $(UNITS:%=$(OBJDIR)/%.o)
HDRS := $(wildcard $(CSRC)/*.cuh) $(wildcard $(CSRC)/*.h) $(wildcard $(CSRC)/*.hpp) include/dehalo.h

all: $(LIB) oracle host_example

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=gfx950 -shared -o $@ $(OBJS) -Wl,-rpath,/opt/rocm/lib -lpthread

oracle:
	$(MAKE) -C oracle liboracle.so

host_example: $(LIB) $(PKG)/host/halo2_backend.hpp $(PKG)/host/example.cpp
	g++ -std=c++17 -O1 -Wall -o $(PKG)/host/example $(PKG)/host/example.cpp -L$(PKG) -ldehalo -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath,/opt/rocm/lib

# the host-only code (witness generation, field arithmetic, Blake2b, random scalars) under AddressSanitizer + UndefinedBehaviorSanitizer (g++, no device needed)
host_sanitize: tests/native_host/host_sanitize.cpp $(CSRC)/witness.hip $(HDRS)
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -x c++ -o tests/native_host/host_sanitize tests/native_host/host_sanitize.cpp -x c++ $(CSRC)/witness.hip

host_tsan: tests/native_host/host_sanitize.cpp $(CSRC)/witness.hip $(HDRS)
	g++ -std=c++17 -O1 -g -fsanitize=thread -x c++ -o tests/native_host/host_tsan tests/native_host/host_sanitize.cpp -x c++ $(CSRC)/witness.hip -lpthread

# the MSM's launch planner (csrc/msm_plan.hpp: no HIP headers) swept over shapes and tunings under the same sanitizers
msm_plan_check: tests/native_host/msm_plan_check.cpp $(CSRC)/msm_plan.hpp $(CSRC)/experiment_env.hpp $(CSRC)/field_constants.h
	g++ -std=c++17 -O2 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/msm_plan_check tests/native_host/msm_plan_check.cpp

# the prover's opening plan (csrc/opening_plan.hpp: host only) printed for the shapes on stdin under the same sanitizers (tests/test_opening_plan.py reads it);
# -O0: the program runs for milliseconds, and builds in a fifth of the time
opening_plan_check: tests/native_host/opening_plan_check.cpp $(CSRC)/opening_plan.hpp
	g++ -std=c++17 -O0 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/opening_plan_check tests/native_host/opening_plan_check.cpp

# the same plan for proofs over several circuits of one key (tests/test_multi_circuit.py reads it)
opening_plan_multi_check: tests/native_host/opening_plan_multi_check.cpp $(CSRC)/opening_plan.hpp
	g++ -std=c++17 -O0 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/opening_plan_multi_check tests/native_host/opening_plan_multi_check.cpp

# the constraint system on the host (csrc/plonk_host.hpp: no HIP headers) with phases and challenges, under the same sanitizers (tests/test_phases_host.py runs it)
host_cs_check: tests/native_host/host_cs_check.cpp $(CSRC)/plonk_host.hpp $(CSRC)/key_format.hpp $(CSRC)/g1_host.hpp $(CSRC)/hostfield.hpp
	g++ -std=c++17 -O0 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/host_cs_check tests/native_host/host_cs_check.cpp

clean:
	rm -rf $(LIB) $(OBJDIR) $(PKG)/host/example; $(MAKE) -C oracle clean
# the shuffle argument on the host (plonk_host.hpp, opening_plan.hpp) under ASan + UBSan (tests/test_shuffle.py)
shuffle_cs_check: tests/native_host/shuffle_cs_check.cpp $(CSRC)/plonk_host.hpp $(CSRC)/key_format.hpp $(CSRC)/g1_host.hpp $(CSRC)/hostfield.hpp $(CSRC)/opening_plan.hpp
	g++ -std=c++17 -O0 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/shuffle_cs_check tests/native_host/shuffle_cs_check.cpp

# the acceptance step of the ChaCha20 generator kinds (csrc/hostrng.hpp, shared by the host and the kernel) on crafted candidates, and HostRng's keyed kind,
# under ASan + UBSan (tests/test_rng_chacha.py)
hostrng_check: tests/native_host/hostrng_check.cpp $(CSRC)/hostrng.hpp $(CSRC)/hostfield.hpp include/dehalo.h
	g++ -std=c++17 -O0 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/hostrng_check tests/native_host/hostrng_check.cpp

# ParamsKZG's on-disk formats (csrc/params_format.hpp: host only): layouts, the header of untrusted bytes and the G2 codec, under ASan + UBSan
# (tests/test_params_format_host.py compares it with the Python mirror)
params_format_check: tests/native_host/params_format_check.cpp $(CSRC)/params_format.hpp $(CSRC)/g1_host.hpp $(CSRC)/hostfield.hpp $(CSRC)/field_constants.h include/dehalo.h
	g++ -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/params_format_check tests/native_host/params_format_check.cpp

# VerifyingKey / ProvingKey on disk (csrc/key_format.hpp: host only): layouts, the header, the length and the count / length words of untrusted bytes, under
# ASan + UBSan (tests/test_key_format_host.py compares it with the Python mirror)
key_format_check: tests/native_host/key_format_check.cpp $(CSRC)/key_format.hpp $(CSRC)/g1_host.hpp $(CSRC)/hostfield.hpp $(CSRC)/field_constants.h include/dehalo.h
	g++ -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/key_format_check tests/native_host/key_format_check.cpp

# the BN254 pairing check (csrc/pairing_host.hpp: host only) under ASan + UBSan (tests/test_pairing_host.py compares its verdicts with the oracle's and the library's)
pairing_check: tests/native_host/pairing_check.cpp $(CSRC)/pairing_host.hpp $(CSRC)/params_format.hpp $(CSRC)/g1_host.hpp $(CSRC)/hostfield.hpp $(CSRC)/field_constants.h include/dehalo.h
	g++ -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/pairing_check tests/native_host/pairing_check.cpp

# verify_proof on the host (csrc/verify_host.hpp: host only) on proofs the test writes to a file, under ASan + UBSan (tests/test_verify_host.py)
verify_host_check: tests/native_host/verify_host_check.cpp tests/native_host/verify_case_reader.hpp $(CSRC)/verify_host.hpp $(CSRC)/blame_search.hpp $(CSRC)/pairing_host.hpp $(CSRC)/transcript_host.hpp $(CSRC)/opening_plan.hpp $(CSRC)/plonk_host.hpp $(CSRC)/key_format.hpp $(CSRC)/params_format.hpp $(CSRC)/g1_host.hpp $(CSRC)/hostfield.hpp $(CSRC)/blake2b.hpp $(CSRC)/field_constants.h include/dehalo.h
	g++ -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/verify_host_check tests/native_host/verify_host_check.cpp

# verify_proof for IPA on the host (the same header, its IPA reduction and the host sums over g and g_lagrange) on proofs the test writes to a file, under ASan + UBSan
# (tests/test_verify_ipa_host.py)
verify_ipa_host_check: tests/native_host/verify_ipa_host_check.cpp tests/native_host/verify_case_reader.hpp $(CSRC)/verify_host.hpp $(CSRC)/blame_search.hpp $(CSRC)/pairing_host.hpp $(CSRC)/transcript_host.hpp $(CSRC)/opening_plan.hpp $(CSRC)/plonk_host.hpp $(CSRC)/key_format.hpp $(CSRC)/params_format.hpp $(CSRC)/g1_host.hpp $(CSRC)/hostfield.hpp $(CSRC)/blake2b.hpp $(CSRC)/field_constants.h include/dehalo.h
	g++ -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/verify_ipa_host_check tests/native_host/verify_ipa_host_check.cpp

# G1 points on the host (csrc/g1_host.hpp: the codec of one point, the status texts, the group law) against the transcript's proof bytes, under ASan + UBSan
# (tests/test_g1_host.py runs it)
g1_host_check: tests/native_host/g1_host_check.cpp $(CSRC)/g1_host.hpp $(CSRC)/transcript_host.hpp $(CSRC)/blake2b.hpp $(CSRC)/hostfield.hpp $(CSRC)/field_constants.h include/dehalo.h
	g++ -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/g1_host_check tests/native_host/g1_host_check.cpp

# the units of witness generation below dehalo_synthesize (csrc/bigint_host.hpp, poseidon_host.hpp, maingate_host.hpp: host only) on the cases on stdin, under
# ASan + UBSan (tests/test_witness.py feeds it Knuth's add-back cases, the reference's Poseidon vectors and the RangeChip tables); -O0 as for opening_plan_check
witness_units_check: tests/native_host/witness_units_check.cpp $(CSRC)/bigint_host.hpp $(CSRC)/poseidon_host.hpp $(CSRC)/maingate_host.hpp $(CSRC)/hostfield.hpp $(CSRC)/field_constants.h include/dehalo.h
	g++ -std=c++17 -O0 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/witness_units_check tests/native_host/witness_units_check.cpp

# the search behind dehalo_verify_proofs_each (csrc/blame_search.hpp: host only) over every bad set of up to 12 members, under ASan + UBSan
# (tests/test_blame_search_host.py runs it); -O0 as for opening_plan_check
blame_search_check: tests/native_host/blame_search_check.cpp $(CSRC)/blame_search.hpp
	g++ -std=c++17 -O0 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/blame_search_check tests/native_host/blame_search_check.cpp

# the line tables of fixed G2 points (csrc/pairing_host.hpp: line_table, miller_table) against miller() word for word, under ASan + UBSan
# (tests/test_pairing_lines_host.py runs it)
pairing_lines_check: tests/native_host/pairing_lines_check.cpp $(CSRC)/pairing_host.hpp $(CSRC)/params_format.hpp $(CSRC)/g1_host.hpp $(CSRC)/hostfield.hpp $(CSRC)/field_constants.h include/dehalo.h
	g++ -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o tests/native_host/pairing_lines_check tests/native_host/pairing_lines_check.cpp

.PHONY: all oracle clean host_example host_sanitize host_tsan witness_units_check msm_plan_check opening_plan_check opening_plan_multi_check host_cs_check shuffle_cs_check hostrng_check params_format_check key_format_check pairing_check verify_host_check verify_ipa_host_check g1_host_check blame_search_check pairing_lines_check
