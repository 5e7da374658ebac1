#!/bin/bash
# The parent commit's tree (tools/ab/parent: `git archive HEAD~ | tar -x -C tools/ab/parent`, then `make` in it) against this one on ONE box, alternating pairs
# (default five): bench.py's delay_enc_k17_ms and the k = 14 / 20 delay_enc proofs -- what a change to the prover's host code must leave alone.  Then the cost of an
# advice phase (RLC3 of tests/phased_circuits.py at k = 17).  Every step has its own time limit; the first failure ends the script.
#   bash tools/ab_parent.sh [pairs]     -> build/ab/ab_parent_vs_this.txt, build/ab/rlc3_k17_phases.txt (build/ is ignored by git; the kept copies live in profiles/)
set -o pipefail
mkdir -p build/ab
pairs=${1:-5}
out=build/ab/ab_parent_vs_this.txt
: > $out
line() { python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
p=d.get('proof') or {}
o={q['k']: q['gpu_ms'] for q in (d.get('proof_other_k') or [])}
print('$1: delay_enc_k17_ms %s (proof gpu_ms %s), k14 %s ms, k20 %s ms; step %.4f ms' % ((d.get('config') or {}).get('delay_enc_k17_ms'), p.get('gpu_ms'), o.get(14), o.get(20), d['ms_per_step']))"; }
args="--gpus 1 --steps 10 --warmup 3 --full --no-cpu-baseline --no-verify --full-out= --proofs 0 --fixed-batch 0"
for r in $(seq 1 $pairs); do
  (cd tools/ab/parent && timeout -k 10 240 python bench.py $args 2>/dev/null) | line "pair $r  parent" | tee -a $out || exit 1
  timeout -k 10 240 python bench.py $args 2>/dev/null | line "pair $r  this  " | tee -a $out || exit 1
done
timeout -k 10 300 python tools/profile_proof.py rlc3 17 9 2>&1 | tee build/ab/rlc3_k17_phases.txt | tail -6
