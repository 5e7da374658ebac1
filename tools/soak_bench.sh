#!/bin/bash
# the FULL bench.py, in process (no supervising parent, no second attempt), N times on one box; one line per run in
# gpurun_out/soak/<tag>.txt: run index, exit code, wall seconds, the line's value / proof ms / batch proofs per s (or the last stderr lines of a failure).
# Stops at the first failure (a GPU fault is never retried on the same box).
tag=${1:-soak}; n=${2:-10}
mkdir -p gpurun_out/soak
out=gpurun_out/soak/$tag.txt
echo "# $(date -u +%FT%TZ) host $(hostname) full bench.py --in-process x $n" > $out
for i in $(seq 1 $n); do
  t0=$(date +%s)
  timeout -k 10 600 python bench.py --full --in-process > ${out%.txt}.$i.json 2> ${out%.txt}.$i.err
  rc=$?
  t1=$(date +%s)
  if [ $rc -eq 0 ]; then
    python - "$tag" "$i" $((t1-t0)) >> $out <<'PY'
import json, sys
tag, i, secs = sys.argv[1:4]
d = json.loads(open("gpurun_out/soak/%s.%s.json" % (tag, i)).read().strip().splitlines()[-1])
print("run %s rc 0 %s s value %.1f Mpoints/s proof_k17 %.3f ms batch %.1f proofs/s attempts %d" % (i, secs, d["value"], d["proof"]["gpu_ms"], d["batch_proofs"]["proofs_per_s"], d["attempts"]))
PY
    rm -f gpurun_out/soak/$tag.$i.err
    [ $i -gt 1 ] && rm -f gpurun_out/soak/$tag.$i.json
  else
    echo "run $i rc $rc $((t1-t0)) s FAILED: $(tail -n 4 gpurun_out/soak/$tag.$i.err | tr '\n' '|' | cut -c1-600)" >> $out
    exit 1
  fi
done
echo "# all $n runs passed" >> $out
