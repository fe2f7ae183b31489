#!/bin/bash
# diagnostic: the raw-map passes in both block orders (LVI_VB_SLOT_ORDER=0: slot in blockIdx.z, 1: slot folded into x) from ONE build, on one box.
# usage: slot_order_prof.sh [tables] [pmc]   -> $LVI_DIAG_OUT/slot_order/ (default build/diag)
#   tables  kernel tables of one handle x 8 scans (kernels serialized by the tracer) and of 4 handles x 8 scans
#   pmc     L2 / fabric counters of vb_plan and vb_scatter_det, one handle x 8 scans; counter passes run alone, no tracing beside them
# every GPU step has its own time limit, and the first step that fails ends the script
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
O=${LVI_DIAG_OUT:-build/diag}/slot_order; mkdir -p $O
COMMON="--repeats 1 --no-cpu --no-tracker --profile-steps 0 --prime-steps 0 --sequential-scans 0 --cached-plan-steps 0"
for what in "$@"; do
  for v in 0 1; do
    export LVI_VB_SLOT_ORDER=$v
    if [ $what = tables ]; then
      for cfg in "1 8" "4 8"; do
        read nh nb <<< "$cfg"; t=${nh}x${nb}_order$v
        timeout -k 10 400 rocprofv3 --kernel-trace --output-format csv -d $O/k_$t -- python3 bench.py --steps 12 --warmup 3 $COMMON --inflight $nh --batch $nb > $O/k_$t.json 2> $O/k_$t.err || { echo "kernel trace $t failed: $?"; tail -5 $O/k_$t.err; exit 1; }
        python3 tools/summarize_prof.py steady $O/k_$t $O/steady_$t.md 12 > /dev/null || exit 1
        rm -rf $O/k_$t
        echo "== $t"; head -1 $O/steady_$t.md; grep -E "vb_|vox_minmax" $O/steady_$t.md
      done
    else
      for pass in "FETCH_SIZE" "WRITE_SIZE" "TCC_HIT_sum TCC_MISS_sum"; do      # (the TCC block has four counter slots: FETCH_SIZE takes three, WRITE_SIZE two)
        t=$(echo $pass | tr ' ' '+')_order$v
        timeout -k 10 400 rocprofv3 --pmc $pass --output-format csv -d $O/p_$t -- python3 bench.py --steps 4 --warmup 2 $COMMON --inflight 1 --batch 8 > $O/p_$t.json 2> $O/p_$t.err || { echo "counter pass $t failed: $?"; tail -5 $O/p_$t.err; exit 1; }
      done
      python3 - $O $v <<'PY' || exit 1
import collections, csv, glob, json, sys
O, v = sys.argv[1], sys.argv[2]
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(f"{O}/p_*_order{v}/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        for k in ("vb_plan_kernel", "vb_scatter_det_kernel", "vb_hist_w_kernel"):
            if k in r["Kernel_Name"]:
                agg[f'{k} [grid {r["Grid_Size"]}]'][r["Counter_Name"]].append(float(r["Counter_Value"]))
res = {}
for k, c in sorted(agg.items()):
    row = {n: round(sum(x[-8:]) / len(x[-8:]), 1) for n, x in c.items()}          # the last launches: steady state
    row["launches"] = max(len(x) for x in c.values())
    if "TCC_HIT_sum" in row and "TCC_MISS_sum" in row:
        row["l2_hit_rate"] = round(row["TCC_HIT_sum"] / max(row["TCC_HIT_sum"] + row["TCC_MISS_sum"], 1.0), 4)
    res[k] = row
    print(f"order {v}", k, row)
json.dump(res, open(f"{O}/pmc_order{v}.json", "w"), indent=1)
PY
      rm -rf $O/p_*_order$v
    fi
  done
done
