#!/bin/bash
# dev aid (GPU box): L2 -> memory write requests (64-byte / all) and WRITE_SIZE, then FETCH_SIZE, of the chain and the
# streaming kernels PER DISPATCH -- a --niter 10 run has ten E-step chains and one Wiener chain of 76 slots, whose mean says
# little.  Counters only, one bounded rocprofv3 pass each.  Run it in each tree to compare two builds (profiles/round4_store_layout.md).
set -o pipefail
cd "$(dirname "$0")/.."
export OUT=${PMC_OUT:-build/pmc_store}      # (build/ is ignored by git)
rm -rf $OUT; mkdir -p $OUT
ARGS="bench.py --full --steps 1 --warmup 0 --niter 10 --no-cpu-baseline --no-parity-mode --no-configs"
timeout -k 10 240 rocprofv3 --pmc TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum WRITE_SIZE --output-format csv -d $OUT/wr -- python $ARGS > $OUT/wr.log 2>&1; echo "wr rc=$?"
timeout -k 10 240 rocprofv3 --pmc FETCH_SIZE TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum --output-format csv -d $OUT/rd -- python $ARGS > $OUT/rd.log 2>&1; echo "rd rc=$?"
python - <<'PY'
import csv, glob, collections, os
short = lambda k: k.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:60]
for p, key in (("wr", "WRITE_SIZE"), ("rd", "FETCH_SIZE")):
    fs = glob.glob(os.environ["OUT"] + "/%s/**/*counter_collection.csv" % p, recursive=True)
    if not fs: print("no csv for pass", p); continue
    d = collections.defaultdict(dict)
    for r in csv.DictReader(open(fs[0])):
        k = short(r["Kernel_Name"])
        if any(s in k for s in ("stream", "wchain", "fused", "group")): d[(k, int(r["Dispatch_Id"]))][r["Counter_Name"]] = float(r["Counter_Value"])
    per = collections.defaultdict(list)
    for (k, i), v in sorted(d.items(), key=lambda x: x[0][1]): per[k].append(v)
    for k, vs in per.items():
        print(p, k, key, "x10^3 KB per dispatch:", [round(v[key] / 1000, 1) for v in vs])
        if p == "wr": print("    32-byte requests:", [int(v["TCC_EA0_WRREQ_sum"] - v["TCC_EA0_WRREQ_64B_sum"]) for v in vs])
PY
