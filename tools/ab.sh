#!/bin/bash
# dev aid (GPU box): time bench.py with several builds of the library in ONE call (box-to-box variance is +-3%)
# usage: tools/ab.sh "<bench args>" tagA tagB ...   (tag "main" = libvaenmf.so)
# a variant libvaenmf_<tag>.so comes from: VAENMF_HIPCC_FLAGS="<extra hipcc flags>" python __graft_entry__.py --tag <tag>
args=$1; shift
out=${AB_LOG_DIR:-$(mktemp -d)}; mkdir -p "$out"; echo "logs: $out"
for t in "$@"; do
  lib=$GRAFT_REPO_ROOT/guided-vae-nmf_amd/vaenmf/libvaenmf_$t.so
  [ "$t" = main ] && lib=$GRAFT_REPO_ROOT/guided-vae-nmf_amd/vaenmf/libvaenmf.so
  VAENMF_LIB=$lib timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-parity-mode $args > "$out/ab_$t.log" 2>&1 || { echo "$t FAILED"; tail -3 "$out/ab_$t.log"; continue; }
  tail -1 "$out/ab_$t.log" | python -c "import json,sys; d=json.loads(sys.stdin.read()); k=d['kernels']; print('$t', round(d['ms_per_step'],2), 'ms/step', {n: round(v['ms_total']/v['launches'],4) for n,v in k.items()}, 'sisdr', round(d.get('si_sdr_mean_db',0),3))"
done
