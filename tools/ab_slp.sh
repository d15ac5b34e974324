#!/bin/bash
# A/B of -fno-slp-vectorize on fused_proj.hip (#5 with convc1 fused); abl/libdvccorr_slp.so is a hand-built variant.
set -u
O=${OUT_DIR:-ab_out}/slp; mkdir -p $O
for i in 1 2; do
for v in default slp; do
  if [ $v = slp ]; then export DVCCORR_LIB=$PWD/abl/libdvccorr_slp.so; else unset DVCCORR_LIB; fi
  timeout -k 10 300 python -u bench.py --full --impl fused --size 128 --encoder 2 --levels 2 --steps 3 --warmup 1 --no-cpu-baseline --convc1 fused > $O/$v$i.json 2>$O/$v$i.err || exit 3
  python -c "import json; d=json.load(open('$O/$v$i.json')); print('$v', d['ms_per_step'], d['lookup_avg_ms'])"
done; done
