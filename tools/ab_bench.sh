#!/bin/bash
# Bench A/B of product builds spatial-intention-maps_amd/simaps/libsimaps_prod_<name>.so (tools/prod_build.sh)
# in one GPU call, alternating:
#   [BENCH_ARGS="--steps 200 --warmup 20"] [AB_ROUNDS=4] [AB_OUT=dir] [AB_OLD_ABI=n] tools/ab_bench.sh NAME1 NAME2 ...
# Each run has its own time limit and the first failure ends the script.  A build of another revision
# is loaded through SIMAPS_LIB with SIMAPS_AB_SOURCE_HASH from libsimaps_prod_<name>.hash.  Every bench
# line goes to $AB_OUT/ab_bench.jsonl (default bench_outputs/ab) with the build's name in "build".
# AB_OLD_ABI: also accept builds of an older revision with ABI version n (get_state's signature unchanged)
cd "$(dirname "$0")/.."
O=${AB_OUT:-bench_outputs/ab}
mkdir -p "$O"
S=spatial-intention-maps_amd/simaps
for i in $(seq 1 "${AB_ROUNDS:-2}"); do for v in "$@"; do
  h=""; [ -f $S/libsimaps_prod_$v.hash ] && h=$(cat $S/libsimaps_prod_$v.hash)
  log=$O/ab_${v}_${i}.log
  SIMAPS_AB_SOURCE_HASH=$h SIMAPS_AB_OLD_ABI=${AB_OLD_ABI:-} SIMAPS_LIB=$S/libsimaps_prod_$v.so timeout -k 10 120 python bench.py --no-cpu-baseline ${BENCH_ARGS:-} > $log 2>&1 || { tail -5 $log; exit 1; }
  grep '^{' $log | tail -1 | python -c "import json,sys; d=json.load(sys.stdin); d['build']='$v'; print(json.dumps(d))" >> $O/ab_bench.jsonl
  echo "$v $(grep -o '"value": [0-9.]*' $log | head -1) $(grep -o '"kernel_ms": [0-9.]*' $log | head -1)"
done; done
