#!/bin/bash
# Reference-faithful step time by (sub-batch streams of the perception pass, CUs its persistent conv launches leave free), same box,
# alternating: ADX_RESNET_STREAMS x ADX_HS_RESERVE_CUS.  usage: tools/ab_walk.sh [rounds] [steps]; ADX_LIB_BASE=<parent libadx.so>
# adds the parent library's default as a fifth column of every round.
set -o pipefail
rounds=${1:-5}
steps=${2:-103}
for rnd in $(seq 1 "$rounds"); do
  for cfg in "2 0" "1 0" "2 16" "1 16"; do
    set -- $cfg
    echo -n "$rnd streams=$1 reserve=$2 "
    STEPS=$steps ADX_RESNET_STREAMS=$1 ADX_HS_RESERVE_CUS=$2 timeout -k 10 240 python tools/faithful_only.py 2>&1 | tail -1 || exit 1
  done
  if [ -n "${ADX_LIB_BASE:-}" ]; then
    echo -n "$rnd parent default "
    STEPS=$steps ADX_LIB=$ADX_LIB_BASE timeout -k 10 240 python tools/faithful_only.py 2>&1 | tail -1 || exit 1
  fi
done
