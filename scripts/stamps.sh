#!/bin/bash
# Per-phase cycle split of the search kernel (stamps build, diagnostic only).
# usage: stamps.sh [output directory, default build/stamps]
cd "$(dirname "$0")/.." || exit 1
O=${1:-build/stamps}; mkdir -p "$O"
NGT_AMD_LIB=$PWD/ngt_amd/libngt_amd_stamps.so timeout -k 10 300 python bench.py --full --steps 2 --warmup 1 --no-cpu \
  --eps 0.0703 > "$O/stamps.json" 2> "$O/stamps.log"
rc=$?; grep -E "phase|eps|graph" "$O/stamps.log"; exit $rc
