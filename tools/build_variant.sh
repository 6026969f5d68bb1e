#!/bin/bash
# Diagnostic build of libupe_gpu with extra -D flags: tools/build_variant.sh <out.so> [-DX=Y ...]
# (timing experiments; the product library is built by `make -C upe_amd/csrc`)
# The flags reach upe_gpu.hip (the classify kernels) alone; every other unit is the product's.
set -e
out=$(realpath -m "$1"); shift
cd "$(dirname "$0")/.."
others=""
for u in upe_rx upe_egress upe_ingress upe_latency upe_hostpath upe_segment upe_rules upe_host upe_worker; do
  others="$others $PWD/build/$u.o"
done
make -s -C upe_amd/csrc $others >/dev/null
tmp=$(mktemp -d)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-result "$@" \
  -c -o $tmp/g.o upe_amd/csrc/upe_gpu.hip
mkdir -p "$(dirname "$out")"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$out" $tmp/g.o $others
rm -rf $tmp
