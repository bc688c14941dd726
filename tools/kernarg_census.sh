#!/bin/bash
# Resource usage and static mnemonic counts of the kernels that read their argument table in place (csrc/common.h PACE_KERNARG),
# both storage types; no GPU needed:   tools/kernarg_census.sh [source-root] > profiles/kernarg_resource_usage_<side>.txt
ROOT=${1:-.}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
D=$(mktemp -d)
for stem in k_dsw k_fvt k_fvt16; do
  for prec in f64 f32; do
    fl=""; [ $prec = f32 ] && fl="-DPACE_REAL_FLOAT"
    ( cd $ROOT && $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Wno-unused-function $fl --cuda-device-only \
        -Rpass-analysis=kernel-resource-usage -S pace_amd/csrc/$stem.hip -o $D/${stem}_$prec.s > $D/${stem}_$prec.remarks 2>&1 ) &
  done
done
wait
echo "# hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Rpass-analysis=kernel-resource-usage -S (_f32: -DPACE_REAL_FLOAT), every kernel of k_dsw.hip, k_fvt.hip, k_fvt16.hip (tools/kernarg_census.sh)"
python3 "$(dirname "$0")/isa_mnemonics.py" --census $D
rm -rf $D
