#!/bin/bash
# Build an experimental variant of libalchemy_hip.so: tools/build_variant.sh NAME "-DFLAG=..." -> alchemy_amd/lib/variants/NAME.so
# Only one instantiation unit is rebuilt with the flags (UNIT=inst_32_15 by default: the n = 2^15 kernels; UNIT=inst_gen: the general-index
# kernels); every other object comes from the normal build.
# The Plantard switches (ntt_engine.hpp), one per part; each is read by the kernels of these units only:
#   -DALCH_PLANT3_FWD=0       forward part off   UNIT=inst_32_15 (k_ks_accum_half<15>, k_crt_half<15>, k_rescale_*_half<15>: the headline,
#                                                full_mul, config2); k_ks_accum_half<11> (stage 2 only) lives in UNIT=inst_32_mid
#   -DALCH_PLANT3_FWD_LB4=1   forward LB = 4 pass as well   UNIT=inst_32_15, inst_32_mid as above
#   -DALCH_PLANT3_INV=0       inverse part off   UNIT=inst_32_15 alone (k_tensor_intt_split<15> is its only reader)
# A variant rebuilds ONE unit: with the default UNIT the n = 2^15 kernels carry the flags and the n = 2^11 key switch keeps the
# product's setting, which is what an A/B on bench.py's headline needs.  e.g.  tools/build_variant.sh fwd_only -DALCH_PLANT3_INV=0
set -e
cd "$(dirname "$0")/../alchemy_amd/csrc"
name=$1; shift
unit=${UNIT:-inst_32_15}
mkdir -p ../lib/variants build/var_$name
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC "$@" -c $unit.hip -o build/var_$name/$unit.o
objs=$(ls build/*.o | grep -v "/$unit.o")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/variants/$name.so $objs build/var_$name/$unit.o
echo built ../lib/variants/$name.so
