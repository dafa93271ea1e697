#!/bin/bash
# tools/isa.sh <tu-name>... : device-only assembly of a translation unit into /tmp/isa/<name>.s and the register / spill
# figures of every kernel in it.  fused_<row>_<f32|i16> (a row of csrc/apt_kernels_fused_variants.hpp, e.g. fused_48k_fast_i16):
# that k_fused instantiation, from csrc/apt_kernels_fused_variant.hip; fused_any_<NTHR>x<PER>: that shape of k_fused_any;
# any other name: csrc/apt_kernels_<name>.hip.  ISA_FLAGS=-DAPT_FUSED_MARKS=1 adds the stage marks tools/isa_budget.py
# --marks reads.
mkdir -p /tmp/isa
cd "$(dirname "$0")/../noaa_apt_amd/csrc" || exit 1
for k in "$@"; do
  src=apt_kernels_$k.hip; defs=
  case $k in
    fused_any_*x*) s=${k#fused_any_}; src=apt_kernels_fused_any_shape.hip; defs="-DAPT_ANY_NTHR=${s%x*} -DAPT_ANY_PER=${s#*x}";;
    fused_*_f32) n=${k#fused_}; src=apt_kernels_fused_variant.hip; defs="-DAPT_FUSED_VARIANT=kFused_${n%_f32} -DAPT_FUSED_XT=float";;
    fused_*_i16) n=${k#fused_}; src=apt_kernels_fused_variant.hip; defs="-DAPT_FUSED_VARIANT=kFused_${n%_i16} -DAPT_FUSED_XT=int16_t";;
  esac
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math \
    -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize $ISA_FLAGS $defs --cuda-device-only -S -o /tmp/isa/$k.s $src 2>&1 | grep -E "error" -A5 &
done
wait
for k in "$@"; do
  echo "== $k"
  grep -E "^\s+\.(name|sgpr_spill_count|vgpr_count|vgpr_spill_count|private_segment_fixed_size):" /tmp/isa/$k.s \
    | sed -e 's/^\s*//' | paste - - - - - | sed -e 's/_ZN3apt3gpu12_GLOBAL__N_1//' | cut -c1-60,110-
done
