#!/bin/bash
# tools/probes/halves_variant.sh: noaa_apt_amd/libaptgpu_nohalves.so = the library with the PHASE stage 1 of one branch per
# thread built the old way (-DAPT_PHASE_HALVES=0: sixteen windows' input in LDS at once), for the same-box A/B of
# tools/probes/exp_halves.sh (profiles/r06_phase_halves_ab.txt).  Run after `make -C noaa_apt_amd/csrc`.
set -e
cd "$(dirname "$0")/../../noaa_apt_amd/csrc"
V=/tmp/aptgpu_nohalves; mkdir -p $V
FLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize -Wall -Wno-unused-result -DAPT_PHASE_HALVES=0"
# the dispatcher and the one-branch PHASE kernels of the standard and fast profiles (rows of apt_kernels_fused_variants.hpp)
ROWS="phase_std phase_std_fast phase_fastp phase_fastp_fast"
/opt/rocm/bin/hipcc --offload-arch=gfx950 $FLAGS -c apt_kernels_fused.hip -o $V/apt_kernels_fused.o &
for r in $ROWS; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 $FLAGS -DAPT_FUSED_VARIANT=kFused_$r -DAPT_FUSED_XT=float -c apt_kernels_fused_variant.hip -o $V/fused_variant_${r}_f32.o &
  /opt/rocm/bin/hipcc --offload-arch=gfx950 $FLAGS -DAPT_FUSED_VARIANT=kFused_$r -DAPT_FUSED_XT=int16_t -c apt_kernels_fused_variant.hip -o $V/fused_variant_${r}_i16.o &
done; wait
OBJS=""
for o in $(ls *.o | grep -v -e '^apt_plan_probe.o$' -e '^probe_'); do
  if [ -f $V/$o ]; then OBJS="$OBJS $V/$o"; else OBJS="$OBJS $o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libaptgpu_nohalves.so $OBJS
ls -la ../libaptgpu_nohalves.so
