#!/bin/bash
# tools/pipeline_costs.sh — what the pipelined step (strict, 16 recordings per call, three calls in flight) is made of:
# (1) what ONE MORE launch of each kernel costs it (probe library: every kernel of the chain is idempotent, so the rows
# stay valid), the front ends alone; (2) two and four calls in flight, as A/B in one process.  One JSON line per
# configuration (tools/sweep.py); `ms per call` = ms_per_recording x 16.
R=${GRAFT_REPO_ROOT:-/root/repo}; cd $R
V="strict:16:3"
V="$V,strict:16:3:APTGPU_DEBUG_REPEAT_WORDS=2"
V="$V,strict:16:3:APTGPU_DEBUG_REPEAT_ORBIT=2"
V="$V,strict:16:3:APTGPU_DEBUG_REPEAT_GATHER=2"
V="$V,strict:16:3:APTGPU_DEBUG_REPEAT_FRONT=2"
V="$V,strict:16:3:APTGPU_DEBUG_SKIP=7"
V="$V,strict:16:2"
V="$V,strict:16:4"
V="$V,strict:16:3"
APTGPU_PROBE_LIB=$R/noaa_apt_amd/libaptgpu_probe.so timeout 600 python tools/sweep.py --configs "$V" --steps 200 --warmup 20 --inputs 16
