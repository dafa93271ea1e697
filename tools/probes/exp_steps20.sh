#!/bin/bash
# usage: exp_steps20.sh OUTPUT_DIR
O=${1:?usage: $0 OUTPUT_DIR}; mkdir -p "$O"
for i in 1 2 3; do
  python bench.py --full --steps 20 --warmup 5 --no-extras --no-cpu-baseline --no-single-launch > "$O/p_$i.json" 2>/dev/null
  python bench.py --full --steps 20 --warmup 5 --no-extras --no-cpu-baseline --no-single-launch --no-power > "$O/np_$i.json" 2>/dev/null
done
python bench.py --full --steps 600 --no-extras --no-cpu-baseline --no-single-launch > "$O/p600.json" 2>/dev/null
python - "$O" <<'PY'
import json,glob,sys
for f in sorted(glob.glob(sys.argv[1] + "/*.json")):
    try:
        d=json.loads(open(f).read().strip().splitlines()[-1])
        print(f, d["ms_per_step"], d.get("power",{}).get("timed_region",{}).get("gfxclk_mhz_at_end"))
    except Exception as e: print(f, "ERR", e)
PY
