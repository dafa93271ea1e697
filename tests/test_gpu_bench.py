"""bench.py's plain line and --dump-outputs: the headline keys, exactly --steps timed steps, nothing of --full, and the
outputs of the last timed step — every dumped recording's rows and sync positions bit-identical to the CPU oracle's
decode of the same synthetic input (input j of rank 0 is synth_apt(rate, seconds, seed=2 + 1000 * j))."""
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import noaa_apt_amd as apt
from noaa_apt_amd.testing.synth import synth_apt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args, "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("seconds,batch,inputs,compared", [(60.0, 4, 6, 4), (600.0, 16, 4, 2)])
def test_plain_line_and_dumped_outputs(oracle, tmp_path, seconds, batch, inputs, compared):
    line = _bench(["--steps", "5", "--warmup", "2", "--seconds", str(seconds), "--batch", str(batch),
                   "--inputs", str(inputs)], tmp_path)
    assert line["steps"] == 5 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    samples_per_step = round(48000 * seconds) * batch
    assert line["value"] == pytest.approx(samples_per_step / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    for k in ("roofline", "pipeline", "power", "extras", "fast_mode", "cpu_baseline", "parity"):
        assert k not in line

    files = sorted(glob.glob(os.path.join(tmp_path, "*.npy")))
    assert sum(os.path.getsize(f) for f in files) <= 64 << 20
    recs = sorted({int(re.match(r"rec(\d+)_", os.path.basename(f)).group(1)) for f in files})
    assert len(recs) == batch and all(0 <= r < max(batch, inputs) for r in recs)
    s = apt.Settings.profile("standard")
    settings = {k: getattr(s, k) for k in ("work_rate", "resample_atten", "resample_delta_freq", "resample_cutout",
                                           "demodulation_atten")}
    for rec in recs[:compared]:
        stem = os.path.join(tmp_path, f"rec{rec:03d}")
        res = np.load(f"{stem}_result.npy")
        rows = np.load(f"{stem}_rows.npy")
        assert res.dtype == np.float64 and rows.dtype == np.float32 and rows.ndim == 2 and rows.shape[1] == 2080
        ref, st = oracle.decode(synth_apt(48000, seconds, seed=2 + 1000 * rec), 48000, True, settings=settings,
                                want_steps=True)
        ref = ref.reshape(-1, 2080)
        assert res[0] == 0 and res[2] == ref.shape[0] and res[5] == ref.size
        if os.path.exists(f"{stem}_rows_index.npy"):  # a sample of the rows
            idx = np.load(f"{stem}_rows_index.npy").astype(np.int64)
            assert idx.size == rows.shape[0] < ref.shape[0] and np.all(np.diff(idx) > 0)
            ref = ref[idx]
        assert np.array_equal(rows.view(np.uint32), ref.view(np.uint32))
        pos = np.load(f"{stem}_sync_pos.npy")
        assert np.array_equal(pos, st["sync_pos"].astype(np.float64))
