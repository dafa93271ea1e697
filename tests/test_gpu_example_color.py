"""The plain-C example (examples/aptgpu_decode.c) with --histogram and --palette: its PGM / PPM holds the pixels
api.process() returns for the same WAV file."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import noaa_apt_amd as apt
from noaa_apt_amd.testing.synth import synth_apt
from noaa_apt_amd.testing.wavfile import make_wav

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_example_histogram_and_palette(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = tmp_path / "aptgpu_decode"
    libdir = os.path.dirname(apt.lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "examples", "aptgpu_decode.c"), "-L", libdir, "-laptgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    x = synth_apt(11025, 130, seed=13)
    wav = tmp_path / "pass.wav"
    wav.write_bytes(make_wav(x.astype(np.int16), 11025))
    signal, _ = apt.load(str(wav))
    rows = apt.decode(apt.Context(), apt.Settings(), signal, apt.Rate.hz(11025), True)
    h = rows.size // 2080

    pgm = tmp_path / "hist.pgm"
    r = subprocess.run([str(exe), str(wav), str(pgm), "--histogram"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Mapping values" in r.stderr and "Generating image" in r.stderr
    header = f"P5\n2080 {h}\n255\n".encode()
    data = pgm.read_bytes()
    assert data.startswith(header)
    assert data[len(header):] == apt.process(apt.Context(), rows, apt.Contrast.HISTOGRAM).tobytes()

    color = apt.ColorSettings(os.path.join(ROOT, "tests", "golden", "palettes", "noaa-apt-daylight.png"))
    raw = tmp_path / "daylight.rgb"
    raw.write_bytes(color.palette.tobytes())
    for contrast, ca in (("percent", apt.Contrast.Percent(0.98)), ("telemetry", apt.Contrast.TELEMETRY)):
        ppm = tmp_path / f"{contrast}.ppm"
        r = subprocess.run([str(exe), str(wav), str(ppm), contrast, "--palette", str(raw)], capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr
        header = f"P6\n2080 {h}\n255\n".encode()
        data = ppm.read_bytes()
        assert data.startswith(header)
        want = apt.process(apt.Context(), rows, ca, color=color)
        assert data[len(header):] == np.ascontiguousarray(want[..., :3]).tobytes()

    # Histogram with false colour is refused (equalisation in CIE Lab is out of scope)
    r = subprocess.run([str(exe), str(wav), str(tmp_path / "x.ppm"), "--histogram", "--palette", str(raw)],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "image stage failed (5)" in r.stderr
