#!/usr/bin/env python3
"""tools/afc_timing.py [--calls N] [--seconds S] [--configs a,b] — device time of the AFC in front of the FM demodulator
(DESIGN.md §27), at tools/fm_timing.py's configurations with a shift of 0.1037 fs:

    rtl_u8     2.4 MS/s u8,    D = 50
    sdr_s16    1.024 MS/s s16, D = 16
    wav_f32    250 kS/s f32,   D = 5

HIP events around FmAfc.demodulate_device (k_afc_sums, k_afc_table and k_fm_tracked: three launches) and, in the same
run on the same recordings, around FmDemodulator.demodulate_device (k_fm), 4 recordings per call.  Per configuration: ms
per call of each (median and minimum of N calls after two warm-up calls), the time of reading the recordings once at
8 TB/s (what k_afc_sums has to move), and the AFC's time over k_fm's.  The per-kernel split comes from running this tool
with --calls 3 under a kernel-trace profiler.  The recordings are random components (the time does not depend on the
values).
GPU box."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import noaa_apt_amd as apt  # noqa: E402
from fm_timing import CONFIGS, HBM_BYTES_PER_S, recording  # noqa: E402


def timed(stream, calls, fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--recordings", type=int, default=4)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--block-frames", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    print(f"# {torch.cuda.get_device_name(0)}; {args.recordings} recordings of {args.seconds:g} s per call, {args.calls} calls, "
          f"B = {args.block_frames}")
    print("config,taps,lag,frames_per_recording,blocks,afc_ms_median,afc_ms_min,fm_ms_median,fm_ms_min,afc_over_fm,"
          "bytes_in,read_once_ms")
    for name in args.configs.split(","):
        fmt, fs, d = CONFIGS[name]
        n_frames = int(fs * args.seconds)
        iq = [recording(fmt, n_frames, dev, 7 + i) for i in range(args.recordings)]
        st = apt.FmSettings(fmt, fs, d, 0.1037 * fs)
        afc = apt.AfcSettings(block_frames=args.block_frames)
        fmd = apt.FmDemodulator(st, stream=stream.cuda_stream)
        dafc = apt.FmAfc(fmd, afc, max_frames=n_frames)
        n_out = fmd.out_len(n_frames)
        audio = [torch.empty(n_out + 16, dtype=torch.float32, device=dev) for _ in iq]
        ptrs = ([t.data_ptr() for t in iq], [n_frames] * len(iq), [t.data_ptr() for t in audio], [n_out] * len(iq))
        fm_med, fm_min = timed(stream, args.calls, lambda: fmd.demodulate_device(*ptrs))
        afc_med, afc_min = timed(stream, args.calls, lambda: dafc.demodulate_device(*ptrs))
        bytes_in = sum(t.numel() * t.element_size() for t in iq)
        print(f"{name},{fmd.info.n_taps},{apt.fm_afc_design(st, afc).lag},{n_frames},{dafc.n_blocks(n_frames)},{afc_med:.3f},"
              f"{afc_min:.3f},{fm_med:.3f},{fm_min:.3f},{afc_med / fm_med:.3f},{bytes_in},{bytes_in / HBM_BYTES_PER_S * 1e3:.3f}")
        dafc.close()
        fmd.close()
        del iq, audio
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
