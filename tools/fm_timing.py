#!/usr/bin/env python3
"""tools/fm_timing.py [--calls N] [--seconds S] [--configs a,b] — device time of the FM demodulator:
HIP events around FmDemodulator.demodulate_device, 4 recordings per call, at

    rtl_u8     2.4 MS/s u8,    D = 50 (48 kHz out,  T = 671)
    sdr_s16    1.024 MS/s s16, D = 16 (64 kHz out,  T = 287)
    wav_f32    250 kS/s f32,   D = 5  (50 kHz out,  T = 71)

each without a shift and with one (0.1037 fs).  Per configuration: ms per call (median and minimum of N calls after two
warm-up calls), the bytes read and written, and that traffic's time at 8 TB/s as a fraction of the measured time
(BASELINE.md §3's roofline).  The recordings are random components (the time does not depend on the values).
--calls 1 --configs NAME is the shape for a counters-only profiler run of one configuration.
GPU box."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import noaa_apt_amd as apt  # noqa: E402

CONFIGS = {
    "rtl_u8": (apt.IqFormat.U8, 2400000, 50),
    "sdr_s16": (apt.IqFormat.S16, 1024000, 16),
    "wav_f32": (apt.IqFormat.F32, 250000, 5),
}
HBM_BYTES_PER_S = 8e12


def recording(fmt, n_frames, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    if fmt == apt.IqFormat.F32:
        return torch.randn(2 * n_frames, dtype=torch.float32, device=dev, generator=g)
    if fmt == apt.IqFormat.S16:
        return torch.randint(-20000, 20000, (2 * n_frames,), dtype=torch.int16, device=dev, generator=g)
    return torch.randint(0, 256, (2 * n_frames,), dtype=torch.uint8, device=dev, generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--recordings", type=int, default=4)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    print(f"# {torch.cuda.get_device_name(0)}; {args.recordings} recordings of {args.seconds:g} s per call, {args.calls} calls")
    print("config,shift_hz,taps,frames_per_recording,ms_median,ms_min,bytes_in,bytes_out,hbm_ms,fraction_of_roofline")
    for name in args.configs.split(","):
        fmt, fs, d = CONFIGS[name]
        n_frames = int(fs * args.seconds)
        iq = [recording(fmt, n_frames, dev, 7 + i) for i in range(args.recordings)]
        for shift in (0.0, 0.1037 * fs):
            fmd = apt.FmDemodulator(apt.FmSettings(fmt, fs, d, shift), stream=stream.cuda_stream)
            n_out = fmd.out_len(n_frames)
            audio = [torch.empty(n_out + 16, dtype=torch.float32, device=dev) for _ in iq]
            ptrs = ([t.data_ptr() for t in iq], [n_frames] * len(iq), [t.data_ptr() for t in audio], [n_out] * len(iq))
            for _ in range(2):
                fmd.demodulate_device(*ptrs)
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fmd.demodulate_device(*ptrs)
                b.record(stream)
                b.synchronize()
                ms.append(a.elapsed_time(b))
            bytes_in = sum(t.numel() * t.element_size() for t in iq)
            bytes_out = 4 * n_out * len(iq)
            hbm_ms = (bytes_in + bytes_out) / HBM_BYTES_PER_S * 1e3
            med = float(np.median(ms))
            print(f"{name},{shift:.1f},{fmd.info.n_taps},{n_frames},{med:.3f},{min(ms):.3f},{bytes_in},{bytes_out},"
                  f"{hbm_ms:.3f},{hbm_ms / med:.3f}")
            fmd.close()
        del iq
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
