#!/usr/bin/env python3
"""tools/fm_stream_timing.py [--pushes N] [--catch-up-seconds S] [--configs a,b] [--out FILE] — wall time of the
streaming FM demodulator and of the live decode from IQ, one run on one GPU, at fm_timing.py's
configurations with a shift of 0.1037 fs:

    rtl_u8     2.4 MS/s u8,    D = 50 (48 kHz out)
    sdr_s16    1.024 MS/s s16, D = 16 (64 kHz out)
    wav_f32    250 kS/s f32,   D = 5  (50 kHz out)

push       ms per push of 0.25 s and of 1 s of frames, host-fed (numpy in, numpy out: includes both copies and the
           wait) and device-resident (the call, then a wait for the stream): median and minimum of N pushes
catch_up   S seconds of frames in ONE device-resident push (launch pairs of max_push_frames back to back) beside the
           one-shot aptgpu_fm_demodulate_device of the same frames in the same run: median of 5 each, and their ratio;
           then the same push with max_push_frames above it (one launch pair), which separates the kernel body's
           time from what each further pair costs
live       LiveIqDecoder.push of the same sizes (host-fed) beside FmStream.push followed by LiveDecoder.push
The recordings are random components: the FM time does not depend on the values, and the decode behind them finds no
sync in noise, so its rows are the few a picker without a signal releases (no finish is called).
Writes the table to --out (default profiles/r21_fm_stream.txt) and to stdout.  GPU box."""
import argparse
import os
import sys
import time

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


def recording(fmt, n_frames, seed):
    rng = np.random.default_rng(seed)
    if fmt == apt.IqFormat.F32:
        return rng.standard_normal(2 * n_frames, dtype=np.float32)
    if fmt == apt.IqFormat.S16:
        return rng.integers(-20000, 20000, 2 * n_frames, dtype=np.int16)
    return rng.integers(0, 256, 2 * n_frames, dtype=np.uint8)


def wall_ms(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return f"{float(np.median(ms)):.3f},{min(ms):.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=20)
    ap.add_argument("--catch-up-seconds", type=float, default=60.0)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_fm_stream.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    ctx = apt.Context(device=0, stream=stream.cuda_stream)
    sync = torch.cuda.synchronize
    lines = [f"# {torch.cuda.get_device_name(0)}; {args.pushes} pushes per row, catch-up of {args.catch_up_seconds:g} s",
             "kind,config,seconds_per_push,form,ms_median,ms_min,note"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    for name in args.configs.split(","):
        fmt, fs, d = CONFIGS[name]
        st = apt.FmSettings(fmt, fs, d, 0.1037 * fs)
        itemsize = apt.IqFormat.dtype(fmt).itemsize
        for seconds in (0.25, 1.0):
            k = int(fs * seconds)
            iq = recording(fmt, k * (args.pushes + 2), 5)
            d_iq = torch.from_numpy(iq).to(dev)
            # ---- FmStream, host-fed and device-resident
            with apt.FmStream(st, context=ctx) as s:
                ms = [wall_ms(lambda i=i: s.push(iq[2 * k * i:2 * k * (i + 1)]), sync) for i in range(args.pushes + 2)][2:]
                emit(f"push,{name},{seconds:g},host_fed,{stats(ms)},T={s.info.n_taps}")
            with apt.FmStream(st, context=ctx) as s:
                out = torch.empty(k // d + 16, dtype=torch.float32, device=dev)
                ms = [wall_ms(lambda i=i: s.push_device(d_iq.data_ptr() + 2 * k * i * itemsize, k, out.data_ptr(), k // d + 2), sync)
                      for i in range(args.pushes + 2)][2:]
                emit(f"push,{name},{seconds:g},device,{stats(ms)},")
            # ---- LiveIqDecoder beside FmStream + LiveDecoder
            try:
                with apt.LiveIqDecoder(apt.Settings(), st, True, context=ctx) as live:
                    ms = [wall_ms(lambda i=i: live.push(iq[2 * k * i:2 * k * (i + 1)]), sync) for i in range(args.pushes + 2)][2:]
                    emit(f"live,{name},{seconds:g},LiveIqDecoder,{stats(ms)},rows={int(live.result.rows_total)}")
                with apt.FmStream(st, context=ctx) as s, apt.LiveDecoder(apt.Settings(), s.rate, True, context=ctx) as dec:
                    ms = [wall_ms(lambda i=i: dec.push(s.push(iq[2 * k * i:2 * k * (i + 1)])), sync)
                          for i in range(args.pushes + 2)][2:]
                    emit(f"live,{name},{seconds:g},FmStream+LiveDecoder,{stats(ms)},rows={int(dec.result.rows_total)}")
            except apt.AptError as e:  # (a decode stream this output rate cannot have)
                emit(f"live,{name},{seconds:g},refused,,,{str(e).splitlines()[0][:80]}")
            del d_iq
        # ---- catch-up: one long push beside the one-shot
        n = int(fs * args.catch_up_seconds)
        d_iq = torch.from_numpy(recording(fmt, n, 6)).to(dev)
        fmd = apt.FmDemodulator(st, stream=stream.cuda_stream)
        n_out = fmd.out_len(n)
        out = torch.empty(n_out + 16, dtype=torch.float32, device=dev)
        one = [wall_ms(lambda: fmd.demodulate_device([d_iq.data_ptr()], [n], [out.data_ptr()], [n_out]), sync) for _ in range(7)][2:]
        fmd.close()
        many = []
        with apt.FmStream(st, context=ctx) as s:
            for _ in range(7):
                s.reset()
                many.append(wall_ms(lambda: s.push_device(d_iq.data_ptr(), n, out.data_ptr(), n_out), sync))
            pairs = -(-n // s.info.max_push_frames)
        many = many[2:]
        single = []  # the same push as ONE launch pair (max_push_frames above it): what the pairs themselves cost
        with apt.FmStream(st, context=ctx, max_push_frames=1 << 28) as s:
            for _ in range(7):
                s.reset()
                single.append(wall_ms(lambda: s.push_device(d_iq.data_ptr(), n, out.data_ptr(), n_out), sync))
        single = single[2:]
        emit(f"catch_up,{name},{args.catch_up_seconds:g},one_shot,{stats(one)},")
        emit(f"catch_up,{name},{args.catch_up_seconds:g},stream,{stats(many)},launch_pairs={pairs} "
             f"ratio={float(np.median(many)) / float(np.median(one)):.3f}")
        emit(f"catch_up,{name},{args.catch_up_seconds:g},stream_one_pair,{stats(single)},launch_pairs=1 "
             f"ratio={float(np.median(single)) / float(np.median(one)):.3f} "
             f"ms_per_extra_pair={(float(np.median(many)) - float(np.median(single))) / max(pairs - 1, 1):.4f}")
        del d_iq, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
