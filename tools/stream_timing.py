#!/usr/bin/env python3
"""tools/stream_timing.py [--seconds S] [--catch-up S] — wall time of live decode, standard profile, at
11 025 Hz and 48 kHz:

    push      a recording of S seconds (60 by default) in pushes of 0.25 s and of 1 s: wall time per push, median and
              maximum, host-fed (LiveDecoder.push: samples up, one record and the final rows back, synchronous) and
              device-resident (push_device on a stream of its own, waited for after every push)
    catch_up  a ten-minute recording in ONE push (the stream splits it into launch sequences of max_push samples) and
              its finish (one record read back), beside one-shot decode() of the same recording in the same run (best of 3 each)

Records, not thresholds.  GPU box."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import noaa_apt_amd as apt  # noqa: E402
from noaa_apt_amd.testing.synth import synth_apt  # noqa: E402


def pushes_host(dec, x, chunk, finish=True):
    ts, rows = [], 0
    for at in range(0, x.size, chunk):
        t0 = time.perf_counter()
        r, _ = dec.push(x[at:at + chunk])
        ts.append(time.perf_counter() - t0)
        rows += r.shape[0]
    if finish:
        rows += dec.finish()[0].shape[0]
    return ts, rows


def pushes_device(dec, d_x, n, chunk, d_rows, d_pos, cap, finish=True):
    ts, rows = [], 0
    for at in range(0, n, chunk):
        c = min(chunk, n - at)
        t0 = time.perf_counter()
        assert dec.rows_bound(c) <= cap  # (two or three on a pass that keeps its sync)
        dec.push_device(d_x.data_ptr() + 4 * at, c, d_rows.data_ptr(), d_pos.data_ptr(), cap)
        rows += int(dec.results().n_rows)
        ts.append(time.perf_counter() - t0)
    if finish:
        dec.finish_device(d_rows.data_ptr(), d_pos.data_ptr(), cap)
        rows += int(dec.results().n_rows)
    return ts, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--catch-up", type=float, default=600.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    settings = apt.Settings.profile("standard")
    print(f"# {torch.cuda.get_device_name(0)}; standard profile; pushes over {args.seconds:g} s, catch-up over {args.catch_up:g} s")
    print("rate,what,form,pushes,ms_median,ms_max,rows,note")
    for rate in (11025, 48000):
        x = synth_apt(rate, args.seconds, 5)
        ref_rows = apt.decode(apt.Context(), settings, x, apt.Rate.hz(rate), True).size // 2080
        for seconds in (0.25, 1.0):
            chunk = int(rate * seconds)
            with apt.LiveDecoder(settings, apt.Rate.hz(rate)) as dec:
                pushes_host(dec, x[:4 * chunk], chunk, finish=False)  # warm-up
                dec.reset()
                ts, rows = pushes_host(dec, x, chunk)
            assert rows == ref_rows, (rows, ref_rows)
            print(f"{rate},push_{seconds:g}s,host_fed,{len(ts)},{np.median(ts) * 1e3:.3f},{max(ts) * 1e3:.3f},{rows},"
                  f"{chunk} samples per push")
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                d_x = torch.from_numpy(x).to(dev)
                with apt.LiveDecoder(settings, apt.Rate.hz(rate), context=apt.Context(device=0, stream=stream.cuda_stream)) as dec:
                    cap = 64
                    d_rows = torch.empty(cap * 2080, dtype=torch.float32, device=dev)
                    d_pos = torch.empty(cap, dtype=torch.int64, device=dev)
                    stream.synchronize()
                    pushes_device(dec, d_x, 4 * chunk, chunk, d_rows, d_pos, cap, finish=False)  # warm-up
                    dec.reset()
                    ts, rows = pushes_device(dec, d_x, x.size, chunk, d_rows, d_pos, cap)
            assert rows == ref_rows, (rows, ref_rows)
            print(f"{rate},push_{seconds:g}s,device,{len(ts)},{np.median(ts) * 1e3:.3f},{max(ts) * 1e3:.3f},{rows},"
                  f"push_device + results() per push")
        # catch-up: ten minutes at once
        y = synth_apt(rate, args.catch_up, 6)
        best_live, best_shot, rows_live, rows_shot = [], [], 0, 0
        with apt.LiveDecoder(settings, apt.Rate.hz(rate)) as dec:
            for _ in range(4):  # (the first is the warm-up)
                dec.reset()
                t0 = time.perf_counter()
                a = dec.push(y)[0].shape[0]
                b = dec.finish()[0].shape[0]
                best_live.append(time.perf_counter() - t0)
                rows_live = a + b
            launches = -(-y.size // dec.info.max_push)
        for _ in range(4):
            t0 = time.perf_counter()
            rows_shot = apt.decode(apt.Context(), settings, y, apt.Rate.hz(rate), True).size // 2080
            best_shot.append(time.perf_counter() - t0)
        assert rows_live == rows_shot, (rows_live, rows_shot)
        print(f"{rate},catch_up,host_fed,1,{min(best_live[1:]) * 1e3:.3f},{max(best_live[1:]) * 1e3:.3f},{rows_live},"
              f"{launches} launch sequences of max_push samples; best and worst of 3")
        print(f"{rate},decode_one_shot,host,1,{min(best_shot[1:]) * 1e3:.3f},{max(best_shot[1:]) * 1e3:.3f},{rows_shot},"
              f"decode() of the same recording; best and worst of 3")


if __name__ == "__main__":
    main()
