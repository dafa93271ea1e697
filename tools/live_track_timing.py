"""Wall time of a tracked live decode beside the untracked one: the median per push of 0.25 s and 1 s of
audio at 11 025 Hz and 48 kHz over a 60 s recording, host-fed (through the Python decoder, which for a tracked stream
also reads the lock indicators and the tracker's record back) and device-resident (push_device and a wait for the
stream), and a ten-minute catch-up in one push, tracked and untracked, beside one-shot decode_tracked() of the same
recording.  Records, not thresholds.  Usage: python tools/live_track_timing.py [OUT.txt] [--host]
(--host: a short dry run on the CPU twin, to check the tool itself)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import noaa_apt_amd as apt  # noqa: E402
from noaa_apt_amd.testing.synth import synth_apt  # noqa: E402


def per_push(dec, x, chunk):
    times = []
    for at in range(0, x.size, chunk):
        t0 = time.perf_counter()
        dec.push(x[at:at + chunk])
        times.append(time.perf_counter() - t0)
    dec.finish()
    return statistics.median(times[2:]) * 1e3


def per_push_device(st, rate, x, chunk, tr):
    """push_device from a device copy of x into preallocated buffers, then a wait for the stream: median ms"""
    import torch
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_x = torch.from_numpy(x.copy()).to(dev)
        with apt.LiveDecoder(st, apt.Rate.hz(rate), track=tr, context=apt.Context(device=0, stream=stream.cuda_stream)) as dec:
            # (an untracked stream that is never asked for its record sees its bound grow by a row per row pushed)
            cap = x.size // (rate // 2) + 64
            d_rows = torch.empty(cap * 2080, dtype=torch.float32, device=dev)
            d_pos = torch.empty(cap, dtype=torch.int64, device=dev)
            times = []
            for rep in range(2):  # (the first walk: module load, allocations)
                times.clear()
                for at in range(0, x.size - chunk + 1, chunk):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    dec.push_device(d_x.data_ptr() + 4 * at, chunk, d_rows.data_ptr(), d_pos.data_ptr(), cap)
                    stream.synchronize()
                    times.append(time.perf_counter() - t0)
                dec.results()
                dec.reset()
    return statistics.median(times[2:]) * 1e3


def main():
    args = [a for a in sys.argv[1:] if a != "--host"]
    host = "--host" in sys.argv[1:]
    minutes = 0.5 if host else 10.0
    lines = []
    st = apt.Settings.profile("standard")
    track = apt.LiveTrackSettings()
    for rate in (11025, 48000):
        x = synth_apt(rate, 60, seed=3, noise_sigma=4000.0)
        for seconds in (0.25, 1.0):
            chunk = int(rate * seconds)
            row = []
            for tr in (None, track):
                with apt.LiveDecoder(st, apt.Rate.hz(rate), track=tr, host=host) as dec:
                    per_push(dec, x[:rate * 8], chunk)  # (first use: module load, allocations)
                    dec.reset()
                    row.append(per_push(dec, x, chunk))
            lines.append(f"{rate} Hz, push of {seconds} s, host-fed, median ms: untracked {row[0]:.3f}  tracked {row[1]:.3f}")
            if not host:
                row = [per_push_device(st, rate, x, chunk, tr) for tr in (None, track)]
                lines.append(f"{rate} Hz, push of {seconds} s, device-resident, median ms: untracked {row[0]:.3f}  tracked {row[1]:.3f}")
        long = synth_apt(rate, 60 * minutes, seed=4, noise_sigma=4000.0)
        catch = []
        for tr in (None, track):
            with apt.LiveDecoder(st, apt.Rate.hz(rate), track=tr, host=host) as dec:
                dec.push(long[:rate])
                dec.reset()
                t0 = time.perf_counter()
                rows, _ = dec.push(long)
                t1 = time.perf_counter()
                dec.finish()
            catch.append(1e3 * (t1 - t0))
        if host:
            lines.append(f"{rate} Hz, {minutes} minutes in one push on the twin: untracked {catch[0]:.1f} ms, tracked {catch[1]:.1f} ms ({rows.shape[0]} rows)")
            continue
        apt.decode_tracked(apt.Context(device=0), st, long[:rate * 20], apt.Rate.hz(rate))
        t2 = time.perf_counter()
        one = apt.decode_tracked(apt.Context(device=0), st, long, apt.Rate.hz(rate))
        t3 = time.perf_counter()
        lines.append(f"{rate} Hz, ten minutes in one host-fed push: untracked stream {catch[0]:.1f} ms, tracked stream {catch[1]:.1f} ms "
                     f"({rows.shape[0]} rows), "
                     f"decode_tracked {1e3 * (t3 - t2):.1f} ms ({one.size // 2080} rows)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args:
        with open(args[0], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
