"""The release schedule of live decode (include/aptgpu.h §4d) from the oracle's outputs for the WHOLE
recording: which work samples, scan positions and rows are final after n input samples.  The model never looks at the
stream under test: it takes the oracle's filters (tap counts), its correlation and its peaks, replays the reference's
sequential scan (decode.rs:239-253) in plain Python to learn at which scan index every peak received its successor, and
applies the definition.  (tests/test_picker_reformulation.py is the precedent for such a scan model.)"""
import math

import numpy as np


class Geometry:
    def __init__(self, input_rate, work_rate, n_resample_taps, n_lowpass_taps):
        g = math.gcd(int(input_rate), int(work_rate))
        self.l, self.m = work_rate // g, input_rate // g
        self.t1, self.t2 = int(n_resample_taps), int(n_lowpass_taps)
        self.off = (self.t1 - 1) // 2
        self.pw = work_rate // 4160
        self.spr = 2080 * work_rate // 4160
        self.md = self.spr * 8 // 10
        self.G = 38 * self.pw

    def work_len(self, n, finish=False):
        """final work samples after n input samples; finish: the recording ends there (fast_resampling's own count)"""
        if self.l == 1:
            return n // self.m  # decimate: k < n / m
        total = n * self.l
        if finish:  # t = off + k m < n l
            return 0 if total <= self.off else -((self.off - total) // self.m)
        # R[k] reads input indices up to floor((off + k m + off) / l): all pushed  <=>  k m + 2 off < n l
        return 0 if total <= 2 * self.off else -((2 * self.off - total) // self.m)

    def scan_end(self, work_len):
        """positions scanned: i + G < work_len"""
        return max(0, work_len - self.G)

    def samples_for(self, work_len):
        """the fewest input samples whose finished recording has at least work_len work samples"""
        n = work_len * self.m // self.l
        while self.work_len(n, True) >= work_len and n > 0:
            n -= 1
        while self.work_len(n, True) < work_len:
            n += 1
        return n


def replay(corr, spr, md):
    """decode.rs:239-253 over the whole correlation.  Returns (positions, succ_at): succ_at[k] is the scan index at
    which peak k's successor was pushed, -1 for the last peak."""
    peaks = [[0, np.float32(0.0)]]
    succ_at = [-1]
    for i in range(len(corr)):
        c = corr[i]
        if i - peaks[-1][0] > md:
            while i // spr > len(peaks):
                succ_at[-1] = i
                peaks.append([i, c])
                succ_at.append(-1)
        elif c > peaks[-1][1]:
            peaks[-1] = [i, c]
    return np.array([p for p, _ in peaks], np.int64), np.array(succ_at, np.int64)


class Model:
    """corr: the oracle's correlation of the complete recording (None: sync off); a recording that the stream sees only
    a prefix of may hand in the correlation of any continuation — what is released before finish() is the same."""

    def __init__(self, geom, corr, sync):
        self.g, self.sync = geom, sync
        if sync:
            self.positions, self.succ_at = replay(np.asarray(corr, np.float32), geom.spr, geom.md)

    def rows_due(self, work_len):
        g = self.g
        if not self.sync:
            return work_len // g.spr  # (r + 1) spr <= work_len
        s_end = g.scan_end(work_len)
        ok = (self.succ_at >= 0) & (self.succ_at < s_end) & (self.positions + g.spr < work_len)
        k = int(ok.sum())
        assert ok[:k].all()  # positions never decrease: the rows that are due are a prefix
        return k

    def n_sync(self, work_len):
        if not self.sync:
            return 0
        s_end = self.g.scan_end(work_len)
        return 1 + int(((self.succ_at >= 0) & (self.succ_at < s_end)).sum())

    def schedule(self, chunk_sizes):
        """(work_len, scan_pos, n_rows, n_sync) after every push"""
        out, n, released = [], 0, 0
        for c in chunk_sizes:
            n += int(c)
            w = self.g.work_len(n)
            due = self.rows_due(w)
            out.append((w, self.g.scan_end(w) if self.sync else 0, due - released, self.n_sync(w)))
            released = due
        return out

    def finish(self, n_total, released):
        """(work_len, scan_pos, n_rows, n_sync, error text or None) of finish()"""
        g = self.g
        w = g.work_len(n_total, True)
        ns = self.n_sync(w)
        err = None
        if w < 10 * g.spr:
            err = "Got less than 10 rows of samples, audio file is too short"
        elif self.sync and ns < 5:
            err = "Found less than 5 sync frames, audio file is too short or too noisy"
        n_rows = 0 if err else self.rows_due(w) - released
        return w, (g.scan_end(w) if self.sync else 0), n_rows, ns, err
