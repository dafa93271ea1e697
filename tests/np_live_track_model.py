"""Live flywheel sync's definition (include/aptgpu.h §4e) in numpy: the yardstick of the twin and the kernels.

s, best and bp are np_track_model's values of the WHOLE signal F (they are causal: position i is final once i + G <=
work_len), so the model computes them once and then replays what a stream does at every push: which checkpoints the push
crosses, which nodes of each checkpoint's survivor it commits, which of them are released.

Rules (L = 2080 pw, G = 38 pw, K = lag_rows, m = work_len - G or 0):
 1. checkpoint e = 1, 2, ... is processed as soon as m >= e L, in order;
 2. at n = e L: end = first maximum of best over [n - L, n); committed, ascending, is every node v of the chain from end
    through bp with v + (K + 1) L <= n and v >= c + L - w (c: the last committed position; void before the first);
 3. a checkpoint that commits at least one node while c is not a node of its chain counts one relock;
 4. a committed position is released in the push that committed it: row F[v + pw c], score s[v];
 5. finish(): checkpoints with e L <= M = n - G, then end = first maximum over [max(0, M - L), M) and every node under
    the second condition alone; released are those with v + L <= n; n < L + G: too short, nothing released."""
import numpy as np

import np_track_model as tm

f32 = np.float32
TOO_SHORT = "track: the signal is shorter than one row and one sync frame"


def dynamic_programme(s, pw, w, lam):
    """np_track_model.track_scores' programme, returning (best, bp) instead of the back-track of the last row"""
    s = np.asarray(s, dtype=f32)
    M, L = s.size, tm.PX * pw
    C = L - w
    lam = f32(lam)
    best = np.zeros(M, f32)
    bp = np.full(M, tm.START, np.int16)
    ds = tm.offsets(w)
    with np.errstate(all="ignore"):
        for c0 in range(0, M, C):
            i = np.arange(c0, min(M, c0 + C))
            cur = np.where(i < L, f32(0.0), f32(-np.inf)).astype(f32)
            b = np.full(i.size, tm.START, np.int16)
            for d in ds:
                j = i - L - d
                ok = j >= 0
                if not ok.any():
                    continue
                assert j[ok].max() < c0
                v = np.full(i.size, -np.inf, f32)
                v[ok] = best[j[ok]] - lam * f32(abs(d))
                take = ok & (v > cur)
                cur = np.where(take, v, cur)
                b = np.where(take, np.int16(d), b)
            best[i] = s[i] + cur
            bp[i] = b
    assert best.dtype == f32
    return best, bp


class Model:
    """f: the oracle's filtered signal of the complete recording (or of any continuation of what the stream sees before
    finish(): the values below work_len are the same)."""

    def __init__(self, f, pw, w=8, lam=0.1, lag_rows=8):
        self.f = np.ascontiguousarray(f, dtype=f32)
        self.pw, self.w, self.K = pw, int(w), int(lag_rows)
        self.L, self.G = tm.PX * pw, 38 * pw
        self.too_short = self.f.size < self.L + self.G
        if not self.too_short:
            self.s = tm.score(self.f, pw)
            self.best, self.bp = dynamic_programme(self.s, pw, w, lam)
            # the restated programme is np_track_model's: same path from the same end
            assert np.array_equal(self._chain(self._end(self.s.size))[::-1], tm.track_scores(self.s, pw, w, lam))
        self.reset()

    def reset(self):
        self.next_checkpoint, self.c, self.n_positions, self.n_relocks, self.m = 1, None, 0, 0, 0

    def _end(self, hi):
        lo = max(0, hi - self.L)
        return lo + int(np.argmax(self.best[lo:hi]))  # the first maximum

    def _chain(self, end):
        """the survivor's nodes, descending"""
        out, p = [], end
        while True:
            out.append(p)
            if self.bp[p] == tm.START:
                return np.array(out, np.int64)
            p = p - self.L - int(self.bp[p])

    def _commit(self, chain, limit):
        nodes = [int(v) for v in chain[::-1] if (limit is None or v <= limit) and (self.c is None or v >= self.c + self.L - self.w)]
        if nodes and self.c is not None and self.c not in set(int(v) for v in chain):
            self.n_relocks += 1
        if nodes:
            self.c = nodes[-1]
            self.n_positions += len(nodes)
        return nodes

    def push(self, work_len, finish=False):
        """the stream's work signal now has work_len final samples -> (positions, scores, rows) released by this push"""
        L = self.L
        m = max(0, work_len - self.G)
        assert m >= self.m and work_len <= self.f.size
        out = []
        self.m = m
        while self.next_checkpoint * L <= m:
            n = self.next_checkpoint * L
            out += self._commit(self._chain(self._end(n)), n - (self.K + 1) * L)
            self.next_checkpoint += 1
        error = None
        if finish:
            assert work_len == self.f.size
            if self.too_short:
                error = TOO_SHORT
            else:
                nodes = self._commit(self._chain(self._end(m)), None)
                out += [v for v in nodes if v + L <= work_len]
        for v in out:
            assert v + L <= work_len
        pos = np.array(out, np.int64)
        rows = np.stack([self.f[v:v + L:self.pw] for v in out]) if out else np.zeros((0, tm.PX), f32)
        sc = self.s[pos] if out else np.zeros(0, f32)
        if finish:
            return pos, sc, rows, error
        return pos, sc, rows

    def record(self):
        """(m, next checkpoint, n_positions, n_relocks, last committed position or None)"""
        return self.m, self.next_checkpoint, self.n_positions, self.n_relocks, self.c


def run(f, pw, work_lens, w=8, lam=0.1, lag_rows=8):
    """work_lens: the final work samples after every push, the last entry being finish()'s.  -> per call
    (positions, scores, rows, record), and finish()'s error text or None"""
    mdl = Model(f, pw, w, lam, lag_rows)
    calls = []
    for wl in work_lens[:-1]:
        calls.append(mdl.push(wl) + (mdl.record(),))
    pos, sc, rows, error = mdl.push(work_lens[-1], True)
    calls.append((pos, sc, rows, mdl.record()))
    return calls, error
