"""The flywheel sync stage's definition (include/aptgpu.h, "flywheel sync") in numpy.

Every value is IEEE f32 and every operation is rounded on its own, in the order the definition writes them: the loops
run over the window index j (or the candidate offset d) and vectorise over the position i, so that numpy performs
exactly one f32 operation per element and step.  The library's twin and kernels must reproduce these bits."""
import numpy as np

f32 = np.float32
START = -128  # back-pointer of a path's first position
PX = 2080


def geometry(n, pw):
    L, G = PX * pw, 38 * pw
    return L, G, n - G


def template_plus(pw):
    """generate_sync_frame (decode.rs:188-198) as booleans: True where the template is +1"""
    j = np.arange(38 * pw)
    pulse = 2 * pw
    return (j >= pulse) & (j < 15 * pulse) & ((((j - pulse) // pulse) & 1) == 1)


def score(x, pw):
    """s[0..M): the zero-mean normalised cross-correlation with the sync template; 0 where there is no evidence"""
    x = np.ascontiguousarray(x, dtype=f32)
    L, G, M = geometry(x.size, pw)
    assert x.size >= L + G
    plus = template_plus(pw)
    c = np.zeros(M, f32)
    s1 = np.zeros(M, f32)
    s2 = np.zeros(M, f32)
    with np.errstate(all="ignore"):
        for j in range(G):
            v = x[j:j + M]
            c = (c + v) if plus[j] else (c - v)
            s1 = s1 + v
            s2 = s2 + v * v
        m = s1 / f32(G)
        var = s2 - s1 * m
        num = c + s1 * f32(10.0 / 38.0)
        den = np.sqrt(var * f32(G * (1.0 - (10.0 / 38.0) * (10.0 / 38.0))))  # the constant in f64, rounded once
        ok = (var > f32(1e-4) * s2) & np.isfinite(num) & np.isfinite(den)
        s = np.where(ok, num / np.where(ok, den, f32(1.0)), f32(0.0)).astype(f32)
    assert s.dtype == f32 and c.dtype == f32 and var.dtype == f32
    return s


def offsets(w):
    """the candidate order 0, -1, +1, -2, +2, ..., -w, +w"""
    out = [0]
    for k in range(1, w + 1):
        out += [-k, k]
    return out


def track_scores(s, pw, w=8, lam=0.1):
    """The dynamic programme over the scores s[0..M) and its back-track: positions (ascending, int64)."""
    s = np.asarray(s, dtype=f32)
    M = s.size
    L = PX * pw
    C = L - w
    lam = f32(lam)
    best = np.zeros(M, f32)
    bp = np.full(M, START, np.int16)
    ds = offsets(w)
    for c0 in range(0, M, C):
        i = np.arange(c0, min(M, c0 + C))
        cur = np.where(i < L, f32(0.0), f32(-np.inf)).astype(f32)
        b = np.full(i.size, START, np.int16)
        for d in ds:
            j = i - L - d
            ok = j >= 0
            if not ok.any():
                continue
            assert j[ok].max() < c0  # every predecessor lies in an earlier chunk
            v = np.full(i.size, -np.inf, f32)
            v[ok] = best[j[ok]] - lam * f32(abs(d))
            take = ok & (v > cur)
            cur = np.where(take, v, cur)
            b = np.where(take, np.int16(d), b)
        best[i] = s[i] + cur
        bp[i] = b
    lo = max(0, M - L)
    p = lo + int(np.argmax(best[lo:M]))  # (argmax: the first maximum)
    pos = []
    while True:
        pos.append(p)
        if bp[p] == START:
            break
        p = p - L - int(bp[p])
    return np.array(pos[::-1], dtype=np.int64)


def rows_of(x, pos, pw):
    x = np.asarray(x, dtype=f32)
    L = PX * pw
    keep = [int(p) for p in pos if int(p) + L <= x.size]
    if not keep:
        return np.zeros((0, PX), f32)
    return np.stack([x[p:p + L:pw] for p in keep])


def track(x, pw, w=8, lam=0.1):
    """(positions, per-position scores, rows, s) of the whole stage"""
    s = score(x, pw)
    pos = track_scores(s, pw, w, lam)
    return pos, s[pos], rows_of(x, pos, pw), s
