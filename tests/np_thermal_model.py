"""The thermal calibration stage (include/aptgpu.h) in numpy: the yardstick of test_thermal_cpu.py and
test_gpu_thermal.py.

The scalars are Python floats (IEEE f64, one rounding per operation, the stated order), so the library's must equal
them bit for bit except n_bb, which goes through one exp.  The pixels are f64 from the f64 scalars: not a restatement
of the kernel's f32 arithmetic but what that arithmetic approximates.  The u8 mapping is f32, as defined.

The telemetry (frame row, the channel's 16 wedge values) is an input: the tests take it from the CPU oracle."""
import math

import numpy as np

f32 = np.float32
PX, HALF, SPACE0, SPACE_N, VIDEO0, VIDEO_N = 2080, 1040, 44, 38, 86, 909
SPACE_ROWS, TRIM = 128, 16
C1, C2 = 1.1910427e-5, 1.4387752
WEDGE_COUNTS = (31.0, 63.0, 95.0, 127.0, 159.0, 191.0, 224.0, 255.0, 0.0)
SET_OF_IDENTITY = {5: 0, 3: 1, 4: 2}  # "3b", "4", "5" -> 3B, 4, 5
REASON_SHORT, REASON_CHANNEL, REASON_DEGENERATE = 2, 13, 14

# Coefficients of the tests: the magnitudes of an AVHRR/3, the values of no satellite.
PRT = ((276.60, 0.051100, 1.400e-6), (276.55, 0.051050, 1.450e-6), (276.65, 0.051150, 1.350e-6),
       (276.58, 0.051080, 1.420e-6))
CH3B = (2670.0, 1.70, 0.99750, 0.0, 0.0, 0.0, 0.0)
CH4 = (928.0, 0.55, 0.99850, -5.5, 5.8, -0.1100, 0.00052)
CH5 = (834.0, 0.40, 0.99900, -3.5, 2.7, -0.0500, 0.00024)
CHANNELS = (CH3B, CH4, CH5)


def key_of(x):
    """IEEE totalOrder as an unsigned compare"""
    b = np.asarray(x, f32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def space_means(rows, telemetry_row, channel):
    """the 128 sequential f32 means of the space view"""
    base = HALF * channel + SPACE0
    band = np.asarray(rows, f32).reshape(-1, PX)[telemetry_row:telemetry_row + SPACE_ROWS, base:base + SPACE_N]
    s = np.zeros(SPACE_ROWS, f32)
    with np.errstate(all="ignore"):
        for i in range(SPACE_N):
            s = (s + band[:, i]).astype(f32)
        return (s / f32(SPACE_N)).astype(f32)


def space_of(means):
    order = np.argsort(key_of(means), kind="stable")  # ties by row
    kept = np.sort(order[TRIM:SPACE_ROWS - TRIM])
    total = 0.0
    for r in kept:
        total = total + float(means[r])
    return total / float(SPACE_ROWS - 2 * TRIM)


def scalars(v, space, prt, ch):
    """v: the channel's wedges 1..16 (f32); ch: nu, A, B, N_s, b0, b1, b2.  -> dict, with ok = not degenerate"""
    x = [float(f32(t)) for t in v[:9]]
    y = list(WEDGE_COUNTS)
    sx = sy = 0.0
    for k in range(9):
        sx = sx + x[k]
        sy = sy + y[k]
    mx, my = sx / 9.0, sy / 9.0
    sxy = sxx = 0.0
    for k in range(9):
        dx = x[k] - mx
        sxy = sxy + dx * (y[k] - my)
        sxx = sxx + dx * dx
    with np.errstate(all="ignore"):
        slope = float(np.float64(sxy) / np.float64(sxx))
        icpt = my - slope * mx

        def count10(u):
            return 4.0 * (slope * float(u) + icpt)

        t = []
        for i in range(4):
            c = count10(f32(v[9 + i]))
            t.append((prt[i][0] + prt[i][1] * c) + prt[i][2] * (c * c))
        t_bb = (((t[0] + t[1]) + t[2]) + t[3]) / 4.0
        nu = ch[0]
        t_eff = ch[1] + ch[2] * t_bb
        try:
            n_bb = float(np.float64(C1 * ((nu * nu) * nu)) / np.float64(math.exp((C2 * nu) / t_eff) - 1.0))
        except (OverflowError, ZeroDivisionError, ValueError):
            n_bb = float("nan")
        c_bb, c_space = count10(f32(v[14])), count10(space)
    out = dict(slope=slope, icpt=icpt, space=space, c_space=c_space, c_bb=c_bb, t_bb=t_bb, n_bb=n_bb)
    out["ok"] = bool(sxx != 0.0 and all(math.isfinite(q) for q in out.values()) and c_space != c_bb)
    return out


def radiance(x, s, ch):
    """N_e of samples x, f64"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        ce = 4.0 * (s["slope"] * x + s["icpt"])
        n_lin = ch[3] + (s["n_bb"] - ch[3]) * (s["c_space"] - ce) / (s["c_space"] - s["c_bb"])
        return n_lin + (ch[4] + ch[5] * n_lin + ch[6] * n_lin * n_lin)


def kelvin_of_radiance(n_e, ch):
    n_e = np.asarray(n_e, np.float64)
    with np.errstate(all="ignore"):
        t = (C2 * ch[0] / np.log(1.0 + C1 * ch[0] ** 3 / n_e) - ch[1]) / ch[2]
    return np.where((n_e > 0) & np.isfinite(n_e), t, np.nan)


def radiance_of_kelvin(t, ch):
    """the inverse of kelvin_of_radiance (to compare cold pixels by their radiance)"""
    t = np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        return C1 * ch[0] ** 3 / np.expm1(C2 * ch[0] / (ch[1] + ch[2] * t))


def calibrate(rows, telemetry_row, values, channel, identity, prt=PRT, channels=CHANNELS):
    """-> (reason, scalars or None, N_e plane f64 or None, Kelvin plane f64 or None)"""
    rows = np.asarray(rows, f32).reshape(-1, PX)
    if identity not in SET_OF_IDENTITY:
        return REASON_CHANNEL, None, None, None
    ch = channels[SET_OF_IDENTITY[identity]]
    means = space_means(rows, telemetry_row, channel)
    s = scalars(values, space_of(means), prt, ch)
    if not s["ok"]:
        return REASON_DEGENERATE, s, None, None
    base = HALF * channel + VIDEO0
    n_e = radiance(rows[:, base:base + VIDEO_N], s, ch)
    return 0, s, n_e, kelvin_of_radiance(n_e, ch)


def levels(kelvin, t_low, t_high, cold_white):
    """the f32 mapping of a Kelvin plane (f32) to levels; NaN -> 0"""
    t = np.asarray(kelvin, f32)
    with np.errstate(all="ignore"):
        s = ((t - f32(t_low)).astype(f32) / f32(f32(t_high) - f32(t_low))).astype(f32)
        s = np.minimum(np.maximum(np.where(np.isnan(t), f32(0), s), f32(0)), f32(1)).astype(f32)
        level = ((s * f32(255)).astype(f32) + f32(0.5)).astype(f32).astype(np.uint8)
    if cold_white:
        level = (255 - level.astype(np.int32)).astype(np.uint8)
    return np.where(np.isnan(t), np.uint8(0), level)


def scale_image(kelvin, channel, image_channels, t_low, t_high, cold_white, palette=None):
    """the scale image of a Kelvin plane (f32, h x 909) in the standard row layout"""
    t = np.asarray(kelvin, f32)
    h = t.shape[0]
    level = levels(t, t_low, t_high, cold_white)
    base = HALF * channel + VIDEO0
    if image_channels == 1:
        img = np.zeros((h, PX), np.uint8)
        img[:, base:base + VIDEO_N] = level
        return img
    table = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1) if palette is None else np.asarray(palette, np.uint8)
    img = np.zeros((h, PX, 4), np.uint8)
    img[:, :, 3] = 255
    rgba = np.concatenate([table[level], np.full(level.shape + (1,), 255, np.uint8)], axis=2)
    rgba[np.isnan(t)] = 0
    img[:, base:base + VIDEO_N] = rgba
    return img


# ---- scenes: row images built directly
WEDGE_OF_IDENTITY = {0: 31.0, 1: 63.0, 2: 95.0, 3: 127.0, 4: 159.0, 5: 191.0}


def scene(h, frame_row, seed, identities=(3, 4), gain=37.5, offset=1200.0, space_noise=0.0, markers=()):
    """h rows: x = gain * count8 + offset.  Wedges 1-9 the count scale, 10-13 the PRTs near 105, 14 the patch, 15 the back
    scan at 100, 16 the wedge of the channel's identity (identities: A's and B's index of the channel-name table);
    space at 248; a count ramp plus seeded texture in the video; a little noise in the telemetry columns (the frame
    search divides by their deviation).  markers: rows (relative to the frame) whose space view is a minute marker."""
    rng = np.random.default_rng(seed)
    c = np.zeros((h, PX), np.float64)
    r = np.arange(h)
    for chn in range(2):
        base = HALF * chn
        c[:, base:base + 39] = 11.0 if chn == 0 else 244.0
        c[:, base + 39:base + 86] = 248.0 + space_noise * rng.standard_normal((h, 47))
        ramp = 40.0 + (252.0 - 40.0) * ((np.arange(VIDEO_N)[None, :] + 3 * r[:, None]) % VIDEO_N) / (VIDEO_N - 1)
        c[:, base + 86:base + 995] = ramp + 1.5 * rng.standard_normal((h, VIDEO_N))
        wedges = np.array(list(WEDGE_COUNTS) + [104.0, 105.0, 106.0, 105.5 + chn, 120.0, 100.0,
                                                WEDGE_OF_IDENTITY[identities[chn]]])
        w = wedges[((r - frame_row) // 8) % 16]
        c[:, base + 995:base + 1040] = w[:, None] + 0.3 * rng.standard_normal((h, 45))
        for m in markers:
            c[frame_row + m, base + 39:base + 86] = 0.0 if chn == 1 else 255.0
    return (gain * c + offset).astype(f32).ravel()
