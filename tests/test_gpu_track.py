"""The flywheel sync stage on the GPU (k_track_score, k_track_dp, k_track_rows) against the numpy model of
np_track_model.py, bit for bit: the small cases of test_track_cpu.py with several recordings of different lengths in
one launch, the plan form behind decode_device on the table's noisy recordings (strict F is bit-identical to the
oracle's, so positions and rows equal the model's on the oracle's filtered signal), decode_tracked on a recording
decode() refuses, and decode()'s own rows around a track_device call."""
import numpy as np
import pytest

import track_cases as tc

import noaa_apt_amd as apt

pytestmark = pytest.mark.gpu

f32 = np.float32
CANARY = f32(-7.25)


def rate_of(pw):
    return apt.Rate.hz(4160 * pw)


def batch(pw):
    """every input kind at every length: twelve recordings of three lengths for one launch"""
    return [(kind, n) for n in tc.lengths(pw) for kind in tc.KINDS]


@pytest.mark.parametrize("pw", tc.PWS)
def test_score_bits(pw):
    cases = batch(pw)
    got = apt.sync_score([tc.signal(kind, pw, n) for kind, n in cases], rate_of(pw))
    for (kind, n), s in zip(cases, got):
        assert s.size == n - 38 * pw
        assert np.array_equal(tc.bits(s), tc.bits(tc.model_score(kind, pw, n))), (pw, kind, n)
    kind, n = cases[-4]
    alone = apt.sync_score(tc.signal(kind, pw, n), rate_of(pw))
    assert np.array_equal(tc.bits(alone), tc.bits(tc.model_score(kind, pw, n)))


@pytest.mark.parametrize("w,lam", tc.SETTINGS)
@pytest.mark.parametrize("pw", tc.PWS)
def test_track_bits(pw, w, lam):
    cases = batch(pw)
    got = apt.track_sync([tc.signal(kind, pw, n) for kind, n in cases], rate_of(pw), apt.TrackSettings(w, lam),
                         return_info=True)
    for (kind, n), g in zip(cases, got):
        tc.check_track(g, tc.model_track(kind, pw, n, w, lam), (pw, kind, n, w, lam))
        tc.check_invariants(g[0], pw, n, w, (pw, kind, n, w, lam))
        info = g[3]
        assert info.status == 0 and info.n == n and info.n_positions == g[0].size and info.n_rows == g[2].shape[0]
        assert info.end == g[0][-1]


def test_track_gain_and_single_signal():
    pw, n = 3, tc.lengths(3)[2]
    for gain in (10, -10):
        pos, sc, rows = apt.track_sync(tc.scaled("noise", pw, n, gain), rate_of(pw))
        want = tc.model_track("noise", pw, n, 8, 0.1)
        assert np.array_equal(pos.astype(np.int64), want[0]) and np.array_equal(tc.bits(sc), tc.bits(want[1]))
    pos, sc, rows = apt.track_sync(tc.signal("noise", pw, n), rate_of(pw), rows=False)
    assert rows is None and np.array_equal(pos.astype(np.int64), tc.model_track("noise", pw, n, 8, 0.1)[0])


@pytest.mark.parametrize("rate,profile,sync", [(11025, "standard", True), (11025, "standard", False),
                                               (48000, "fast", True)])
def test_plan_track_device(rate, profile, sync):
    """table rows 2 and 5 (sigma 8 000; sigma 20 000 with a dropout), 40 s, in one call; and decode()'s own rows,
    records and positions on the same plan are what they were before the track_device call in between"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    rows_of_table = (1, 4)
    recs = [tc.recording_at(r, rate) for r in rows_of_table]
    recs[1] = recs[1][:-rate]  # (two lengths in the launch; the model below is of the same cut)
    k = len(recs)
    settings = apt.Settings.profile(profile)
    pw = settings.work_rate // 4160
    plan = apt.Plan(settings, apt.Rate.hz(rate), sync, max_samples=max(r.size for r in recs), max_batch=k)
    plan.enable_timing(2)
    cap = int(plan.info.max_rows)
    floats = cap * 2080 if sync else int(plan.info.max_work_len) + 2080
    d_in = [torch.from_numpy(np.array(r)).to(dev) for r in recs]
    d_rows = [torch.zeros(floats, dtype=torch.float32, device=dev) for _ in recs]
    d_trk = [torch.full((cap * 2080 + 64,), float(CANARY), dtype=torch.float32, device=dev) for _ in recs]
    in_p, rows_p, trk_p = ([t.data_ptr() for t in ts] for ts in (d_in, d_rows, d_trk))
    with pytest.raises(apt.InvalidError):
        plan.track_device(trk_p, [cap] * k)  # nothing decoded yet
    plan.decode_device(in_p, [r.size for r in recs], rows_p, [cap if sync else floats // 2080] * k)
    res0 = [(r.status, r.reason, r.n_rows, r.n_sync, r.work_len, r.n_out) for r in plan.results(k)]
    before = [t.clone() for t in d_rows]  # (results() waited for the plan's streams)
    pos0 = [plan.sync_positions(i) for i in range(k)] if sync else None
    plan.track_device(trk_p, [cap] * k, apt.TrackSettings(8, 0.1))
    tres = plan.track_results(k)
    from oracle import binding as oracle
    import np_track_model as tm
    for i, row in enumerate(rows_of_table):
        if i == 0:
            wpos, wsc, wrows = tc.model_at(row, rate, profile)
        else:
            osettings = {"standard": oracle.STANDARD, "fast": oracle.FAST}[profile]
            _, steps = oracle.decode(recs[i], rate, False, settings=osettings, want_steps=True)
            wpos, wsc, wrows, _ = tm.track(steps["filtered"], pw, 8, 0.1)
        pos, sc = plan.track_positions(i)
        got = d_trk[i].cpu().numpy()
        h = wrows.shape[0]
        assert (tres[i].status, tres[i].reason, tres[i].n_positions, tres[i].n_rows) == (0, 0, wpos.size, h), (i, tres[i].n_rows)
        assert tres[i].n == res0[i][4]
        tc.check_track((pos, sc, got[:h * 2080].reshape(h, 2080)), (wpos, wsc, wrows), (rate, profile, sync, i))
        assert np.all(got[h * 2080:] == CANARY), "a write behind the rows"
        if row == 4:  # the rows the reference loses: within one pixel of truth at the standard profile
            if rate == tc.RATE:
                assert tc.errors(pos, 0.0).max() <= 3.0
    # the decode's own outputs are untouched, and a decode after the stage gives the same again
    assert [(r.status, r.reason, r.n_rows, r.n_sync, r.work_len, r.n_out) for r in plan.results(k)] == res0
    for t, b in zip(d_rows, before):
        assert torch.equal(t, b)
    if sync:
        for i in range(k):
            assert np.array_equal(plan.sync_positions(i), pos0[i])
    for t in d_rows:
        t.zero_()
    plan.decode_device(in_p, [r.size for r in recs], rows_p, [cap if sync else floats // 2080] * k)
    assert [(r.status, r.reason, r.n_rows, r.n_sync, r.work_len, r.n_out) for r in plan.results(k)] == res0
    for t, b in zip(d_rows, before):
        assert torch.equal(t, b)
    # a rows_cap below the path's rows: truncated, recorded as reason 4, nothing written behind
    for t in d_trk:
        t.fill_(float(CANARY))
    plan.track_device(trk_p, [5, 0], apt.TrackSettings(8, 0.1))
    tres = plan.track_results(k)
    assert (tres[0].status, tres[0].reason, tres[0].n_rows) == (0, 4, 5)
    assert (tres[1].status, tres[1].reason, tres[1].n_rows) == (0, 4, 0)
    assert np.all(d_trk[0].cpu().numpy()[5 * 2080:] == CANARY) and np.all(d_trk[1].cpu().numpy() == CANARY)
    timing = plan.collect_timing()
    assert {"track_score", "track_dp", "track_rows"} <= set(timing)
    with pytest.raises(apt.InvalidError):
        plan.track_device(trk_p, [cap] * k, apt.TrackSettings(65, 0.1))
    plan.close()


def test_decode_tracked_where_decode_refuses(oracle):
    x = tc.weak_recording()
    st = apt.Settings.profile("standard")
    with pytest.raises(apt.InternalError, match="less than 5 sync frames"):
        apt.decode(apt.Context(device=0), st, x, apt.Rate.hz(tc.RATE), True)
    f, wpos, wsc, wrows = tc.weak_model()
    rows, pos, sc, info = apt.decode_tracked(apt.Context(device=0), st, x, apt.Rate.hz(tc.RATE), return_info=True)
    assert rows.size == wrows.size and rows.size >= 10 * 2080
    tc.check_track((pos, sc, rows.reshape(-1, 2080)), (wpos, wsc, wrows), "decode_tracked")
    assert info.status == 0 and info.n == f.size and (sc[:3] > 0.8).all()
    assert np.array_equal(tc.bits(apt.decode_tracked(None, st, x, apt.Rate.hz(tc.RATE))), tc.bits(rows))
    # the reference's "less than 10 rows" stays
    with pytest.raises(apt.InternalError, match="less than 10 rows"):
        apt.decode_tracked(None, st, x[:tc.RATE * 4], apt.Rate.hz(tc.RATE))


def test_plan_track_after_a_decode_with_too_few_frames_and_after_a_too_short_one():
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    recs = [np.array(tc.weak_recording()), np.array(tc.weak_recording()[:tc.RATE * 4])]
    st = apt.Settings.profile("standard")
    plan = apt.Plan(st, apt.Rate.hz(tc.RATE), True, max_samples=recs[0].size, max_batch=2)
    cap = int(plan.info.max_rows)
    d_in = [torch.from_numpy(r).to(dev) for r in recs]
    d_rows = [torch.zeros(cap * 2080, dtype=torch.float32, device=dev) for _ in recs]
    rows_p = [t.data_ptr() for t in d_rows]
    plan.decode_device([t.data_ptr() for t in d_in], [r.size for r in recs], rows_p, [cap] * 2)
    res = plan.results(2)
    assert (res[0].status, res[0].reason) == (1, 2) and (res[1].status, res[1].reason) == (1, 1)
    plan.track_device(rows_p, [cap] * 2)  # (the decode wrote no rows: its own buffer takes the tracked ones)
    tres = plan.track_results(2)
    f, wpos, wsc, wrows = tc.weak_model()
    pos, sc = plan.track_positions(0)
    h = wrows.shape[0]
    assert (tres[0].status, tres[0].n_rows) == (0, h)
    tc.check_track((pos, sc, d_rows[0].cpu().numpy()[:h * 2080].reshape(h, 2080)), (wpos, wsc, wrows), "plan, few frames")
    assert (tres[1].status, tres[1].reason, tres[1].n_positions, tres[1].n_rows) == (1, 1, 0, 0)
    plan.close()
