"""The AFC in front of the FM demodulator on the GPU (k_afc_sums, k_afc_table, k_fm_tracked; include/aptgpu.h §4b',
DESIGN.md §27) through the assertions of afc_cases.py that test_afc_cpu.py makes on the twin, the device-resident form
(batch position, pointer alignment, the table left in the caller's buffers) and the decode behind it."""
import numpy as np
import pytest

import afc_cases as ac
import fm_cases as fc
import np_afc_model as am
import np_fm_model as fm

import noaa_apt_amd as apt

pytestmark = pytest.mark.gpu

B = ac.GPU
f32 = np.float32
CANARY = f32(-7.25)


# ---------------------------------------------------------------- 1. sums
@pytest.mark.parametrize("case", ac.SUMS_CASES, ids=[c[0] for c in ac.SUMS_CASES])
def test_sums_bit_for_bit(case):
    ac.check_sums_case(B, case)


def test_sums_f32():
    ac.check_sums_f32(B)


def _device_run(st, afc, recordings, offset_components=0, max_frames=1 << 16):
    """FmAfc.demodulate_device on a batch with every optional output given: -> list of (audio, sums, records, coherence,
    good).  Every output carries canaries behind its length; the inputs sit `offset_components` components behind an
    aligned base."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    fmd = apt.FmDemodulator(st)
    dafc = apt.FmAfc(fmd, afc, max_frames=max_frames)
    cb = fm.DTYPES[st.format].itemsize
    keep, args, lens = [], {k: [] for k in ("iq", "n", "audio", "cap", "sums", "table", "coh", "good")}, []
    for iq in recordings:
        raw = np.frombuffer(np.ascontiguousarray(iq).tobytes(), np.uint8)
        buf = torch.zeros(raw.size + 64, dtype=torch.uint8, device=dev)
        off = offset_components * cb
        if raw.size:
            buf[off:off + raw.size] = torch.from_numpy(raw.copy()).to(dev)
        n = len(iq) // 2
        nb, cap = dafc.n_blocks(n), fmd.out_len(n)
        outs = dict(audio=torch.full((cap + 32,), float(CANARY), dtype=torch.float32, device=dev),
                    sums=torch.full((3 * nb + 8,), float(CANARY), dtype=torch.float64, device=dev),
                    table=torch.full((4 * nb + 8,), float(CANARY), dtype=torch.float32, device=dev),
                    coh=torch.full((nb + 8,), float(CANARY), dtype=torch.float32, device=dev),
                    good=torch.full((nb + 8,), 77, dtype=torch.uint8, device=dev))
        keep.append((buf, outs))
        lens.append((cap, nb))
        args["iq"].append(buf.data_ptr() + off)
        args["n"].append(n)
        args["cap"].append(cap)
        for k, t in outs.items():
            args[k].append(t.data_ptr())
    dafc.demodulate_device(args["iq"], args["n"], args["audio"], args["cap"], d_table=args["table"],
                           d_coherence=args["coh"], d_good=args["good"], d_sums=args["sums"])
    torch.cuda.synchronize()
    got = []
    for (_, outs), (cap, nb) in zip(keep, lens):
        h = {k: t.cpu().numpy() for k, t in outs.items()}
        assert np.all(h["audio"][cap:] == CANARY) and np.all(h["sums"][3 * nb:] == float(CANARY))
        assert np.all(h["table"][4 * nb:] == CANARY) and np.all(h["coh"][nb:] == CANARY) and np.all(h["good"][nb:] == 77)
        got.append((h["audio"][:cap].copy(), h["sums"][:3 * nb].reshape(-1, 3).copy(),
                    h["table"][:4 * nb].copy().view(apt.AFC_RECORD_DTYPE), h["coh"][:nb].copy(), h["good"][:nb].astype(bool)))
    dafc.close()
    fmd.close()
    return got


@pytest.mark.parametrize("fmt,b,lag", [(fm.S16, 64, 7), (fm.U8, 4096, 1)], ids=["s16-B64-L7", "u8-B4096-L1"])
def test_sums_four_recordings_in_one_launch_and_an_unaligned_pointer(fmt, b, lag):
    base = ac._base(fmt)
    st, afc = ac.settings(5, fmt), apt.AfcSettings(block_frames=b, lag=lag)
    recs = [base[:2 * 1003], base[:0], base[:2 * 24000], base[:2 * 5]]
    for off in (0, 1):  # 1: one component off a 16-byte boundary, the narrow loads
        for iq, (_, s, _, _, _) in zip(recs, _device_run(st, afc, recs, offset_components=off)):
            ac.check_sums_exact(s, iq, fmt, b, lag, False, f"device form, offset {off}, n={iq.size // 2}")


# ---------------------------------------------------------------- 2. table
def test_table_gated_signal():
    ac.check_table_gated(B)


def test_table_no_good_block():
    ac.check_table_no_good_block(B)


def test_table_window_of_one_and_wider_than_the_recording():
    ac.check_table_windows(B)


def test_table_nan_frame():
    ac.check_table_nan_frame(B)


def test_table_base_shift_of_100_khz_with_lag_3():
    ac.check_table_base_shift(B)


def test_table_of_more_blocks_than_one_scan_chunk():
    """B = 64 over 2 s: 7500 blocks, eight chunks of the table kernel's scans, with the hold carried across them"""
    iq, _ = ac.swept(5, fm.U8, 2.0, sigma=0.05, gate=0.4)
    afc = apt.AfcSettings(block_frames=64, smooth_blocks=255)
    ac.run_table_case(B, iq, ac.settings(5, fm.U8), afc, "B=64, 7500 blocks",
                      lambda g: g.any() and not g[:1200].any() and not g[-1200:].any())


# ---------------------------------------------------------------- 3. tracked demodulation
@pytest.mark.parametrize("b", [64, 1 << 16], ids=["B64", "B65536"])
@pytest.mark.parametrize("case", fc.BOUND_CASES, ids=fc.IDS)
def test_tracked_bound(case, b):
    ac.check_tracked_bound(B, case, b)


def test_constant_table_equals_fm_demodulate():
    ac.check_constant_table_is_plain(B)


@pytest.mark.parametrize("fmt", [fm.S16, fm.U8, fm.F32], ids=["s16", "u8", "f32"])
def test_batch_position_and_pointer_alignment(fmt):
    iq, _ = ac.swept(5, fmt, 0.5, sigma=0.05)
    st, afc = ac.settings(5, fmt), apt.AfcSettings(block_frames=1024, smooth_blocks=5)
    t = apt.fm_design(st).n_taps
    alone, _, table = apt.fm_demodulate_afc(iq, st, afc)
    recs = [iq[:0], iq[:2 * (t - 1)], iq, iq[:2 * 30001]]
    batch = _device_run(st, afc, recs, max_frames=iq.size // 2)
    assert [r[0].size for r in batch][:3] == [0, 0, alone.size]
    shifted = _device_run(st, afc, [iq], offset_components=1, max_frames=iq.size // 2)[0]
    for audio, _, records, coh, good in (batch[2], shifted):
        assert audio.tobytes() == alone.tobytes()
        assert records.tobytes() == table.records.tobytes() and coh.tobytes() == table.coherence.tobytes()
        assert good.tolist() == table.good.tolist()
    part, _, _ = apt.fm_demodulate_afc(recs[3], st, afc)
    assert batch[3][0].tobytes() == part.tobytes()


def test_device_form_refusals():
    st = ac.settings(5, fm.S16)
    fmd = apt.FmDemodulator(st)
    dafc = apt.FmAfc(fmd, apt.AfcSettings(), max_frames=10000)
    t, d = fmd.info.n_taps, 5
    with pytest.raises(apt.InvalidError, match="max_frames"):
        dafc.demodulate_device([256], [10001], [256], [1 << 20])
    with pytest.raises(apt.InvalidError, match="audio_cap"):
        dafc.demodulate_device([256], [t + d], [256], [0])
    with pytest.raises(apt.InvalidError, match="null"):
        dafc.demodulate_device([0], [t + d], [256], [1])
    with pytest.raises(apt.InvalidError, match="aligned"):
        dafc.demodulate_device([257], [t + d], [256], [1])
    with pytest.raises(apt.InvalidError, match="d_table"):
        dafc.demodulate_device([256], [t + d], [256], [1], d_table=[264])
    dafc.demodulate_device([], [], [], [])
    fmd.close()  # the demodulator first: the FmAfc refuses to run without it and still closes
    with pytest.raises(apt.InvalidError, match="closed"):
        dafc.demodulate_device([], [], [], [])
    dafc.close()


# ---------------------------------------------------------------- 4. end to end
@pytest.mark.parametrize("case", ac.E2E_CASES, ids=ac.E2E_IDS)
def test_end_to_end_table_and_audio(case):
    ac.check_end_to_end_table(B, case)


def test_end_to_end_rows():
    """6 s, D = 5, u8, the carrier sweeping 12 -> 6 kHz with shift_hz = 0: the rows of decode(audio_afc) against the rows
    of decode() of the stage-C model's audio for the same table: the same row count and sync positions, pixels within
    test_gpu_fm.py's end-to-end tolerance (1e-4 of their range)."""
    d, fmt = 5, fm.U8
    iq, _ = ac.swept(d, fmt, 6.0, seed=23)
    st, afc = ac.settings(d, fmt), apt.AfcSettings()
    audio, rate, table = apt.fm_demodulate_afc(iq, st, afc)
    model, _ = am.demodulate_tracked(iq, fmt, st.sample_rate, d, apt.fm_design(st).taps, table.records, afc.block_frames)
    assert rate.get_hz() == 48000 and audio.size == model.size
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n = audio.size
    plan = apt.Plan(apt.Settings(), rate, True, max_samples=n, max_batch=1)
    cap = int(plan.info.max_rows)
    d_rows = torch.zeros(cap * 2080, dtype=torch.float32, device=dev)

    def decode_on(a):
        d_audio = torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(dev)
        plan.decode_device([d_audio.data_ptr()], [n], [d_rows.data_ptr()], [cap])
        res = plan.results(1)[0]
        assert res.status == 0
        return d_rows[:int(res.n_out)].cpu().numpy().copy(), plan.sync_positions(0).copy()

    rows, pos = decode_on(audio)
    rows_model, pos_model = decode_on(model)
    plan.close()
    assert rows.size == rows_model.size and rows.size >= 8 * 2080
    assert pos.tolist() == pos_model.tolist()
    span = float(rows_model.max() - rows_model.min())
    delta = float(np.abs(rows.astype(np.float64) - rows_model.astype(np.float64)).max())
    print(f"afc end to end: {rows.size // 2080} rows, max|rows - rows_model| = {delta:.3e} = {delta / span:.3e} of the range")
    assert delta <= 1e-4 * span
    # ... and without the AFC the picture is not there: shift_hz = 0 wraps the discriminator
    plain, _ = apt.fm_demodulate(iq, st)
    assert float(np.abs(plain.astype(np.float64) - model).max()) > 0.5
