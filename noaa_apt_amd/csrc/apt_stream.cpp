// apt_stream.cpp — live decode on the CPU: the design and every refusal the entry points share (all of them before a
// device is touched), and the state machine of apt_kernels_stream.hpp in plain C++ over host rings
// (aptgpu_stream_create_host), which the kernels are tested against besides the model of tests/np_stream_model.py.
// The twin indexes its rings exactly as the kernels do and refuses to read an index that is no longer (or not yet) live.
// HostLive::push, the splitting of a push into segments of max_push for either twin, is here too.
#include "apt_kernels_stream.hpp"

#include <algorithm>

#include "apt_front_end.hpp"

namespace apt::stream {

namespace {

uint32_t pow2_ceil(uint64_t v)
{
    uint64_t c = 64;
    while (c < v) c <<= 1;
    if (c > (1ull << 31)) throw Error{ErrorKind::Invalid, "stream: max_push too large for the rings"};
    return static_cast<uint32_t>(c);
}

[[noreturn]] void overrun(const char *which)
{
    throw Error{ErrorKind::Internal, std::string("stream: read of a ") + which + " ring index that is not live"};
}

}  // namespace

Design design_stream(const aptgpu_settings *settings, const aptgpu_stream_settings *ss, int mode, bool mfma_switch)
{
    if (!settings || !ss) throw Error{ErrorKind::Invalid, "stream: null argument"};
    if (ss->struct_size < sizeof(aptgpu_stream_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_stream_settings: struct_size not set"};
    if (ss->format != APTGPU_STREAM_F32 && ss->format != APTGPU_STREAM_S16)
        throw Error{ErrorKind::Invalid, "stream: unknown sample format"};
    if (ss->input_rate_hz == 0) throw Error{ErrorKind::Invalid, "stream: input rate must not be 0"};
    if (ss->max_push > kMaxMaxPush) throw Error{ErrorKind::Invalid, "stream: max_push must be at most 2^24 samples"};
    if (mode != APTGPU_MODE_STRICT && mode != APTGPU_MODE_GENERIC)
        throw Error{ErrorKind::Unsupported, "stream: strict mode only (no MODE_FAST, no fp16 taps)"};
    if (mfma_switch) throw Error{ErrorKind::Unsupported, "stream: strict mode only (the matrix-core switch is set)"};
    if (settings->export_wav || settings->export_resample_filtered)
        throw Error{ErrorKind::Unsupported, "stream: export_wav and export_resample_filtered are not offered"};

    const bool sync = ss->sync != 0;
    const PlanDesign pd = design_plan(*settings, ss->input_rate_hz, sync);  // the reference's messages
    if (!pd.work_is_multiple) throw Error{ErrorKind::Internal, "work_rate is not multiple of FINAL_RATE"};  // decode.rs:172-176

    Design d;
    d.work_rate = settings->work_rate;
    Params &P = d.P;
    P.l = pd.l;
    P.m = pd.m;
    P.t1 = static_cast<uint32_t>(pd.taps_resample.size());
    if (P.t1 == 0 || pd.taps_lowpass.empty()) throw Error{ErrorKind::Invalid, "stream: empty filter"};
    P.jlim = 2 * ((P.t1 - 1) / 2) + 1;
    P.t2 = static_cast<uint32_t>(pd.taps_lowpass.size());
    P.pw = pd.pw;
    P.spr = pd.spr;
    P.md = pd.md;
    P.g = 38 * pd.pw;
    P.cosphi2 = pd.cosphi2;
    P.sinphi = pd.sinphi;
    P.sync = sync ? 1 : 0;
    P.s16 = ss->format == APTGPU_STREAM_S16 ? 1 : 0;
    P.max_push = ss->max_push ? ss->max_push : kDefaultMaxPush;
    if (P.l > 1) {
        P.tpp = (P.jlim + P.l - 1) / P.l;
        d.table.assign(static_cast<size_t>(P.l) * P.tpp, 0.f);
        for (uint32_t ph = 0; ph < P.l; ++ph)
            for (uint32_t i = 0; ph + i * P.l < P.jlim; ++i) d.table[static_cast<size_t>(ph) * P.tpp + i] = pd.taps_resample[ph + i * P.l];
    } else {
        P.tpp = P.t1;
        d.table = pd.taps_resample;
    }
    d.h2 = pd.taps_lowpass;

    // the rings.  Input: a front launch recomputes R from T2 work samples before the first new one, whose
    // window starts (2 off + T2 m) / l samples (l == 1: T1 + (T2 + 1) m) before the samples pushed so far.
    const uint64_t back = (static_cast<uint64_t>(P.t1) + static_cast<uint64_t>(P.t2 + 2) * P.m) / P.l + 3;
    P.cap_in = pow2_ceil(P.max_push + back + 1);
    // F and corr: the oldest pending peak lies at most 2 spr + G before the work samples of the push before, and a
    // push adds at most new_work_max.
    P.cap_f = pow2_ceil(2ull * P.spr + P.g + new_work_max(P, P.max_push) + 1);
    P.cap_c = P.cap_f;
    const uint64_t win = (static_cast<uint64_t>(kTile + P.t2) * P.m + P.t1) / P.l + 3;
    const uint64_t lds = (win + 2ull * (kTile + P.t2) + 2) * sizeof(float);
    if (lds > kLdsLimit) throw Error{ErrorKind::Unsupported, "stream: this rate combination needs more LDS than a workgroup has"};
    P.win_cap = static_cast<uint32_t>(win);
    return d;
}

void fill_info(const Design &d, uint64_t device_bytes, aptgpu_stream_info *info)
{
    const uint32_t size = info->struct_size;
    *info = aptgpu_stream_info{};
    info->struct_size = size;
    info->work_rate = d.work_rate;
    info->pw = d.P.pw;
    info->samples_per_row = d.P.spr;
    info->l = d.P.l;
    info->m = d.P.m;
    info->n_resample_taps = d.P.t1;
    info->n_lowpass_taps = d.P.t2;
    info->max_push = d.P.max_push;
    info->cap_in = d.P.cap_in;
    info->cap_f = d.P.cap_f;
    info->cap_corr = d.P.sync ? d.P.cap_c : 0;
    info->device_bytes = device_bytes;
}

const char *reason_text(int reason)
{
    switch (reason) {
    case kReasonTooShort: return "Got less than 10 rows of samples, audio file is too short";
    case kReasonFewSync: return "Found less than 5 sync frames, audio file is too short or too noisy";
    case kReasonTripCap: return "stream: the picker exceeded its trip-count bound";
    case kReasonOverflow: return "stream: more rows or pending peaks than the bound allows";
    case kReasonWindow: return "stream: a tile's input window exceeds its LDS";
    case kReasonTrackTooShort: return "track: the signal is shorter than one row and one sync frame";
    case kReasonTrackWalkCap: return "stream: the tracker's back-track exceeded its bound";
    case kReasonTrackTripCap: return "stream: the tracker's checkpoint loop exceeded its trip-count bound";
    default: return "stream failed";
    }
}

HostStream::HostStream(Design d) : d_(std::move(d))
{
    const Params &P = d_.P;
    if (P.s16) in_s16_.assign(P.cap_in, 0);
    else in_f32_.assign(P.cap_in, 0.f);
    f_.assign(P.cap_f, 0.f);
    if (P.sync) c_.assign(P.cap_c, 0.f);
    st_.struct_size = sizeof(aptgpu_stream_result);
    reset();
}

void HostStream::reset() { state_reset(st_); }

uint64_t HostStream::bytes() const
{
    return in_f32_.size() * 4 + in_s16_.size() * 2 + (f_.size() + c_.size() + d_.table.size() + d_.h2.size()) * 4 + sizeof(State);
}

float HostStream::in_at(uint64_t i) const
{
    const Params &P = d_.P;
    if (i >= st_.n_in || i + P.cap_in < st_.n_in) overrun("input");
    const size_t q = static_cast<size_t>(i & (P.cap_in - 1));
    return P.s16 ? static_cast<float>(in_s16_[q]) : in_f32_[q];
}

float HostStream::f_at(uint64_t i) const
{
    const Params &P = d_.P;
    if (i >= st_.work_len || i + P.cap_f < st_.work_len) overrun("F");
    return f_[static_cast<size_t>(i & (P.cap_f - 1))];
}

void HostStream::front_segment(const void *samples, uint64_t n, bool finish)
{
    const Params &P = d_.P;
    if (n > P.max_push) throw Error{ErrorKind::Internal, "stream: segment longer than max_push"};
    for (uint64_t i = 0; i < n; ++i) {
        const size_t q = static_cast<size_t>((st_.n_in + i) & (P.cap_in - 1));
        if (P.s16) in_s16_[q] = static_cast<const int16_t *>(samples)[i];
        else in_f32_[q] = static_cast<const float *>(samples)[i];
    }
    const uint64_t w0 = st_.work_len;
    st_.n_in += n;
    const uint64_t n_avail = st_.n_in;
    const uint64_t w1 = work_count(P, n_avail, finish);

    // ---- front: R over [ka, w1) (the T2 samples before w0 recomputed), D, F
    if (w1 > w0) {
        const uint64_t ka = w0 > P.t2 ? w0 - P.t2 : 0;
        std::vector<float> R(static_cast<size_t>(w1 - ka)), D(static_cast<size_t>(w1 - ka), 0.f);
        for (uint64_t k = ka; k < w1; ++k)
            R[static_cast<size_t>(k - ka)] = resample_at(P, k, n_avail, [&](uint64_t i) { return in_at(i); },
                                                         [&](uint32_t ph, uint32_t i) { return d_.table[static_cast<size_t>(ph) * P.tpp + i]; });
        for (uint64_t k = std::max<uint64_t>(ka + 1, 1); k < w1; ++k)
            D[static_cast<size_t>(k - ka)] = envelope_at(R[static_cast<size_t>(k - 1 - ka)], R[static_cast<size_t>(k - ka)], P.cosphi2, P.sinphi);
        for (uint64_t i = w0; i < w1; ++i)
            f_[static_cast<size_t>(i & (P.cap_f - 1))] =
                lowpass_at(i, P.t2, [&](uint64_t q) { return D[static_cast<size_t>(q - ka)]; }, [&](uint32_t j) { return d_.h2[j]; });
    }
    st_.work_len = w1;
}

void HostLive::push(const void *samples, uint64_t n, bool first, bool finish, float *rows, uint64_t *positions, float *scores,
                    uint32_t rows_cap)
{
    const Params &P = params();
    const size_t es = P.s16 ? 2 : 4;
    uint64_t done = 0;
    do {
        const uint64_t seg = std::min<uint64_t>(n - done, P.max_push);
        const bool head = first && done == 0;
        done += seg;
        push_segment(static_cast<const char *>(samples) + (done - seg) * es, seg, finish && done == n, head, rows, positions, scores, rows_cap);
    } while (done < n);
}

void HostStream::push_segment(const void *samples, uint64_t n, bool finish, bool first, float *rows, uint64_t *positions, float *,
                              uint32_t rows_cap)
{
    const Params &P = d_.P;
    release_begin(st_, first);
    front_segment(samples, n, finish);
    const uint64_t w1 = st_.work_len;

    // ---- sync: corr for the newly scannable positions, then the picker
    if (P.sync && st_.status == 0) {
        const uint64_t s_end = w1 > P.g ? w1 - P.g : 0;
        for (uint64_t i = st_.corr_done; i < s_end; ++i)
            c_[static_cast<size_t>(i & (P.cap_c - 1))] = sync_corr_at(P.pw, [&](uint32_t j) { return f_at(i + j); });
        if (s_end > st_.corr_done) st_.corr_done = s_end;
        auto c_at = [&](uint64_t i) {
            if (i >= st_.corr_done || i + P.cap_c < st_.corr_done) overrun("corr");
            return c_[static_cast<size_t>(i & (P.cap_c - 1))];
        };
        auto reduce = [&](uint64_t a, uint64_t e) {
            Best b{kNone, 0.f};
            for (uint64_t i = a; i <= e; ++i) {
                const float v = c_at(i);
                if (!is_nan(v)) b = best_of(b, Best{i, v});
            }
            return b;
        };
        Pick pk = pick_load(st_);
        const bool ok = picker_run(P, pk, s_end, reduce, c_at, [&](uint64_t p_old, uint64_t istar, uint64_t copies) {
            pend_event(P, st_, p_old, istar, copies, w1, finish, positions, rows_cap);
        });
        pick_store(pk, st_);
        if (!ok) {
            st_.status = 1;
            st_.reason = kReasonTripCap;
        }
    }

    // ---- rows
    release_rows(P, st_, finish, positions, rows_cap);
    for (uint32_t j = 0; j < st_.rel_n; ++j) {
        const uint32_t r = st_.rel_base + j;
        const uint64_t pos = positions[r];
        float *dst = rows + static_cast<size_t>(r) * kPx;
        for (int c = 0; c < kPx; ++c) dst[c] = row_pixel(f_at(pos + static_cast<uint64_t>(P.pw) * c), st_.rel_first + j == 0 && c == 0);
    }
}

}  // namespace apt::stream
