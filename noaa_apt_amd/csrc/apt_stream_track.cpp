// apt_stream_track.cpp — live flywheel sync on the CPU (include/aptgpu.h §4e): the design of a tracked
// stream with every refusal (all of them before a device is touched) and the tracker of apt_kernels_stream_track.hpp in
// plain C++ over host rings (aptgpu_stream_create_tracked_host), which the kernels are tested against besides the model
// of tests/np_live_track_model.py.  The twin indexes its rings exactly as the kernels do and refuses to read an index
// that is not live, so that a capacity derived too small fails here.
#include "apt_kernels_stream_track.hpp"

#include <algorithm>

namespace apt::stream_track {

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

Design design_tracked(const aptgpu_settings *settings, const aptgpu_stream_settings *ss, const aptgpu_live_track_settings *ts, int mode,
                      bool mfma_switch)
{
    if (!settings || !ss) throw Error{ErrorKind::Invalid, "stream: null argument"};
    uint32_t lag = 8;
    aptgpu_track_settings tr{sizeof(aptgpu_track_settings), 8u, 0.1f, 0u};
    if (ts) {
        if (ts->struct_size < sizeof(aptgpu_live_track_settings))
            throw Error{ErrorKind::Invalid, "aptgpu_live_track_settings: struct_size not set"};
        if (ts->lag_rows > kMaxLag) throw Error{ErrorKind::Invalid, "stream: lag_rows must be 0..64"};
        lag = ts->lag_rows;
        tr.max_jitter = ts->max_jitter;
        tr.penalty = ts->penalty;
    }
    const apt::track::Settings s = apt::track::check_settings(&tr);
    if (ss->struct_size < sizeof(aptgpu_stream_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_stream_settings: struct_size not set"};
    aptgpu_stream_settings plain = *ss;
    plain.struct_size = sizeof(aptgpu_stream_settings);
    plain.sync = 0;  // the front end alone: the picker's correlation ring is not created
    Design d;
    d.stream = apt::stream::design_stream(settings, &plain, mode, mfma_switch);
    Params &T = d.T;
    T.pw = apt::track::pixel_width(d.stream.work_rate, s);  // (a work rate above 8 x 4160 Hz, 4 w >= L)
    T.L = static_cast<uint32_t>(apt::track::kPx) * T.pw;
    T.G = 38u * T.pw;
    T.w = s.w;
    T.lam = s.lam;
    T.lag = lag;
    // the rings.  F and s: a launch sequence that starts at work_len w0 processes checkpoints n > w0 - G
    // only, and the oldest node one of them commits lies above n - (K + 3) L - w; its row and score are read while F
    // reaches to w0 + new_work_max.
    apt::stream::Params &P = d.stream.P;
    const uint64_t reach = static_cast<uint64_t>(lag + 3) * T.L + T.G + 2ull * static_cast<uint64_t>(T.w);
    P.cap_f = pow2_ceil(reach + apt::stream::new_work_max(P, P.max_push) + 1);
    T.cap_s = P.cap_f;
    T.cap_best = pow2_ceil(2ull * T.L);  // a piece of L - w positions reads [i - L - w, i - L + w]
    // bp: the programme stops at every checkpoint, so a back-track starts below the newest byte and ends above
    // n - (K + 3) L - w (a finish: M < n + L above the same)
    T.cap_bp = pow2_ceil(static_cast<uint64_t>(lag + 4) * T.L + 2ull * static_cast<uint64_t>(T.w));
    T.walk_cap = 2 * lag + 16;
    return d;
}

HostTrackStream::HostTrackStream(Design d) : d_(std::move(d)), front_(d_.stream)
{
    s_.assign(d_.T.cap_s, 0.f);
    best_.assign(d_.T.cap_best, 0.f);
    bp_.assign(d_.T.cap_bp, 0);
    rec_.struct_size = sizeof(aptgpu_stream_track_result);
    reset();
}

void HostTrackStream::reset()
{
    front_.reset();
    front_.state_mut().n_sync = 0;
    record_reset(rec_, d_.T);
    dp_done_ = 0;
}

uint64_t HostTrackStream::bytes() const { return front_.bytes() + (s_.size() + best_.size()) * 4 + bp_.size() + sizeof(Record); }

void HostTrackStream::push_segment(const void *samples, uint64_t n, bool finish, bool first, float *rows, uint64_t *positions,
                                   float *scores, uint32_t rows_cap)
{
    namespace st = apt::stream;
    const st::Params &P = d_.stream.P;
    const Params &T = d_.T;
    st::State &S = front_.state_mut();
    st::release_begin(S, first);
    front_.front_segment(samples, n, finish);
    const uint64_t w1 = S.work_len;
    if (finish) S.finished = 1;
    if (S.status != 0) return;

    // ---- the scores of the newly final positions
    const uint64_t m0 = rec_.m, m1 = positions_final(T, w1);
    {
        const float fg = static_cast<float>(T.G), norm = apt::track::norm_of(T.G), wmean = apt::track::mean_weight();
        for (uint64_t i = m0; i < m1; ++i) {
            float c = 0.f, s1 = 0.f, s2 = 0.f;
            for (uint32_t j = 0; j < T.G; ++j)
                apt::track::score_step(front_.f_at(i + j), apt::track::template_plus(static_cast<int>(j), static_cast<int>(T.pw)), c, s1, s2);
            s_[static_cast<size_t>(i & (T.cap_s - 1))] = apt::track::score_finish(c, s1, s2, fg, norm, wmean);
        }
    }
    rec_.m = m1;
    auto s_at = [&](uint64_t i) {
        if (i >= m1 || i + T.cap_s < m1) overrun("score");
        return s_[static_cast<size_t>(i & (T.cap_s - 1))];
    };

    // ---- the programme, checkpoint by checkpoint
    uint64_t piece_end = dp_done_;  // (a piece's own positions are being written: not live for its reads)
    auto best_at = [&](uint64_t j) {
        if (j >= dp_done_ || j + T.cap_best < piece_end) overrun("best");
        return best_[static_cast<size_t>(j & (T.cap_best - 1))];
    };
    auto bp_at = [&](uint64_t v) {
        if (v >= dp_done_ || v + T.cap_bp < dp_done_) overrun("back-pointer");
        return static_cast<int>(bp_[static_cast<size_t>(v & (T.cap_bp - 1))]);
    };
    auto advance = [&](uint64_t target) {
        const uint64_t C = T.L - static_cast<uint64_t>(T.w);
        while (dp_done_ < target) {
            piece_end = std::min(dp_done_ + C, target);
            for (uint64_t i = dp_done_; i < piece_end; ++i) {
                float b;
                int back;
                dp_position(T, i, s_at(i), best_at, b, back);
                best_[static_cast<size_t>(i & (T.cap_best - 1))] = b;
                bp_[static_cast<size_t>(i & (T.cap_bp - 1))] = static_cast<int8_t>(back);
            }
            dp_done_ = piece_end;
        }
    };
    auto first_maximum = [&](uint64_t lo, uint64_t hi) {
        uint64_t end = lo;
        float bv = best_at(lo);
        for (uint64_t i = lo + 1; i < hi; ++i) {
            const float v = best_at(i);
            if (v > bv) {
                bv = v;
                end = i;
            }
        }
        return end;
    };
    std::vector<uint64_t> tmp(T.walk_cap);
    auto commit = [&](uint64_t v) {
        if (S.status != 0) return;
        if (v + T.L <= w1) put_row(S, v, s_at(v), positions, scores, rows_cap);
    };
    uint64_t trips = (m1 - dp_done_) / T.L + 2;
    for (;;) {
        if (trips-- == 0) {
            S.status = 1;
            S.reason = kReasonTripCap;
            break;
        }
        const uint64_t cpn = rec_.next_checkpoint * T.L;
        advance(std::min(cpn, m1));
        if (cpn > m1) break;
        if (!checkpoint(T, rec_, cpn, true, first_maximum(cpn - T.L, cpn), tmp.data(), bp_at, commit)) {
            S.status = 1;
            S.reason = kReasonWalkCap;
            break;
        }
        rec_.next_checkpoint += 1;
    }
    if (finish && S.status == 0) {
        if (w1 < static_cast<uint64_t>(T.L) + T.G) {
            S.status = 1;
            S.reason = kReasonTooShort;
        } else if (!checkpoint(T, rec_, m1, false, first_maximum(m1 > T.L ? m1 - T.L : 0, m1), tmp.data(), bp_at, commit)) {
            S.status = 1;
            S.reason = kReasonWalkCap;
        }
    }
    S.n_sync = rec_.n_positions;
    S.scan_pos = m1;

    // ---- rows: the samples' own bits
    for (uint32_t j = 0; j < S.rel_n; ++j) {
        const uint32_t r = S.rel_base + j;
        const uint64_t pos = positions[r];
        float *dst = rows + static_cast<size_t>(r) * st::kPx;
        for (int c = 0; c < st::kPx; ++c) dst[c] = front_.f_at(pos + static_cast<uint64_t>(P.pw) * static_cast<uint64_t>(c));
    }
}

}  // namespace apt::stream_track
