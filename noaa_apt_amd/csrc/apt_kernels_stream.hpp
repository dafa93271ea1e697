// apt_kernels_stream.hpp — live decode (include/aptgpu.h §4d): audio is pushed in chunks and the rows
// that are FINAL come back — final = present with the same bits in strict decode() of the complete recording whatever is
// pushed later.  The per-sample arithmetic, the peak picker's state machine and the release rules below are ONE text for
// the kernels (apt_kernels_stream.hip) and the host twin (apt_stream.cpp); every operation is a separately rounded IEEE
// f32 one (both sides are built with contraction off).  Two exceptions, device-only texts the other kernels share: on
// the GPU the envelope is apt_envelope.hpp's general form and the sync chain apt_sync_corr.hpp's; envelope_at and
// sync_corr_at below are the same operations in the same order for the twin (tests/test_gpu_stream.py compares the bits).
//
//   R[k]  the first resample (dsp.rs:186-289 in the polyphase closed form of k_resample_generic, or filter + decimate
//         for l == 1, dsp.rs:386-410 + 294-307)
//   D[i]  the two-sample envelope (dsp.rs:369-377), D[0] = 0
//   F[i]  the low-pass (dsp.rs:396-404): sum over j < T2, j < i of D[i-j] h2[j], ascending j
//   corr  the +-1 sync chain (decode.rs:225-233), scanned while i + 38 pw < work_len
//   picker decode.rs:239-253 as window-maximum jumps (picker_run)
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define APT_STR_HD __host__ __device__ inline
#else
#define APT_STR_HD inline
#endif

namespace apt::stream {

constexpr int kPx = 2080;
constexpr int kTile = 256;      // work samples per workgroup of k_stream_front
constexpr int kMaxPend = 16;    // pending entries (position, count): at most 3 after a drain, 2 more per event (pend_event)
constexpr uint32_t kDefaultMaxPush = 1u << 16;
constexpr uint32_t kMaxMaxPush = 1u << 24;
constexpr uint32_t kLdsLimit = 64u * 1024u;  // dynamic LDS of k_stream_front

// reasons of a record whose status is not 0
constexpr int kReasonTooShort = 1;   // "Got less than 10 rows of samples, audio file is too short"
constexpr int kReasonFewSync = 2;    // "Found less than 5 sync frames, ..."
constexpr int kReasonTripCap = 5;    // the picker's loop reached its trip-count cap (a defect if it happens: DESIGN.md §22)
constexpr int kReasonOverflow = 6;   // the pending list or the caller's row buffer is full (a defect if it happens)
constexpr int kReasonWindow = 7;     // a tile's input window exceeds the LDS the launch reserved (a defect if it happens)
// ... of a tracked stream (apt_kernels_stream_track.hpp)
constexpr int kReasonTrackTooShort = 8;  // finish: shorter than one row and one sync frame (the one-shot tracker's refusal)
constexpr int kReasonTrackWalkCap = 9;   // a back-track reached its bound (a defect if it happens)
constexpr int kReasonTrackTripCap = 10;  // the checkpoint loop reached its bound (likewise)

// What a stream is created with (host-designed; by value in the kernel arguments).
struct Params {
    uint32_t l, m;
    uint32_t t1;        // resampler taps
    uint32_t jlim;      // taps fast_resampling uses: 2 * ((t1 - 1) / 2) + 1
    uint32_t tpp;       // taps per phase of the phase-major table (l > 1)
    uint32_t t2;        // low-pass taps
    uint32_t pw, spr, md, g;  // pixel width, samples per row, min distance, sync frame length 38 pw
    float cosphi2, sinphi;
    uint32_t cap_in, cap_f, cap_c;  // ring capacities (powers of two)
    uint32_t win_cap;   // floats of LDS a tile's input window may take
    int32_t sync;
    int32_t s16;        // input ring holds int16
    uint32_t max_push;
};

// The device-resident record.  Its head is aptgpu_stream_result (include/aptgpu.h); the rest is the carried state.
struct State {
    uint32_t struct_size;
    int32_t status, reason;
    uint32_t n_rows;      // rows released by this push
    uint64_t rows_total;
    uint64_t n_sync;      // peaks so far (len)
    uint64_t n_in;
    uint64_t work_len;    // final F samples
    uint64_t scan_pos;    // positions the picker has consumed
    // ---- carried state
    uint64_t p;           // the last peak's position ...
    float v;              // ... and value
    uint32_t n_pend;
    uint64_t pend[kMaxPend];        // positions of peaks that have a successor and whose row is not out, oldest first
    uint32_t pend_count[kMaxPend];  // ... and how many peaks share each (the copies of one event are one entry)
    uint64_t corr_done;   // corr[i] is in the ring for i < corr_done
    uint64_t next_row;    // no-sync: rows released
    uint64_t rel_first;   // rows_total before this launch's releases
    uint32_t rel_base;    // index of this launch's first row in the caller's buffers
    uint32_t rel_n;       // rows this launch released
    int32_t finished;
    uint32_t reserved;
};

APT_STR_HD void state_reset(State &s)
{
    const uint32_t size = s.struct_size;
    s = State{};
    s.struct_size = size;
    s.n_sync = 1;  // peaks = [(0, 0.)], decode.rs:208-209
}

APT_STR_HD bool is_nan(float v) { return v != v; }

// ---- how much is final after n samples (finish: the recording ends there)
APT_STR_HD uint64_t work_count(const Params &P, uint64_t n, bool finish)
{
    if (P.l == 1) return n / P.m;  // decimate: k < n / m (dsp.rs:301)
    const uint64_t total = n * P.l, off = (P.jlim - 1) / 2;
    if (finish) return total <= off ? 0 : (total - off + P.m - 1) / P.m;  // t = off + k m < n l
    // every index of the window pushed: floor((k m + 2 off) / l) < n  <=>  k m + 2 off < n l
    return total <= 2 * off ? 0 : (total - 2 * off + P.m - 1) / P.m;
}
// upper bound of the work samples one push of n samples (or a finish) makes final
APT_STR_HD uint64_t new_work_max(const Params &P, uint64_t n) { return (n * P.l + (P.jlim - 1)) / P.m + 2; }
// Upper bound of the rows a push that brings the sample count to n_after (or a finish there) can release.  One event
// of the picker can push any number of copies (a correlation that climbs for rows on end keeps `len` where it was), so
// no bound follows from the push's size alone; what holds is rows_total <= len - 1 and len <= work_len / spr after
// every event (sync off: rows_total = work_len / spr).  rows_seen: any earlier value of rows_total.
APT_STR_HD uint32_t rows_bound(const Params &P, uint64_t n_after, uint64_t rows_seen)
{
    const uint64_t most = work_count(P, n_after, true) / P.spr + 1;
    const uint64_t b = most > rows_seen ? most - rows_seen : 1;
    return b > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(b);
}

// ---- the input window of the work samples [ka, k1): first index and one past the last
APT_STR_HD void input_window(const Params &P, uint64_t ka, uint64_t k1, uint64_t n_avail, uint64_t &lo, uint64_t &hi)
{
    if (P.l > 1) {
        lo = (ka * P.m + P.l - 1) / P.l;
        hi = ((k1 - 1) * P.m + (P.jlim - 1)) / P.l + 1;
    } else {
        const uint64_t i0 = ka * P.m;
        lo = i0 >= P.t1 - 1 ? i0 - (P.t1 - 1) : 0;
        hi = (k1 - 1) * P.m + 1;
    }
    if (hi > n_avail) hi = n_avail;
    if (lo > hi) lo = hi;
}

// ---- R[k].  x(i): input sample i, called only for i < n_avail; tap(ph, i): coeff[ph + i l]; h(j): coeff[j]
template <typename X, typename Tap>
APT_STR_HD float resample_at(const Params &P, uint64_t k, uint64_t n_avail, X &&x, Tap &&tap)
{
#pragma clang fp contract(off)
    const uint64_t km = k * P.m;
    float sum = 0.f;
    if (P.l > 1) {
        uint64_t xi = (km + P.l - 1) / P.l;
        const uint32_t ph = static_cast<uint32_t>(xi * P.l - km);
        const uint32_t cnt = ph < P.jlim ? (P.jlim - ph + P.l - 1) / P.l : 0u;
        for (uint32_t i = 0; i < cnt; ++i, ++xi) {
            if (xi < n_avail) {  // an absent sample is skipped, not multiplied by zero (dsp.rs:257)
                const float pr = tap(ph, i) * x(xi);
                sum = sum + pr;
            }
        }
    } else {
        const uint32_t jn = km < P.t1 ? static_cast<uint32_t>(km) : P.t1;  // i > j (dsp.rs:399)
        for (uint32_t j = 0; j < jn; ++j) {
            const float pr = x(km - j) * tap(0u, j);
            sum = sum + pr;
        }
    }
    return sum;
}

// ---- D[i], i >= 1, in the reference's evaluation order (dsp.rs:373); sqrt and divide correctly rounded
APT_STR_HD float envelope_at(float prev, float curr, float cosphi2, float sinphi)
{
#pragma clang fp contract(off)
    const float a = prev * prev, b = curr * curr;
    const float s = a + b;
    const float c0 = prev * curr;
    const float c = c0 * cosphi2;
    const float r = s - c;
    return __builtin_sqrtf(r) / sinphi;
}

// ---- F[i].  d(q): D[q], called for i - T2 < q <= i, q >= 1
template <typename Dv, typename H>
APT_STR_HD float lowpass_at(uint64_t i, uint32_t t2, Dv &&d, H &&h)
{
#pragma clang fp contract(off)
    const uint32_t jn = i < t2 ? static_cast<uint32_t>(i) : t2;
    float sum = 0.f;
    for (uint32_t j = 0; j < jn; ++j) {
        const float pr = d(i - j) * h(j);
        sum = sum + pr;
    }
    return sum;
}

// ---- corr[i]: the reference's chain; f(j) = F[i + j]
template <typename Fv>
APT_STR_HD float sync_corr_at(uint32_t pw, Fv &&f)
{
#pragma clang fp contract(off)
    const uint32_t pulse = 2 * pw;
    float c = 0.f;
    uint32_t j = 0;
    for (uint32_t e = 0; e < pulse; ++e, ++j) c = c - f(j);
    for (int rep = 0; rep < 7; ++rep) {
        for (uint32_t e = 0; e < pulse; ++e, ++j) c = c - f(j);
        for (uint32_t e = 0; e < pulse; ++e, ++j) c = c + f(j);
    }
    for (uint32_t e = 0; e < 8 * pw; ++e, ++j) c = c - f(j);
    return c;
}

// ---- a pixel of a row through the final NoFilter stage (filter([1.]) + decimate(pw)): 0.0 + x * 1.0
APT_STR_HD float row_pixel(float f, bool very_first)
{
#pragma clang fp contract(off)
    const float pr = f * 1.f;
    const float s = 0.f + pr;
    return very_first ? 0.f : s;
}

// ---- the window maximum of a reduction: NaNs ignored, the lowest index among equals
struct Best {
    uint64_t idx;  // ~0: nothing found
    float val;
};
constexpr uint64_t kNone = ~0ull;
APT_STR_HD Best best_of(Best a, Best b)
{
    if (b.idx == kNone) return a;
    if (a.idx == kNone) return b;
    if (b.val > a.val || (b.val == a.val && b.idx < a.idx)) return b;
    return a;
}

// ---- the picker (decode.rs:241-253) from settled state over the positions [scan_pos, s_end).
// reduce(a, e): best_of over corr[a .. e] (a <= e, e - a < md + 1); corr(i): corr[i].  On the device every thread of the
// workgroup runs this with the same state (the reductions are collective).
// From (p, v, len): positions up to p + md may replace the peak — the sequential scan climbs the strict running maxima
// and ends on the first maximum of the window, each record being within md of the one before; after the window nothing
// happens until i* = max(p + md + 1, (len + 1) spr), where i* / spr - len copies of (i*, corr[i*]) are pushed.
// Returns false when the trip-count cap was reached.
struct Pick {  // the picker's scalars (every thread of the device's workgroup holds a copy)
    uint64_t p, scan_pos, n_sync;
    float v;
    int32_t status, reason;
};
APT_STR_HD Pick pick_load(const State &s) { return Pick{s.p, s.scan_pos, s.n_sync, s.v, s.status, s.reason}; }
APT_STR_HD void pick_store(const Pick &k, State &s)
{
    s.p = k.p;
    s.scan_pos = k.scan_pos;
    s.n_sync = k.n_sync;
    s.v = k.v;
    if (k.status != 0) {  // (the record's own status may have been set by an event meanwhile)
        s.status = k.status;
        s.reason = k.reason;
    }
}
// event(p_old, istar, copies): the peak at p_old and copies - 1 of the copies at istar now have a successor; called in
// the scan's order (on the device: by every thread, the leader acts).
// Trip count, with c = ceil(new positions / md).  Pushes: events lie more than md apart, at most c.  Landings: one on a
// window's first maximum leaves nothing greater before that window's end, so the landing after the next lies more than md
// further on, across events too (an event lies more than md behind the landing before it): at most 2 c.  Window ends
// without a landing: each is followed by a push or by the end of the loop, at most c + 1.  The end itself (the scan
// limit inside a window, or the next event beyond it): 1.  Together 4 c + 2, the loop's hard cap.
template <typename Reduce, typename Corr, typename Event>
APT_STR_HD bool picker_run(const Params &P, Pick &st, uint64_t s_end, Reduce &&reduce, Corr &&corr, Event &&event)
{
    if (st.scan_pos >= s_end) return true;
    const uint64_t fresh = s_end - st.scan_pos;
    const uint64_t c = (fresh + P.md - 1) / P.md;
    uint64_t trips = 4 * c + 2;
    while (st.scan_pos < s_end) {
        if (trips-- == 0) return false;
        const uint64_t wend = st.p + P.md;  // last position that may replace the peak
        if (st.scan_pos <= wend) {
            const uint64_t e = wend < s_end - 1 ? wend : s_end - 1;
            if (!is_nan(st.v)) {  // `corr > NaN` is false: a NaN peak is never replaced
                const Best b = reduce(st.scan_pos, e);
                if (b.idx != kNone && b.val > st.v) {
                    st.p = b.idx;
                    st.v = b.val;
                    st.scan_pos = b.idx + 1;
                    continue;
                }
            }
            st.scan_pos = e + 1;
            continue;
        }
        const uint64_t a = wend + 1, b = (st.n_sync + 1) * P.spr;
        const uint64_t istar = a > b ? a : b;
        if (istar >= s_end) {
            st.scan_pos = s_end;
            break;
        }
        const uint64_t copies = istar / P.spr - st.n_sync;  // >= 1, and as many as the rows the peak was carried over
        event(st.p, istar, copies);
        st.n_sync += copies;
        st.p = istar;
        st.v = corr(istar);
        st.scan_pos = istar + 1;
    }
    return true;
}

// ---- rows (one thread).  positions[n_rows] receives the work-rate position of a released row; the rows themselves are
// gathered from the F ring afterwards.
APT_STR_HD bool put_row(State &st, uint64_t pos, uint64_t *positions, uint32_t rows_cap)
{
    if (st.n_rows >= rows_cap) {
        st.status = 1;
        st.reason = kReasonOverflow;
        return false;
    }
    positions[st.n_rows] = pos;
    st.n_rows += 1;
    st.rel_n += 1;
    st.rows_total += 1;
    return true;
}
// the pending rows that fit below work_len.  Positions never decrease, so they are a prefix of the list
// (decode.rs:125-131); drop_rest (finish): the others never fit.
APT_STR_HD void drain_pending(const Params &P, State &st, uint64_t work_len, bool drop_rest, uint64_t *positions, uint32_t rows_cap)
{
    uint32_t k = 0;
    while (k < st.n_pend && st.pend[k] + P.spr < work_len) {
        while (st.pend_count[k] > 0) {
            if (!put_row(st, st.pend[k], positions, rows_cap)) return;
            st.pend_count[k] -= 1;
        }
        ++k;
    }
    if (drop_rest) k = st.n_pend;
    for (uint32_t q = k; q < st.n_pend; ++q) {
        st.pend[q - k] = st.pend[q];
        st.pend_count[q - k] = st.pend_count[q];
    }
    st.n_pend -= k;
}
// Before the picker of a launch.
APT_STR_HD void release_begin(State &st, bool first)
{
    if (first) st.n_rows = 0;
    st.rel_first = st.rows_total;
    st.rel_base = st.n_rows;
    st.rel_n = 0;
}
// One event of the picker: two entries at most, then (hold: not in a finish, whose verdict comes first) what fits is
// released at once, so that the list holds what a launch leaves pending and never what it covers.  An entry that stays
// has position + spr >= work_len: the copies of the at most two events that close to the end, and the peak before the
// last of them (it lies more than md before its event) — three entries after a drain, two more per event of a finish.
APT_STR_HD void pend_event(const Params &P, State &st, uint64_t p_old, uint64_t istar, uint64_t copies, uint64_t work_len, bool hold,
                           uint64_t *positions, uint32_t rows_cap)
{
    if (st.status != 0) return;
    const uint32_t need = copies > 1 ? 2u : 1u;
    if (st.n_pend + need > static_cast<uint32_t>(kMaxPend) || copies > 0xFFFFFFFFull) {
        st.status = 1;
        st.reason = kReasonOverflow;
        return;
    }
    st.pend[st.n_pend] = p_old;
    st.pend_count[st.n_pend] = 1;
    st.n_pend += 1;
    if (copies > 1) {
        st.pend[st.n_pend] = istar;
        st.pend_count[st.n_pend] = static_cast<uint32_t>(copies - 1);
        st.n_pend += 1;
    }
    if (!hold) drain_pending(P, st, work_len, false, positions, rows_cap);
}
// After the picker of a launch: finish's verdict, then the rows that are due.
APT_STR_HD void release_rows(const Params &P, State &st, bool finish, uint64_t *positions, uint32_t rows_cap)
{
    if (finish) {
        st.finished = 1;
        if (st.status == 0) {
            if (st.work_len < 10ull * P.spr) {  // decode.rs:79-83
                st.status = 1;
                st.reason = kReasonTooShort;
            } else if (P.sync && st.n_sync < 5) {  // decode.rs:112-118
                st.status = 1;
                st.reason = kReasonFewSync;
            }
        }
    }
    if (st.status != 0) return;
    if (!P.sync) {
        st.n_sync = 0;
        while ((st.next_row + 1) * P.spr <= st.work_len) {  // decode.rs:141-147
            if (!put_row(st, st.next_row * P.spr, positions, rows_cap)) return;
            st.next_row += 1;
        }
        return;
    }
    drain_pending(P, st, st.work_len, finish, positions, rows_cap);
}

}  // namespace apt::stream

// ---- the host side (apt_stream.cpp; CPU only)
#include <memory>
#include <vector>

#include "../../include/aptgpu.h"
#include "apt_host.hpp"

namespace apt::stream_track {
struct Record;  // apt_kernels_stream_track.hpp
}

namespace apt::stream {

// The design of a stream: every refusal of §4d (none touches a device), the taps and the ring capacities.
struct Design {
    Params P{};
    std::vector<float> table;  // l > 1: phase-major [l][tpp] (absent taps 0, never read); l == 1: the taps
    std::vector<float> h2;
    uint32_t work_rate = 0;
};
// mode: aptgpu_context.mode; mfma_switch: APTGPU_FAST_MFMA is set to 1
Design design_stream(const aptgpu_settings *settings, const aptgpu_stream_settings *ss, int mode, bool mfma_switch);
void fill_info(const Design &d, uint64_t device_bytes, aptgpu_stream_info *info);
const char *reason_text(int reason);

// What the C API asks of a twin (picker or tracker): one interface, so that a handle holds one engine and never names
// the concrete class outside creation.
class HostLive {
public:
    virtual ~HostLive() = default;
    virtual void reset() = 0;
    virtual const State &state() const = 0;
    virtual uint64_t bytes() const = 0;
    // aptgpu_stream_rows_bound: the rows a push of n more samples (or a finish there) can release
    virtual uint32_t rows_bound(uint64_t n) const = 0;
    virtual const apt::stream_track::Record *track_record() const { return nullptr; }  // null: the picker
    // n samples in segments of at most max_push (first: this call opens a push, false continues one whose samples arrive
    // in pieces; finish closes the recording with the last segment); scores: the tracker's lock indicators, null for the picker
    void push(const void *samples, uint64_t n, bool first, bool finish, float *rows, uint64_t *positions, float *scores, uint32_t rows_cap);
    // one segment of at most max_push samples (finish: none); rows / positions (/ scores) as the kernels would write them
    virtual void push_segment(const void *samples, uint64_t n, bool finish, bool first, float *rows, uint64_t *positions, float *scores,
                              uint32_t rows_cap) = 0;

protected:
    virtual const Params &params() const = 0;
};

// The picker's twin: the same state machine over host rings.
class HostStream final : public HostLive {
public:
    explicit HostStream(Design d);
    void reset() override;
    void push_segment(const void *samples, uint64_t n, bool finish, bool first, float *rows, uint64_t *positions, float *scores,
                      uint32_t rows_cap) override;
    // the front end alone (what push_segment begins with): the samples into the input ring, F up to the new work_len
    void front_segment(const void *samples, uint64_t n, bool finish);
    float f_at(uint64_t i) const;  // refuses an index that is not live
    State &state_mut() { return st_; }
    const State &state() const override { return st_; }
    uint64_t bytes() const override;
    uint32_t rows_bound(uint64_t n) const override { return apt::stream::rows_bound(d_.P, st_.n_in + n, st_.rows_total); }

private:
    const Params &params() const override { return d_.P; }
    float in_at(uint64_t i) const;
    Design d_;
    State st_{};
    std::vector<float> in_f32_;
    std::vector<int16_t> in_s16_;
    std::vector<float> f_, c_;
};

}  // namespace apt::stream

#if defined(__HIPCC__)
namespace apt::gpu {

// what the launches of one stream share (all device pointers)
struct StreamBuffers {
    apt::stream::State *state;
    void *ring_in;       // cap_in floats or int16
    float *ring_f;       // cap_f
    float *ring_c;       // cap_c (sync)
    const float *table;  // resampler taps, phase-major
    const float *h2;     // low-pass taps
};
size_t stream_front_lds_bytes(const apt::stream::Params &P);
// k_stream_front: F[w0 .. w1) from the input ring, which holds the samples below n_avail
void stream_front(hipStream_t s, const apt::stream::Params &P, const StreamBuffers &b, uint64_t w0, uint64_t w1, uint64_t n_avail);
// k_stream_corr: corr[i] for the positions the work samples [w0, w1) make scannable (i + 38 pw < w1)
void stream_corr(hipStream_t s, const apt::stream::Params &P, const StreamBuffers &b, uint64_t w0, uint64_t w1);
// k_stream_sync: the picker up to w1 - 38 pw, then the record and the positions of the rows that became final
// (appended at positions[n_rows of the push so far]; first: the push's first launch sequence)
void stream_sync(hipStream_t s, const apt::stream::Params &P, const StreamBuffers &b, uint64_t *positions, uint32_t rows_cap,
                 uint64_t n_in, uint64_t w1, bool first, bool finish);
// k_stream_rows: the rows of those positions; grid_rows workgroup rows walk however many the record counts
void stream_rows(hipStream_t s, const apt::stream::Params &P, const StreamBuffers &b, const uint64_t *positions, float *rows,
                 uint32_t rows_cap, uint32_t grid_rows);

}  // namespace apt::gpu
#endif
