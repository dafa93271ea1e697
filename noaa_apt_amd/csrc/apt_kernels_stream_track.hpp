// apt_kernels_stream_track.hpp — live flywheel sync (include/aptgpu.h §4e): the tracker of §21 behind the
// streaming front end of §22.  The scores s, the sums best and the back-pointers bp are the one-shot's values bit for bit
// (they are causal: position i is final once i + G <= work_len); what is new is WHEN a position of the path is handed out.
// At every checkpoint n = e L the best survivor over [n - L, n) is followed back and the nodes that lie at least
// lag_rows + 1 rows behind n are committed.  The record, the ring indexing and the commit rule below are ONE text for the
// kernels (apt_kernels_stream_track.hip) and the host twin (apt_stream_track.cpp); the per-sample arithmetic is §21's
// (apt_kernels_track_sync.hpp).
#pragma once

#include "apt_kernels_stream.hpp"
#include "apt_kernels_track_sync.hpp"

namespace apt::stream_track {

constexpr uint32_t kMaxLag = 64;
// reasons of a record whose status is not 0: apt::stream's own (one list, one reason_text)
constexpr int kReasonTooShort = apt::stream::kReasonTrackTooShort;
constexpr int kReasonWalkCap = apt::stream::kReasonTrackWalkCap;
constexpr int kReasonTripCap = apt::stream::kReasonTrackTripCap;

// What a tracked stream is created with besides apt::stream::Params (by value in the kernel arguments).
struct Params {
    uint32_t pw, L, G;
    int32_t w;
    float lam;
    uint32_t lag;       // K
    uint32_t cap_s;     // score ring (= cap_f: s[v] of a committed node is read when its row is)
    uint32_t cap_best;  // >= 2 L
    uint32_t cap_bp;    // >= (K + 4) L + 2 w
    uint32_t walk_cap;  // nodes a back-track may visit: 2 K + 16
};

// The tracker's device-resident record.  Its head is aptgpu_stream_track_result (include/aptgpu.h).
struct Record {
    uint32_t struct_size;
    uint32_t n_relocks;
    uint64_t n_positions;      // committed so far (a last one without a full row included)
    uint64_t m;                // positions whose s, best and bp are final
    uint64_t next_checkpoint;  // e of the next checkpoint (the first is 1)
    uint64_t last_position;    // c (valid when has_position)
    int32_t has_position;
    uint32_t reserved;
    uint32_t cap_best, cap_bp;  // (for the caller: the two rings the stream's info does not list)
};

APT_STR_HD void record_reset(Record &r, const Params &T)
{
    const uint32_t size = r.struct_size;
    r = Record{};
    r.struct_size = size;
    r.next_checkpoint = 1;
    r.cap_best = T.cap_best;
    r.cap_bp = T.cap_bp;
}

APT_STR_HD uint64_t positions_final(const Params &T, uint64_t work_len) { return work_len > T.G ? work_len - T.G : 0; }

// Upper bound of the rows one call can release when it moves m from m0 to m1 (rule 2).  After a checkpoint at n >= (K + 2) L
// the last committed position lies above n - (K + 3) L, and the next checkpoint commits between c + L - w and n - K L:
// less than 2 L + w samples, at most 3 nodes (steps are >= L - w, 4 w < L).  A finish commits up to M < n + L as well:
// less than (K + 4) L + w samples.
APT_STR_HD uint32_t rows_bound(const Params &T, uint64_t m0, uint64_t m1)
{
    const uint64_t cps = m1 / T.L - m0 / T.L;
    const uint64_t fin = (static_cast<uint64_t>(T.lag + 4) * T.L + static_cast<uint64_t>(T.w)) / (T.L - static_cast<uint64_t>(T.w)) + 2;
    const uint64_t b = 3 * cps + fin;
    return b > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(b);
}

// aptgpu_stream_rows_bound of a tracked stream: m stands at m0 and the sample count comes to n_after
// (a finish makes more work samples final than a push of the same samples: the bound serves both)
APT_STR_HD uint32_t rows_bound_after(const Params &T, const apt::stream::Params &P, uint64_t m0, uint64_t n_after)
{
    return rows_bound(T, m0, positions_final(T, apt::stream::work_count(P, n_after, true)));
}

// One position of the dynamic programme.  s_at(i), best_at(j): the rings; returns best[i] and the back-pointer.
template <typename Best>
APT_STR_HD void dp_position(const Params &T, uint64_t i, float s, Best &&best_at, float &best_out, int &bp_out)
{
#pragma clang fp contract(off)
    // best_predecessor only asks whether i < L and whether i - L -+ k >= 0: beyond 4 L the answers no longer change
    const int32_t L = static_cast<int32_t>(T.L);
    const int32_t ie = i < 4ull * T.L ? static_cast<int32_t>(i) : 4 * L;
    float cur;
    int b;
    apt::track::best_predecessor(
        ie, L, T.w, T.lam, [&](int d) { return best_at(i - T.L - static_cast<uint64_t>(static_cast<int64_t>(d))); }, cur, b);
    best_out = s + cur;
    bp_out = b;
}

// Rules 2, 3 and 5 for one checkpoint (one thread).  end: the first maximum of best over the checkpoint's window; n: the
// checkpoint's boundary; lagged: false for the commit of finish(), which holds nothing back.  bp_at(v): the back-pointer
// byte; commit(v): called ascending for every committed node.  tmp: walk_cap entries.  Returns false when the walk
// reached its bound.
template <typename Bp, typename Commit>
APT_STR_HD bool checkpoint(const Params &T, Record &r, uint64_t n, bool lagged, uint64_t end, uint64_t *tmp, Bp &&bp_at, Commit &&commit)
{
    const uint64_t hold = static_cast<uint64_t>(T.lag + 1) * T.L;
    uint32_t k = 0, steps = 0;
    bool on_chain = false;
    for (uint64_t v = end;;) {
        if (r.has_position && v + static_cast<uint64_t>(T.w) < r.last_position + T.L) {  // v < c + L - w: nothing below commits
            on_chain = v == r.last_position;  // (the nodes below v are below c)
            break;
        }
        if (steps++ >= T.walk_cap) return false;
        if (!lagged || v + hold <= n) tmp[k++] = v;
        const int d = bp_at(v);
        if (d == apt::track::kStart) break;
        v = v - T.L - static_cast<uint64_t>(static_cast<int64_t>(d));
    }
    if (k > 0 && r.has_position && !on_chain) r.n_relocks += 1;
    while (k > 0) {
        const uint64_t v = tmp[--k];
        r.last_position = v;
        r.has_position = 1;
        r.n_positions += 1;
        commit(v);
    }
    return true;
}

// A committed position whose row exists goes to the caller's lists (one thread); the rows are gathered afterwards.
APT_STR_HD bool put_row(apt::stream::State &st, uint64_t pos, float score, uint64_t *positions, float *scores, uint32_t rows_cap)
{
    if (st.n_rows >= rows_cap) {
        st.status = 1;
        st.reason = apt::stream::kReasonOverflow;
        return false;
    }
    scores[st.n_rows] = score;
    return apt::stream::put_row(st, pos, positions, rows_cap);
}

}  // namespace apt::stream_track

// ---- the host side (apt_stream_track.cpp; CPU only)
namespace apt::stream_track {

// NULL = lag 8 and the track defaults.  A struct_size that is too small, lag_rows > 64 and everything
// apt::track::check_settings and pixel_width refuse: Error{Invalid}.
struct Design {
    apt::stream::Design stream;  // sync off; cap_f sized for the tracker
    Params T{};
};
Design design_tracked(const aptgpu_settings *settings, const aptgpu_stream_settings *ss, const aptgpu_live_track_settings *ts, int mode,
                      bool mfma_switch);

// The twin: the front end of apt::stream::HostStream, then the same tracker over host rings.
class HostTrackStream final : public apt::stream::HostLive {
public:
    explicit HostTrackStream(Design d);
    void reset() override;
    void push_segment(const void *samples, uint64_t n, bool finish, bool first, float *rows, uint64_t *positions, float *scores,
                      uint32_t rows_cap) override;
    const apt::stream::State &state() const override { return front_.state(); }
    const Record *track_record() const override { return &rec_; }
    uint64_t bytes() const override;
    uint32_t rows_bound(uint64_t n) const override { return rows_bound_after(d_.T, d_.stream.P, rec_.m, state().n_in + n); }

private:
    const apt::stream::Params &params() const override { return d_.stream.P; }
    Design d_;
    apt::stream::HostStream front_;
    Record rec_{};
    uint64_t dp_done_ = 0;
    std::vector<float> s_, best_;
    std::vector<int8_t> bp_;
};

}  // namespace apt::stream_track

#if defined(__HIPCC__)
namespace apt::gpu {

struct StreamTrackBuffers {
    apt::stream_track::Record *record;
    float *ring_s;
    float *ring_best;
    int8_t *ring_bp;
};
// k_stream_track_score: s[i] for i in [m0, m1) from the F ring (final below w1)
void stream_track_score(hipStream_t s, const apt::stream::Params &P, const apt::stream_track::Params &T, const StreamBuffers &b,
                        const StreamTrackBuffers &t, uint64_t m0, uint64_t m1, uint64_t w1);
// k_stream_track_dp: best / bp from m0 to m1 with the checkpoints on the way, the commit of a finish, the records and
// the released positions and their scores (appended at the push's row count so far)
void stream_track_dp(hipStream_t s, const apt::stream::Params &P, const apt::stream_track::Params &T, const StreamBuffers &b,
                     const StreamTrackBuffers &t, uint64_t *positions, float *scores, uint32_t rows_cap, uint64_t n_in, uint64_t m0,
                     uint64_t m1, uint64_t w1, bool first, bool finish);
// k_stream_track_rows: row[c] = F[v + pw c] for the positions this launch sequence released
void stream_track_rows(hipStream_t s, const apt::stream::Params &P, const StreamBuffers &b, const uint64_t *positions, float *rows,
                       uint32_t rows_cap, uint32_t grid_rows);

}  // namespace apt::gpu
#endif
