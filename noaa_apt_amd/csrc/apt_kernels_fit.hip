// apt_kernels_fit.hip — the gfx950 kernels of the overlay fit (definition: apt_kernels_fit.hpp, include/aptgpu.h;
// DESIGN.md §26).  Once per call:
//
//  k_fit_edge    G and its box sums through an LDS tile, one plane per round (blockIdx.z): the tile's G with a halo of
//                R as u16, the horizontal sums as u32 beside it, the vertical sums into HBM.  O(R) adds per sum.
//
// and per round, reading the round's centre from the record in HBM (no launch waits on the host):
//
//  k_fit_frames  one workgroup per shift of the round: the frame and D of its slice, bx[r] of its h rows, ky of every
//                vscale of the round; workgroup 0 also kx of every hscale and the record's SGP4 check.
//  k_fit_angles  one thread per shift and sample point: (a, b), and the valid ones compacted per shift (one atomic per
//                wave), so a point that is invalid for a shift costs the score kernel nothing.
//  k_fit_score   the hot one.  A workgroup takes one shift and a tile of 2048 valid points, eight per thread in
//                registers, the shift's bx in LDS (global reads above kBxLds rows), and walks the yaw x hscale x vscale
//                candidates.  Per candidate a lane packs its points' score and count into one u64; a wave with a
//                nonzero lane reduces it with shuffles and adds it to the candidate's LDS word; every 1024 candidates
//                the nonzero words go to HBM with one 64-bit and one 32-bit atomic add per workgroup and candidate.
//                Integer sums: exact in any order.
//  k_fit_pick    one workgroup: the candidates below min_points zeroed, the arg-max by exact rationals with the lowest
//                index on a tie, the round's entry and the next round's centre.
#include "apt_kernels_fit.hpp"

#include <memory>
#include <vector>

#include "apt_plan.hpp"

#pragma clang fp contract(off)

namespace apt::gpu {

using namespace apt::fit;

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 8;
constexpr uint32_t kTile = kThreads * kPerThread;
constexpr uint32_t kChunk = 1024;   // candidates per LDS pass
constexpr uint32_t kBxLds = 4096;   // rows of bx held in LDS (32 KiB)
constexpr int kCountShift = 40;     // packed word: score below (2048 points * 129 * 129 * 510 < 2^35), count above

struct Tables {
    aptgpu_fit_result *rec;
    const uint32_t *err;      // SGP4's error word (0 with a caller's track)
    const double *track;      // h + 2 M pairs
    const double *points;     // n_points (lon, lat) pairs in degrees
    Shift *shifts;            // per shift index of the round
    uint32_t *shift_ok;
    uint32_t *n_valid;        // per shift index: compacted points
    double *bx;               // ns * h
    double *ky;               // ns * nv
    double *kx;               // nh
    double2 *ab;              // ns * n_points, the first n_valid[is] of each row
    Sum *sums;                // rounds * total
    const uint32_t *planes;   // rounds * h * 909
    uint32_t h, n_points;
    int32_t margin;
    uint32_t min_points;
    int32_t rounds;
};

__device__ inline bool stopped(const Tables &t) { return t.rec->done != 0 || *t.err != 0; }

__device__ inline int64_t shift_at(const Tables &t, const Grid &g, int round, uint32_t is)
{
    return static_cast<int64_t>(t.rec->round[round].c_shift) +
           (static_cast<int64_t>(is) - g.n_shift) * static_cast<int64_t>(g.shift_step);
}

// image: h rows of 2080 bytes.  Dynamic LDS: (th + 2 R0) * (tw + 2 R0) u16, then (th + 2 R0) * tw u32.
__global__ __launch_bounds__(kThreads) void k_fit_edge(const uint8_t *__restrict__ image, uint32_t h, int base,
                                                       int radius_last, int rounds, int tw, int th,
                                                       uint32_t hs_offset, uint32_t *__restrict__ planes)
{
    extern __shared__ __align__(16) unsigned char lds[];
    const int round = blockIdx.z;
    const int R = radius_last << (rounds - 1 - round);
    const int w2 = tw + 2 * R, h2 = th + 2 * R;
    uint16_t *g = reinterpret_cast<uint16_t *>(lds);
    uint32_t *hs = reinterpret_cast<uint32_t *>(lds + hs_offset);
    const int k0 = static_cast<int>(blockIdx.x) * tw, r0 = static_cast<int>(blockIdx.y) * th;
    const int hh = static_cast<int>(h);
    const uint8_t *v = image + base + kVideo0;
    for (int i = threadIdx.x; i < w2 * h2; i += kThreads) {
        const int r = r0 - R + i / w2, k = k0 - R + i % w2;
        uint32_t val = 0;
        if (r >= 0 && r < hh && k >= 0 && k < kVideoN) {
            const uint8_t *row = v + static_cast<size_t>(r) * kPx;
            const int dh = static_cast<int>(row[k + 1 < kVideoN ? k + 1 : kVideoN - 1]) - static_cast<int>(row[k > 0 ? k - 1 : 0]);
            const int dv = static_cast<int>(v[static_cast<size_t>(r + 1 < hh ? r + 1 : hh - 1) * kPx + k]) -
                           static_cast<int>(v[static_cast<size_t>(r > 0 ? r - 1 : 0) * kPx + k]);
            val = static_cast<uint32_t>((dh < 0 ? -dh : dh) + (dv < 0 ? -dv : dv));
        }
        g[i] = static_cast<uint16_t>(val);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < tw * h2; i += kThreads) {
        const int j = i / tw, c = i % tw;
        uint32_t acc = 0;
        for (int d = 0; d <= 2 * R; ++d) acc += g[j * w2 + c + d];
        hs[i] = acc;
    }
    __syncthreads();
    uint32_t *plane = planes + static_cast<size_t>(round) * h * kVideoN;
    for (int i = threadIdx.x; i < tw * th; i += kThreads) {
        const int j = i / tw, c = i % tw;
        const int r = r0 + j, k = k0 + c;
        if (r >= hh || k >= kVideoN) continue;
        uint32_t acc = 0;
        for (int d = 0; d <= 2 * R; ++d) acc += hs[(j + d) * tw + c];
        plane[static_cast<size_t>(r) * kVideoN + k] = acc;
    }
}

__global__ __launch_bounds__(kThreads) void k_fit_frames(Tables t, Grid g, int round)
{
    __shared__ Shift f;
    const uint32_t is = blockIdx.x;
    if (is == 0 && threadIdx.x == 0 && *t.err != 0 && t.rec->done == 0) {
        t.rec->status = APTGPU_ERR_INTERNAL;
        t.rec->reason = apt::geoloc::kReasonSgp4;
        t.rec->done = 1;
    }
    if (stopped(t)) return;
    const aptgpu_fit_round &e = t.rec->round[round];
    if (is == 0)
        for (uint32_t ih = threadIdx.x; ih < g.nh(); ih += kThreads)
            t.kx[ih] = kx_of(axis_value(e.c_hscale, static_cast<int>(ih) - g.n_hscale, g.hscale_step));
    const int64_t s = shift_at(t, g, round, is);
    const bool ok = s >= -static_cast<int64_t>(t.margin) && s <= static_cast<int64_t>(t.margin);
    if (threadIdx.x == 0) {
        t.shift_ok[is] = ok ? 1u : 0u;
        t.n_valid[is] = 0;
    }
    if (!ok) return;
    const double *tr = t.track + 2 * (static_cast<int64_t>(t.margin) + s);
    if (threadIdx.x == 0) {
        f = shift_of(tr[0], tr[1], tr[2 * (t.h - 1)], tr[2 * (t.h - 1) + 1]);
        t.shifts[is] = f;
    }
    __syncthreads();
    const Shift fr = f;
    for (uint32_t r = threadIdx.x; r < t.h; r += kThreads)
        t.bx[static_cast<size_t>(is) * t.h + r] = bx_of(fr, tr[2 * r], tr[2 * r + 1], r);
    for (uint32_t iv = threadIdx.x; iv < g.nv(); iv += kThreads)
        t.ky[static_cast<size_t>(is) * g.nv() + iv] =
            ky_of(t.h, axis_value(e.c_vscale, static_cast<int>(iv) - g.n_vscale, g.vscale_step), fr.d);
}

__global__ __launch_bounds__(kThreads) void k_fit_angles(Tables t)
{
    const uint32_t is = blockIdx.y;
    if (stopped(t) || t.shift_ok[is] == 0) return;
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    double a = 0., b = 0.;
    bool valid = false;
    if (i < t.n_points) {
        const Shift f = t.shifts[is];
        double p[3];
        unit_of_deg(t.points[2 * static_cast<size_t>(i)], t.points[2 * static_cast<size_t>(i) + 1], p);
        valid = angles_of(f, p, a, b);
    }
    const unsigned long long m = __ballot(valid);
    if (m == 0) return;
    const int lane = threadIdx.x & 63;
    uint32_t first = 0;
    if (lane == 0) first = atomicAdd(&t.n_valid[is], static_cast<uint32_t>(__popcll(m)));
    first = static_cast<uint32_t>(__shfl(static_cast<int>(first), 0));
    if (valid) {
        const uint32_t slot = first + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
        t.ab[static_cast<size_t>(is) * t.n_points + slot] = make_double2(a, b);
    }
}

__device__ inline uint32_t shfl_xor_u32(uint32_t v, int d) { return static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), d)); }

template <bool BX_LDS>
__global__ __launch_bounds__(kThreads) void k_fit_score(Tables t, Grid g, int round)
{
    __shared__ unsigned long long acc[kChunk];
    __shared__ double bx_lds[BX_LDS ? kBxLds : 1];
    const uint32_t is = blockIdx.y;
    if (stopped(t) || t.shift_ok[is] == 0) return;
    const uint32_t n_valid = t.n_valid[is];
    const uint32_t tile0 = blockIdx.x * kTile;
    if (tile0 >= n_valid) return;
    const uint32_t h = t.h;
    const double *bx_g = t.bx + static_cast<size_t>(is) * h;
    if (BX_LDS)
        for (uint32_t r = threadIdx.x; r < h; r += kThreads) bx_lds[r] = bx_g[r];
    const double *bx = BX_LDS ? bx_lds : bx_g;

    double pa[kPerThread], pb[kPerThread];
    const double2 *ab = t.ab + static_cast<size_t>(is) * t.n_points;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const uint32_t j = tile0 + static_cast<uint32_t>(k) * kThreads + threadIdx.x;
        double2 v = make_double2(apt::geoloc::quiet_nan64(), 0.);  // (a NaN place is outside)
        if (j < n_valid) v = ab[j];
        pa[k] = v.x;
        pb[k] = v.y;
    }

    const aptgpu_fit_round &e = t.rec->round[round];
    const double c_yaw = e.c_yaw, c_hscale = e.c_hscale, c_vscale = e.c_vscale;
    const uint32_t nh = g.nh(), nv = g.nv(), per_shift = g.per_shift();
    const uint32_t *plane = t.planes + static_cast<size_t>(round) * h * kVideoN;
    Sum *out = t.sums + static_cast<size_t>(round) * g.total() + static_cast<size_t>(is) * per_shift;
    const double *ky_tab = t.ky + static_cast<size_t>(is) * nv;

    for (uint32_t c0 = 0; c0 < per_shift; c0 += kChunk) {
        const uint32_t c1 = c0 + kChunk < per_shift ? c0 + kChunk : per_shift;
        __syncthreads();  // (bx_lds is written; the previous chunk's words have been read)
        for (uint32_t k = threadIdx.x; k < c1 - c0; k += kThreads) acc[k] = 0ull;
        __syncthreads();
        for (uint32_t c = c0; c < c1; ++c) {
            const uint32_t iv = c % nv, ih = c / nv % nh, iy = c / (nv * nh);
            const double hscale = axis_value(c_hscale, static_cast<int>(ih) - g.n_hscale, g.hscale_step);
            const double vscale = axis_value(c_vscale, static_cast<int>(iv) - g.n_vscale, g.vscale_step);
            if (!(hscale > 0.) || !(vscale > 0.)) continue;
            const double yaw = axis_value(c_yaw, static_cast<int>(iy) - g.n_yaw, g.yaw_step);
            const double kx = t.kx[ih], ky = ky_tab[iv];
            unsigned long long mine = 0ull;
#pragma unroll
            for (int k = 0; k < kPerThread; ++k) {
                const int64_t at = place_of(pa[k], pb[k], yaw, kx, ky, h, bx);
                if (at >= 0) mine += static_cast<unsigned long long>(plane[at]) + (1ull << kCountShift);
            }
            if (__ballot(mine != 0ull) == 0ull) continue;
            uint32_t lo = static_cast<uint32_t>(mine), hi = static_cast<uint32_t>(mine >> 32);
            for (int d = 32; d >= 1; d >>= 1) {
                const uint32_t olo = shfl_xor_u32(lo, d), ohi = shfl_xor_u32(hi, d);
                const unsigned long long sum = ((static_cast<unsigned long long>(hi) << 32) | lo) +
                                               ((static_cast<unsigned long long>(ohi) << 32) | olo);
                lo = static_cast<uint32_t>(sum);
                hi = static_cast<uint32_t>(sum >> 32);
            }
            if ((threadIdx.x & 63) == 0) atomicAdd(&acc[c - c0], (static_cast<unsigned long long>(hi) << 32) | lo);
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < c1 - c0; k += kThreads) {
            const unsigned long long v = acc[k];
            if (v == 0ull) continue;
            Sum *o = out + c0 + k;
            atomicAdd(reinterpret_cast<unsigned long long *>(&o->score), v & ((1ull << kCountShift) - 1ull));
            atomicAdd(&o->count, static_cast<uint32_t>(v >> kCountShift));
        }
    }
}

struct Best {
    uint64_t score;
    uint32_t count, index;  // count 0: none
};
__device__ inline bool wins(const Best &a, const Best &b)
{
    if (a.count == 0) return false;
    if (b.count == 0) return true;
    if (better(a.score, a.count, b.score, b.count)) return true;
    if (better(b.score, b.count, a.score, a.count)) return false;
    return a.index < b.index;
}

__global__ __launch_bounds__(kThreads) void k_fit_pick(Tables t, Grid g, int round)
{
    __shared__ Best best[kThreads];
    if (stopped(t)) return;
    const uint32_t total = g.total();
    Sum *sums = t.sums + static_cast<size_t>(round) * total;
    Best mine{0, 0, 0};
    for (uint32_t c = threadIdx.x; c < total; c += kThreads) {
        const Sum s = sums[c];
        if (s.count < t.min_points) {
            if (s.count != 0 || s.score != 0) sums[c] = Sum{0, 0, 0};
            continue;
        }
        const Best b{s.score, s.count, c};
        if (wins(b, mine)) mine = b;
    }
    best[threadIdx.x] = mine;
    __syncthreads();
    for (int d = kThreads / 2; d >= 1; d >>= 1) {
        if (static_cast<int>(threadIdx.x) < d && wins(best[threadIdx.x + d], best[threadIdx.x]))
            best[threadIdx.x] = best[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    aptgpu_fit_result &rec = *t.rec;
    aptgpu_fit_round &e = rec.round[round];
    const Best w = best[0];
    rec.n_rounds = static_cast<uint32_t>(round) + 1u;
    if (w.count == 0) {
        rec.status = APTGPU_ERR_INTERNAL;
        rec.reason = kReasonNoCandidate;
        rec.done = 1;
        return;
    }
    const uint32_t ny = g.ny(), nh = g.nh(), nv = g.nv();
    const uint32_t iv = w.index % nv, ih = w.index / nv % nh, iy = w.index / (nv * nh) % ny, is = w.index / (nv * nh * ny);
    e.w_shift = static_cast<int32_t>(shift_at(t, g, round, is));
    e.w_yaw = axis_value(e.c_yaw, static_cast<int>(iy) - g.n_yaw, g.yaw_step);
    e.w_hscale = axis_value(e.c_hscale, static_cast<int>(ih) - g.n_hscale, g.hscale_step);
    e.w_vscale = axis_value(e.c_vscale, static_cast<int>(iv) - g.n_vscale, g.vscale_step);
    e.score = w.score;
    e.count = w.count;
    e.index = w.index;
    e.q = static_cast<double>(w.score) / static_cast<double>(w.count);
    if (w.score == 0) {
        rec.reason = kReasonFlat;  // the result is the initial settings
        rec.yaw = rec.round[0].c_yaw;
        rec.hscale = rec.round[0].c_hscale;
        rec.vscale = rec.round[0].c_vscale;
        rec.shift_rows = 0;
        rec.time_offset_ms = 0;
        rec.q = -1.;
        rec.count = 0;
        rec.done = 1;
        return;
    }
    rec.yaw = e.w_yaw;
    rec.hscale = e.w_hscale;
    rec.vscale = e.w_vscale;
    rec.shift_rows = e.w_shift;
    rec.time_offset_ms = kLineMs * static_cast<int64_t>(e.w_shift);
    rec.q = e.q;
    rec.count = e.count;
    if (round + 1 < t.rounds) {
        aptgpu_fit_round &n = rec.round[round + 1];
        n.c_yaw = e.w_yaw;
        n.c_hscale = e.w_hscale;
        n.c_vscale = e.w_vscale;
        n.c_shift = e.w_shift;
    } else {
        rec.done = 1;
    }
}

uint32_t blocks(uint64_t n, uint32_t per)
{
    const uint64_t b = (n + per - 1) / per;
    return static_cast<uint32_t>(b ? b : 1);
}

}  // namespace

struct FitWorkspace {
    apt::DeviceBuffer<char> rec;
    apt::DeviceBuffer<uint32_t> words;  // [0] SGP4's error; then shift_ok and n_valid per shift
    apt::DeviceBuffer<double> track, points, bx, ky, kx;
    apt::DeviceBuffer<char> shifts, ab, sums;
    apt::DeviceBuffer<uint32_t> planes;
    aptgpu_fit_result first{};
    size_t n_sums = 0;
    std::vector<hipEvent_t> events;
    ~FitWorkspace()
    {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
    }
};

FitWorkspace *fit_ws_create(const FitLaunch &l)
{
    auto ws = std::make_unique<FitWorkspace>();
    const Grid &g = l.st.grid;
    const size_t ns = g.ns(), np = l.n_points ? l.n_points : 1;
    ws->rec.alloc(sizeof(aptgpu_fit_result));
    ws->words.alloc(1 + 2 * ns);
    ws->track.alloc(2 * (static_cast<size_t>(l.h) + 2 * static_cast<size_t>(l.st.margin)));
    ws->points.alloc(2 * np);
    ws->bx.alloc(ns * l.h);
    ws->ky.alloc(ns * g.nv());
    ws->kx.alloc(g.nh());
    ws->shifts.alloc(ns * sizeof(Shift));
    ws->ab.alloc(ns * np * sizeof(double2));
    ws->n_sums = static_cast<size_t>(l.st.rounds) * g.total();
    ws->sums.alloc(ws->n_sums * sizeof(Sum));
    ws->planes.alloc(static_cast<size_t>(l.st.rounds) * l.h * kVideoN);
    return ws.release();
}

void fit_ws_destroy(FitWorkspace *ws) { delete ws; }
const aptgpu_fit_result *fit_ws_record(const FitWorkspace *ws) { return reinterpret_cast<const aptgpu_fit_result *>(ws->rec.ptr); }
const apt::fit::Sum *fit_ws_scores(const FitWorkspace *ws) { return reinterpret_cast<const Sum *>(ws->sums.ptr); }

void fit_enqueue(hipStream_t s, const FitLaunch &l, FitWorkspace *ws, float *ms)
{
    const Settings &st = l.st;
    const uint32_t h = l.h, ns = st.grid.ns();
    const size_t track_rows = static_cast<size_t>(h) + 2 * static_cast<size_t>(st.margin);
    ws->first = first_record(h, l.geom, st, l.n_points);
    apt::hip_check(hipMemcpyAsync(ws->rec.ptr, &ws->first, sizeof ws->first, hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D (fit record)");
    apt::hip_check(hipMemsetAsync(ws->words.ptr, 0, (1 + 2 * static_cast<size_t>(ns)) * sizeof(uint32_t), s), "hipMemsetAsync");
    apt::hip_check(hipMemsetAsync(ws->sums.ptr, 0, ws->n_sums * sizeof(Sum), s), "hipMemsetAsync");
    if (l.n_points)
        apt::hip_check(hipMemcpyAsync(ws->points.ptr, l.points, 2 * static_cast<size_t>(l.n_points) * sizeof(double), hipMemcpyHostToDevice, s),
                       "hipMemcpyAsync H2D (fit points)");
    if (l.sat)
        apt::sat::track(s, *l.sat, nullptr, static_cast<uint32_t>(track_rows), static_cast<uint32_t>(track_rows), ws->track.ptr, ws->words.ptr);
    else
        apt::hip_check(hipMemcpyAsync(ws->track.ptr, l.positions, 2 * track_rows * sizeof(double), hipMemcpyHostToDevice, s),
                       "hipMemcpyAsync H2D (fit track)");

    Tables t{};
    t.rec = reinterpret_cast<aptgpu_fit_result *>(ws->rec.ptr);
    t.err = ws->words.ptr;
    t.track = ws->track.ptr;
    t.points = ws->points.ptr;
    t.shifts = reinterpret_cast<Shift *>(ws->shifts.ptr);
    t.shift_ok = ws->words.ptr + 1;
    t.n_valid = ws->words.ptr + 1 + ns;
    t.bx = ws->bx.ptr;
    t.ky = ws->ky.ptr;
    t.kx = ws->kx.ptr;
    t.ab = reinterpret_cast<double2 *>(ws->ab.ptr);
    t.sums = reinterpret_cast<Sum *>(ws->sums.ptr);
    t.planes = ws->planes.ptr;
    t.h = h;
    t.n_points = l.n_points;
    t.margin = st.margin;
    t.min_points = st.min_points;
    t.rounds = st.rounds;

    // event pairs around the launches of each group: 0 edge, 1 angles (with the frames), 2 score, 3 pick
    std::vector<int> group;
    auto timed = [&](int which, auto &&launch) {
        if (!ms) return launch();
        hipEvent_t a, b;
        apt::hip_check(hipEventCreate(&a), "hipEventCreate");
        ws->events.push_back(a);
        apt::hip_check(hipEventCreate(&b), "hipEventCreate");
        ws->events.push_back(b);
        group.push_back(which);
        apt::hip_check(hipEventRecord(a, s), "hipEventRecord");
        launch();
        apt::hip_check(hipEventRecord(b, s), "hipEventRecord");
    };

    const int r0 = radius_of_round(st, 0);
    const int tw = r0 <= 32 ? 64 : 32, th = r0 <= 32 ? 16 : 8;
    const uint32_t hs_offset = (static_cast<uint32_t>((th + 2 * r0) * (tw + 2 * r0)) * 2u + 15u) & ~15u;
    const uint32_t lds = hs_offset + static_cast<uint32_t>((th + 2 * r0) * tw) * 4u;  // at most 60 944 bytes
    timed(0, [&] {
        hipLaunchKernelGGL(k_fit_edge, dim3(blocks(kVideoN, tw), blocks(h, th), st.rounds), dim3(kThreads), lds, s, l.image, h,
                           kHalfPx * st.channel, st.radius, st.rounds, tw, th, hs_offset, ws->planes.ptr);
    });
    for (int round = 0; round < st.rounds; ++round) {
        const Grid g = grid_of_round(st, round);
        timed(1, [&] {
            hipLaunchKernelGGL(k_fit_frames, dim3(ns), dim3(kThreads), 0, s, t, g, round);
            if (l.n_points) hipLaunchKernelGGL(k_fit_angles, dim3(blocks(l.n_points, kThreads), ns), dim3(kThreads), 0, s, t);
        });
        timed(2, [&] {
            if (!l.n_points) return;
            const dim3 grid(blocks(l.n_points, kTile), ns);
            if (h <= kBxLds)
                hipLaunchKernelGGL(k_fit_score<true>, grid, dim3(kThreads), 0, s, t, g, round);
            else
                hipLaunchKernelGGL(k_fit_score<false>, grid, dim3(kThreads), 0, s, t, g, round);
        });
        timed(3, [&] { hipLaunchKernelGGL(k_fit_pick, dim3(1), dim3(kThreads), 0, s, t, g, round); });
    }
    apt::hip_check(hipGetLastError(), "kernel launch (overlay fit)");
    if (ms) {
        apt::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        ms[0] = ms[1] = ms[2] = ms[3] = 0.f;
        for (size_t i = 0; i < group.size(); ++i) {
            float v = 0.f;
            apt::hip_check(hipEventElapsedTime(&v, ws->events[2 * i], ws->events[2 * i + 1]), "hipEventElapsedTime");
            ms[group[i]] += v;
        }
    }
}

}  // namespace apt::gpu
