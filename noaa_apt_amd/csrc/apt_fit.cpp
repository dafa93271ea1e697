// apt_fit.cpp — the overlay fit on the CPU: the checks every entry point shares, the sampler of the layer set and the
// definition of apt_kernels_fit.hpp in plain C++ (aptgpu_fit_overlay_host), which the kernels are tested against and
// which a stand-alone program can call without a GPU.
#include "apt_kernels_fit.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace apt::fit {

Settings check_settings(const aptgpu_fit_settings *s)
{
    if (!s) throw Error{ErrorKind::Invalid, "fit: settings are required"};
    if (s->struct_size < sizeof(aptgpu_fit_settings))
        throw Error{ErrorKind::Invalid, "aptgpu_fit_settings: struct_size not set"};
    if (s->flags) throw Error{ErrorKind::Invalid, "fit: unknown flag"};
    if (s->channel != 0 && s->channel != 1) throw Error{ErrorKind::Invalid, "fit: channel must be 0 (A) or 1 (B)"};
    if (s->layer_mask & ~7u) throw Error{ErrorKind::Invalid, "fit: unknown layer in layer_mask"};
    if (s->rounds < 1 || s->rounds > kMaxRounds) throw Error{ErrorKind::Invalid, "fit: rounds must lie in 1 .. 8"};
    if (s->margin_rows < 0 || s->radius < 0 || s->n_shift < 0 || s->n_yaw < 0 || s->n_hscale < 0 || s->n_vscale < 0)
        throw Error{ErrorKind::Invalid, "fit: negative count, margin or radius"};
    if (!(s->yaw_step >= 0.) || !(s->hscale_step >= 0.) || !(s->vscale_step >= 0.) || !std::isfinite(s->yaw_step) ||
        !std::isfinite(s->hscale_step) || !std::isfinite(s->vscale_step))
        throw Error{ErrorKind::Invalid, "fit: steps must be finite and not negative"};
    if (s->shift_step < 1) throw Error{ErrorKind::Invalid, "fit: shift_step must be at least 1"};
    if (s->min_points < 1) throw Error{ErrorKind::Invalid, "fit: min_points must be at least 1"};
    if (s->radius > kMaxRadius || (static_cast<int64_t>(s->radius) << (s->rounds - 1)) > kMaxRadius)
        throw Error{ErrorKind::Invalid, "fit: radius << (rounds - 1) must not exceed 64"};
    if (!(s->spacing_deg > 0.) || !std::isfinite(s->spacing_deg))
        throw Error{ErrorKind::Invalid, "fit: spacing_deg must be positive"};
    uint64_t total = 1;
    for (int32_t n : {s->n_shift, s->n_yaw, s->n_hscale, s->n_vscale}) {
        total *= 2u * static_cast<uint64_t>(n) + 1u;
        if (total > kMaxCandidates) throw Error{ErrorKind::Invalid, "fit: more than 2^20 candidates in a round"};
    }
    Settings o{};
    o.channel = s->channel;
    o.mask = s->layer_mask ? s->layer_mask : (1u << apt::map::Layers::kCountries) | (1u << apt::map::Layers::kLakes);
    o.margin = s->margin_rows;
    o.rounds = s->rounds;
    o.radius = s->radius;
    o.min_points = static_cast<uint32_t>(s->min_points);
    o.spacing = s->spacing_deg;
    o.timing = s->timing != 0;
    o.grid = Grid{s->n_shift, s->n_yaw, s->n_hscale, s->n_vscale, s->shift_step, s->yaw_step, s->hscale_step, s->vscale_step};
    return o;
}

void check_call(const void *positions, const void *orbit, size_t h, const Settings &st)
{
    if ((positions != nullptr) == (orbit != nullptr))
        throw Error{ErrorKind::Invalid, "fit: exactly one of sat_positions and orbit is required"};
    if (h < kMinHeight) throw Error{ErrorKind::Invalid, "fit: fewer than 16 rows (APTGPU_GEOLOC_REASON_HEIGHT)"};
    if (h + 2 * static_cast<size_t>(st.margin) > apt::geoloc::kMaxRows)
        throw Error{ErrorKind::Invalid, "fit: more than 2^22 rows"};
}

Grid grid_of_round(const Settings &st, int round)
{
    Grid g = st.grid;
    const int32_t step = round < 31 ? st.grid.shift_step >> round : 0;
    g.shift_step = step > 1 ? step : 1;
    const double scale = std::ldexp(1., -round);
    g.yaw_step = st.grid.yaw_step * scale;
    g.hscale_step = st.grid.hscale_step * scale;
    g.vscale_step = st.grid.vscale_step * scale;
    return g;
}

int radius_of_round(const Settings &st, int round) { return st.radius << (st.rounds - 1 - round); }

const char *reason_text(int reason)
{
    switch (reason) {
    case apt::geoloc::kReasonCount: return "fit: the number of satellite positions differs from the image height plus twice margin_rows";
    case apt::geoloc::kReasonSgp4: return "satellite track: SGP4 failed for a row of the track (APTGPU_SAT_REASON_SGP4)";
    case apt::geoloc::kReasonHeight: return "fit: fewer than 16 rows (APTGPU_GEOLOC_REASON_HEIGHT)";
    case kReasonNoCandidate: return "fit: a round has no candidate with min_points points inside the image (APTGPU_FIT_REASON_NO_CANDIDATE)";
    default: return "overlay fit failed";
    }
}

void put_result(aptgpu_fit_result *out, aptgpu_fit_result r)
{
    if (!out) return;
    const uint32_t size = out->struct_size;
    r.struct_size = size;
    std::memcpy(out, &r, size < sizeof r ? size : sizeof r);
}

aptgpu_fit_result first_record(uint32_t h, const apt::geoloc::Geom &g, const Settings &st, uint32_t n_points)
{
    aptgpu_fit_result r{};
    r.struct_size = sizeof r;
    r.height = h;
    r.n_points = n_points;
    r.n_candidates = st.grid.total();
    r.yaw = g.yaw;
    r.hscale = g.hscale;
    r.vscale = g.vscale;
    r.q = -1.;
    r.round[0].c_yaw = g.yaw;
    r.round[0].c_hscale = g.hscale;
    r.round[0].c_vscale = g.vscale;
    for (aptgpu_fit_round &e : r.round) e.q = -1.;
    return r;
}

std::vector<double> sample_points(const apt::map::Layers &layers, uint32_t mask, double spacing_deg)
{
    std::vector<double> out;
    auto push = [&](double lon, double lat) {
        if (out.size() / 2 >= kMaxPoints) throw Error{ErrorKind::Invalid, "fit: more than 2^22 sample points"};
        out.push_back(lon);
        out.push_back(lat);
    };
    for (int k = 0; k < 3; ++k) {
        if (!(mask >> k & 1u) || !layers.present[k]) continue;
        const apt::map::Layer &l = layers.layer[k];
        for (size_t p = 0; p + 1 < l.parts.size(); ++p) {
            const size_t from = l.parts[p], to = l.parts[p + 1];
            if (to - from == 1) push(l.xy[2 * from], l.xy[2 * from + 1]);
            for (size_t j = from; j + 1 < to; ++j) {
                const double x0 = l.xy[2 * j], y0 = l.xy[2 * j + 1], x1 = l.xy[2 * j + 2], y1 = l.xy[2 * j + 3];
                const double dx = x1 - x0, dy = y1 - y0;
                const double span = std::fmax(std::fabs(dx), std::fabs(dy));
                const double steps = std::ceil(span / spacing_deg);
                // (a non-finite vertex gives one point, itself: its place is outside every image)
                if (steps > static_cast<double>(kMaxPoints)) throw Error{ErrorKind::Invalid, "fit: more than 2^22 sample points"};
                const uint32_t n = steps >= 1. ? static_cast<uint32_t>(steps) : 1u;
                for (uint32_t i = 0; i < n; ++i) {
                    const double f = static_cast<double>(i) / static_cast<double>(n);
                    push(x0 + dx * f, y0 + dy * f);
                }
            }
        }
    }
    return out;
}

namespace {

// G and its box sums, directly
std::vector<uint32_t> edge_plane(const uint8_t *image, uint32_t h, int channel, int radius)
{
    const int w = kVideoN, hh = static_cast<int>(h);
    const uint8_t *v = image + kHalfPx * channel + kVideo0;
    auto px = [&](int r, int k) { return static_cast<int>(v[static_cast<size_t>(r) * kPx + static_cast<size_t>(k)]); };
    std::vector<uint32_t> g(static_cast<size_t>(h) * w), rowsum(g.size()), e(g.size());
    for (int r = 0; r < hh; ++r)
        for (int k = 0; k < w; ++k) {
            const int dh = px(r, k + 1 < w ? k + 1 : w - 1) - px(r, k > 0 ? k - 1 : 0);
            const int dv = px(r + 1 < hh ? r + 1 : hh - 1, k) - px(r > 0 ? r - 1 : 0, k);
            g[static_cast<size_t>(r) * w + k] = static_cast<uint32_t>((dh < 0 ? -dh : dh) + (dv < 0 ? -dv : dv));
        }
    for (int r = 0; r < hh; ++r)
        for (int k = 0; k < w; ++k) {
            uint32_t acc = 0;
            for (int j = (k - radius > 0 ? k - radius : 0); j <= (k + radius < w - 1 ? k + radius : w - 1); ++j)
                acc += g[static_cast<size_t>(r) * w + j];
            rowsum[static_cast<size_t>(r) * w + k] = acc;
        }
    for (int r = 0; r < hh; ++r)
        for (int k = 0; k < w; ++k) {
            uint32_t acc = 0;
            for (int j = (r - radius > 0 ? r - radius : 0); j <= (r + radius < hh - 1 ? r + radius : hh - 1); ++j)
                acc += rowsum[static_cast<size_t>(j) * w + k];
            e[static_cast<size_t>(r) * w + k] = acc;
        }
    return e;
}

}  // namespace

void run_host(const uint8_t *image, size_t h_in, const double *track, size_t count, const std::vector<double> &points,
              const apt::geoloc::Geom &geom, const Settings &st, Sum *scores, aptgpu_fit_result *info)
{
    const uint32_t h = static_cast<uint32_t>(h_in);
    const size_t n_points = points.size() / 2;
    aptgpu_fit_result rec = first_record(h, geom, st, static_cast<uint32_t>(n_points));
    const uint32_t total = st.grid.total();
    if (scores) std::memset(scores, 0, sizeof(Sum) * total * static_cast<size_t>(st.rounds));
    auto fail = [&](int reason) {
        rec.status = APTGPU_ERR_INTERNAL;
        rec.reason = reason;
        rec.done = 1;
        put_result(info, rec);
        throw Error{ErrorKind::Internal, reason_text(reason)};
    };
    if (count != h + 2 * static_cast<size_t>(st.margin)) fail(apt::geoloc::kReasonCount);

    std::vector<double> unit(3 * n_points);
    for (size_t i = 0; i < n_points; ++i) {
        double p[3];
        unit_of_deg(points[2 * i], points[2 * i + 1], p);
        unit[3 * i] = p[0];
        unit[3 * i + 1] = p[1];
        unit[3 * i + 2] = p[2];
    }
    std::vector<double> ab, bx(h);
    std::vector<Sum> sums(total);
    for (int round = 0; round < st.rounds && !rec.done; ++round) {
        const Grid g = grid_of_round(st, round);
        const std::vector<uint32_t> plane = edge_plane(image, h, st.channel, radius_of_round(st, round));
        aptgpu_fit_round &e = rec.round[round];
        std::fill(sums.begin(), sums.end(), Sum{});
        const uint32_t ny = g.ny(), nh = g.nh(), nv = g.nv();
        for (uint32_t is = 0; is < g.ns(); ++is) {
            const int64_t s = static_cast<int64_t>(e.c_shift) + (static_cast<int64_t>(is) - g.n_shift) * g.shift_step;
            if (s < -st.margin || s > st.margin) continue;
            const double *t = track + 2 * (st.margin + s);
            const Shift f = shift_of(t[0], t[1], t[2 * (h - 1)], t[2 * (h - 1) + 1]);
            for (uint32_t r = 0; r < h; ++r) bx[r] = bx_of(f, t[2 * r], t[2 * r + 1], r);
            ab.clear();
            for (size_t i = 0; i < n_points; ++i) {
                const double p[3] = {unit[3 * i], unit[3 * i + 1], unit[3 * i + 2]};
                double a, b;
                if (angles_of(f, p, a, b)) {
                    ab.push_back(a);
                    ab.push_back(b);
                }
            }
            Sum *out = sums.data() + static_cast<size_t>(is) * g.per_shift();
            for (uint32_t iy = 0; iy < ny; ++iy) {
                const double yaw = axis_value(e.c_yaw, static_cast<int>(iy) - g.n_yaw, g.yaw_step);
                for (uint32_t ih = 0; ih < nh; ++ih) {
                    const double hscale = axis_value(e.c_hscale, static_cast<int>(ih) - g.n_hscale, g.hscale_step);
                    if (!(hscale > 0.)) continue;
                    const double kx = kx_of(hscale);
                    for (uint32_t iv = 0; iv < nv; ++iv) {
                        const double vscale = axis_value(e.c_vscale, static_cast<int>(iv) - g.n_vscale, g.vscale_step);
                        if (!(vscale > 0.)) continue;
                        const double ky = ky_of(h, vscale, f.d);
                        uint64_t score = 0;
                        uint32_t inside = 0;
                        for (size_t i = 0; i < ab.size(); i += 2) {
                            const int64_t at = place_of(ab[i], ab[i + 1], yaw, kx, ky, h, bx.data());
                            if (at >= 0) {
                                score += plane[static_cast<size_t>(at)];
                                inside += 1;
                            }
                        }
                        out[(iy * nh + ih) * nv + iv] = Sum{score, inside, 0};
                    }
                }
            }
        }
        // the winner: the greatest score / count among the candidates with min_points points, the lowest index on a tie
        int64_t best = -1;
        for (uint32_t c = 0; c < total; ++c) {
            if (sums[c].count < st.min_points) {
                sums[c] = Sum{};
                continue;
            }
            if (best < 0 || better(sums[c].score, sums[c].count, sums[static_cast<size_t>(best)].score, sums[static_cast<size_t>(best)].count))
                best = c;
        }
        if (scores) std::memcpy(scores + static_cast<size_t>(round) * total, sums.data(), sizeof(Sum) * total);
        rec.n_rounds = static_cast<uint32_t>(round) + 1;
        if (best < 0) fail(kReasonNoCandidate);
        const uint32_t b = static_cast<uint32_t>(best);
        const uint32_t iv = b % nv, ih = b / nv % nh, iy = b / (nv * nh) % ny, is = b / (nv * nh * ny);
        e.w_shift = static_cast<int32_t>(e.c_shift + (static_cast<int64_t>(is) - g.n_shift) * g.shift_step);
        e.w_yaw = axis_value(e.c_yaw, static_cast<int>(iy) - g.n_yaw, g.yaw_step);
        e.w_hscale = axis_value(e.c_hscale, static_cast<int>(ih) - g.n_hscale, g.hscale_step);
        e.w_vscale = axis_value(e.c_vscale, static_cast<int>(iv) - g.n_vscale, g.vscale_step);
        e.score = sums[b].score;
        e.count = sums[b].count;
        e.index = b;
        e.q = static_cast<double>(e.score) / static_cast<double>(e.count);
        if (e.score == 0) {
            rec.reason = kReasonFlat;  // the result is the initial settings
            rec.yaw = rec.round[0].c_yaw;
            rec.hscale = rec.round[0].c_hscale;
            rec.vscale = rec.round[0].c_vscale;
            rec.shift_rows = 0;
            rec.time_offset_ms = 0;
            rec.q = -1.;
            rec.count = 0;
            rec.done = 1;
            break;
        }
        rec.yaw = e.w_yaw;
        rec.hscale = e.w_hscale;
        rec.vscale = e.w_vscale;
        rec.shift_rows = e.w_shift;
        rec.time_offset_ms = kLineMs * e.w_shift;
        rec.q = e.q;
        rec.count = e.count;
        if (round + 1 < st.rounds) {
            aptgpu_fit_round &n = rec.round[round + 1];
            n.c_yaw = e.w_yaw;
            n.c_hscale = e.w_hscale;
            n.c_vscale = e.w_vscale;
            n.c_shift = e.w_shift;
        } else {
            rec.done = 1;
        }
    }
    put_result(info, rec);
}

}  // namespace apt::fit
