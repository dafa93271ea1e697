// apt_image_request.hpp — one checked image call (ImageRequest), where a recording's stages run (ImageJob), and the
// one sequence of launches both the one-shot entry points and the plan go through (apt_plan.hip).
#pragma once

#include <vector>

#include "apt_kernels_color.hpp"
#include "apt_kernels_composite.hpp"
#include "apt_kernels_despeckle.hpp"
#include "apt_kernels_geoloc.hpp"
#include "apt_kernels_map.hpp"
#include "apt_kernels_project.hpp"
#include "apt_kernels_thermal.hpp"
#include "apt_kernels_track.hpp"

struct aptgpu_plan;

namespace apt {

// What the aptgpu_process_image* / aptgpu_plan_process_device_image* entry points ask for, after their argument
// checks.  Which stages run follows from the flags here and nowhere else.  The entry points fill it in their own
// check order: color_args writes the per-call block down to `palette` and nothing else; everything per recording is
// written after `rec` has its final size.
struct ImageRequest {
    int contrast = APTGPU_CONTRAST_MINMAX;
    float percent = 0.f;
    int channels = 1;
    bool colored = false, lab = false;  // false colour; Histogram with it (equalised in CIE Lab)
    apt::gpu::ColorTune tune{};
    const uint8_t *palette = nullptr;
    // The overlay is drawn: with a projection a layer set is given (its settings are the projection's), without one
    // the map settings are (draw_map in the orbit forms).  `layers` is then the set.
    bool overlay = false;
    const apt::map::Layers *layers = nullptr;
    bool project = false;  // the image goes through the reprojection onto every recording's grid
    bool png = false;      // the output is the PNG file of the image (of the grid with a projection)
    // The recordings are the passes of one composite: each one's track stage runs, then one launch
    // combines them onto rec[0]'s grid (with its graticule) into `comp`'s destinations.  Excludes `project`.
    bool composite = false;
    struct Composite {
        int blend = APTGPU_COMPOSITE_NADIR;
        apt::composite::Device *dev = nullptr;  // the plan's, or the one-shot call's
        uint8_t *d_out = nullptr, *d_coverage = nullptr, *d_png = nullptr;  // (coverage nullable; d_png with `png`)
        size_t out_cap = 0, png_cap = 0;
    } comp;
    enum class Track { None, Positions, Sat };
    struct Recording {
        bool rotate = false;  // (Rotate::Orbit resolved)
        Track track = Track::None;
        const double *positions = nullptr;  // Track::Positions: n_positions (lat, lon) pairs on the host
        size_t n_positions = 0;
        apt::sat::TrackCall sat{};          // Track::Sat: the track is computed on the device
        aptgpu_map_settings geom{sizeof(aptgpu_map_settings), 0, 0., 1., 1.};  // yaw / hscale / vscale
        int channels = 0;                   // with `composite`: this pass's source, 1 or 4 (the passes may differ)
        apt::project::Grid grid{};          // with `project`, and its graticule
        std::vector<uint8_t> flags;
        uint64_t grid_bytes() const { return static_cast<uint64_t>(grid.width) * grid.height * 4u; }
        // the destinations in HBM: the caller's for a plan, call-local buffers for a one-shot call
        uint8_t *d_image = nullptr, *d_png = nullptr, *d_out = nullptr;
        size_t png_cap = 0, out_cap = 0;
    };
    std::vector<Recording> rec;
    explicit ImageRequest(size_t recordings = 0) : rec(recordings) {}
};

// Where one recording's stages run: a plan slot, or the buffers of a one-shot call.  The launches read
// (res, n, cap) as given: (null, n, n) for a one-shot call, (the decode's record, 0, capacity) for a plan.
struct ImageJob {
    hipStream_t stream;
    const float *rows;
    const apt::gpu::Result *res;
    uint64_t n, cap;
    void *ws;                     // image_ws_bytes scratch
    apt::gpu::ImageResult *info;  // the record
    void *color_ws, *lab_ws, *eqfloat_ws, *png_ws;  // (each null unless the request runs its stage)
    apt::map::Device *map;
    apt::project::Device *project;
    uint64_t stream_cap;          // the filtered stream png_ws is sized for
};

// The launches, in `plan` (null: a one-shot call).  A plan brackets every launch with its timer under the launch's
// name and checks each stage's launches under a label of their own; a one-shot call does neither and checks once
// behind everything.
// The contrast limits of one job (noaa_apt.rs:141-175): the first kernel of every variant, which resets the record.
void enqueue_image_limits(aptgpu_plan *plan, const ImageJob &j, int contrast, float percent);
// The row stages in front of the image stage, one job each.  Of the job they read (stream, rows, res, n, cap, ws) and
// `info` where it is said; the stage's own scratch and outputs travel as arguments.
// Despeckle (apt_kernels_despeckle.hpp): with a threshold the 98 % limits of the rows into j.ws, their record into
// j.info, then one k_despeckle launch into d_out with its record in *rec.  (A one-shot call of less than a row has no
// limits to take: its launch is left out.)
void enqueue_despeckle(aptgpu_plan *plan, const ImageJob &j, int radius, float threshold, float *d_out,
                       apt::gpu::DespeckleResult *rec);
// Thermal calibration (apt_kernels_thermal.hpp): the telemetry launches into j.ws with their record in thermal_ws, then
// k_thermal_space, k_thermal_setup and k_thermal_map.  l.x is the job's rows; l.res, n and cap are filled in here.
void enqueue_thermal(aptgpu_plan *plan, const ImageJob &j, apt::gpu::ThermalLaunch l, const apt::gpu::ThermalCoeffs &coeffs,
                     const apt::gpu::ThermalTable &table, void *thermal_ws);
// Geolocation (apt_kernels_geoloc.hpp): the track's launches into dev, prepared here for cap / 2080 rows, then
// k_geoloc_rows and k_geoloc.  l.x is the job's rows; l.res, n and cap are filled in here.
void enqueue_geoloc(aptgpu_plan *plan, const ImageJob &j, apt::gpu::GeolocLaunch l, apt::map::Device &dev, void *geoloc_ws);
// Equalisation and colour of one job, behind its limits.
void enqueue_image_color(aptgpu_plan *plan, const ImageRequest &q, const ImageRequest::Recording &r, const ImageJob &j);
// What follows the colour, stage by stage and job by job within a stage: the overlay, then the reprojection (behind
// its track when no overlay left one) or the PNG; or, for a composite, every pass's track and then the one launch of
// all of them on the first job's stream, behind one event per pass that ran elsewhere.
void enqueue_image_outputs(aptgpu_plan *plan, const ImageRequest &q, const ImageJob *jobs, int count);

}  // namespace apt
