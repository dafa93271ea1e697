// apt_map.hpp — the map overlay of noaa_apt::process (map.rs:14-200): the ESRI shapefile reader and the layer set
// (apt_map.cpp, host).  The gfx950 kernels that project, rasterise and blend it: apt_kernels_map.hpp.
//
// SGP4 stays with the caller: it passes one (lat, lon) per image row, in radians (map.rs:41-58).  Everything after
// that vector runs here: the per-call scalars on the host with the C library's f64 libm (map.rs:59-69), the
// projection, x-offset correction, culling, Xiaolin Wu walk and the ordered src-over blend on the device.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>


namespace apt::map {

constexpr int32_t kShpPolyline = 3;
constexpr int32_t kShpPolygon = 5;

// One layer as the reader returns it: (x = lon°, y = lat°) pairs in file order, part k = points
// [parts[k], parts[k + 1]) (parts holds n_parts + 1 entries, parts[0] = 0).
struct Layer {
    std::vector<double> xy;
    std::vector<uint32_t> parts{0};
    size_t points() const { return xy.size() / 2; }
};

// shapefile::ShapeReader::from_path(path) + iter_shapes_as::<Polyline or Polygon>() of the records' parts.
// shape_type: kShpPolyline or kShpPolygon.  Errors: a file that cannot be opened is Internal("Could not load
// {:?}") as map.rs:136-137; a record of another type than shape_type is Internal (iter_shapes_as); a header
// type other than 3 or 5 is Unsupported; an empty part (the reference panics on points[0]) is Invalid.
Layer read_shp(const std::string &path, int32_t shape_type);
Layer read_shp_bytes(const uint8_t *data, size_t size, int32_t shape_type);

// The three layers in the reference's draw order (map.rs:133-198) with their RGBA colours (packed R | G<<8 |
// B<<16 | A<<24).  The flattened form is what the device reads: per vertex its (lon°, lat°), the index of the
// other end of its segment (itself for the first point of a part: draw_line(p0, p0)) and its layer.
struct Layers {
    enum { kStates = 0, kCountries = 1, kLakes = 2 };
    Layer layer[3];
    bool present[3] = {false, false, false};
    uint32_t color[3] = {0x96'00'ff'ffu, 0xff'00'ff'ffu, 0xff'c8'c8'32u};  // default_settings.toml:72-74
    uint64_t gen = 0;  // changes whenever a layer's points change (process-wide unique)
    std::vector<double> xy;       // flattened, all present layers
    std::vector<int32_t> meta;    // per vertex: prev index, layer
    void set(int which, Layer l);
    void clear(int which);
    void flatten();
};

// The per-call scalars of map.rs:59-69 (host libm).
struct Scalars {
    double start_lat, start_lon;  // sat_positions[0]
    double ref_az;                // geo::azimuth(start, end)
    double y_res, x_res, yaw;
};
double geo_distance(double lat1, double lon1, double lat2, double lon2);
double geo_azimuth(double lat1, double lon1, double lat2, double lon2);
Scalars scalars(const double *positions, size_t count, double yaw, double hscale, double vscale);

// Bounds of the device path.  A segment whose Xiaolin Wu walk runs more than kMaxWalk steps along its major axis, or
// has a non-finite end (the reference spends billions of iterations there, or panics in NumCast), and a call with
// more than kMaxFragments fragments, or a pixel that more than kMaxPixelFragments of them land on, are reported in
// the image record (status 1, reasons below), never truncated.
constexpr uint32_t kMaxWalk = 1u << 20;
constexpr uint32_t kMaxFragments = 1u << 21;
constexpr uint32_t kMaxPixelFragments = 1u << 16;
enum Reason : int32_t { kReasonOverflow = 5, kReasonWalk = 6, kReasonCount = 7, kReasonPixel = 8 };

struct Colors {
    uint32_t c[3];
};

}  // namespace apt::map
