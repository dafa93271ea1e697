// apt_map.cpp — host side of the map overlay (apt_map.hpp): the ESRI shapefile reader, the layer set and the
// per-call scalars of map.rs:59-69 with the C library's f64 libm (what Rust's f64::sin & co. call on Linux).
#include "apt_map.hpp"

#include <atomic>
#include <cmath>
#include <cstring>
#include <fstream>
#include <iterator>

#include "apt_host.hpp"

namespace apt::map {

namespace {

int32_t be32(const uint8_t *p)
{
    return static_cast<int32_t>((uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3]);
}

int32_t le32(const uint8_t *p)
{
    return static_cast<int32_t>(uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24));
}

double le64f(const uint8_t *p)
{
    uint64_t u = 0;
    for (int i = 7; i >= 0; --i) u = (u << 8) | p[i];
    double d;
    std::memcpy(&d, &u, sizeof d);
    return d;
}

[[noreturn]] void fail(ErrorKind kind, const std::string &msg)
{
    throw Error{kind, "shapefile: " + msg};
}

const char *type_name(int32_t t)
{
    return t == kShpPolyline ? "Polyline" : t == kShpPolygon ? "Polygon" : "other";
}

// Rust's `{:?}` of a path string
std::string debug_str(const std::string &s)
{
    std::string out = "\"";
    for (char ch : s) {
        if (ch == '"' || ch == '\\') out += '\\', out += ch;
        else if (ch == '\n') out += "\\n";
        else if (ch == '\r') out += "\\r";
        else if (ch == '\t') out += "\\t";
        else out += ch;
    }
    return out + "\"";
}

std::atomic<uint64_t> g_gen{0};

}  // namespace

Layer read_shp_bytes(const uint8_t *d, size_t size, int32_t want)
{
    if (want != kShpPolyline && want != kShpPolygon) fail(ErrorKind::Unsupported, "only Polyline and Polygon layers");
    if (size < 100) fail(ErrorKind::Internal, "file shorter than its 100-byte header");
    if (be32(d) != 9994) fail(ErrorKind::Internal, "not a shapefile (file code != 9994)");
    const int32_t header_type = le32(d + 32);
    if (header_type != kShpPolyline && header_type != kShpPolygon)
        fail(ErrorKind::Unsupported, "shape type " + std::to_string(header_type) + " is not supported");
    // the file length field (16-bit words) bounds the records; a longer buffer is ignored beyond it
    const uint64_t file_len = static_cast<uint64_t>(static_cast<uint32_t>(be32(d + 24))) * 2u;
    const uint64_t end = file_len < size ? file_len : size;
    Layer out;
    uint64_t pos = 100;
    while (pos + 8 <= end) {
        const uint64_t len = static_cast<uint64_t>(static_cast<uint32_t>(be32(d + pos + 4))) * 2u;
        const uint64_t body = pos + 8;
        if (len < 4 || body + len > end) fail(ErrorKind::Internal, "truncated record");
        const int32_t type = le32(d + body);
        if (type != want)
            fail(ErrorKind::Internal, std::string("record of type ") + std::to_string(type) + ", expected " +
                                          type_name(want) + " (" + std::to_string(want) + ")");
        if (len < 44) fail(ErrorKind::Internal, "truncated record");
        const int32_t n_parts = le32(d + body + 36), n_points = le32(d + body + 40);
        if (n_parts < 0 || n_points < 0 ||
            44 + 4 * static_cast<uint64_t>(n_parts) + 16 * static_cast<uint64_t>(n_points) > len)
            fail(ErrorKind::Internal, "truncated record");
        const uint8_t *parts = d + body + 44;
        const uint8_t *pts = parts + 4 * static_cast<size_t>(n_parts);
        for (int32_t k = 0; k < n_parts; ++k) {
            const int32_t a = le32(parts + 4 * k);
            const int32_t b = k + 1 < n_parts ? le32(parts + 4 * (k + 1)) : n_points;
            if (a < 0 || b > n_points || a > b) fail(ErrorKind::Internal, "part offsets out of order");
            if (a == b) fail(ErrorKind::Invalid, "empty part (the reference indexes points[0] of every part)");
            for (int32_t j = a; j < b; ++j) {
                out.xy.push_back(le64f(pts + 16 * static_cast<size_t>(j)));
                out.xy.push_back(le64f(pts + 16 * static_cast<size_t>(j) + 8));
            }
            out.parts.push_back(static_cast<uint32_t>(out.points()));
        }
        pos = body + len;
    }
    return out;
}

Layer read_shp(const std::string &path, int32_t want)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw Error{ErrorKind::Internal, "Could not load " + debug_str(path)};  // map.rs:136-137
    std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    return read_shp_bytes(bytes.data(), bytes.size(), want);
}

void Layers::set(int which, Layer l)
{
    if (l.parts.empty() || l.parts.front() != 0 || l.parts.back() != l.points())
        throw Error{ErrorKind::Invalid, "layer: part offsets must start at 0 and end at the point count"};
    for (size_t k = 0; k + 1 < l.parts.size(); ++k)
        if (l.parts[k + 1] <= l.parts[k]) throw Error{ErrorKind::Invalid, "layer: empty or unordered part"};
    layer[which] = std::move(l);
    present[which] = true;
    flatten();
}

void Layers::clear(int which)
{
    layer[which] = Layer{};
    present[which] = false;
    flatten();
}

void Layers::flatten()
{
    size_t n = 0;
    for (int k = 0; k < 3; ++k)
        if (present[k]) n += layer[k].points();
    if (n >= (1u << 31)) throw Error{ErrorKind::Invalid, "layer set: too many points"};
    xy.clear();
    meta.clear();
    xy.reserve(2 * n);
    meta.reserve(2 * n);
    for (int k = 0; k < 3; ++k) {
        if (!present[k]) continue;
        const Layer &l = layer[k];
        const int32_t base = static_cast<int32_t>(xy.size() / 2);
        xy.insert(xy.end(), l.xy.begin(), l.xy.end());
        for (size_t p = 0; p + 1 < l.parts.size(); ++p)
            for (uint32_t j = l.parts[p]; j < l.parts[p + 1]; ++j) {
                meta.push_back(base + static_cast<int32_t>(j == l.parts[p] ? j : j - 1));
                meta.push_back(k);
            }
    }
    gen = ++g_gen;
}

// geo.rs:34-46
double geo_distance(double lat1, double lon1, double lat2, double lon2)
{
    const double delta_lon = lon2 - lon1;
    double c = std::sin(lat1) * std::sin(lat2) + std::cos(lat1) * std::cos(lat2) * std::cos(delta_lon);
    c = std::fmin(std::fmax(c, -1.), 1.);
    return std::acos(c);
}

// geo.rs:54-62
double geo_azimuth(double lat1, double lon1, double lat2, double lon2)
{
    const double delta_lon = lon2 - lon1;
    return std::atan2(std::sin(delta_lon), std::cos(lat1) * std::tan(lat2) - std::sin(lat1) * std::cos(delta_lon));
}

Scalars scalars(const double *pos, size_t count, double yaw, double hscale, double vscale)
{
    Scalars s{};
    s.yaw = yaw;
    s.x_res = 0.0005 / hscale;
    if (count == 0) return s;
    const double lat0 = pos[0], lon0 = pos[1], lat1 = pos[2 * (count - 1)], lon1 = pos[2 * (count - 1) + 1];
    s.start_lat = lat0;
    s.start_lon = lon0;
    s.y_res = geo_distance(lat0, lon0, lat1, lon1) / static_cast<double>(count) / vscale;
    s.ref_az = geo_azimuth(lat0, lon0, lat1, lon1);
    return s;
}

}  // namespace apt::map
