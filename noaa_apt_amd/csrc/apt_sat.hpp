// apt_sat.hpp — host side of the satellite track (apt_sat.cpp): TLE text -> elements -> sgp4init, the track of an
// image on the CPU and the pass direction of processing.rs:40-81.  The propagator itself is apt_sgp4.hpp, shared
// with the gfx950 kernel (apt_kernels_track.hpp).
#pragma once

#include <string>
#include <vector>

#include "apt_sgp4.hpp"

namespace apt::sat {

// One satellite of a TLE text as satellite::io::parse_multiple reads it: the trimmed title line and the fields SGP4
// uses, angles in rad, mean motion in rad / min (still Kozai's).
struct Elements {
    std::string name;
    double jdsatepoch, bstar, inclo, nodeo, ecco, argpo, mo, no_kozai;
};

// Every well-formed title / line 1 / line 2 group of the text, in order; malformed groups are skipped (the reference
// ignores parse_multiple's error list).  LF or CRLF line ends.
std::vector<Elements> parse_multiple(const std::string &tle);

// sgp4init, WGS-72, "improved" mode.  An orbit with a period of 225 minutes or more needs the deep-space branch:
// Error{Unsupported}.
Satrec sgp4init(const Elements &e);

// parse_multiple + find by name + sgp4init; keeps the last (text, name) pair's result.  A name that is not in the
// text: Error{Internal, `Satellite "NAME" not found in TLE`} (map.rs:37).
Satrec satrec_for(const std::string &tle, const std::string &name);

// "SGP4 error N: ..." for the error returns of apt_sgp4.hpp
std::string error_text(int32_t code);

// map.rs:41-58 on the CPU: out receives `height` (lat, lon) pairs in rad.  An SGP4 error in any row: Error{Internal}.
void track_host(const Satrec &s, bool ref_is_end, int64_t ref_ms, uint32_t height, double *out);

// processing.rs:40-81: two propagations, at the reference time as given (Start and End alike) and 2 s later, and
// geo::azimuth between the two sub-points.  True when the heading lies in the northward half, |azimuth| < pi/2 (the
// reference's own comparison is true for every heading of a retrograde orbit).
bool south_to_north_pass(const Satrec &s, int64_t ref_ms);

}  // namespace apt::sat
