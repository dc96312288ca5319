// scan_ground_tables.h -- the host's part of marking a scan's ground: the parameters' limits and the tables
// the kernels of tsdf_scan_ground.hip.h search.  Plain C++ (no HIP, no device types), like launch_geometry.h, so that
// tests/scan_ground_tables_check.cpp can sweep it on the CPU under -fsanitize=address,undefined.
//
// The device uses no transcendental function: every angle of the rule becomes a table entry, computed here ONCE per parameter
// set in double and rounded to float.
//     T[r] = tan((r * ang_res_y - ang_bottom) deg),  r = 0 ... n_rings              the ring boundaries' slopes
//     C[c], S[c] = cos, sin(beta_c),  beta_c = (c - n_columns / 2 - 0.5) * 360 / n_columns deg   (integer n_columns / 2)
//     tlo, thi = tan((mount_deg -+ tol_deg) deg)                                      the level step's slopes
// A direction (a, b) -- a point's (x, y), a boundary's (C[c], S[c]) -- lies in quadrant
//     0: a > 0 && b >= 0     1: a <= 0 && b > 0     2: a < 0 && b <= 0     3: a >= 0 && b < 0        (x forward, y left)
// by the signs of the FLOATS, the same test on both sides.  The boundaries of one quadrant are a contiguous run
// first[q] ... first[q] + len[q] - 1 of columns, taken cyclically mod n_columns (beta_0 is just below -180 degrees, so one
// run wraps), in angular order.  Along a run C and S are each monotone (which way depends on the quadrant), rounding keeps
// that, and so for a point of the same quadrant C[c] * y never increases and S[c] * x never decreases along the run: the test
// C[c] * y >= S[c] * x ("the point is at or past boundary c") is true up to some column of the run and false behind it.
// Likewise T never decreases and h >= 0, so z >= T[r] * h is true up to some ring and false behind it.  Both counts of the rule
// are therefore found by bisection on the device and by a linear count in the restatement, with the same result;
// build_scan_ground_tables CHECKS that T never decreases, that every quadrant's run is contiguous and not empty, that the
// runs cover every column once and that C and S are monotone along each, and refuses a parameter set where one fails.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "tsdf_hip.h"

namespace tsdf_host {

constexpr int kGroundMinRings = 2, kGroundMaxRings = 128, kGroundMinColumns = 4, kGroundMaxColumns = 16384;

enum class GroundLimit { Ok, Rings, Columns, NotFinite, AngRes, RingBoundary, Tolerance, MinRange, GroundRings, MarkUpper, Tables };

inline const char *ground_limit_text(GroundLimit l)
{
    switch (l) {
    case GroundLimit::Ok: return "ok";
    case GroundLimit::Rings: return "n_rings must lie in [2, 128]";
    case GroundLimit::Columns: return "n_columns must lie in [4, 16384]";
    case GroundLimit::NotFinite: return "every value must be finite";
    case GroundLimit::AngRes: return "ang_res_y must be > 0";
    case GroundLimit::RingBoundary: return "every ring boundary r * ang_res_y - ang_bottom must lie inside (-90, 90) degrees";
    case GroundLimit::Tolerance: return "tol_deg must be >= 0 and |mount_deg| + tol_deg < 90";
    case GroundLimit::MinRange: return "min_range must be >= 0";
    case GroundLimit::GroundRings: return "ground_rings must lie in [0, n_rings - 1]";
    case GroundLimit::MarkUpper: return "mark_upper must be 0 or 1";
    case GroundLimit::Tables: return "the tables of these angles are not monotone";
    }
    return "?";
}

inline GroundLimit scan_ground_limits_ok(const tsdf_scan_ground_params &p)
{
    if (p.n_rings < kGroundMinRings || p.n_rings > kGroundMaxRings) return GroundLimit::Rings;
    if (p.n_columns < kGroundMinColumns || p.n_columns > kGroundMaxColumns) return GroundLimit::Columns;
    if (!std::isfinite(p.ang_res_y) || !std::isfinite(p.ang_bottom) || !std::isfinite(p.mount_deg) || !std::isfinite(p.tol_deg) ||
        !std::isfinite(p.min_range))
        return GroundLimit::NotFinite;
    if (!(p.ang_res_y > 0.0f)) return GroundLimit::AngRes;
    const double lowest = -(double)p.ang_bottom, highest = (double)p.n_rings * (double)p.ang_res_y - (double)p.ang_bottom;
    if (!(lowest > -90.0 && highest < 90.0)) return GroundLimit::RingBoundary;
    if (!(p.tol_deg >= 0.0f) || !(std::fabs((double)p.mount_deg) + (double)p.tol_deg < 90.0)) return GroundLimit::Tolerance;
    if (!(p.min_range >= 0.0f)) return GroundLimit::MinRange;
    if (p.ground_rings < 0 || p.ground_rings > p.n_rings - 1) return GroundLimit::GroundRings;
    if (p.mark_upper != 0 && p.mark_upper != 1) return GroundLimit::MarkUpper;
    return GroundLimit::Ok;
}

inline int ground_quadrant(float a, float b)
{
    if (a > 0.0f && b >= 0.0f) return 0;
    if (a <= 0.0f && b > 0.0f) return 1;
    if (a < 0.0f && b <= 0.0f) return 2;
    if (a >= 0.0f && b < 0.0f) return 3;
    return -1;      // (0, 0) or a NaN: no direction
}

struct ScanGroundTables {
    std::vector<float> T;          // n_rings + 1
    std::vector<float> C, S;       // n_columns each
    float tlo = 0.0f, thi = 0.0f;
    int32_t first[4] = {0, 0, 0, 0}, len[4] = {0, 0, 0, 0};
};

inline GroundLimit build_scan_ground_tables(const tsdf_scan_ground_params &p, ScanGroundTables &t)
{
    const GroundLimit l = scan_ground_limits_ok(p);
    if (l != GroundLimit::Ok) return l;
    const double rad = 3.14159265358979323846 / 180.0;
    const int nr = p.n_rings, nc = p.n_columns;
    t.T.assign((size_t)nr + 1, 0.0f);
    t.C.assign((size_t)nc, 0.0f);
    t.S.assign((size_t)nc, 0.0f);
    for (int r = 0; r <= nr; ++r) t.T[(size_t)r] = (float)std::tan(((double)r * (double)p.ang_res_y - (double)p.ang_bottom) * rad);
    for (int c = 0; c < nc; ++c) {
        const double beta = ((double)(c - nc / 2) - 0.5) * 360.0 / (double)nc * rad;
        t.C[(size_t)c] = (float)std::cos(beta);
        t.S[(size_t)c] = (float)std::sin(beta);
    }
    t.tlo = (float)std::tan(((double)p.mount_deg - (double)p.tol_deg) * rad);
    t.thi = (float)std::tan(((double)p.mount_deg + (double)p.tol_deg) * rad);
    if (!std::isfinite(t.tlo) || !std::isfinite(t.thi) || !(t.tlo <= t.thi)) return GroundLimit::Tables;
    for (int r = 0; r <= nr; ++r)
        if (!std::isfinite(t.T[(size_t)r]) || (r > 0 && !(t.T[(size_t)r] >= t.T[(size_t)r - 1]))) return GroundLimit::Tables;
    // the quadrants' runs: a run begins at the column whose predecessor (cyclically) lies in another quadrant
    int starts = 0;
    for (int q = 0; q < 4; ++q) t.first[q] = t.len[q] = 0;
    for (int c = 0; c < nc; ++c) {
        const int q = ground_quadrant(t.C[(size_t)c], t.S[(size_t)c]);
        const int prev = (c + nc - 1) % nc, qp = ground_quadrant(t.C[(size_t)prev], t.S[(size_t)prev]);
        if (q < 0) return GroundLimit::Tables;
        ++t.len[q];
        if (q != qp) {
            if (qp != (q + 3) % 4) return GroundLimit::Tables;      // the quadrants follow one another in angular order
            t.first[q] = c;
            ++starts;
        }
    }
    if (starts != 4) return GroundLimit::Tables;                   // each quadrant begins once: its columns are one run
    for (int q = 0; q < 4; ++q) {
        if (t.len[q] < 1) return GroundLimit::Tables;
        // along the run: quadrant 0: C falls, S rises; 1: C falls, S falls; 2: C rises, S falls; 3: C rises, S rises
        const bool c_rises = q >= 2, s_rises = q == 0 || q == 3;
        for (int k = 1; k < t.len[q]; ++k) {
            const size_t a = (size_t)((t.first[q] + k - 1) % nc), b = (size_t)((t.first[q] + k) % nc);
            if (ground_quadrant(t.C[b], t.S[b]) != q) return GroundLimit::Tables;
            if (c_rises ? t.C[b] < t.C[a] : t.C[b] > t.C[a]) return GroundLimit::Tables;
            if (s_rises ? t.S[b] < t.S[a] : t.S[b] > t.S[a]) return GroundLimit::Tables;
        }
    }
    return GroundLimit::Ok;
}

}  // namespace tsdf_host
