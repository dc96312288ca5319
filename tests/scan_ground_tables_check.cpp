// scan_ground_tables_check.cpp -- the host's part of marking a scan's ground (semantic_slam_amd/csrc/scan_ground_tables.h) without
// a device: a stand-alone program (tests/test_scan_ground_spec.py builds it with -fsanitize=address,undefined and runs it).
// Every expectation below is stated from the rule, not computed with the function under test:
//   the limits admit exactly n_rings 2 ... 128, n_columns 4 ... 16384, finite values, ang_res_y > 0, ring borders inside (-90, 90)
//   degrees, tol_deg >= 0 with |mount_deg| + tol_deg < 90, min_range >= 0, ground_rings 0 ... n_rings - 1, mark_upper 0 or 1;
//   T has n_rings + 1 entries that never decrease, with the sign of their angle; C and S have n_columns entries on the unit
//   circle; tlo <= thi; each quadrant's borders are ONE run of columns (cyclically), the four runs follow one another, are not
//   empty and cover every column once; every border of a run lies in the run's quadrant; along a run C[c] y never increases and
//   S[c] x never decreases for points (x, y) of that quadrant, which is what lets the device bisect.
// Prints one line per failed expectation and exits with their number (0 = all good), then "checked N cases".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "scan_ground_tables.h"

using namespace tsdf_host;

static int failures = 0;
static long long cases = 0;
static const char *g_what = "";
static long long g_ctx[3];

static void expect(bool ok, const char *what)
{
    if (ok) return;
    if (++failures > 50) return;
    std::printf("FAILED %s (%s): %lld %lld %lld\n", what, g_what, g_ctx[0], g_ctx[1], g_ctx[2]);
}

static tsdf_scan_ground_params defaults()
{
    tsdf_scan_ground_params p;
    p.n_rings = 64; p.n_columns = 4500; p.ang_res_y = 26.9f / 63.0f; p.ang_bottom = 15.1f; p.mount_deg = 0.0f; p.tol_deg = 2.5f;
    p.min_range = 0.1f; p.ground_rings = 63; p.mark_upper = 0;
    return p;
}

// quadrant by the rule's four sign tests, written out once more
static int quadrant_by_rule(float a, float b)
{
    if (a > 0 && b >= 0) return 0;
    if (a <= 0 && b > 0) return 1;
    if (a < 0 && b <= 0) return 2;
    if (a >= 0 && b < 0) return 3;
    return -1;
}

static void check_tables(const tsdf_scan_ground_params &p)
{
    ++cases;
    g_ctx[0] = p.n_rings; g_ctx[1] = p.n_columns; g_ctx[2] = (long long)(p.ang_bottom * 1000);
    ScanGroundTables t;
    const GroundLimit l = build_scan_ground_tables(p, t);
    expect(l == GroundLimit::Ok, "a valid parameter set builds");
    if (l != GroundLimit::Ok) return;
    const int nr = p.n_rings, nc = p.n_columns;
    expect((int)t.T.size() == nr + 1 && (int)t.C.size() == nc && (int)t.S.size() == nc, "table sizes");
    for (int r = 0; r <= nr; ++r) {
        const double deg = (double)r * p.ang_res_y - p.ang_bottom;
        expect(std::isfinite(t.T[r]), "T is finite");
        if (r > 0) expect(t.T[r] >= t.T[r - 1], "T never decreases");
        if (std::fabs(deg) > 1e-3) expect((t.T[r] > 0) == (deg > 0), "T has its angle's sign");
    }
    expect(t.tlo <= t.thi && std::isfinite(t.tlo) && std::isfinite(t.thi), "tlo <= thi, finite");
    // the runs: walk the columns once round from first[0]; the quadrant may only step to the next one, four times in all
    std::vector<int> seen((size_t)nc, 0);
    int total = 0;
    for (int q = 0; q < 4; ++q) {
        expect(t.len[q] >= 1 && t.first[q] >= 0 && t.first[q] < nc, "a run is not empty and starts at a column");
        total += t.len[q];
        if (q > 0) expect(t.first[q] == (t.first[q - 1] + t.len[q - 1]) % nc, "the runs follow one another");
        for (int k = 0; k < t.len[q] && k < nc; ++k) {
            const int c = (t.first[q] + k) % nc;
            ++seen[(size_t)c];
            expect(quadrant_by_rule(t.C[c], t.S[c]) == q, "a border of a run lies in the run's quadrant");
            expect(std::fabs((double)t.C[c] * t.C[c] + (double)t.S[c] * t.S[c] - 1.0) < 1e-6, "C, S on the unit circle");
            if (k > 0) {
                const int b = (t.first[q] + k - 1) % nc;
                // a point of quadrant q with the signs of (C, S) at the run's middle: both products monotone along the run
                const float xs[4] = {1.5f, -0.25f, -3.0f, 2.0f}, ys[4] = {0.75f, 2.0f, -1.0f, -0.5f};
                expect(quadrant_by_rule(xs[q], ys[q]) == q, "the probe lies in the quadrant");
                expect(t.C[c] * ys[q] <= t.C[b] * ys[q], "C[c] y never increases along the run");
                expect(t.S[c] * xs[q] >= t.S[b] * xs[q], "S[c] x never decreases along the run");
            }
        }
    }
    expect(total == nc, "the runs cover n_columns borders");
    for (int c = 0; c < nc; ++c) expect(seen[(size_t)c] == 1, "every border in exactly one run");
    expect((t.first[0] + t.len[0] + t.len[1] + t.len[2] + t.len[3]) % nc == t.first[0], "the runs close the circle");
}

static void check_limit(tsdf_scan_ground_params p, GroundLimit want, const char *what)
{
    ++cases;
    g_what = what;
    g_ctx[0] = p.n_rings; g_ctx[1] = p.n_columns; g_ctx[2] = p.ground_rings;
    expect(scan_ground_limits_ok(p) == want, "the limit that is reported");
    ScanGroundTables t;
    expect(build_scan_ground_tables(p, t) == want, "the builder reports it too");
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- limits: each on both sides ----
    tsdf_scan_ground_params p = defaults();
    check_limit(p, GroundLimit::Ok, "the defaults");
    p = defaults(); p.n_rings = 1; check_limit(p, GroundLimit::Rings, "n_rings 1");
    p = defaults(); p.n_rings = 2; p.ground_rings = 1; check_limit(p, GroundLimit::Ok, "n_rings 2");
    p = defaults(); p.n_rings = 128; p.ang_res_y = 0.5f; check_limit(p, GroundLimit::Ok, "n_rings 128");
    p = defaults(); p.n_rings = 129; p.ang_res_y = 0.5f; check_limit(p, GroundLimit::Rings, "n_rings 129");
    p = defaults(); p.n_rings = -5; check_limit(p, GroundLimit::Rings, "n_rings -5");
    p = defaults(); p.n_columns = 3; check_limit(p, GroundLimit::Columns, "n_columns 3");
    p = defaults(); p.n_columns = 4; check_limit(p, GroundLimit::Ok, "n_columns 4");
    p = defaults(); p.n_columns = 16384; check_limit(p, GroundLimit::Ok, "n_columns 16384");
    p = defaults(); p.n_columns = 16385; check_limit(p, GroundLimit::Columns, "n_columns 16385");
    const float bad_values[3] = {inf, -inf, nan};
    for (float v : bad_values) {
        p = defaults(); p.ang_res_y = v; check_limit(p, GroundLimit::NotFinite, "ang_res_y not finite");
        p = defaults(); p.ang_bottom = v; check_limit(p, GroundLimit::NotFinite, "ang_bottom not finite");
        p = defaults(); p.mount_deg = v; check_limit(p, GroundLimit::NotFinite, "mount_deg not finite");
        p = defaults(); p.tol_deg = v; check_limit(p, GroundLimit::NotFinite, "tol_deg not finite");
        p = defaults(); p.min_range = v; check_limit(p, GroundLimit::NotFinite, "min_range not finite");
    }
    p = defaults(); p.ang_res_y = 0.0f; check_limit(p, GroundLimit::AngRes, "ang_res_y 0");
    p = defaults(); p.ang_res_y = -0.4f; check_limit(p, GroundLimit::AngRes, "ang_res_y < 0");
    p = defaults(); p.ang_bottom = 90.0f; check_limit(p, GroundLimit::RingBoundary, "lowest border at -90");
    p = defaults(); p.ang_bottom = 89.5f; check_limit(p, GroundLimit::Ok, "lowest border at -89.5");
    p = defaults(); p.n_rings = 64; p.ang_res_y = 1.0f; p.ang_bottom = -26.0f; check_limit(p, GroundLimit::RingBoundary, "highest border at 90");
    p = defaults(); p.n_rings = 64; p.ang_res_y = 1.0f; p.ang_bottom = -25.5f; check_limit(p, GroundLimit::Ok, "highest border at 89.5");
    p = defaults(); p.tol_deg = -0.01f; check_limit(p, GroundLimit::Tolerance, "tol_deg < 0");
    p = defaults(); p.tol_deg = 0.0f; check_limit(p, GroundLimit::Ok, "tol_deg 0");
    p = defaults(); p.mount_deg = 45.0f; p.tol_deg = 45.0f; check_limit(p, GroundLimit::Tolerance, "mount + tol at 90");
    p = defaults(); p.mount_deg = -45.0f; p.tol_deg = 45.0f; check_limit(p, GroundLimit::Tolerance, "-mount + tol at 90");
    p = defaults(); p.mount_deg = -45.0f; p.tol_deg = 44.5f; check_limit(p, GroundLimit::Ok, "-mount + tol at 89.5");
    p = defaults(); p.min_range = -0.001f; check_limit(p, GroundLimit::MinRange, "min_range < 0");
    p = defaults(); p.min_range = 0.0f; check_limit(p, GroundLimit::Ok, "min_range 0");
    p = defaults(); p.ground_rings = -1; check_limit(p, GroundLimit::GroundRings, "ground_rings -1");
    p = defaults(); p.ground_rings = 0; check_limit(p, GroundLimit::Ok, "ground_rings 0");
    p = defaults(); p.ground_rings = 64; check_limit(p, GroundLimit::GroundRings, "ground_rings n_rings");
    p = defaults(); p.mark_upper = 2; check_limit(p, GroundLimit::MarkUpper, "mark_upper 2");
    p = defaults(); p.mark_upper = -1; check_limit(p, GroundLimit::MarkUpper, "mark_upper -1");
    p = defaults(); p.mark_upper = 1; check_limit(p, GroundLimit::Ok, "mark_upper 1");

    // ---- tables: every column count up to 600, then sizes around powers of two and the largest; ring counts at their ends ----
    g_what = "column sweep";
    for (int nc = 4; nc <= 600; ++nc) {
        p = defaults(); p.n_columns = nc;
        check_tables(p);
    }
    const int big[] = {1023, 1024, 1025, 1800, 2047, 2048, 4095, 4096, 4097, 4500, 8191, 8192, 16383, 16384};
    for (int nc : big) {
        p = defaults(); p.n_columns = nc;
        check_tables(p);
    }
    g_what = "ring sweep";
    for (int nr = 2; nr <= 128; ++nr) {
        p = defaults(); p.n_rings = nr; p.ground_rings = nr - 1; p.n_columns = 36; p.ang_res_y = 170.0f / (float)nr; p.ang_bottom = 85.0f;
        check_tables(p);
        p.ang_res_y = 0.01f; p.ang_bottom = 0.005f * (float)nr;                   // borders around 0: T changes sign
        check_tables(p);
        p.ang_res_y = 1e-12f; p.ang_bottom = 30.0f;                               // rings too thin for float: T must still not decrease
        check_tables(p);
    }
    g_what = "slopes";
    for (float mount = -80.0f; mount <= 80.0f; mount += 10.0f)
        for (float tol = 0.0f; std::fabs(mount) + tol < 89.9f; tol += 2.25f) {
            p = defaults(); p.mount_deg = mount; p.tol_deg = tol; p.n_columns = 8;
            check_tables(p);
        }
    std::printf("checked %lld cases\n", cases);
    return failures;
}
