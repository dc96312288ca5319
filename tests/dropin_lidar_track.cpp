// dropin_lidar_track.cpp -- test harness: the reference's lidar call site through include/tsdf.hpp, as tests/dropin_lidar_ground.cpp
// replays it, with the pose of a scan estimated by the object itself (TSDF::TrackScan) where the reference reads it from the
// trajectory of a stereo SLAM run (ref: examples/label_instance_lidar.cpp:36-40).
// Reads the grid, the camera and its depth limit, base2world, velo2cam, the ground's parameters, the depth frames that build the model, the scan and
// three guesses from argv[1].  Writes results.bin into the working directory: per call one int (TrackScan's answer) and the 16
// floats of cam2world_vec behind it,
//     call 1   TrackScan from the first guess (inside the basin)
//     call 2   TrackScan from the second guess (outside it: lost)
//     call 3   SetScanGround, TrackScan from the first guess
//     call 4   ClearScanGround, TrackScan from the first guess (== call 1)
//     call 5   TrackScan of no points at all (lost)
#include <cstdio>
#include <cstring>
#include <vector>

#include "tsdf.hpp"

namespace {
bool read_floats(FILE *fp, float *dst, size_t n) { return std::fread(dst, sizeof(float), n, fp) == n; }

bool write_call(FILE *out, bool ok, const std::vector<float> &pose)
{
    const int answer = ok ? 1 : 0;
    return pose.size() == 16 && std::fwrite(&answer, sizeof answer, 1, out) == 1 && std::fwrite(pose.data(), sizeof(float), 16, out) == 16;
}
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *fp = std::fopen(argv[1], "rb");
    if (!fp) return 2;
    int hdr[7];   // h, w, frames, dims, points
    float vs, max_depth, origin[3], K[9], base2world[16], velo2cam[16];
    tsdf_scan_ground_params ground;
    if (std::fread(hdr, sizeof(int), 7, fp) != 7 || !read_floats(fp, &vs, 1) || !read_floats(fp, &max_depth, 1) || !read_floats(fp, origin, 3) || !read_floats(fp, K, 9) ||
        !read_floats(fp, base2world, 16) || !read_floats(fp, velo2cam, 16) || std::fread(&ground, sizeof ground, 1, fp) != 1)
        return 2;
    const int h = hdr[0], w = hdr[1], n_frames = hdr[2], n_pts = hdr[6];
    const size_t px = (size_t)h * w;
    if (n_pts < 0) return 2;

    tsdf_config cfg;
    tsdf_config_default(&cfg, h, w);
    cfg.dim_x = hdr[3]; cfg.dim_y = hdr[4]; cfg.dim_z = hdr[5];
    cfg.z_begin = 0; cfg.z_end = hdr[5];
    cfg.voxel_size = vs;
    cfg.trunc_margin = vs * 5;
    cfg.max_depth = max_depth;
    std::memcpy(cfg.origin, origin, sizeof origin);
    std::memcpy(cfg.cam_K, K, sizeof K);
    std::memcpy(cfg.base2world, base2world, sizeof base2world);

    TSDF::ThrowOnError(false);
    TSDF tsdf(cfg);
    tsdf.SetSaveOnDestroy(false);
    for (int k = 0; k < n_frames; ++k) {
        std::vector<float> pose(16), depth(px);
        if (!read_floats(fp, pose.data(), 16) || !read_floats(fp, depth.data(), px)) return 2;
        tsdf.Integrate(depth.data(), pose);                     // ref: src/Object.cpp:160-164
    }
    std::vector<float> scan((size_t)n_pts * 4), inside(16), outside(16);
    if (!read_floats(fp, scan.data(), scan.size()) || !read_floats(fp, inside.data(), 16) || !read_floats(fp, outside.data(), 16)) return 2;
    std::fclose(fp);

    FILE *out = std::fopen("results.bin", "wb");
    if (!out) return 2;
    // the pose of the scan, then (not replayed here) tsdf->IntegrateScan(scan, velo2img, pose)      ref: examples/label_instance_lidar.cpp:76-77
    std::vector<float> pose = inside;
    bool ok = tsdf.TrackScan(scan.data(), (size_t)n_pts, velo2cam, pose);
    if (!write_call(out, ok, pose)) return 3;
    pose = outside;
    ok = tsdf.TrackScan(scan.data(), (size_t)n_pts, velo2cam, pose);
    if (!write_call(out, ok, pose)) return 3;
    tsdf.SetScanGround(ground);
    pose = inside;
    ok = tsdf.TrackScan(scan.data(), (size_t)n_pts, velo2cam, pose);
    if (!write_call(out, ok, pose)) return 3;
    tsdf.ClearScanGround();
    pose = inside;
    ok = tsdf.TrackScan(scan.data(), (size_t)n_pts, velo2cam, pose);
    if (!write_call(out, ok, pose)) return 3;
    pose = inside;
    ok = tsdf.TrackScan(NULL, 0, velo2cam, pose);
    if (!write_call(out, ok, pose)) return 3;
    std::fclose(out);
    std::printf("done\n");
    return 0;
}
