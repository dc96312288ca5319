// dropin_lidar_ground.cpp -- test harness: the reference's lidar call sequence through include/tsdf.hpp, as tests/dropin_lidar.cpp
// replays it, with the scan's ground marked on the device and kept out of the volume (TSDF::SetScanGround) and the gaps between
// beams filled (TSDF::SetScanFill).  The reference has both steps in front of its object loop, dormant and on the CPU:
// projectPointCloud() and groundRemoval() (ref: examples/label_instance_lidar.cpp:85-91, src/Utility.cpp:452-553).
// Reads the grid, the camera, velo2img, the ground's and the fill's parameters and the frames from argv[1]; argv[2] = "slabs"
// cuts the grid into two z-slabs on one device.  Writes into the working directory
//     tsdf1.{ply,bin}   SetScanGround(DROP_GROUND), SetScanFill, IntegrateScan
//     tsdf2.{ply,bin}   Integrate of the restated image of those calls, read from the file
//     tsdf3.{ply,bin}   SetScanGround(DROP_GROUND) alone, IntegrateScan
//     tsdf4.{ply,bin}   SetScanGround(ONLY_GROUND), SetScanFill, IntegrateScan
//     tsdf5.{ply,bin}   SetScanGround, then ClearScanGround; SetScanFill, IntegrateScan
//     tsdf6.{ply,bin}   SetScanFill, IntegrateScan by an object that never set the ground
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tsdf.hpp"

namespace {
bool read_floats(FILE *fp, float *dst, size_t n) { return std::fread(dst, sizeof(float), n, fp) == n; }
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const bool slabs = argc > 2 && std::string(argv[2]) == "slabs";
    FILE *fp = std::fopen(argv[1], "rb");
    if (!fp) return 2;
    int hdr[8];   // h, w, frames, dims, max_span_u, max_span_v
    float vs, origin[3], K[9], velo2img[12], jump_rel;
    tsdf_scan_ground_params ground;
    if (std::fread(hdr, sizeof(int), 8, fp) != 8 || !read_floats(fp, &jump_rel, 1) || !read_floats(fp, &vs, 1) || !read_floats(fp, origin, 3) ||
        !read_floats(fp, K, 9) || !read_floats(fp, velo2img, 12) || std::fread(&ground, sizeof ground, 1, fp) != 1)
        return 2;
    const int h = hdr[0], w = hdr[1], n_frames = hdr[2];
    const size_t px = (size_t)h * w;

    tsdf_config cfg;
    tsdf_config_default(&cfg, h, w);
    cfg.dim_x = hdr[3]; cfg.dim_y = hdr[4]; cfg.dim_z = hdr[5];
    cfg.z_begin = 0; cfg.z_end = hdr[5];
    cfg.voxel_size = vs;
    cfg.trunc_margin = vs * 5;
    std::memcpy(cfg.origin, origin, sizeof origin);
    std::memcpy(cfg.cam_K, K, sizeof K);

    TSDF::ThrowOnError(false);
    const std::vector<int> devices(2, 0);
    TSDF *obj[6];
    for (int i = 0; i < 6; ++i) {
        cfg.id = i + 1;
        obj[i] = slabs ? new TSDF(cfg, devices) : new TSDF(cfg);
    }
    obj[0]->SetScanGround(ground);                                  // (DROP_GROUND is the default)
    obj[0]->SetScanFill(hdr[6], hdr[7], jump_rel);
    obj[2]->SetScanGround(ground, TSDF_SCAN_DROP_GROUND);
    obj[3]->SetScanGround(ground, TSDF_SCAN_ONLY_GROUND);
    obj[3]->SetScanFill(hdr[6], hdr[7], jump_rel);
    obj[4]->SetScanGround(ground);
    obj[4]->ClearScanGround();
    obj[4]->SetScanFill(hdr[6], hdr[7], jump_rel);
    obj[5]->SetScanFill(hdr[6], hdr[7], jump_rel);

    for (int k = 0; k < n_frames; ++k) {
        std::vector<float> pose(16), restated(px);
        int n_pts = 0;
        if (!read_floats(fp, pose.data(), 16) || std::fread(&n_pts, sizeof(int), 1, fp) != 1 || n_pts < 0) return 2;
        std::vector<float> scan((size_t)n_pts * 4);
        if (!read_floats(fp, scan.data(), scan.size()) || !read_floats(fp, restated.data(), px)) return 2;
        // projectPointCloud(); groundRemoval();                              ref: examples/label_instance_lidar.cpp:85-91
        // imD = GetRangeImageFromBinaryFile(...); tsdf->Integrate(imD, pose)   ref: :76-77, src/Object.cpp:160-164
        obj[1]->Integrate(restated.data(), pose);
        for (int i = 0; i < 6; ++i)
            if (i != 1) obj[i]->IntegrateScan(scan.data(), (size_t)n_pts, velo2img, pose);
    }
    std::fclose(fp);
    for (int i = 0; i < 6; ++i) delete obj[i];   // writes tsdf<i+1>.ply, tsdf<i+1>.bin
    std::printf("done\n");
    return 0;
}
