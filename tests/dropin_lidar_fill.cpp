// dropin_lidar_fill.cpp -- test harness: the reference's lidar call sequence through include/tsdf.hpp, as
// tests/dropin_lidar.cpp replays it, with the gaps between beams filled (TSDF::SetScanFill).  Per keyframe the labeller makes
// a range image of the scan (ref: examples/label_instance_lidar.cpp:76-77), Engine::Run masks it per instance (ref:
// src/Engine.cpp:192-193) and gives the masked image to the object's TSDF (ref: src/Object.cpp:160-164).  The fill runs
// behind the mask, on the masked image, so it stays inside the mask.
// Reads the grid, the camera, velo2img, the fill's parameters and the frames from argv[1]; argv[2] = "slabs" cuts the grid
// into two z-slabs on one device.  Writes into the working directory
//     tsdf1.{ply,bin}   SetScanFill, IntegrateRange of the masked range image
//     tsdf2.{ply,bin}   Integrate of the restated filled z-depth of that image, read from the file
//     tsdf3.{ply,bin}   SetScanFill, IntegrateScan of the scan itself (unmasked)
//     tsdf4.{ply,bin}   SetScanFill, then ClearScanFill, IntegrateScan
//     tsdf5.{ply,bin}   IntegrateScan by an object that never set it
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
    if (std::fread(hdr, sizeof(int), 8, fp) != 8 || !read_floats(fp, &jump_rel, 1) || !read_floats(fp, &vs, 1) || !read_floats(fp, origin, 3) ||
        !read_floats(fp, K, 9) || !read_floats(fp, velo2img, 12))
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
    TSDF *obj[5];
    for (int i = 0; i < 5; ++i) {
        cfg.id = i + 1;
        obj[i] = slabs ? new TSDF(cfg, devices) : new TSDF(cfg);
    }
    obj[0]->SetScanFill(hdr[6], hdr[7], jump_rel);
    obj[2]->SetScanFill(hdr[6], hdr[7], jump_rel);
    obj[3]->SetScanFill(hdr[6], hdr[7], jump_rel);
    obj[3]->ClearScanFill();
    tsdf_scanner *scanner = NULL;
    if (tsdf_scanner_create(0, h, w, &scanner) != TSDF_OK) return 3;

    for (int k = 0; k < n_frames; ++k) {
        std::vector<float> pose(16), restated(px), imD(px), masked(px);
        std::vector<unsigned char> mask(px);
        int n_pts = 0;
        if (!read_floats(fp, pose.data(), 16) || std::fread(&n_pts, sizeof(int), 1, fp) != 1 || n_pts < 0) return 2;
        std::vector<float> scan((size_t)n_pts * 4);
        if (!read_floats(fp, scan.data(), scan.size()) || std::fread(mask.data(), 1, px, fp) != px || !read_floats(fp, restated.data(), px))
            return 2;
        // imD = GetRangeImageFromBinaryFile(...)                             ref: examples/label_instance_lidar.cpp:76-77
        if (tsdf_scan_project(scanner, velo2img, NULL, scan.data(), n_pts, imD.data(), NULL, NULL) != TSDF_OK) {
            std::fprintf(stderr, "%s\n", tsdf_last_error());
            return 3;
        }
        // multiply( imD, masks[i]/255, masked, 1, imD.type() )               ref: src/Engine.cpp:192-193
        for (size_t i = 0; i < px; ++i) masked[i] = imD[i] * (float)(mask[i] / 255);
        // tsdf->Integrate(depth, cam2world_vec), for an image of ranges      ref: src/Object.cpp:160-164
        obj[0]->IntegrateRange(masked.data(), pose);
        obj[1]->Integrate(restated.data(), pose);
        for (int i = 2; i < 5; ++i) obj[i]->IntegrateScan(scan.data(), (size_t)n_pts, velo2img, pose);
    }
    std::fclose(fp);
    tsdf_scanner_destroy(scanner);
    for (int i = 0; i < 5; ++i) delete obj[i];   // writes tsdf<i+1>.ply, tsdf<i+1>.bin
    std::printf("done\n");
    return 0;
}
