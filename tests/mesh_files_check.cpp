// mesh_files_check.cpp -- semantic_slam_amd/csrc/mesh_files.h by itself, for tests/test_mesh_files.py: built with
// -fsanitize=address,undefined and run as a child process, no device and no Python in the process.
//
//   mesh_files_check INPUT OUTDIR [PATH ...]
//
// INPUT: int32 dim_x, dim_y, dim_z, z_begin, z_end, n_triangles, has_colour; float32 origin[3], voxel_size, trunc_margin;
// float32 triangles[n][3][3]; uint32 colour[(z_end - z_begin) * dim_y * dim_x] when has_colour.
// Every format goes into OUTDIR; then every writer is pointed at each PATH and its result codes are printed, one line per PATH.
#include <cstdio>
#include <string>
#include <vector>

#include "mesh_files.h"

namespace mf = mesh_files;

template <class T> static bool read_n(FILE *fp, T *dst, size_t n) { return n == 0 || std::fread(dst, sizeof(T), n, fp) == n; }

struct Input {
    tsdf_config cfg = {};
    int64_t n = 0;
    std::vector<float> tri;
    std::vector<uint32_t> colour;
    const uint32_t *grid() const { return colour.empty() ? nullptr : colour.data(); }
};

// the five writers at `path`: points (the soup's vertices as a point list), soup, welded, both with colour where there is
// one, and the .bin header
static void write_all(const Input &in, const std::string &dir, const char *one_path, int codes[6])
{
    auto at = [&](const char *name) { return one_path ? std::string(one_path) : dir + "/" + name; };
    const mf::Welded m = mf::weld(in.tri.data(), in.n);
    codes[0] = (int)mf::write_points_ply(at("points.ply").c_str(), in.tri.data(), 3 * in.n);
    codes[1] = (int)mf::write_mesh_ply(at("soup.ply").c_str(), in.tri.data(), in.n, in.cfg);
    codes[2] = (int)mf::write_welded_ply(at("welded.ply").c_str(), m, in.cfg);
    codes[3] = in.grid() ? (int)mf::write_mesh_ply(at("soup_rgb.ply").c_str(), in.tri.data(), in.n, in.cfg, in.grid()) : -1;
    codes[4] = in.grid() ? (int)mf::write_welded_ply(at("welded_rgb.ply").c_str(), m, in.cfg, in.grid()) : -1;
    mf::OutFile f(at("header.bin").c_str(), "wb");
    mf::write_bin_header(f, in.cfg);
    codes[5] = (int)f.close();
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s INPUT OUTDIR [PATH ...]\n", argv[0]); return 2; }
    Input in;
    FILE *fp = std::fopen(argv[1], "rb");
    int32_t head[7];
    float scal[5];
    if (!fp || !read_n(fp, head, 7) || !read_n(fp, scal, 5)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    tsdf_config &c = in.cfg;
    c.dim_x = head[0]; c.dim_y = head[1]; c.dim_z = head[2]; c.z_begin = head[3]; c.z_end = head[4];
    in.n = head[5];
    c.origin[0] = scal[0]; c.origin[1] = scal[1]; c.origin[2] = scal[2]; c.voxel_size = scal[3]; c.trunc_margin = scal[4];
    in.tri.resize((size_t)in.n * 9);
    if (head[6]) in.colour.resize((size_t)(c.z_end - c.z_begin) * c.dim_y * c.dim_x);
    const bool ok = read_n(fp, in.tri.data(), in.tri.size()) && read_n(fp, in.colour.data(), in.colour.size());
    std::fclose(fp);
    if (!ok) { std::fprintf(stderr, "%s is short\n", argv[1]); return 2; }

    const std::string dir = argv[2];
    int codes[6];
    write_all(in, dir, nullptr, codes);
    for (int k = 0; k < 6; ++k)
        if (codes[k] > 0) { std::fprintf(stderr, "writer %d into %s: code %d\n", k, dir.c_str(), codes[k]); return 1; }
    // the nearest voxel of every vertex of the soup, and its colour
    {
        std::vector<int64_t> idx((size_t)in.n * 3);
        for (size_t k = 0; k < idx.size(); ++k) idx[k] = (int64_t)mf::nearest_voxel(c, in.tri.data() + 3 * k);
        mf::OutFile f((dir + "/nearest.i64").c_str(), "wb");
        f.write(idx.data(), sizeof(int64_t), idx.size());
        if (f.close() != mf::Result::Ok) return 1;
    }
    if (in.grid()) {
        const std::vector<unsigned char> rgb = mf::vertex_rgb(c, in.grid(), in.tri.data(), (size_t)in.n * 3);
        mf::OutFile f((dir + "/rgb.u8").c_str(), "wb");
        f.write(rgb.data(), 1, rgb.size());
        if (f.close() != mf::Result::Ok) return 1;
    }
    for (int a = 3; a < argc; ++a) {
        write_all(in, dir, argv[a], codes);
        std::printf("%s", argv[a]);
        for (int k = 0; k < 6; ++k) std::printf(" %d", codes[k]);
        std::printf("\n");
    }
    return 0;
}
