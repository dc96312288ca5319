// mesh_files.h -- everything that turns arrays into files: the points .ply, the .bin header, the mesh .ply as a triangle
// soup and welded with normals, and the colour a vertex takes from its nearest voxel.  Plain C++ (no HIP, no device types):
// tsdf_extract_host.hip.h includes it for the product and tests/mesh_files_check.cpp compiles it by itself with
// -fsanitize=address,undefined (tests/test_mesh_files.py; tests/files_spec.py states the formats byte for byte).
// Nothing here knows the library's error channel: a writer returns a Result, the caller words it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "tsdf_hip.h"

namespace mesh_files {

enum class Result { Ok, CannotOpen, ShortWrite };

// A file being written.  A failure is remembered, later writes are dropped, and close() tells what went wrong, once: a file
// that could not be opened, or one that did not take every byte (what fclose says counts: it flushes the last buffer).
class OutFile {
public:
    OutFile(const char *path, const char *mode) : fp_(std::fopen(path, mode)) {}
    ~OutFile() { if (fp_) std::fclose(fp_); }
    OutFile(const OutFile &) = delete;
    OutFile &operator=(const OutFile &) = delete;

    bool good() const { return fp_ && !short_; }
    FILE *get() const { return fp_; }       // for a writer that reports its own failures (the device-to-file streamer)

    __attribute__((format(__printf__, 2, 3))) void print(const char *fmt, ...)
    {
        if (!good()) return;
        va_list ap;
        va_start(ap, fmt);
        if (std::vfprintf(fp_, fmt, ap) <= 0) short_ = true;
        va_end(ap);
    }
    void write(const void *data, size_t size, size_t count)
    {
        if (good() && count > 0 && std::fwrite(data, size, count, fp_) != count) short_ = true;   // (no items: data may be null)
    }
    Result close()
    {
        if (!fp_) return Result::CannotOpen;
        const int bad = std::fclose(fp_);
        fp_ = nullptr;
        return short_ || bad ? Result::ShortWrite : Result::Ok;
    }

private:
    FILE *fp_;
    bool short_ = false;
};

// ---- surface points ----------------------------------------------------------------------------------------------------
// header text of ref: src/tsdf.cu:185-192 (the vertex count is printed with %d there: the caller bounds n by 2^31 - 1)
inline void points_ply_header(OutFile &f, int64_t n)
{
    f.print("ply\nformat binary_little_endian 1.0\nelement vertex %d\n", (int)n);
    f.print("property float x\nproperty float y\nproperty float z\nend_header\n");
}

inline Result write_points_ply(const char *path, const float *xyz, int64_t n)
{
    OutFile f(path, "w");
    points_ply_header(f, n);
    f.write(xyz, sizeof(float), (size_t)n * 3);
    return f.close();
}

// ---- .bin ----------------------------------------------------------------------------------------------------------------
// ref: src/tsdf.cu:118-129 -- the dims of the slab the file holds as floats, origin, voxel size, truncation margin; the TSDF
// values follow
inline void write_bin_header(OutFile &f, const tsdf_config &c)
{
    const float hdr[8] = {(float)c.dim_x, (float)c.dim_y, (float)(c.z_end - c.z_begin), c.origin[0], c.origin[1], c.origin[2],
                          c.voxel_size, c.trunc_margin};
    f.write(hdr, sizeof(float), 8);
}

// ---- vertex colour -------------------------------------------------------------------------------------------------------
// The voxel of the slab [z_begin, z_end) nearest to p, as an index into the slab's arrays (x fastest): per axis the float
// quotient rounded half away from zero, clamped into the slab (what the reference's Python glue does with the rounded vertex
// indices, ref: src/TSDFfusion.py.in:48-53).
inline size_t nearest_voxel(const tsdf_config &c, const float p[3])
{
    long ix = std::lround((p[0] - c.origin[0]) / c.voxel_size), iy = std::lround((p[1] - c.origin[1]) / c.voxel_size);
    long iz = std::lround((p[2] - c.origin[2]) / c.voxel_size) - c.z_begin;
    ix = std::min<long>(std::max<long>(ix, 0), c.dim_x - 1);
    iy = std::min<long>(std::max<long>(iy, 0), c.dim_y - 1);
    iz = std::min<long>(std::max<long>(iz, 0), c.z_end - c.z_begin - 1);
    return ((size_t)iz * c.dim_y + (size_t)iy) * c.dim_x + (size_t)ix;
}

// r, g, b of every vertex: its nearest voxel's packed 0x00BBGGRR (tsdf_colour.hip.h)
inline std::vector<unsigned char> vertex_rgb(const tsdf_config &c, const uint32_t *colour, const float *xyz, size_t n_vertices)
{
    std::vector<unsigned char> rgb(n_vertices * 3);
    for (size_t k = 0; k < n_vertices; ++k) {
        const uint32_t q = colour[nearest_voxel(c, xyz + 3 * k)];
        rgb[3 * k] = (unsigned char)(q & 255u); rgb[3 * k + 1] = (unsigned char)((q >> 8) & 255u);
        rgb[3 * k + 2] = (unsigned char)((q >> 16) & 255u);
    }
    return rgb;
}

// ---- meshes --------------------------------------------------------------------------------------------------------------
// one record per vertex: its three floats from each of the n_arrays arrays in turn, then, when rgb is given, its 3 colour bytes
inline void write_vertices(OutFile &f, const float *const *floats, int n_arrays, const unsigned char *rgb, size_t n_vertices)
{
    const size_t rec = 12 * (size_t)n_arrays + (rgb ? 3 : 0);
    std::vector<unsigned char> out(n_vertices * rec);
    for (size_t i = 0; i < n_vertices; ++i) {
        unsigned char *r = out.data() + i * rec;
        for (int a = 0; a < n_arrays; ++a) std::memcpy(r + 12 * a, floats[a] + 3 * i, 12);
        if (rgb) std::memcpy(r + 12 * n_arrays, rgb + 3 * i, 3);
    }
    f.write(out.data(), rec, n_vertices);
}

// n_faces records {3, i0, i1, i2}
inline void write_faces(OutFile &f, const int32_t *idx, size_t n_faces)
{
    std::vector<unsigned char> out(n_faces * 13);
    for (size_t k = 0; k < n_faces; ++k) { out[13 * k] = 3; std::memcpy(out.data() + 13 * k + 1, idx + 3 * k, 12); }
    f.write(out.data(), 13, n_faces);
}

// Binary .ply of n triangles as a soup, three vertices each; colour (may be null): the slab's colour grid, see vertex_rgb
inline Result write_mesh_ply(const char *path, const float *tri, int64_t n, const tsdf_config &c, const uint32_t *colour = nullptr)
{
    OutFile f(path, "wb");
    f.print("ply\nformat binary_little_endian 1.0\nelement vertex %lld\n", (long long)(3 * n));
    f.print("property float x\nproperty float y\nproperty float z\n");
    if (colour) f.print("property uchar red\nproperty uchar green\nproperty uchar blue\n");
    f.print("element face %lld\nproperty list uchar int vertex_indices\nend_header\n", (long long)n);
    if (colour) write_vertices(f, &tri, 1, vertex_rgb(c, colour, tri, (size_t)n * 3).data(), (size_t)n * 3);
    else f.write(tri, sizeof(float), (size_t)n * 9);
    std::vector<int32_t> idx((size_t)n * 3);
    for (size_t k = 0; k < idx.size(); ++k) idx[k] = (int32_t)k;
    write_faces(f, idx.data(), (size_t)n);
    return f.close();
}

// The mesh as the reference's Python glue saves it (ref: src/TSDFfusion.py.in:48-53: get_mesh -> verts, faces, norms,
// colors -> meshwrite): shared vertices, a normal per vertex.  The soup's edge vertices are bit-identical between
// neighbouring cubes (tsdf_extract.hip.h), so welding is an exact match on the three coordinates' bits (+0 and -0 differ);
// a vertex is numbered at its first appearance; faces keep the soup's order and winding; a normal is the sum, in double and
// in face order, of 2 x area x unit normal of the vertex's faces, normalised, or (0, 0, 0) where the sum is.
struct Welded {
    std::vector<float> verts, normals;    // 3 per vertex
    std::vector<int32_t> faces;           // 3 per triangle
};

inline Welded weld(const float *tri, int64_t n)
{
    struct Key { uint32_t x, y, z; bool operator==(const Key &o) const { return x == o.x && y == o.y && z == o.z; } };
    struct Hash { size_t operator()(const Key &k) const { uint64_t h = k.x * 0x9E3779B97F4A7C15ull; h ^= (h >> 29) + k.y * 0xBF58476D1CE4E5B9ull; h ^= (h >> 31) + k.z * 0x94D049BB133111EBull; return (size_t)(h ^ (h >> 32)); } };
    Welded m;
    std::unordered_map<Key, int32_t, Hash> ids;
    ids.reserve((size_t)n);
    m.faces.resize((size_t)n * 3);
    for (int64_t k = 0; k < 3 * n; ++k) {
        Key key;
        std::memcpy(&key, tri + 3 * k, 12);
        auto it = ids.find(key);
        if (it == ids.end()) {
            it = ids.emplace(key, (int32_t)(m.verts.size() / 3)).first;
            m.verts.insert(m.verts.end(), tri + 3 * k, tri + 3 * k + 3);
        }
        m.faces[(size_t)k] = it->second;
    }
    const size_t nv = m.verts.size() / 3;
    std::vector<double> acc(nv * 3, 0.0);
    for (int64_t f = 0; f < n; ++f) {
        const float *a = tri + 9 * f, *b = a + 3, *c = a + 6;
        const double ux = (double)b[0] - a[0], uy = (double)b[1] - a[1], uz = (double)b[2] - a[2];
        const double wx = (double)c[0] - a[0], wy = (double)c[1] - a[1], wz = (double)c[2] - a[2];
        const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
        for (int k = 0; k < 3; ++k) { double *q = acc.data() + 3 * (size_t)m.faces[(size_t)(3 * f + k)]; q[0] += nx; q[1] += ny; q[2] += nz; }
    }
    m.normals.resize(nv * 3);
    for (size_t i = 0; i < nv; ++i) {
        const double *q = acc.data() + 3 * i;
        const double len = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
        for (int k = 0; k < 3; ++k) m.normals[3 * i + k] = len > 0 ? (float)(q[k] / len) : 0.0f;
    }
    return m;
}

// Binary .ply of a welded mesh: x y z nx ny nz per vertex, and its nearest voxel's colour when a colour grid is given
inline Result write_welded_ply(const char *path, const Welded &m, const tsdf_config &c, const uint32_t *colour = nullptr)
{
    const size_t nv = m.verts.size() / 3, nf = m.faces.size() / 3;
    OutFile f(path, "wb");
    f.print("ply\nformat binary_little_endian 1.0\nelement vertex %zu\n", nv);
    f.print("property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n");
    if (colour) f.print("property uchar red\nproperty uchar green\nproperty uchar blue\n");
    f.print("element face %lld\nproperty list uchar int vertex_index\nend_header\n", (long long)nf);
    const float *arrays[2] = {m.verts.data(), m.normals.data()};
    write_vertices(f, arrays, 2, colour ? vertex_rgb(c, colour, m.verts.data(), nv).data() : nullptr, nv);
    write_faces(f, m.faces.data(), nf);
    return f.close();
}

}  // namespace mesh_files
