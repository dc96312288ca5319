// tsdf_extract_host.hip.h -- host side of extraction, the file writers and the checkpoint calls (include/tsdf_hip.h:
// tsdf_count_surface ... tsdf_load_state; the group's are in tsdf_group.hip.h and use what is here), included at the end of
// tsdf_capi.hip; tsdf_extract.hip.h states the extraction rules, mesh_files.h the file formats (host-only, tested on the CPU).
#pragma once
#include <functional>
#include <mutex>

#include "mesh_files.h"

namespace {

// ---- files -----------------------------------------------------------------------------------------------------------------
// what a writer of mesh_files.h returned, in the library's words
int io_result(mesh_files::Result r, const char *who, const char *path)
{
    if (r == mesh_files::Result::CannotOpen) return fail(TSDF_ERR_IO, "%s: cannot open %s", who, path);
    if (r == mesh_files::Result::ShortWrite) return fail(TSDF_ERR_IO, "%s: short write to %s", who, path);
    return TSDF_OK;
}

// the end of a saver that streamed device memory into f: what the streaming said comes first, then the file's own result
int close_streamed(mesh_files::OutFile &f, int rc, const char *who, const char *path)
{
    const mesh_files::Result r = f.close();
    return rc ? rc : io_result(r, who, path);
}

// A file being read: every read has to deliver in full.
struct InFile {
    explicit InFile(const char *path) : fp(std::fopen(path, "rb")) {}
    ~InFile() { if (fp) std::fclose(fp); }
    InFile(const InFile &) = delete;
    InFile &operator=(const InFile &) = delete;
    bool read(void *dst, size_t size, size_t count) { return fp && (count == 0 || std::fread(dst, size, count, fp) == count); }
    FILE *fp;
};

// Device memory to an open file at the rate of the slower of PCIe and the file system: pieces of 32 MiB go device -> pinned host
// buffer on the handle's stream while the previous piece is being written (the reference's writers scan and write float by
// float, ref: src/tsdf.cu:130-131,210-212; a whole-array download into a fresh std::vector first costs a zero fill, a pageable
// copy and the write, one after the other: 300 ms for a 512^3 .bin against 150 ms this way).  The two buffers are process-wide
// (files are written rarely and the disk serialises writers anyway); the lock is held for the length of one array.
struct FileStager {
    std::mutex mu;
    HostPtr<char> pin[2];                    // portable: any device may copy into them
    static constexpr size_t kPiece = (size_t)32 << 20;
};
FileStager &file_stager() { static FileStager s; return s; }

// bytes of device memory `src` (on v's device) appended to fp; the stream must already hold everything `src` depends on
int stream_device_to_file(tsdf_volume *v, FILE *fp, const void *src, size_t bytes, const char *who, const char *path)
{
    if (bytes == 0) return TSDF_OK;
    FileStager &fs = file_stager();
    std::lock_guard<std::mutex> lk(fs.mu);
    for (int i = 0; i < 2; ++i)
        if (!fs.pin[i]) HIP_TRY(host_alloc(fs.pin[i], FileStager::kPiece, hipHostMallocPortable));
    // the events belong to the device of v's stream (the current one: every caller has bound it), so they live for the call
    Event ev[2];
    hipError_t e = event_create(ev[0]);
    if (e == hipSuccess) e = event_create(ev[1]);
    const size_t pieces = (bytes + FileStager::kPiece - 1) / FileStager::kPiece;
    auto len = [&](size_t k) { return k + 1 < pieces ? FileStager::kPiece : bytes - k * FileStager::kPiece; };
    bool short_write = false;
    for (size_t k = 0; e == hipSuccess && k <= pieces; ++k) {
        if (k < pieces) {     // piece k on its way ...
            e = hipMemcpyAsync(fs.pin[k & 1], (const char *)src + k * FileStager::kPiece, len(k), hipMemcpyDeviceToHost, v->stream);
            if (e == hipSuccess) e = hipEventRecord(ev[k & 1], v->stream);
        }
        if (e == hipSuccess && k > 0) {          // ... while piece k - 1 is written
            e = hipEventSynchronize(ev[(k - 1) & 1]);
            if (e == hipSuccess && !short_write && std::fwrite(fs.pin[(k - 1) & 1], 1, len(k - 1), fp) != len(k - 1)) short_write = true;
        }
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(v->stream);     // nothing may still be writing into the buffers
    if (e != hipSuccess) return fail(TSDF_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    if (short_write) return fail(TSDF_ERR_IO, "%s: short write to %s", who, path);
    return TSDF_OK;
}

// ---- the extraction pass ---------------------------------------------------------------------------------------------------
// surface points (ref: src/tsdf.cu:170-218), zero-crossing vertices, marching-tetrahedra triangles (3 vertices each)
enum class ListKind { Surface, Crossings, Mesh };
constexpr size_t list_item_floats(ListKind kind) { return kind == ListKind::Mesh ? 9 : 3; }

// Where a pass leaves its list: nowhere (it only counts), the first `capacity` items in a host array, or all of it in
// v->d_list (tsdf_save_ply streams it from there).
struct ListDest {
    float *host = nullptr;
    int64_t capacity = 0;
    bool on_device = false;
    static ListDest to_host(float *dst, int64_t capacity) { return {dst, capacity, false}; }
    static ListDest left_on_device() { return {nullptr, INT64_MAX, true}; }
};

// One pass over the slab: count per chunk, scan, read the total back and -- where the list goes somewhere -- emit at the
// scanned offsets.  halo_*: slice z_end from the upper neighbour (host or device memory) or NULL; the surface rule is per
// voxel and takes none.
int extract_pass(tsdf_volume *v, ListKind kind, const float *halo_tsdf, const float *halo_weight, float weight_thresh,
                 const ListDest &dest, int64_t *count)
{
    const bool surface = kind == ListKind::Surface;
    const char *what = surface ? "surface extraction" : "zero crossings";
    int rc = bind_device(v);
    if (rc) return rc;
    *count = 0;
    if (v->geo.n_vox == 0) return TSDF_OK;
    if (!surface && (halo_tsdf == nullptr) != (halo_weight == nullptr))
        return fail(TSDF_ERR_INVALID, "zero crossings: give both halo arrays or neither");
    const tsdf_config &c = v->cfg;
    const int64_t n = v->geo.n_vox;
    const int64_t n_chunks = (n + tsdfx::kChunk - 1) / tsdfx::kChunk;
    if (n_chunks > 0x7fffffff) return fail(TSDF_ERR_INVALID, "%s: slab too large", what);
    const size_t slice = (size_t)c.dim_x * c.dim_y;
    // scratch: per-chunk counts (u32) | per-chunk offsets (i64) | total (i64) | halo copy (2 slices of floats)
    tsdf_host::Regions r;
    const size_t o_counts = r.add((size_t)n_chunks * sizeof(uint32_t)), o_offsets = r.add((size_t)n_chunks * sizeof(int64_t));
    const size_t o_total = r.add(sizeof(int64_t)), o_halo = surface ? 0 : r.add(2 * slice * sizeof(float));
    HIP_TRY(v->d_scratch.ensure(r.total()));
    char *s = (char *)v->d_scratch;
    uint32_t *d_counts = (uint32_t *)(s + o_counts);
    int64_t *d_offsets = (int64_t *)(s + o_offsets);
    int64_t *d_total = (int64_t *)(s + o_total);
    tsdfx::CrossingGrid g = {};     // what the crossing and mesh kernels read; the surface kernels take the arrays themselves
    if (!surface) {
        float *d_halo = (float *)(s + o_halo);
        g.tsdf = v->d_tsdf; g.weight = v->d_weight; g.halo_tsdf = nullptr; g.halo_weight = nullptr;
        if (halo_tsdf) {   // host or device source: stage both slices in our scratch
            HIP_TRY(hipMemcpyAsync(d_halo, halo_tsdf, slice * sizeof(float), hipMemcpyDefault, v->stream));
            HIP_TRY(hipMemcpyAsync(d_halo + slice, halo_weight, slice * sizeof(float), hipMemcpyDefault, v->stream));
            g.halo_tsdf = d_halo; g.halo_weight = d_halo + slice;
        }
        g.n = n; g.dim_x = c.dim_x; g.dim_y = c.dim_y; g.nz = c.z_end - c.z_begin; g.z_begin = c.z_begin;
        g.thr = weight_thresh; g.ox = c.origin[0]; g.oy = c.origin[1]; g.oz = c.origin[2]; g.vs = c.voxel_size;
        g.flags = v->geo.nseg > 0 ? v->d_flags : nullptr; g.nseg = v->geo.nseg;     // segments that are all free / unseen space are skipped
    }
    const dim3 grid((unsigned)n_chunks), block(256);
    if (surface) hipLaunchKernelGGL(tsdfx::surface_count, grid, block, 0, v->stream, v->d_tsdf, v->d_weight, n, weight_thresh, d_counts);
    else if (kind == ListKind::Mesh) hipLaunchKernelGGL(tsdfx::mesh_count, grid, block, 0, v->stream, g, d_counts);
    else hipLaunchKernelGGL(tsdfx::crossing_count, grid, block, 0, v->stream, g, d_counts);
    hipLaunchKernelGGL(tsdfx::scan_counts, dim3(1), dim3(1024), 0, v->stream, d_counts, n_chunks, d_offsets, d_total);
    HIP_TRY(hipGetLastError());
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    *count = total;
    if ((!dest.host && !dest.on_device) || dest.capacity <= 0 || total == 0) return TSDF_OK;

    const size_t item_bytes = list_item_floats(kind) * sizeof(float);
    const int64_t n_out = total < dest.capacity ? total : dest.capacity;
    HIP_TRY(v->d_list.ensure((size_t)total * item_bytes));
    float *d_xyz = reinterpret_cast<float *>(v->d_list.get());
    if (surface)
        hipLaunchKernelGGL(tsdfx::surface_emit, grid, block, 0, v->stream, v->d_tsdf, v->d_weight, n, weight_thresh, d_offsets,
                           c.dim_x, c.dim_y, c.z_begin, c.origin[0], c.origin[1], c.origin[2], c.voxel_size, d_xyz);
    else if (kind == ListKind::Mesh) hipLaunchKernelGGL(tsdfx::mesh_emit_kernel, grid, block, 0, v->stream, g, d_offsets, d_xyz);
    else hipLaunchKernelGGL(tsdfx::crossing_emit, grid, block, 0, v->stream, g, d_offsets, d_xyz);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && dest.host) e = hipMemcpyAsync(dest.host, d_xyz, (size_t)n_out * item_bytes, hipMemcpyDeviceToHost, v->stream);
    if (e == hipSuccess && dest.host) e = hipStreamSynchronize(v->stream);
    if (e != hipSuccess) return fail(TSDF_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return TSDF_OK;
}

// ---- count, then fill ------------------------------------------------------------------------------------------------------
// A source of lists as its callers ask for them: list(kind, nullptr, 0, &n) counts, list(kind, dst, capacity, &n) fills.
using ListFn = std::function<int(ListKind kind, float *dst, int64_t capacity, int64_t *count)>;

// The whole list in `out`: count, size the vector, call again to fill it.  admit (may be empty) can refuse the count before
// anything is allocated.
int count_then_fill(const ListFn &list, ListKind kind, std::vector<float> &out, int64_t *n, const std::function<int(int64_t)> &admit = nullptr)
{
    int rc = list(kind, nullptr, 0, n);
    if (rc == TSDF_OK && admit) rc = admit(*n);
    if (rc) return rc;
    out.resize((size_t)*n * list_item_floats(kind));
    return *n > 0 ? list(kind, out.data(), *n, n) : TSDF_OK;
}

// a handle's own mesh (no halo) and, where colour is enabled, its colour grid for the vertex colours (else `colour` stays empty)
int mesh_for_file(tsdf_volume *v, float weight_thresh, std::vector<float> &tri, int64_t *n, std::vector<uint32_t> &colour,
                  const std::function<int(int64_t)> &admit = nullptr)
{
    int rc = count_then_fill([&](ListKind kind, float *dst, int64_t capacity, int64_t *count) {
        return extract_pass(v, kind, nullptr, nullptr, weight_thresh, ListDest::to_host(dst, capacity), count);
    }, ListKind::Mesh, tri, n, admit);
    if (rc || !v->d_colour) return rc;
    colour.resize((size_t)(v->geo.n_vox > 0 ? v->geo.n_vox : 1));
    return tsdf_download_colour(v, colour.data());
}

const char kStateMagic[8] = {'T', 'S', 'D', 'F', 'H', 'I', 'P', '1'};

}  // namespace

extern "C" {

int tsdf_count_surface(tsdf_volume *v, float weight_thresh, int64_t *count)
{
    if (!v || !count) return fail(TSDF_ERR_INVALID, "tsdf_count_surface: NULL argument");
    return extract_pass(v, ListKind::Surface, nullptr, nullptr, weight_thresh, ListDest(), count);
}

int tsdf_extract_surface(tsdf_volume *v, float weight_thresh, float *xyz_host, int64_t capacity,
                         int64_t *count)
{
    if (!v || !count) return fail(TSDF_ERR_INVALID, "tsdf_extract_surface: NULL argument");
    return extract_pass(v, ListKind::Surface, nullptr, nullptr, weight_thresh, ListDest::to_host(xyz_host, capacity), count);
}

int tsdf_extract_crossings(tsdf_volume *v, const float *halo_tsdf, const float *halo_weight, float weight_thresh,
                           float *xyz_host, int64_t capacity, int64_t *count)
{
    if (!v || !count) return fail(TSDF_ERR_INVALID, "tsdf_extract_crossings: NULL argument");
    return extract_pass(v, ListKind::Crossings, halo_tsdf, halo_weight, weight_thresh, ListDest::to_host(xyz_host, capacity), count);
}

int tsdf_extract_mesh(tsdf_volume *v, const float *halo_tsdf, const float *halo_weight, float weight_thresh,
                      float *triangles_host, int64_t capacity, int64_t *count)
{
    if (!v || !count) return fail(TSDF_ERR_INVALID, "tsdf_extract_mesh: NULL argument");
    return extract_pass(v, ListKind::Mesh, halo_tsdf, halo_weight, weight_thresh, ListDest::to_host(triangles_host, capacity), count);
}

// the triangle soup; a vertex takes its nearest voxel's colour when colour is enabled (mesh_files.h)
int tsdf_save_mesh_ply(tsdf_volume *v, const char *path, float weight_thresh)
{
    const char *who = "tsdf_save_mesh_ply";
    if (!v || !path) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    std::vector<float> tri;
    std::vector<uint32_t> colour;
    int64_t n = 0;
    int rc = mesh_for_file(v, weight_thresh, tri, &n, colour);
    if (rc) return rc;
    return io_result(mesh_files::write_mesh_ply(path, tri.data(), n, v->cfg, colour.empty() ? nullptr : colour.data()), who, path);
}

// the mesh as the reference's Python glue saves it: shared vertices, a normal and (colour enabled) a colour per vertex (mesh_files.h)
int tsdf_save_mesh_welded_ply(tsdf_volume *v, const char *path, float weight_thresh)
{
    const char *who = "tsdf_save_mesh_welded_ply";
    if (!v || !path) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    std::vector<float> tri;
    std::vector<uint32_t> colour;
    int64_t n = 0;
    int rc = mesh_for_file(v, weight_thresh, tri, &n, colour, [&](int64_t k) {
        return 3 * k > 0x7fffffffll ? fail(TSDF_ERR_INVALID, "%s: %lld triangles exceed 32-bit vertex indices", who, (long long)k) : TSDF_OK;
    });
    if (rc) return rc;
    return io_result(mesh_files::write_welded_ply(path, mesh_files::weld(tri.data(), n), v->cfg, colour.empty() ? nullptr : colour.data()), who, path);
}

int tsdf_save_ply(tsdf_volume *v, const char *path, float weight_thresh)
{
    const char *who = "tsdf_save_ply";
    if (!v || !path) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    // one counting + emitting pass that leaves the points in device memory, then header + list streamed to the file
    int64_t n = 0;
    int rc = extract_pass(v, ListKind::Surface, nullptr, nullptr, weight_thresh, ListDest::left_on_device(), &n);
    if (rc) return rc;
    if (n > 0x7fffffffll)   // the header's "element vertex %d" (ref: src/tsdf.cu:188) cannot hold it
        return fail(TSDF_ERR_INVALID, "%s: %lld surface points exceed the format's 2^31 - 1 (write slabs separately)", who, (long long)n);
    mesh_files::OutFile f(path, "w");
    mesh_files::points_ply_header(f, n);
    if (f.good()) rc = stream_device_to_file(v, f.get(), v->d_list, (size_t)n * 3 * sizeof(float), who, path);
    return close_streamed(f, rc, who, path);
}

int tsdf_save_bin(tsdf_volume *v, const char *path)
{
    const char *who = "tsdf_save_bin";
    if (!v || !path) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    int rc = bind_device(v);
    if (rc) return rc;
    mesh_files::OutFile f(path, "wb");
    mesh_files::write_bin_header(f, v->cfg);
    if (f.good()) rc = stream_device_to_file(v, f.get(), v->d_tsdf, (size_t)v->geo.n_vox * sizeof(float), who, path);
    return close_streamed(f, rc, who, path);
}

// ---------------------------------------------------------------------------------------------
// checkpoint / resume (the reference only ever writes: ref src/tsdf.cu:114-132; nothing reads a .bin back)
// ---------------------------------------------------------------------------------------------
int tsdf_load_bin(tsdf_volume *v, const char *path)
{
    if (!v || !path) return fail(TSDF_ERR_INVALID, "tsdf_load_bin: NULL argument");
    const tsdf_config &c = v->cfg;
    const int nz = c.z_end - c.z_begin;
    std::vector<float> host;
    {
        InFile f(path);
        if (!f.fp) return fail(TSDF_ERR_IO, "tsdf_load_bin: cannot open %s", path);
        host.resize((size_t)(v->geo.n_vox > 0 ? v->geo.n_vox : 1));
        float hdr[8];
        const bool ok = f.read(hdr, sizeof(float), 8) && hdr[0] == (float)c.dim_x && hdr[1] == (float)c.dim_y && hdr[2] == (float)nz &&
                        f.read(host.data(), sizeof(float), (size_t)v->geo.n_vox);
        if (!ok) return fail(TSDF_ERR_IO, "tsdf_load_bin: %s is not a %dx%dx%d TSDF dump", path, c.dim_x, c.dim_y, nz);
    }
    return tsdf_upload(v, host.data(), nullptr);   // weights are not in the reference's format
}

int tsdf_save_state(tsdf_volume *v, const char *path)
{
    const char *who = "tsdf_save_state";
    if (!v || !path) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    int rc = bind_device(v);
    if (rc) return rc;
    mesh_files::OutFile f(path, "wb");
    f.write(kStateMagic, 1, 8);
    f.write(&v->cfg, sizeof(tsdf_config), 1);
    if (f.good()) rc = stream_device_to_file(v, f.get(), v->d_tsdf, (size_t)v->geo.n_vox * sizeof(float), who, path);
    if (f.good() && rc == TSDF_OK) rc = stream_device_to_file(v, f.get(), v->d_weight, (size_t)v->geo.n_vox * sizeof(float), who, path);
    return close_streamed(f, rc, who, path);
}

int tsdf_load_state(tsdf_volume *v, const char *path)
{
    if (!v || !path) return fail(TSDF_ERR_INVALID, "tsdf_load_state: NULL argument");
    std::vector<float> t, w;
    {
        InFile f(path);
        if (!f.fp) return fail(TSDF_ERR_IO, "tsdf_load_state: cannot open %s", path);
        t.resize((size_t)(v->geo.n_vox > 0 ? v->geo.n_vox : 1));
        w.resize(t.size());
        char magic[8];
        tsdf_config c;
        const bool ok = f.read(magic, 1, 8) && std::memcmp(magic, kStateMagic, 8) == 0 && f.read(&c, sizeof c, 1) &&
                        c.dim_x == v->cfg.dim_x && c.dim_y == v->cfg.dim_y && c.dim_z == v->cfg.dim_z &&
                        c.z_begin == v->cfg.z_begin && c.z_end == v->cfg.z_end &&
                        f.read(t.data(), sizeof(float), (size_t)v->geo.n_vox) && f.read(w.data(), sizeof(float), (size_t)v->geo.n_vox);
        if (!ok) return fail(TSDF_ERR_IO, "tsdf_load_state: %s does not hold the state of this slab", path);
    }
    return tsdf_upload(v, t.data(), w.data());
}

}  // extern "C"
