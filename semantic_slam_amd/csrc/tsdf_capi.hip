// tsdf_capi.hip -- implementation of include/tsdf_hip.h (libtsdf_hip.so).  Handles, integration, labels and colour are here;
// batches, raycasting, tracking, merging, registration, extents, association, segmentation and lidar scans each in a
// tsdf_<feature>_host.hip.h (the last eight beside their kernels), extraction, the file writers and the checkpoint calls in
// tsdf_extract_host.hip.h (the file formats themselves in mesh_files.h, host-only), the group in tsdf_group.hip.h and
// include/tsdf_hip_diag.h in tsdf_diag.hip.h, all included at the end (one translation unit).
//
// One handle = one z-slab of the voxel grid resident in HBM on one device + one HIP stream.
// Host work per frame is the 4x4 pose composition (pose_math.h) and one kernel launch; the
// depth frame is staged through a small ring of pinned buffers so the caller's pointer can be
// released as soon as tsdf_integrate returns (ref: the reference's blocking cudaMemcpy of the
// caller's buffer, src/tsdf.cu:162).
//
// There is no CPU fallback: without a HIP device every compute entry point fails with
// TSDF_ERR_NO_DEVICE / TSDF_ERR_HIP.
#include "../../include/tsdf_hip.h"
#include "../../include/tsdf_hip_diag.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pose_math.h"
#include "host_derive.h"
#include "launch_geometry.h"
#include "scan_ground_tables.h"
#include "host_copy.h"
#include "hip_owned.h"
#include "frame_store.h"
#include "tsdf_kernels.hip.h"
#include "tsdf_multiframe.hip.h"
#include "tsdf_labels.hip.h"
#include "tsdf_colour.hip.h"
#include "tsdf_extract.hip.h"
#include "tsdf_raycast.hip.h"
#include "tsdf_track.hip.h"
#include "tsdf_batch_track.hip.h"
#include "tsdf_photo.hip.h"
#include "tsdf_fuse.hip.h"
#include "tsdf_fuse_carry.hip.h"
#include "tsdf_align.hip.h"
#include "tsdf_extent.hip.h"
#include "tsdf_associate.hip.h"
#include "tsdf_segment.hip.h"
#include "tsdf_scan.hip.h"
#include "tsdf_scan_fill.hip.h"
#include "tsdf_scan_ground.hip.h"
#include "tsdf_scan_track.hip.h"
#ifdef TSDF_EXPERIMENTS
#include "tsdf_experiments.hip.h"
#endif

using namespace hip_owned;   // DevPtr, HostPtr, Event, Stream and their allocation helpers

namespace {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// HIP_TRY_OR(undo, expr): on failure, return undo(code) -- undo puts right what the function has queued so far
#define HIP_TRY_OR(undo, expr)                                                                 \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return undo(fail(TSDF_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                     \
                             hipGetErrorString(_e), __FILE__, __LINE__));                      \
    } while (0)
#define HIP_TRY(expr) HIP_TRY_OR(, expr)

constexpr int kStageSlots = 3;

// The measurement build (-DTSDF_EXPERIMENTS, `make experiments`) adds the kernel variants of tsdf_experiments.hip.h.
#ifdef TSDF_EXPERIMENTS
constexpr bool kExperiments = true;
#else
constexpr bool kExperiments = false;
#endif

// Volume accesses of the brick kernels are ordinary (temporal) loads and stores, not the non-temporal ones of the row-shaped
// kernels: a brick's row piece is 32 bytes (two lanes), the four x-neighbours a workgroup takes make up a 128-byte line between
// them, and only with the line kept in L2 do their pieces leave as ONE memory request.  With the nt hint every piece went out
// alone: PMC WRITE_SIZE 1 064 MB per 512^3 launch for 537 MB of weights.  Same box, nt -> temporal: the all-free-space launch
// 0.0160 -> 0.0126 ms per frame, S-surf 512^3 0.0387 -> 0.0370, fr3 trajectory 1024^3 0.186 -> 0.178, S-surf 200^3 0.0077 -> 0.0072.
#ifndef TSDF_BRICK_NT
#define TSDF_BRICK_NT 0
#endif
constexpr bool kBrickNT = TSDF_BRICK_NT != 0;
// one launch's counter block: the sharded counters / list heads, then the frames' table for classify_patch
constexpr size_t kClaimBlockBytes = (tsdfk::kCounterBytes + sizeof(tsdfk::ClassPoseTable) + 255) / 256 * 256;
// How classify_brick_list deals super-bricks to the 64 sub-lists (tsdf_multiframe.hip.h, list_bucket): 0 = hashed, 1 = the XCD
// by image-row wedges.
#ifndef TSDF_WEDGE_MODE
#define TSDF_WEDGE_MODE 0
#endif
constexpr int kWedgeMode = TSDF_WEDGE_MODE;

}  // namespace

// What projecting a lidar scan needs on a device (tsdf_scan_host.hip.h), held by a tsdf_scanner and by every handle that has
// been given a scan; allocated on first use.  keys: one 64-bit key per pixel, all zero between calls (scan_resolve leaves
// them so; keys_clean is false from the splat's launch until the resolve's, so a call that failed in between costs the next
// one a clear).  The points' pinned block and its copy in HBM grow with the scan; pts_read, recorded behind the kernel that
// read them, is what the next call waits for before it refills or regrows either.
struct ScanStage {
    DevBuf<unsigned long long> d_keys;
    bool keys_clean = false;
    DevBuf<float4> d_pts;
    HostBuf<float4> h_pts;
    Event pts_read;
    bool pts_in_use = false;
};

// What marking a scan's ground needs on a device (tsdf_scan_ground_host.hip.h), held like a ScanStage and beside one, whose
// points it reads; allocated at the first call that marks, the grid's parts again when n_rings / n_columns grow.  keys: one
// 64-bit key per cell of the spherical image, all zero between calls (cleared behind ground_mark; keys_clean as in ScanStage).
// tables: T | C | S of `params`, in HBM and pinned, rebuilt when a call brings other parameters.  cells: one per point.
// counts: one word per workgroup of the counting kernels, with its pinned mirror.  Whatever regrows or refills any of this
// first waits for the ScanStage's pts_read, recorded behind the last kernel of a call.
struct ScanGroundStage {
    tsdf_scan_ground_params params = {};
    bool have_tables = false;
    tsdf_host::ScanGroundTables tables;
    DevBuf<unsigned long long> d_keys;
    bool keys_clean = false;
    DevBuf<float> d_tables;
    HostBuf<float> h_tables;
    DevBuf<int8_t> d_state;
    DevBuf<int32_t> d_winner;
    DevBuf<uint32_t> d_cells;
    DevBuf<uint8_t> d_flags;
    DevBuf<uint32_t> d_counts;
    HostBuf<char> h_out;             // what tsdf_scan_mark_ground brings back: states | winners | flags | counts
};

struct tsdf_volume {
    tsdf_config cfg = {};
    float base2world_inv[16] = {};
    float last_cam2base[16] = {};
    // the slab's geometry and the layout of its brick work list (launch_geometry.h): set at creation and again wherever the
    // wavefront brick changes (set_brick); every launch takes its grids and buffer sizes from here
    tsdf_host::SlabGeometry geo;
    tsdf_host::WorkListLayout work;
    DevPtr<float> d_tsdf;
    DevPtr<float> d_weight;
    Stream own_stream;
    hipStream_t stream = nullptr;   // the stream work is queued on (own_stream unless overridden)
    // Staging and deferral memory is not the handle's: pinned frames, frame / mask slots in HBM and depth tile tables come from
    // the store all handles of this device and image size share (frame_store.h) and go back to it by stream order.
    tsdf_store::FrameStore *store = nullptr;
    // the H2D copy of a frame runs on its own stream and overlaps the previous frame's kernel; the kernel waits for it
    hipStream_t copy_stream = nullptr;   // the store's
    Event flush_done[2];              // recorded on `stream` after every launch that read store slots: what they are released after;
    int flush_parity = 0;             // two, used in turn, so that a slot of pass k is not held until pass k + 1 has run as well
    // Deferred integration of host frames (tsdf_integrate): the reference reads results back only in its destructor
    // (ref: src/tsdf.cu:101-104) and this library only at download / extraction / save, so the frames of successive
    // calls are collected -- copied into a pool in HBM, poses composed at call time -- and applied defer_n at a time as
    // ONE fused, classified sequence launch; every entry point that observes or changes the volume flushes first.
    int defer_n = tsdfk::kMaxFramesPerLaunch;   // frames per deferred launch (<= 1: every call launches)
    Event pend_copied;
    int pend_count = 0;
    int pend_slot[tsdfk::kMaxFramesPerLaunch] = {}, pend_mask_slot[tsdfk::kMaxFramesPerLaunch] = {};   // store slots of the collected frames (-1: none)
    const float *pend_depth[tsdfk::kMaxFramesPerLaunch] = {};
    struct tsdf_batch *owner = nullptr;         // the batch this handle is a member of (its collected frames come first), or null
    struct tsdf_group *group_owner = nullptr;   // the group this handle is a slab of (likewise), or null
    bool in_flush = false;
    float pend_c2b[16 * tsdfk::kMaxFramesPerLaunch] = {};
    const uint8_t *pend_mask[tsdfk::kMaxFramesPerLaunch] = {};   // instance masks of collected masked frames (in the store's mask slots)
    int variant = 0;
    int sweep_parity = 0;    // direction of the next integrate_tile sweep (flips every launch; a performance hint only)
#ifdef TSDF_EXPERIMENTS
    // per-launch frame blocks of integrate_multi: pinned host ring -> device ring (allocated on first use)
    StageRing<Staged<tsdfk::FramePose>, kStageSlots> frames;
#endif
    // per-voxel label fusion (allocated by tsdf_labels_enable)
    DevPtr<uint16_t> d_label;
    DevPtr<float> d_fp, d_bp;
    float prob_thd = 0.0f;
    // per-voxel colour (allocated by tsdf_colour_enable): packed 0x00BBGGRR; staging of the RGB frames of tsdf_integrate_rgbd
    DevPtr<uint32_t> d_colour;
    StageRing<Staged<uint8_t>, kStageSlots> rgb;
    // free-space summary (one word per 256-voxel row segment), see tsdf_kernels.hip.h
    DevPtr<uint32_t> d_flags;
    tsdf_host::SummaryRecord summary;   // what the host knows of the words; every weight-writing launch asks it first (summary_before)
#ifdef TSDF_EXPERIMENTS
    DevBuf<unsigned int> d_super;    // per super-brick frame words of the current fused brick launch (classify_superbricks)
#endif
    DevBuf<uint4> d_work;        // work list of the current fused brick launch: {brick, slice group, free frames, skipped frames}
                                 // per live brick (classify_brick_list); capacity = every brick of the slab, once per list parity
    // optional diagnostic counters (tsdf_shortcut_stats)
    DevPtr<unsigned int> d_shortcut_stats;
    // adaptive use of the classification: claims of the last classifying launch, read back without blocking
    DevPtr<unsigned long long> d_claims;   // TWO counter blocks (+ frame table each), one per list parity
    HostPtr<unsigned long long> h_claims;
    Event claims_done;
    // A sequence call's launches are pipelined: the pre-pass of launch k + 1 (tile tables, classify_brick_list: small grids, 11 % of
    // a 512^3 S-surf launch, reading only the frames and the poses) runs on pre_stream beside launch k's Integrate kernel.  Two work
    // lists, two counter blocks, two table slots (list_parity); pre_done[p]: pre-pass of parity p queued on pre_stream; list_free[p]:
    // the Integrate kernel that read parity p's list has been queued on the handle's stream; seq_ready: a sequence's inputs.
    Stream pre_stream, rb_stream;   // rb_stream: the counters' read-back of a pipelined launch
    int rb_parity = -1;             // parity of the block the read-back in flight on rb_stream reads, or -1
    Event pre_done[2], list_free[2], seq_ready;
    int list_parity = 0;
    bool list_used[2] = {false, false};
    bool pipeline_ok = false;       // sequence calls are pipelined (tsdf_host::pipelines)
    bool claims_pending = false, claims_known = false;
    double claims_total = 0.0;      // workgroup-frames of the launch the pending read-back belongs to
    double claim_fraction = 0.0;    // claimed / total of the last launch that was read back
    int launches_unclassified = 0;  // since the last classifying launch
    // scratch for surface extraction (allocated on first use)
    DevBuf<char> d_scratch;
    // class of every workgroup of a one-frame masked launch (classify_workgroups), grown on demand
    DevBuf<uint8_t> d_wg_class;
    // output list of the extraction passes (points / vertices / triangles), grown on demand and kept
    DevBuf<char> d_list;
    // tracking (tsdf_track*), allocated on first use and grown with the image: the model render (depth | normal), the partial
    // rows of an association pass and the pose state, in one block; the state's pinned host copy
    DevBuf<char> d_track;
    HostPtr<tsdfk::TrackState> h_track;
    // photometric tracking (tsdf_track_rgbd*, tsdf_render_intensity), allocated on first use and grown with the image: the staged
    // host frame (depth | rgb | mask), the live and model intensity pyramids, the photometric partial rows and state in one
    // block; its pinned mirror (depth | rgb | mask | state), free again when a call returns
    DevBuf<char> d_photo;
    HostBuf<char> h_photo;
    // merging (tsdf_fuse_volume* with this handle as the destination), allocated on first use, all or none: the eight counts
    // (four of the merge, four of the labels carried: tsdf_fuse_volume_carry) in HBM and pinned; src_ready is recorded on the source's stream before the kernel, done on this handle's stream after it
    DevPtr<unsigned long long> d_fuse;
    HostPtr<unsigned long long> h_fuse;
    Event fuse_src_ready, fuse_done;
    // registration (tsdf_align_* with this handle as the destination), allocated on first use, all or none: the partial rows of
    // a pass and the pose state in one block of HBM, the state's pinned copy, and the two events of the merge's order; no size
    // of either volume enters it, so one handle aligns against sources of any size in turn
    DevPtr<char> d_align;
    HostPtr<tsdfk::TrackState> h_align;
    Event align_src_ready, align_done;
    // extent (tsdf_volume_extent), allocated on first use, both or neither: the record and behind it one partial record per
    // workgroup of the launch in HBM (the slab's dims fix their number); the record's pinned host copy
    DevPtr<unsigned long long> d_extent;
    HostPtr<unsigned long long> h_extent;
    // lidar scans (tsdf_integrate_scan), allocated on first use: a handle that never sees a scan allocates nothing
    ScanStage scan;
    ScanGroundStage ground;          // ... and the ground marking in front of it (tsdf_integrate_scan_ground), likewise
    // tracking a scan (tsdf_scan_track*), allocated on first use: the partial rows of a pass and the pose state in one block
    // of HBM and the state's pinned copy (no size of the scan enters them; the points go through `scan`), and the points'
    // flags in HBM and pinned, grown with the scan at the first call that brings flags
    DevBuf<char> d_scan_track;
    HostPtr<tsdfk::TrackState> h_scan_track;
    DevBuf<uint8_t> d_scan_flags;
    HostBuf<uint8_t> h_scan_flags;
};

using tsdf_host::kBatchSideStreams;

// Many volumes integrated by one launch per frame (include/tsdf_hip.h, tsdf_batch_*).
struct tsdf_batch {
    int device = 0;
    std::vector<tsdf_volume *> vols;
    Stream stream;
    // per-frame parameter blocks: pinned host ring -> device ring
    struct FrameBlocks { Staged<tsdfk::IntegrateParams> params; Staged<tsdfk::FramePose> poses; };
    StageRing<FrameBlocks, kStageSlots> blocks;
    DevPtr<int2> d_slice_map;
    int total_slices = 0, max_blocks = 0;
    DevPtr<int2> d_group_map;    // {object, slice group}: the brick launches' z index (a brick spans brick_s slices)
    int total_groups = 0;
    std::vector<int> group_s;    // the brick_s of every member the group map was built with
    // per-object depth tile tables of the current frame and the class of every workgroup of the launch
    DevPtr<float2> d_tiles;
    size_t tiles_per_object = 0;
    DevPtr<uint8_t> d_wg_class;
    DevBuf<uint8_t> d_brick_class;   // class per wavefront brick of the launch (classify_bricks_batched), on first use
    // Deferred integration of a batch of large members (tsdf_batch_integrate_device): frames are collected in HBM -- the
    // depth image once, every member's mask beside it -- and applied by ONE fused launch per member per 32 frames
    // (the volume then moves once per 32 frames instead of once per frame); flushed by anything that observes a member.
    DevPtr<float> d_depth_pool;              // kMaxFramesPerLaunch frames
    DevPtr<uint8_t> d_mask_pool;             // kMaxFramesPerLaunch x members masks
    std::vector<float> pend_c2b;             // [member][frame][16], composed at collection time
    std::vector<const uint8_t *> pend_mask;  // [member][frame], null = the member's frame has no mask
    int pend_count = 0;
    bool in_flush = false;
    // the members' fused launches of a flush are independent of each other: they go out on a few side streams (forked
    // from and joined back into the batch's stream by events), so one member's tail and table kernels overlap the next
    // member's launch
    Stream side[kBatchSideStreams];
    Event side_done[kBatchSideStreams];
    Event collected;
    // the members as tsdf_batch_raycast_device's kernel reads them: pinned host block -> HBM (allocated on first use); the host
    // block is refilled only after the copy out of it has run: a ring of one slot
    StageRing<Staged<tsdfk::RayVolume>, 1> ray;
    // association (tsdf_batch_associate), allocated on first use and grown with the image and the count block: the render
    // (member | depth) and the counts in HBM; the counts' pinned host copy
    DevBuf<char> d_assoc;
    HostBuf<uint32_t> h_assoc;
    // joint tracking (tsdf_batch_track*), allocated on first use and grown with the image and the members: the render (depth,
    // normal, member), its depth with the members that are out zeroed, the partial rows of both reductions, the state, the
    // member systems and member_use in HBM; the pinned mirror of state, systems and member_use
    DevBuf<char> d_track;
    HostBuf<char> h_track;
    // extents (tsdf_batch_extents), allocated on first use, all or none: one record per member and behind them one partial
    // record per workgroup of the launch in HBM; the records' pinned host copy; the members as the kernels read them (filled
    // and copied once: a batch's members do not change)
    DevPtr<unsigned long long> d_extent;
    HostPtr<unsigned long long> h_extent;
    Staged<tsdfk::ExtentVolume> extent_vols;
    int extent_blocks = 0;       // workgroups per slice of that launch
};

namespace {

int flush_pending(tsdf_volume *v);
int batch_flush(tsdf_batch *b);
int group_flush(tsdf_group *g);   // tsdf_group.hip.h
int batch_collect(tsdf_batch *b, const float *depth_dev, const uint8_t *const *masks_dev, const float cam2world[16]);

// Every entry point starts here: make the handle's device current and, unless the caller is the collecting call itself,
// apply the host frames tsdf_integrate has collected (deferred integration, see struct tsdf_volume).
int bind_device(tsdf_volume *v, bool flush = true)
{
    HIP_TRY(hipSetDevice(v->cfg.device));
    if (v->owner && !v->in_flush) {   // frames its batch has collected were given first
        int rc = batch_flush(v->owner);
        if (rc) return rc;
    }
    if (v->group_owner && !v->in_flush) {   // likewise the frames its group has collected (a slab handle borrowed with tsdf_group_volume)
        int rc = group_flush(v->group_owner);
        if (rc) return rc;
    }
    if (flush && v->pend_count > 0 && !v->in_flush) return flush_pending(v);
    return TSDF_OK;
}

// ---- the shared store (frame_store.h) -----------------------------------------------------------------------------
// One slot of the store while a call of this handle holds it, move-only like the owners of hip_owned.h.  The call that has
// queued the slot's last reader gives it back (release, release_after) or hands it to the collected frames (hand_over); a
// call that returns early does neither, and the destructor gives the slot back behind everything the call has queued.
class StoreSlot {
public:
    StoreSlot() = default;
    StoreSlot(StoreSlot &&o) noexcept : v_(o.v_), c_(o.c_), dev_(o.dev_), idx_(std::exchange(o.idx_, -1)) {}
    StoreSlot &operator=(StoreSlot &&) = delete;
    // Still held, i.e. a failure path: the handle's stream waits for what is queued on the copy stream, and the slot goes back
    // after flush_done recorded behind that.  Should one of these calls fail as well, the slot stays held until tsdf_destroy.
    ~StoreSlot()
    {
        if (idx_ < 0) return;
        if (hipEventRecord(v_->pend_copied, v_->copy_stream) == hipSuccess && hipStreamWaitEvent(v_->stream, v_->pend_copied, 0) == hipSuccess)
            (void)release_all(v_, c_, &idx_, 1);
    }
    // A slot of class c whose first access is queued on `first_user`.  When the store is at its soft cap and every slot is
    // held by collecting handles, this handle applies what IT has collected (never another handle's: that one may be in use
    // on another thread) and asks again.
    int take(tsdf_volume *v, tsdf_store::SlotClass *c, hipStream_t first_user)
    {
        v_ = v; c_ = c;
        hipError_t e = tsdf_store::slot_acquire(v->store, c, v, first_user, false, &idx_, &dev_);
        if (e == hipSuccess && idx_ < 0) {
            if (v->pend_count > 0 && !v->in_flush) {
                int rc = flush_pending(v);
                if (rc) return rc;
            }
            e = tsdf_store::slot_acquire(v->store, c, v, first_user, true, &idx_, &dev_);
        }
        if (e != hipSuccess) return fail(TSDF_ERR_HIP, "frame store%s: %s", c == &v->store->tables ? " (tile tables)" : "", hipGetErrorString(e));
        return TSDF_OK;
    }
    template <typename T> T *as() const { return idx_ < 0 ? nullptr : static_cast<T *>(dev_); }
    // everything queued on the handle's stream so far has read the slot (nothing to do for a holder that is empty)
    int release()
    {
        const hipError_t e = idx_ < 0 ? hipSuccess : release_all(v_, c_, &idx_, 1);
        return e == hipSuccess ? TSDF_OK : fail(TSDF_ERR_HIP, "frame store: hipEventRecord failed: %s", hipGetErrorString(e));
    }
    // the slot's last reader sits on another stream, in front of *evt (an event of this handle)
    void release_after(const Event *evt)
    {
        tsdf_store::slots_release_after(v_->store, c_, &idx_, 1, evt, v_);
        idx_ = -1;
    }
    // the collected frames own the slot from here on (pend_slot[] / pend_mask_slot[], until flush_pending); -1: there is none
    int hand_over() { return std::exchange(idx_, -1); }
    // Slots that were handed over, or a holder's own: they go back after flush_done, recorded now on the handle's stream.
    static hipError_t release_all(tsdf_volume *v, tsdf_store::SlotClass *c, int *idx, int n)
    {
        const Event *evt = &v->flush_done[v->flush_parity];
        const hipError_t e = hipEventRecord(*evt, v->stream);
        if (e != hipSuccess) return e;
        tsdf_store::slots_release_after(v->store, c, idx, n, evt, v);
        std::fill(idx, idx + n, -1);
        return hipSuccess;
    }
private:
    tsdf_volume *v_ = nullptr;
    tsdf_store::SlotClass *c_ = nullptr;
    void *dev_ = nullptr;
    int idx_ = -1;
};

// the pass (a flush of collected frames, or one one-kernel-per-call frame) is queued: the next one records the other event
void store_next_pass(tsdf_volume *v) { v->flush_parity ^= 1; }

// The wavefront brick of classified launches and the library's choice of it: host arithmetic only (host_derive.h; also behind
// tsdf_default_brick_shape, which needs no device).
using tsdf_host::brick_shape_ok;

void choose_brick_for(const tsdf_config &c, int &bq, int &br, int &bs)
{
#ifdef TSDF_EXPERIMENTS
    if (const char *e = std::getenv("TSDF_BRICK3D")) {      // A/B knob of the measurement build: "q,r,s" (the product: tsdf_set_brick_shape)
        int q = 0, r = 0, sl = 0;
        if (c.dim_x % 4 == 0 && std::sscanf(e, "%d,%d,%d", &q, &r, &sl) == 3 && brick_shape_ok(c, q, r, sl)) {
            bq = q; br = r; bs = sl;
            return;
        }
    }
#endif
    tsdf_host::choose_brick_default(c, bq, br, bs);
}

dim3 to_dim3(const tsdf_host::Grid3 &g) { return dim3(g.x, g.y, g.z); }

// The handle's wavefront brick (q = 0: none), and with it the brick view of its geometry and its work list's layout.
void set_brick(tsdf_volume *v, int q, int r, int s)
{
    int wedge_mode = kWedgeMode;
#ifdef TSDF_EXPERIMENTS
    if (const char *e = std::getenv("TSDF_WEDGE_MODE")) wedge_mode = std::atoi(e);     // A/B knob of the measurement build
#endif
    v->geo = tsdf_host::slab_geometry(v->cfg, v->geo.tile, v->geo.fine, q, r, s);
    v->work = tsdf_host::work_list_layout(v->cfg, v->geo, wedge_mode);
}

void choose_brick(tsdf_volume *v)
{
    int q, r, s;
    choose_brick_for(v->cfg, q, r, s);
    set_brick(v, q, r, s);
}

tsdfk::IntegrateParams make_params(const tsdf_volume *v, const float *depth_dev,
                                   const uint8_t *mask_dev, const float *c2b, int vx)
{
    const tsdf_config &c = v->cfg;
    tsdfk::IntegrateParams p;
    p.depth = depth_dev;
    p.mask = mask_dev;
    p.tsdf = v->d_tsdf;
    p.weight = v->d_weight;
    p.fx = c.cam_K[0]; p.fy = c.cam_K[4]; p.cx = c.cam_K[2]; p.cy = c.cam_K[5];
    p.rx0 = c2b[0]; p.rx1 = c2b[4]; p.rx2 = c2b[8];
    p.ry0 = c2b[1]; p.ry1 = c2b[5]; p.ry2 = c2b[9];
    p.rz0 = c2b[2]; p.rz1 = c2b[6]; p.rz2 = c2b[10];
    p.tx = c2b[3]; p.ty = c2b[7]; p.tz = c2b[11];
    p.ox = c.origin[0]; p.oy = c.origin[1]; p.oz = c.origin[2];
    p.vs = c.voxel_size; p.trunc = c.trunc_margin; p.max_depth = c.max_depth;
    const tsdf_host::SlabGeometry &geo = v->geo;
    p.dim_x = geo.dim_x; p.dim_y = geo.dim_y;
    p.nz = geo.nz; p.z_begin = c.z_begin;
    p.H = c.im_height; p.W = c.im_width;
    p.xgroups = geo.xgroups(vx);
    p.flags = v->d_flags;
    p.nseg = geo.nseg;
    p.quads_per_row = geo.quads_per_row;
    p.quads_per_slice = geo.quads_per_slice;
    p.chunks_per_slice = geo.chunks_per_slice;
    // brick view (tsdf_multiframe.hip.h, BRICK): the volume's wavefront brick, chosen at creation (choose_brick)
    p.brick_q = geo.brick_q; p.brick_r = geo.brick_r; p.brick_s = geo.brick_s;
    p.bricks_per_group = geo.bricks_per_group; p.brick_groups = geo.brick_groups;
    p.brick_q_magic = geo.brick_q_magic; p.brick_per_magic = geo.brick_per_magic;
    // guards of the exact shortcuts and margins of the box claims: host_derive.h (derive_projection_guards)
    const tsdf_host::ProjectionGuards g = tsdf_host::derive_projection_guards(c, c2b);
    p.cz_margin = g.cz_margin; p.fast_ok = g.fast_ok; p.trunc_fast = g.trunc_fast;
    p.cz_short = g.cz_short; p.cz_pad = g.cz_pad;
    p.tiles_w = geo.tiles_w; p.tiles_h = geo.tiles_h;
    p.tile_inv = geo.tile_inv;
    p.fine = nullptr;                // set by the launch that builds the fine tables
    p.fine_w = geo.fine_w; p.fine_h = geo.fine_h;
    p.px_margin_u = g.px_margin_u; p.px_margin_v = g.px_margin_v;
    p.shortcut_stats = v->d_shortcut_stats;
    p.claim_counter = nullptr;
    p.wg_class = nullptr;
    return p;
}

// The per-frame block of the fused / flat kernels from a full parameter set.
void pose_from_params(tsdfk::FramePose &fp, const tsdfk::IntegrateParams &q)
{
    fp.depth = q.depth; fp.mask = q.mask;
    fp.rx0 = q.rx0; fp.rx1 = q.rx1; fp.rx2 = q.rx2;
    fp.ry0 = q.ry0; fp.ry1 = q.ry1; fp.ry2 = q.ry2;
    fp.rz0 = q.rz0; fp.rz1 = q.rz1; fp.rz2 = q.rz2;
    fp.tx = q.tx; fp.ty = q.ty; fp.tz = q.tz;
    fp.fast_ok = q.fast_ok; fp.cz_margin = q.cz_margin;
    fp.label_im = nullptr; fp.score_im = nullptr;
    fp.tiles = nullptr;
    fp.cz_short = q.cz_short; fp.cz_pad = q.cz_pad;
}

// The launch policy (tile tables, pipelining, classification, sweeps, batches) is host arithmetic in host_derive.h, which
// restates the kernels' constants it needs.
static_assert(tsdf_host::kMaxFramesPerLaunch == tsdfk::kMaxFramesPerLaunch, "host_derive.h: kMaxFramesPerLaunch");
static_assert(tsdf_host::kTileLdsEntries == tsdfk::kTileLdsEntries, "host_derive.h: kTileLdsEntries");
static_assert(tsdf_host::kFineTile == tsdfk::kFineTile, "host_derive.h: kFineTile");
static_assert(tsdf_host::kFineLevels == tsdfk::kFineLevels, "host_derive.h: kFineLevels");
static_assert(tsdf_host::kListBuckets == tsdfk::kListBuckets, "launch_geometry.h: kListBuckets");
static_assert(tsdf_host::kSuperBX == tsdfk::kSuperBX && tsdf_host::kSuperBY == tsdfk::kSuperBY && tsdf_host::kSuperBZ == tsdfk::kSuperBZ &&
              tsdf_host::kSuperBricks == tsdfk::kSuperBricks, "launch_geometry.h: kSuperBX / BY / BZ");
using tsdf_host::tiles_fit;

// Depth tile tables (summary + sparse table, tsdf_multiframe.hip.h) of n images depth[i] x mask[i] into tables[i], queued
// on `stream`; two small launches per 32 images.
// fine (may be null; 8-pixel tiles only): the launch's fine tables (p.fine_w x p.fine_h tiles of 4 pixels, nine levels per frame),
// built by the same two launches whenever the coarse tables fit tile_sparse_table's LDS, else by two more.
// beside_a_launch: the kernels are queued on a side stream while another launch fills the chip -- the sparse-table kernel then takes
// 256-thread workgroups (a 1024-thread one needs sixteen free wavefront slots on ONE compute unit at once and waited for the other
// launch to drain: 634 us instead of 20).
int build_tile_tables(hipStream_t stream, const tsdf_config &c, const tsdfk::IntegrateParams &p, const float *const *depth,
                      const uint8_t *const *masks, int n, float2 *tables, unsigned long long *zero_me = nullptr, float2 *fine = nullptr,
                      bool beside_a_launch = false)
{
    const size_t per = tsdf_host::tile_table_elems(p.tiles_w, p.tiles_h);
    if (fine != nullptr && (p.tile_inv != 0.125f || n > tsdfk::kMaxFramesPerLaunch))
        return fail(TSDF_ERR_INVALID, "build_tile_tables: fine tables go with 8-pixel tiles, one launch at a time");
    for (int k = 0; k < n; k += tsdfk::kMaxFramesPerLaunch) {
        const int m = std::min(tsdfk::kMaxFramesPerLaunch, n - k);
        tsdfk::TileSummaryParams tp;
        for (int f = 0; f < tsdfk::kMaxFramesPerLaunch; ++f) {
            tp.depth[f] = depth[k + (f < m ? f : 0)];
            tp.mask[f] = masks ? masks[k + (f < m ? f : 0)] : nullptr;
        }
        tp.tiles = tables + (size_t)k * per;
        tp.H = c.im_height; tp.W = c.im_width; tp.tiles_w = p.tiles_w; tp.tiles_h = p.tiles_h;
        tp.max_depth = c.max_depth;
        tp.fine = fine; tp.fw = p.fine_w; tp.fh = p.fine_h;      // level (0, 0) of the fine tables in the same pass (8-pixel tiles)
        // whole-row reads: one wavefront per strip of 64 pixels (four 16-pixel tiles or eight 8-pixel ones)
        if (p.tile_inv == 0.0625f)
            hipLaunchKernelGGL(tsdfk::depth_tile_summary<16>, to_dim3(tsdf_host::grid_tile_strips(p.tiles_w, p.tiles_h, 16, m)), dim3(64, 4), 0, stream, tp);
        else
            hipLaunchKernelGGL(tsdfk::depth_tile_summary<8>, to_dim3(tsdf_host::grid_tile_strips(p.tiles_w, p.tiles_h, 8, m)), dim3(64, 4), 0, stream, tp);
        if (p.tiles_w * p.tiles_h <= tsdfk::kTileLdsEntries) {
            // (1024 threads when the frame has thousands of tiles: each of the kernel's ~12 barrier-separated passes visits every tile)
            const unsigned threads = (p.tiles_w * p.tiles_h > 2048 && !beside_a_launch) ? 1024 : 256;
            const unsigned fine_blocks = fine ? ((unsigned)(p.fine_w * p.fine_h) + threads - 1) / threads : 0u;   // the fine tables' upper levels ride along
            hipLaunchKernelGGL(tsdfk::tile_sparse_table, dim3((unsigned)tsdf_host::tile_levels(p.tiles_w) + fine_blocks, m), dim3(threads), 0, stream, tp.tiles,
                               p.tiles_w, p.tiles_h, k == 0 ? zero_me : (unsigned long long *)nullptr, fine, p.fine_w, p.fine_h);
        } else {
            if (zero_me && k == 0) HIP_TRY(hipMemsetAsync(zero_me, 0, tsdfk::kCounterBytes, stream));
            hipLaunchKernelGGL(tsdfk::tile_sparse_table_scan, dim3((unsigned)tsdf_host::tile_levels(p.tiles_w), m), dim3(256), 0, stream, tp.tiles,
                               p.tiles_w, p.tiles_h);
            if (fine)
                hipLaunchKernelGGL(tsdfk::fine_tile_levels, dim3((unsigned)((p.fine_w * p.fine_h + 255) / 256), m), dim3(256), 0, stream, fine, p.fine_w, p.fine_h);
        }
    }
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

// Ahead of every launch that writes weights: what the launch keeps of the summary words decides what is queued first on the
// handle's stream (launch_geometry.h, SummaryRecord).  A kernel that keeps nothing must not leave stale words behind, so they
// are zeroed, unless they are known to be; one that keeps bits 0 and 1 only does not know the weight runs integrate_tile keeps,
// so they are forgotten: one small pass over the words (2 MB at 512^3), once, since no such launch sets a run again.  A failed
// call leaves the record as it was, but for "known zero", which goes.
int summary_before(tsdf_volume *v, tsdf_host::Keeps keeps)
{
    tsdf_host::SummaryRecord next = v->summary;
    const tsdf_host::SummaryAction act = next.before_launch(keeps);
    v->summary.known_zero = false;
    if (act == tsdf_host::SummaryAction::Zero && v->geo.n_flags != 0)
        HIP_TRY(hipMemsetAsync(v->d_flags, 0, v->geo.n_flags * sizeof(uint32_t), v->stream));
    if (act == tsdf_host::SummaryAction::ForgetRuns && v->geo.n_flags != 0) {
        hipLaunchKernelGGL(tsdfk::forget_runs, to_dim3(tsdf_host::grid_summary_words(v->geo)), dim3(256), 0, v->stream, v->d_flags.get(), v->geo.n_flags);
        HIP_TRY(hipGetLastError());
    }
    v->summary = next;
    return TSDF_OK;
}

// The same with wavefront bricks (rows that divide into them): class per brick, then the brick kernel.  Queues the launch.
int launch_masked_bricks(tsdf_volume *v, tsdfk::IntegrateParams &p)
{
    int rcf = summary_before(v, tsdf_host::Keeps::Bits);
    if (rcf) return rcf;
    const tsdf_host::BrickGrid bg = tsdf_host::brick_grid(v->geo);   // workgroups of four bricks x slice groups, and the class table's bytes
    StoreSlot table;      // the frame's depth tile tables, first written on the handle's stream
    int rc0 = table.take(v, &v->store->tables, v->stream);
    if (rc0) return rc0;
    HIP_TRY(v->d_wg_class.ensure(bg.class_elems));
    const float *d = p.depth;
    const uint8_t *m = p.mask;
    int rc = build_tile_tables(v->stream, v->cfg, p, &d, &m, 1, table.as<float2>());
    if (rc) return rc;
    tsdfk::FramePose pose;
    pose_from_params(pose, p);
    pose.tiles = table.as<float2>();
    hipLaunchKernelGGL(tsdfk::classify_bricks, dim3((unsigned)((bg.class_elems + 255) / 256)), dim3(256), 0, v->stream, p, pose,
                       v->d_wg_class, (int)bg.grid.x, (int)bg.grid.z);
    p.wg_class = v->d_wg_class;
    hipLaunchKernelGGL((tsdfk::integrate_single_bricks<kBrickNT>), to_dim3(bg.grid), dim3(64, 4, 1), 0, v->stream, p, pose);
    HIP_TRY(hipGetLastError());
    return table.release();
}

int rebuild_summary(tsdf_volume *v)
{
    if (v->geo.n_flags == 0 || v->geo.n_vox == 0) return TSDF_OK;
    hipLaunchKernelGGL(tsdfk::recompute_flags, to_dim3(tsdf_host::grid_recompute_flags(v->geo)), dim3(64, 4, 1), 0, v->stream, v->d_tsdf,
                       v->d_weight, v->d_flags, v->geo.quads_per_slice, v->geo.chunks_per_slice);
    HIP_TRY(hipGetLastError());
    v->summary.after_rebuild();
    return TSDF_OK;
}

int launch_multi(tsdf_volume *v, const float *const *depth_dev, const uint8_t *const *masks_dev, const float *c2b, int n,
                 const uint16_t *const *label_ims = nullptr, const float *const *score_ims = nullptr, hipEvent_t inputs_ready = nullptr);

// Claimed share of the launch whose counter block has arrived in h_claims: (free << 32 | skipped) per bucket, added up.
double claims_read_back(const tsdf_volume *v)
{
    double claimed = 0.0;
    for (int b = 0; b < tsdfk::kListBuckets; ++b) {
        const unsigned long long w = v->h_claims[(size_t)b * (tsdfk::kBucketStride / sizeof(unsigned long long)) + 1];
        claimed += (double)(w >> 32) + (double)(w & 0xffffffffull);
    }
    return v->claims_total > 0 ? claimed / v->claims_total : 0.0;
}

#ifdef TSDF_EXPERIMENTS
tsdf_host::Variant experiment_variant(int variant);
void experiment_adjust(const tsdf_volume *v, bool labels, bool *classify, int *z_fastest);
int launch_integrate_experiment(tsdf_volume *v, const float *depth_dev, const uint8_t *mask_dev, const float *c2b);
int launch_multi_experiment(tsdf_volume *v, tsdfk::MultiParamsInline &mi, const float *const *depth_dev, const uint8_t *const *masks_dev,
                            const float *c2b, int n, bool labels, bool any_mask, bool classify, bool *handled, double *claims_total);
bool experiment_takes_multi(const tsdf_volume *v, bool labels, bool classify);
int launch_single_experiment(tsdf_volume *v, tsdfk::IntegrateParams &common, tsdfk::FramePose &pose, const float *depth_dev,
                             const float *c2b, bool *handled);
#endif

// What a kernel variant number means (tsdf_host::decode_variant), the measurement build's own numbers first.  A handle holds
// only numbers its build knows (tsdf_set_kernel_variant).
tsdf_host::Variant variant_of(int variant)
{
#ifdef TSDF_EXPERIMENTS
    const tsdf_host::Variant e = experiment_variant(variant);
    if (e.known) return e;
#endif
    return tsdf_host::decode_variant(variant);
}

// Direction and Infinity Cache window of a one-frame sweep (tsdf_host::sweep_window): the handle's launches alternate.
void set_sweep(tsdf_volume *v, tsdfk::IntegrateParams &p)
{
    int64_t window = tsdf_host::kWindowBytes;
    bool forward_only = false;
#ifdef TSDF_EXPERIMENTS
    if (const char *e = std::getenv("TSDF_MALL_WINDOW_MB")) window = (int64_t)std::atoi(e) << 20;    // A/B knobs of the measurement build
    forward_only = std::getenv("TSDF_SWEEP_FORWARD") && std::atoi(std::getenv("TSDF_SWEEP_FORWARD")) != 0;
    p.head_plain_loads = std::getenv("TSDF_HEAD_PLAIN_LOADS") && std::atoi(std::getenv("TSDF_HEAD_PLAIN_LOADS")) != 0;
#endif
    p.sweep_reverse = forward_only ? 0 : v->sweep_parity;
    v->sweep_parity ^= 1;
    const tsdf_host::SweepWindow w = tsdf_host::sweep_window(p.nz, p.dim_x, p.dim_y, window, p.sweep_reverse != 0);
    p.cache_lo = w.cache_lo;
    p.cache_hi = w.cache_hi;
}

// Queue one Integrate launch.  Shapes are validated at tsdf_create, so the grid covers exactly
// the slab and every access stays inside the two allocations.
int launch_integrate(tsdf_volume *v, const float *depth_dev, const uint8_t *mask_dev,
                     const float *c2b)
{
    const tsdf_host::SlabGeometry &geo = v->geo;
    if (geo.nz == 0) return TSDF_OK;  // empty slab: nothing to do
    std::memcpy(v->last_cam2base, c2b, sizeof v->last_cam2base);
#ifdef TSDF_EXPERIMENTS
    if (geo.quad_rows && (v->variant == 2 || (v->variant >= 16 && !mask_dev) ||
                          (v->variant == 11 && mask_dev && !geo.flat && tiles_fit(geo.tiles_w, geo.tiles_h))))
        return launch_integrate_experiment(v, depth_dev, mask_dev, c2b);
#endif
    // which kernel, and what it keeps of the summary words (launch_geometry.h)
    const tsdf_host::OneFrame one = tsdf_host::one_frame(geo, variant_of(v->variant), mask_dev != nullptr, tiles_fit(geo.tiles_w, geo.tiles_h));
    if (one.kernel == tsdf_host::OneFrameKernel::Scalar) {
        // rows that are not 16-byte aligned (or the scalar kernel asked for): one voxel per lane
        int rc = summary_before(v, one.keeps);
        if (rc) return rc;
        const tsdfk::IntegrateParams p = make_params(v, depth_dev, mask_dev, c2b, 1);
        const dim3 block(64, 4, 1), grid = to_dim3(tsdf_host::grid_scalar_rows(geo));
        if (mask_dev) hipLaunchKernelGGL((tsdfk::integrate_scalar<true>), grid, block, 0, v->stream, p);
        else hipLaunchKernelGGL((tsdfk::integrate_scalar<false>), grid, block, 0, v->stream, p);
        HIP_TRY(hipGetLastError());
        return TSDF_OK;
    }
    if (geo.flat) {
        // rows that are not a multiple of 256 voxels: the flat mapping (every lane busy, summary kept)
        return launch_multi(v, &depth_dev, mask_dev ? &mask_dev : nullptr, c2b, 1);
    }
    tsdfk::IntegrateParams p = make_params(v, depth_dev, mask_dev, c2b, 4);
    // per-object volumes see their instance only, so the bricks the tile table of depth x mask proves untouched are told to
    // leave (variant 7: never; small launches: not worth the three small dispatches ahead of it): per wavefront brick, skipped
    // by rows, slices and columns
    if (one.kernel == tsdf_host::OneFrameKernel::MaskedBricks) return launch_masked_bricks(v, p);
    int rc = summary_before(v, one.keeps);   // integrate_tile keeps the free-space summary up to date, and the weight runs
    if (rc) return rc;
    const dim3 block(64, 4, 1), grid = to_dim3(tsdf_host::grid_quad_rows(geo, 8));
    set_sweep(v, p);
    if (mask_dev) hipLaunchKernelGGL((tsdfk::integrate_tile<2, true>), grid, block, 0, v->stream, p);
    else hipLaunchKernelGGL((tsdfk::integrate_tile<2, false>), grid, block, 0, v->stream, p);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

void compose_cam2base(const tsdf_volume *v, const float *cam2world, float *c2b)
{
    tsdf_host::multiply_matrix(v->base2world_inv, cam2world, c2b);  // ref: src/tsdf.cu:142
}

// n frames (n <= kMaxFramesPerLaunch) in one pass over the slab.  c2b: n x 16 relative poses.
// label_ims / score_ims (both or neither): the frames' label evidence is fused in the same pass (LABELS kernels).
// inputs_ready (may be null): an event after which the frames (and masks) may be read from ANY stream -- a sequence call records it
// once on the handle's stream at its start; with it the pre-pass of a classified launch runs on the handle's side stream, i.e.
// beside the previous launch's Integrate kernel (see tsdf_volume::pre_stream).  Null: everything on the handle's stream.
int launch_multi(tsdf_volume *v, const float *const *depth_dev, const uint8_t *const *masks_dev,
                 const float *c2b, int n, const uint16_t *const *label_ims, const float *const *score_ims, hipEvent_t inputs_ready)
{
    const tsdf_config &c = v->cfg;
    const tsdf_host::SlabGeometry &geo = v->geo;
    if (geo.nz == 0 || n == 0) return TSDF_OK;
    {
        int rc = summary_before(v, tsdf_host::Keeps::Bits);    // every kernel below keeps bits 0 and 1 of the summary only
        if (rc) return rc;
    }
    auto fill_pose = [&](tsdfk::FramePose &fp, int f) {
        pose_from_params(fp, make_params(v, depth_dev[f], masks_dev ? masks_dev[f] : nullptr, c2b + 16 * f, 4));
        fp.label_im = label_ims ? label_ims[f] : nullptr;
        fp.score_im = label_ims ? score_ims[f] : nullptr;
    };
    const dim3 block(64, 4, 1);
    if (n == 1 && !label_ims) {   // pose by value: nothing to stage
        tsdfk::IntegrateParams common = make_params(v, depth_dev[0], nullptr, c2b, 4);
        tsdfk::FramePose pose;
        fill_pose(pose, 0);
        std::memcpy(v->last_cam2base, c2b, sizeof v->last_cam2base);
#ifdef TSDF_EXPERIMENTS
        {
            bool handled = false;
            int rc = launch_single_experiment(v, common, pose, depth_dev[0], c2b, &handled);
            if (rc || handled) return rc;
        }
#endif
        const tsdf_host::OneFrame one = tsdf_host::one_frame(geo, variant_of(v->variant), pose.mask != nullptr, tiles_fit(geo.tiles_w, geo.tiles_h));
        if (geo.flat && one.kernel == tsdf_host::OneFrameKernel::MaskedBricks) {
            // one masked frame into a flat-mapped volume (the reference's 200^3 object grids), large enough to repay a class table
            tsdfk::IntegrateParams cp = make_params(v, depth_dev[0], pose.mask, c2b, 4);
            return launch_masked_bricks(v, cp);
        }
        if (geo.flat)
            hipLaunchKernelGGL((tsdfk::integrate_multi_single<true, true>), to_dim3(tsdf_host::grid_flat(geo)), block, 0, v->stream, common, pose);
        else
            hipLaunchKernelGGL((tsdfk::integrate_multi_single<true, false>), to_dim3(tsdf_host::grid_quad_rows(geo, 4)), block, 0, v->stream, common, pose);
        HIP_TRY(hipGetLastError());
        return TSDF_OK;
    }
    std::memcpy(v->last_cam2base, c2b + 16 * (n - 1), sizeof v->last_cam2base);
    // the frame blocks travel in the kernarg: nothing is staged on the stream ahead of the launch
    tsdfk::MultiParamsInline mi;
    mi.common = make_params(v, depth_dev[0], nullptr, c2b, 4);
    mi.n_frames = n;
    for (int f = 0; f < n; ++f) fill_pose(mi.frames[f], f);
    for (int f = n; f < tsdfk::kMaxFramesPerLaunch; ++f) mi.frames[f] = mi.frames[0];
    mi.labels.label = v->d_label; mi.labels.fp = v->d_fp; mi.labels.bp = v->d_bp; mi.labels.prob_thd = v->prob_thd;
    bool any_mask = false;
    for (int f = 0; f < n && masks_dev; ++f) any_mask = any_mask || masks_dev[f] != nullptr;

    // Patch classification: tables of at most 4 MiB per frame, used while they pay
    // (tsdf_host::classify_fused).  The count is read back asynchronously: a decision never waits for the GPU.
    if (v->claims_pending) {
        const hipError_t qe = hipEventQuery(v->claims_done);
        if (qe == hipSuccess) {
            v->claim_fraction = claims_read_back(v);
            v->claims_pending = false;
            v->claims_known = true;
        } else if (qe == hipErrorNotReady) {
            (void)hipGetLastError();   // "not ready" is an answer, not an error to be found by a later check
        } else {
            // a real failure: forget the stale count (the next launch classifies and counts afresh) and report it
            v->claims_pending = false;
            v->claims_known = false;
            (void)hipGetLastError();
            return fail(TSDF_ERR_HIP, "claims read-back: hipEventQuery failed: %s", hipGetErrorString(qe));
        }
    }
    // classified launches run over wavefront bricks (every grid whose rows are a multiple of 4 voxels has a brick view)
    bool classify = tiles_fit(mi.common.tiles_w, mi.common.tiles_h) && mi.common.brick_q > 0;
    mi.z_fastest = 2;
#ifdef TSDF_EXPERIMENTS
    experiment_adjust(v, label_ims != nullptr, &classify, &mi.z_fastest);
#endif
    classify = classify && tsdf_host::classify_fused(variant_of(v->variant).classify, v->claims_known, v->claim_fraction,
                                                     v->launches_unclassified);
    v->launches_unclassified = classify ? 0 : v->launches_unclassified + 1;
    const bool count_claims = classify && !v->claims_pending;
    if (classify && !v->d_claims) {
        // the launch's counter block (tsdf_multiframe.hip.h, kListBuckets): per bucket the lengths of its brick sub-list and
        // its share of the claims, cleared by the table kernel below; behind it the frames' table for classify_patch
        // all or none: a launch that finds d_claims set relies on the host mirror and the events being there too
        DevPtr<unsigned long long> dc;
        HostPtr<unsigned long long> hc;
        Event ev[6];
        hipError_t e = dev_alloc(dc, 2 * kClaimBlockBytes);
        if (e == hipSuccess) e = host_alloc(hc, tsdfk::kCounterBytes, hipHostMallocDefault);
        for (int i = 0; i < 6 && e == hipSuccess; ++i) e = event_create(ev[i]);
        if (e != hipSuccess) return fail(TSDF_ERR_HIP, "claim counters: %s", hipGetErrorString(e));
        v->d_claims = std::move(dc); v->h_claims = std::move(hc); v->claims_done = std::move(ev[0]);
        v->pre_done[0] = std::move(ev[1]); v->pre_done[1] = std::move(ev[2]); v->list_free[0] = std::move(ev[3]);
        v->list_free[1] = std::move(ev[4]); v->seq_ready = std::move(ev[5]);
    }
    // this launch's parity: its counter block, its half of the work list, its table slot
    // (slabs too large to be pipelined -- see pipeline_ok -- keep one list and one parity)
    const int P = v->pipeline_ok ? v->list_parity : 0;
    unsigned long long *const claims_p = classify ? v->d_claims + (size_t)P * (kClaimBlockBytes / sizeof(unsigned long long)) : nullptr;
    bool pipelined = classify && inputs_ready != nullptr && v->pipeline_ok;
#ifdef TSDF_EXPERIMENTS
    if (!tsdf_host::decode_variant(v->variant).known || std::getenv("TSDF_NO_PIPELINE")) pipelined = false;   // the measurement build's own kernels run on the handle's stream
#endif
    if (pipelined && !v->pre_stream) {
        // the two side streams of a pipelined handle, at its first pipelined launch (a stream costs about 2 MiB of device memory:
        // the per-object handles of a scene, which are fed frame by frame and never pipeline, do not pay for them)
        Stream a, b;
        int prio = 0;
#ifdef TSDF_EXPERIMENTS
        if (std::getenv("TSDF_PRE_PRIORITY")) { int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi); prio = hi; }   // (numerically lower = higher)
#endif
        // (default priority: with the highest one the pre-pass finished 180 us into the launch beside it, which then ran 65 us longer)
        hipError_t e = hipStreamCreateWithPriority(a.put(), hipStreamNonBlocking, prio);
        if (e == hipSuccess) e = stream_create(b);
        if (e != hipSuccess) return fail(TSDF_ERR_HIP, "side streams: %s", hipGetErrorString(e));
        v->pre_stream = std::move(a); v->rb_stream = std::move(b);
    }
    // the brick work list (below), sized and allocated before anything is queued on the side stream
    bool listed = classify;
#ifdef TSDF_EXPERIMENTS
    listed = listed && !experiment_takes_multi(v, label_ims != nullptr, classify);
#endif
    const tsdf_host::WorkListLayout &wl = v->work;
    const size_t lists = v->pipeline_ok ? 2 : 1;     // one list per parity
    if (listed) {
        // A pre-pass compacts the bricks some frame may touch into a work list and the launch runs one wavefront per entry.
        if (!wl.fits) return fail(TSDF_ERR_INVALID, "fused launch: %lld bricks exceed the work list's 32-bit index", (long long)wl.total);
        if (!v->d_work.fits(lists * (size_t)wl.total) && v->d_work) {      // (a list in flight on either stream is done before its memory goes)
            if (v->pre_stream) HIP_TRY(hipStreamSynchronize(v->pre_stream));
            HIP_TRY(hipStreamSynchronize(v->stream));
        }
        HIP_TRY(v->d_work.ensure(lists * (size_t)wl.total));
    }
    const hipStream_t ps = pipelined ? v->pre_stream : v->stream;
    // a failure from here on joins the side stream back into the handle's stream (the table slot then goes back behind the join)
    StoreSlot table;
    auto unwind = [&](int code) {
        if (pipelined && hipEventRecord(v->pre_done[P], ps) == hipSuccess) (void)hipStreamWaitEvent(v->stream, v->pre_done[P], 0);
        return code;
    };
    if (pipelined) {
        HIP_TRY_OR(unwind, hipStreamWaitEvent(ps, inputs_ready, 0));
        if (v->list_used[P]) HIP_TRY_OR(unwind, hipStreamWaitEvent(ps, v->list_free[P], 0));   // the Integrate kernel two launches back has read this parity's buffers
        if (v->rb_parity == P) HIP_TRY_OR(unwind, hipStreamWaitEvent(ps, v->claims_done, 0)); // ... and its counters have left for the host
    } else if (classify && v->rb_parity == P) {
        HIP_TRY(hipStreamWaitEvent(v->stream, v->claims_done, 0));
    }
    if (count_claims) mi.common.claim_counter = claims_p + 1;   // bucket 0's claims word (the pre-pass adds the bucket's offset)
    if (classify) {
        // depth tile tables of the n frames (two small launches), then the kernels that consult them
        const tsdf_host::TableSlotLayout slot = tsdf_host::table_slot_layout(c, geo.tile, geo.fine);
        int rc = table.take(v, &v->store->tables, ps);
        if (rc) return unwind(rc);
        float2 *const tiles = table.as<float2>();
        float2 *fine = geo.fine ? tiles + slot.fine_begin : nullptr;   // behind the coarse tables, in the same slot
        rc = build_tile_tables(ps, c, mi.common, depth_dev, masks_dev, n, tiles, claims_p, fine, pipelined);
        if (rc) return unwind(rc);
        mi.common.fine = fine;
        for (int f = 0; f < n; ++f) mi.frames[f].tiles = tiles + (size_t)f * slot.coarse_elems;
        for (int f = n; f < tsdfk::kMaxFramesPerLaunch; ++f) mi.frames[f] = mi.frames[0];
    }
    double claims_total = 0.0;
    bool launched = false;
#ifdef TSDF_EXPERIMENTS
    {
        int rc = launch_multi_experiment(v, mi, depth_dev, masks_dev, c2b, n, label_ims != nullptr, any_mask, classify, &launched, &claims_total);
        if (rc) return unwind(rc);
    }
#endif
    if (listed) {
        const int64_t per_group = (int64_t)geo.brick_groups * geo.bricks_per_group;
        uint4 *const work_p = v->d_work + (size_t)P * (v->d_work.capacity() / lists);
        tsdfk::BrickListParams bl;
        bl.list = work_p;
        bl.counters = reinterpret_cast<unsigned char *>(claims_p);
        bl.bucket_cap = (unsigned int)wl.bucket_cap;
        bl.poses = reinterpret_cast<tsdfk::ClassPoseTable *>(bl.counters + tsdfk::kCounterBytes);
        bl.nsx = wl.nsx; bl.nsy = wl.nsy; bl.nsz = wl.nsz;
        bl.wedge_mode = wl.wedge_mode; bl.wedge_oy = wl.wedge_oy; bl.wedge_oz = wl.wedge_oz;
        bl.super_h = wl.super_h; bl.super_d = wl.super_d; bl.fy_px = wl.fy_px;
        hipLaunchKernelGGL(tsdfk::classify_brick_list, to_dim3(tsdf_host::grid_classify_list(wl)), block, 0, ps, mi, bl);
        if (pipelined) {       // the Integrate kernel waits for its pre-pass; everything before it on the handle's stream does not
            HIP_TRY_OR(unwind, hipEventRecord(v->pre_done[P], ps));
            HIP_TRY_OR(unwind, hipStreamWaitEvent(v->stream, v->pre_done[P], 0));
        }
        const dim3 grid_list = to_dim3(tsdf_host::grid_brick_list(wl));   // front groups + back groups of every sub-list
        const uint4 *wlist = work_p;
        const unsigned char *wc = bl.counters;
        const tsdfk::ClassPoseTable *wp = bl.poses;
        if (label_ims)
            hipLaunchKernelGGL((tsdfk::integrate_brick_list<kBrickNT, true, false>), grid_list, block, 0, v->stream, mi, wlist, wc, bl.bucket_cap, wp);
        else if (any_mask)
            hipLaunchKernelGGL((tsdfk::integrate_brick_list<kBrickNT, false, true>), grid_list, block, 0, v->stream, mi, wlist, wc, bl.bucket_cap, wp);
        else
            hipLaunchKernelGGL((tsdfk::integrate_brick_list<kBrickNT, false, false>), grid_list, block, 0, v->stream, mi, wlist, wc, bl.bucket_cap, wp);
        claims_total = (double)per_group * geo.nz_groups * n;   // wavefront-frames = bricks x frames
        launched = true;
    }
    if (!launched) {
        // The per-voxel fused kernel.  Workgroup order: slices fastest -- consecutively dispatched workgroups share their
        // (x, y) footprint, i.e. the windows of the launch's up to 32 depth frames (39 MB, more than the L2s hold) they gather
        // from (512^3 S-surf with a depth frame per pose: 0.1325 -> 0.1148 ms per frame; 1024^3 fr3 trajectory 0.529 ->
        // 0.376) -- and rotated, (z + x + y) mod n, so that a slice group's workgroups are spread over all eight XCDs.
        tsdf_host::Grid3 g0 = geo.flat ? tsdf_host::grid_flat(geo) : tsdf_host::grid_quad_rows(geo, 4);
        if (g0.x > 65535u) mi.z_fastest = 0;   // slices fastest puts the blocks of a slice into grid.z: 65535 at most (then: memory order)
        if (mi.z_fastest) std::swap(g0.x, g0.z);
        const dim3 grid = to_dim3(g0);
        if (label_ims && geo.flat)
            hipLaunchKernelGGL((tsdfk::integrate_multi_inline<1, true, true, true, false>), grid, block, 0, v->stream, mi);
        else if (label_ims)
            hipLaunchKernelGGL((tsdfk::integrate_multi_inline<1, true, false, true, false>), grid, block, 0, v->stream, mi);
        else if (geo.flat && any_mask)
            hipLaunchKernelGGL((tsdfk::integrate_multi_inline<1, true, true, false, true>), grid, block, 0, v->stream, mi);
        else if (geo.flat)
            hipLaunchKernelGGL((tsdfk::integrate_multi_inline<1, true, true, false, false>), grid, block, 0, v->stream, mi);
        else if (any_mask)
            hipLaunchKernelGGL((tsdfk::integrate_multi_inline<1, true, false, false, true>), grid, block, 0, v->stream, mi);
        else
            hipLaunchKernelGGL((tsdfk::integrate_multi_inline<1, true, false, false, false>), grid, block, 0, v->stream, mi);
    }
    if (listed) {
        // after this parity's Integrate kernel: its buffers may be rebuilt (a pre-pass on the side stream waits for it)
        HIP_TRY_OR(unwind, hipEventRecord(v->list_free[P], v->stream));
        v->list_used[P] = true;
        v->list_parity = v->pipeline_ok ? P ^ 1 : 0;
    }
    if (count_claims) {
        // the counters' way to the host: on a stream of its own when the launch is pipelined (behind list_free, i.e. after the
        // Integrate kernel), so that the copy sits neither between two Integrate kernels on the handle's stream nor in front of the
        // next pre-pass on the side stream; the pre-pass that clears this block again waits for it (rb_done)
        v->claims_total = claims_total;
        const hipStream_t rs = (pipelined && listed) ? v->rb_stream : v->stream;
        if (rs != v->stream) HIP_TRY_OR(unwind, hipStreamWaitEvent(rs, v->list_free[P], 0));
        HIP_TRY_OR(unwind, hipMemcpyAsync(v->h_claims, claims_p, tsdfk::kCounterBytes, hipMemcpyDeviceToHost, rs));
        HIP_TRY_OR(unwind, hipEventRecord(v->claims_done, rs));
        v->claims_pending = true;
        v->rb_parity = (rs != v->stream) ? P : -1;
    }
    HIP_TRY_OR(unwind, hipGetLastError());
    const int rc_end = table.release();
    // (pipelined) the next launch's table slot is released after the OTHER of the handle's two events: a slot taken two launches
    // later then waits for this launch's Integrate kernel, not for the one in between
    if (pipelined) store_next_pass(v);
    return rc_end;
}

// Frames applied per pass over the slab.  Per frame the time is a + b / n: the weights are read and written,
// the summary word and the voxel coordinates set up, the launch filled and drained once per pass (b), and
// 512^3 measures 0.156 / 0.141 / 0.136 / 0.132 ms per frame at n = 4 / 8 / 16 / 32 (a = 0.129).
int frames_per_launch(const tsdf_volume *)
{
    return tsdfk::kMaxFramesPerLaunch;
}

bool can_fuse(const tsdf_volume *v) { return variant_of(v->variant).fuses && v->geo.quad_rows; }

// A sequence of frames: fused frames_per_launch() at a time when the default kernel is selected.
// label_ims / score_ims (both or neither): as launch_multi takes them; such a sequence is always fused.
int integrate_frames(tsdf_volume *v, const float *const *depth_dev, const uint8_t *const *masks_dev,
                     const float *cam2world, int n_frames, const uint16_t *const *label_ims = nullptr,
                     const float *const *score_ims = nullptr)
{
    const bool fuse = label_ims != nullptr || can_fuse(v);
    int rc = TSDF_OK;
    // every frame of the sequence is readable once what precedes this call on the handle's stream has run: one event for all its
    // launches, so that their pre-passes may run beside the launches ahead of them (launch_multi, inputs_ready)
    bool seq_event = false;
    for (int k = 0; k < n_frames && rc == TSDF_OK;) {
        const int n = fuse ? std::min(frames_per_launch(v), n_frames - k) : 1;
        float c2b[16 * tsdfk::kMaxFramesPerLaunch];
        for (int i = 0; i < n; ++i) compose_cam2base(v, cam2world + 16 * (k + i), c2b + 16 * i);
        if (fuse && !seq_event && v->seq_ready && v->pipeline_ok && n_frames > n) {
            HIP_TRY(hipEventRecord(v->seq_ready, v->stream));
            seq_event = true;
        }
        if (fuse) rc = launch_multi(v, depth_dev + k, masks_dev ? masks_dev + k : nullptr, c2b, n, label_ims ? label_ims + k : nullptr,
                                    label_ims ? score_ims + k : nullptr, seq_event ? v->seq_ready : nullptr);
        else rc = launch_integrate(v, depth_dev[k], masks_dev ? masks_dev[k] : nullptr, c2b);
        k += n;
    }
    return rc;
}

// n collected frames (c2b: their n x 16 composed poses; masks[f] null: frame f has no mask): one fused launch, or with a single
// frame (or a variant that does not fuse) the one-frame kernels.  *some_mask (may be null): some frame has a mask.
int apply_collected(tsdf_volume *v, const float *const *depth, const uint8_t *const *masks, const float *c2b, int n, bool *some_mask = nullptr)
{
    bool any_mask = false;
    for (int f = 0; f < n; ++f) any_mask = any_mask || masks[f] != nullptr;
    if (some_mask) *some_mask = any_mask;
    if (can_fuse(v) && n > 1) return launch_multi(v, depth, any_mask ? masks : nullptr, c2b, n);
    int rc = TSDF_OK;
    for (int f = 0; f < n && rc == TSDF_OK; ++f) rc = launch_integrate(v, depth[f], masks[f], c2b + 16 * f);
    return rc;
}

// Apply the collected frames (poses already composed) as one sequence; their store slots go back after the launch.
int flush_pending(tsdf_volume *v)
{
    if (v->pend_count == 0 || v->in_flush) return TSDF_OK;
    v->in_flush = true;
    const int n = v->pend_count;
    v->pend_count = 0;
    int rc = TSDF_OK;
    hipError_t e = hipSetDevice(v->cfg.device);
    // the frames' copies ran in order on the copy stream: one event after the last of them covers all
    if (e == hipSuccess) e = hipEventRecord(v->pend_copied, v->copy_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(v->stream, v->pend_copied, 0);
    if (e == hipSuccess) {
        bool any_mask = false;
        rc = apply_collected(v, v->pend_depth, v->pend_mask, v->pend_c2b, n, &any_mask);
        // whatever the launch returned: kernels it queued on the handle's stream may read the slots, so they go back behind them
        // (and without a word when the launch has failed: its message is the one to report)
        hipError_t re = StoreSlot::release_all(v, &v->store->frames, v->pend_slot, n);
        const hipError_t rm = any_mask ? StoreSlot::release_all(v, &v->store->masks, v->pend_mask_slot, n) : hipSuccess;
        if (re == hipSuccess) re = rm;
        store_next_pass(v);
        if (rc == TSDF_OK && re != hipSuccess) rc = fail(TSDF_ERR_HIP, "deferred integration: hipEventRecord failed: %s", hipGetErrorString(re));
    }
    v->in_flush = false;
    if (e != hipSuccess) return fail(TSDF_ERR_HIP, "deferred integration: %s", hipGetErrorString(e));
    return rc;
}

// Deferred integration, collecting side: the frame in `frame` (and its instance mask in `mask`, which may be empty) joins the
// collected ones, which own both slots from here on, with its pose composed now (or given as the relative pose itself); the
// batch is launched when it is full.
int pool_slot_commit(tsdf_volume *v, StoreSlot &frame, StoreSlot &mask, const float cam2world[16], const float *cam2base = nullptr)
{
    const int slot = v->pend_count;
    v->pend_depth[slot] = frame.as<float>();
    v->pend_mask[slot] = mask.as<uint8_t>();
    v->pend_slot[slot] = frame.hand_over();
    v->pend_mask_slot[slot] = mask.hand_over();
    if (cam2base) std::memcpy(v->pend_c2b + 16 * slot, cam2base, 16 * sizeof(float));
    else compose_cam2base(v, cam2world, v->pend_c2b + 16 * slot);
    std::memcpy(v->last_cam2base, v->pend_c2b + 16 * slot, sizeof v->last_cam2base);
    v->pend_count = slot + 1;
    if (v->pend_count >= std::min(v->defer_n, (int)tsdfk::kMaxFramesPerLaunch)) return flush_pending(v);
    return TSDF_OK;
}

// A device-resident frame (and its instance mask) collected like a host frame: copied device to device into a store slot on
// the handle's stream -- the same ordering the frame's kernel would have had -- so the caller's buffer is free for reuse under
// the stream's order, as before.
int collect_device_frame(tsdf_volume *v, const float *depth_dev, const uint8_t *mask_dev, const float *cam2world,
                         const float *cam2base)
{
    const size_t px = (size_t)v->cfg.im_height * v->cfg.im_width;
    StoreSlot frame, mask;
    int rc = frame.take(v, &v->store->frames, v->stream);   // (may apply the frames collected so far to make room)
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(frame.as<float>(), depth_dev, px * sizeof(float), hipMemcpyDeviceToDevice, v->stream));
    if (mask_dev) {
        rc = mask.take(v, &v->store->masks, v->stream);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(mask.as<uint8_t>(), mask_dev, px, hipMemcpyDeviceToDevice, v->stream));
    }
    return pool_slot_commit(v, frame, mask, cam2world, cam2base);
}

// A device-resident frame from the caller: collected, or launched at once.  Exactly one of cam2world and cam2base is given.
int integrate_device_frame(const char *who, tsdf_volume *v, const float *depth_dev, const uint8_t *mask_dev, bool masked,
                           const float *cam2world, const float *cam2base)
{
    if (!v || !depth_dev || (masked && !mask_dev) || (!cam2world && !cam2base)) return fail(TSDF_ERR_INVALID, "%s: NULL argument", who);
    const bool defer = v->defer_n > 1 && can_fuse(v);
    int rc = bind_device(v, !defer);
    if (rc) return rc;
    if (defer) return collect_device_frame(v, depth_dev, mask_dev, cam2world, cam2base);
    float c2b[16];
    if (cam2world) compose_cam2base(v, cam2world, c2b);
    return launch_integrate(v, depth_dev, mask_dev, cam2world ? c2b : cam2base);
}

// ---- a host frame: staged on the copy stream, then collected or launched -----------------------------------------
// Staging: pinned ring slot -> `frame`, a frame slot of the store, H2D on the copy stream (it overlaps the previous frame's
// kernel).  `fill_host(pinned)` writes the pinned frame; the caller may free its buffer when we return.
template <typename F>
int stage_frame(tsdf_volume *v, size_t bytes, F fill_host, StoreSlot &frame)
{
    int r = -1;
    hipError_t e = tsdf_store::ring_acquire(v->store, &r);
    if (e != hipSuccess) return fail(TSDF_ERR_HIP, "frame store (pinned ring): %s", hipGetErrorString(e));
    fill_host(v->store->ring[r].host);
    int rc = frame.take(v, &v->store->frames, v->copy_stream);
    if (rc) { (void)tsdf_store::ring_release(v->store, r, v->copy_stream); return rc; }
    e = hipMemcpyAsync(frame.as<void>(), v->store->ring[r].host, bytes, hipMemcpyHostToDevice, v->copy_stream);
    const hipError_t e2 = tsdf_store::ring_release(v->store, r, v->copy_stream);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(TSDF_ERR_HIP, "staging copy: %s", hipGetErrorString(e));
    return TSDF_OK;
}

// The same for a raw 16-bit frame (half the bytes of the float frame): staged into a slot of its own and converted on the copy
// stream into `frame`, the one Integrate reads.  pend_copied is recorded behind the conversion, and the raw slot goes back after it.
int stage_frame_u16(tsdf_volume *v, const uint16_t *raw_host, float depth_factor, int row_step, int col_step, StoreSlot &frame)
{
    const size_t px = (size_t)v->cfg.im_height * v->cfg.im_width;
    StoreSlot raw;
    int rc = stage_frame(v, px * sizeof(uint16_t), [&](float *pinned) { tsdf_host::copy_to_pinned(pinned, raw_host, px * sizeof(uint16_t)); }, raw);
    if (rc == TSDF_OK) rc = frame.take(v, &v->store->frames, v->copy_stream);
    if (rc) return rc;
    hipLaunchKernelGGL(tsdfk::depth_u16_to_f32, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, v->copy_stream, raw.as<uint16_t>(),
                       frame.as<float>(), v->cfg.im_height, v->cfg.im_width, 1.0f / depth_factor, row_step,
                       col_step);   // ref: examples/label_instance_rgbd.cpp:99-100 (fp32 reciprocal)
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(v->pend_copied, v->copy_stream));
    raw.release_after(&v->pend_copied);
    return TSDF_OK;
}

// The colour pass of a frame (tsdf_colour.hip.h), queued behind its Integrate launch.
int launch_colour(tsdf_volume *v, const float *depth_dev, const uint8_t *rgb_dev, const float *c2b)
{
    if (v->geo.nz == 0) return TSDF_OK;
    tsdfk::ColourParams cp;
    cp.g = make_params(v, depth_dev, nullptr, c2b, 4);
    cp.rgb = rgb_dev;
    cp.colour = v->d_colour;
    hipLaunchKernelGGL(tsdfk::integrate_colour, to_dim3(tsdf_host::grid_quad_rows(v->geo, 4)), dim3(64, 4, 1), 0, v->stream, cp);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

// The tail of a one-kernel-per-call frame whose copy the handle's stream already waits for: the launch, the colour launch when
// there is an image (rgb_dev), and the slot's release behind them.  A failed launch returns at once: kernels it queued on the
// handle's stream may read the slot, and the holder gives it back behind them.
int launch_staged_frame(tsdf_volume *v, StoreSlot &frame, const float cam2world[16], const uint8_t *rgb_dev = nullptr)
{
    float c2b[16];
    compose_cam2base(v, cam2world, c2b);
    int rc = launch_integrate(v, frame.as<float>(), nullptr, c2b);
    if (rc == TSDF_OK && rgb_dev) rc = launch_colour(v, frame.as<float>(), rgb_dev, c2b);
    if (rc) return rc;
    rc = frame.release();
    store_next_pass(v);
    return rc;
}

// Applying a staged frame.  Deferred: collected, its pose composed now, and launched defer_n at a time (or at the next call that
// observes the volume) as one fused sequence.  Else one kernel per call, which waits for the copy: pend_copied, recorded now on
// the copy stream unless the staging has (copies_marked).
int apply_host_frame(tsdf_volume *v, StoreSlot &frame, const float cam2world[16], bool defer, bool copies_marked, const uint8_t *rgb_dev = nullptr)
{
    StoreSlot no_mask;
    if (defer) return pool_slot_commit(v, frame, no_mask, cam2world);
    if (!copies_marked) HIP_TRY(hipEventRecord(v->pend_copied, v->copy_stream));
    HIP_TRY(hipStreamWaitEvent(v->stream, v->pend_copied, 0));
    return launch_staged_frame(v, frame, cam2world, rgb_dev);
}

int fill(tsdf_volume *v)
{
    if (v->geo.n_vox == 0) return TSDF_OK;
    hipLaunchKernelGGL(tsdfk::fill_grid, to_dim3(tsdf_host::grid_fill(v->geo)), dim3(256), 0, v->stream, v->d_tsdf, v->d_weight, (size_t)v->geo.n_vox);
    HIP_TRY(hipGetLastError());
    if (v->geo.n_flags) {  // every TSDF value is 1: every segment flag is set
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)v->d_flags, (int)tsdf_host::kSummaryFresh, v->geo.n_flags, v->stream));   // ... and every weight is the count 0
        v->summary.after_fill();
    }
    return TSDF_OK;
}

#ifdef TSDF_EXPERIMENTS
#include "tsdf_experiments_host.hip.h"
#endif

}  // namespace

extern "C" {

const char *tsdf_last_error(void) { return g_last_error.c_str(); }

const char *tsdf_version(void)
{
    return kExperiments ? "tsdf_hip 0.3 (gfx950) +experiments" : "tsdf_hip 0.3 (gfx950)";
}

void tsdf_multiply_matrix(const float a[16], const float b[16], float out[16])
{
    tsdf_host::multiply_matrix(a, b, out);
}

int tsdf_invert_matrix(const float m[16], float inv_out[16])
{
    return tsdf_host::invert_matrix(m, inv_out) ? 1 : 0;
}

int tsdf_config_default(tsdf_config *cfg, int32_t im_height, int32_t im_width)
{
    if (!cfg) return fail(TSDF_ERR_INVALID, "tsdf_config_default: cfg is NULL");
    std::memset(cfg, 0, sizeof *cfg);
    cfg->im_height = im_height;
    cfg->im_width = im_width;
    cfg->dim_x = cfg->dim_y = cfg->dim_z = 200;  // ref: include/tsdf.hpp:65-67
    cfg->z_begin = 0;
    cfg->z_end = 200;
    cfg->voxel_size = 0.004f;                    // ref: include/tsdf.hpp:63
    cfg->trunc_margin = cfg->voxel_size * 5;     // ref: include/tsdf.hpp:64
    cfg->max_depth = 6.0f;                       // ref: src/tsdf.cu:46
    const float K[9] = {535.4f, 0, 320.1f, 0, 539.2f, 247.6f, 0, 0, 1};  // ref: include/tsdf.hpp:96
    std::memcpy(cfg->cam_K, K, sizeof K);
    for (int i = 0; i < 4; ++i) cfg->base2world[5 * i] = 1.0f;
    return TSDF_OK;
}

// What tsdf_create refuses in a configuration before it looks for a device (also behind tsdf_extent_regrid: host arithmetic only).
static int config_ok(const tsdf_config *cfg)
{
    using tsdf_host::ConfigLimit;
    switch (tsdf_host::config_limits_ok(*cfg)) {
        case ConfigLimit::Ok: break;
        case ConfigLimit::GridDims:
            return fail(TSDF_ERR_INVALID, "tsdf_create: grid dims must be positive (%d,%d,%d)",
                        cfg->dim_x, cfg->dim_y, cfg->dim_z);
        case ConfigLimit::SlabRange:
            return fail(TSDF_ERR_INVALID, "tsdf_create: slab [%d,%d) outside grid z range [0,%d)",
                        cfg->z_begin, cfg->z_end, cfg->dim_z);
        case ConfigLimit::ImageSize:
            return fail(TSDF_ERR_INVALID, "tsdf_create: bad image size %dx%d", cfg->im_height, cfg->im_width);
        case ConfigLimit::VoxelAndTrunc:
            return fail(TSDF_ERR_INVALID, "tsdf_create: voxel_size and trunc_margin must be > 0");
        case ConfigLimit::LaunchLimits:
            return fail(TSDF_ERR_INVALID, "tsdf_create: slab exceeds launch limits (dim_y <= 262140, slices <= 65535)");
        case ConfigLimit::SliceVoxels:
            return fail(TSDF_ERR_INVALID, "tsdf_create: a slice may hold at most 2^31 voxels (dim_x * dim_y)");
    }
    return TSDF_OK;
}

// tsdf_create, and tsdf_batch_create for its members (batch_member: one table layout for all of them, tsdf_host::tile_edge)
static int create_volume(const tsdf_config *cfg, bool batch_member, tsdf_volume **out)
{
    *out = nullptr;
    int ok = config_ok(cfg);
    if (ok) return ok;

    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return fail(TSDF_ERR_NO_DEVICE, "tsdf_create: no HIP device visible (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= n_dev)
        return fail(TSDF_ERR_INVALID, "tsdf_create: device %d not in [0,%d)", cfg->device, n_dev);

    tsdf_volume *v = new (std::nothrow) tsdf_volume();
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_create: out of host memory");
    v->cfg = *cfg;
    // geometry: the depth tiles (tsdf_host::tile_edge, fine_tables), then the wavefront brick with the views that follow from it
    v->geo.tile = tsdf_host::tile_edge(*cfg, batch_member);
    v->geo.fine = tsdf_host::fine_tables(*cfg, v->geo.tile);
#ifdef TSDF_EXPERIMENTS
    if (const char *e = std::getenv("TSDF_FINE_TILES")) v->geo.fine = v->geo.tile == 8 && std::atoi(e) != 0;   // A/B knob of the measurement build
#endif
    choose_brick(v);
    // ref: src/tsdf.cu:74 -- the inverse stays zero when base2world is singular, silently
    tsdf_host::invert_matrix(cfg->base2world, v->base2world_inv);

    int rc = TSDF_OK;
    auto cleanup = [&](int code) { tsdf_destroy(v); return code; };
    if (hipSetDevice(cfg->device) != hipSuccess)
        return cleanup(fail(TSDF_ERR_HIP, "tsdf_create: hipSetDevice(%d) failed", cfg->device));
    hipError_t e;
    if ((e = stream_create(v->own_stream)) != hipSuccess)
        return cleanup(fail(TSDF_ERR_HIP, "tsdf_create: hipStreamCreate: %s", hipGetErrorString(e)));
    v->stream = v->own_stream;
    size_t bytes = (size_t)(v->geo.n_vox > 0 ? v->geo.n_vox : 1) * sizeof(float);
    if ((e = dev_alloc(v->d_tsdf, bytes)) != hipSuccess ||
        (e = dev_alloc(v->d_weight, bytes)) != hipSuccess)
        return cleanup(fail(TSDF_ERR_HIP, "tsdf_create: hipMalloc of %zu bytes x2: %s", bytes, hipGetErrorString(e)));
    if ((e = dev_alloc(v->d_flags, (v->geo.n_flags ? v->geo.n_flags : 1) * sizeof(uint32_t))) != hipSuccess)
        return cleanup(fail(TSDF_ERR_HIP, "tsdf_create: hipMalloc of the summary: %s", hipGetErrorString(e)));
    // staging, deferral and tile-table memory: the store shared by every handle of this device and image size (nothing is
    // allocated until a frame arrives)
    v->pipeline_ok = tsdf_host::pipelines(*cfg);
#ifdef TSDF_EXPERIMENTS
    if (const char *e = std::getenv("TSDF_PIPELINE")) v->pipeline_ok = std::atoi(e) != 0;   // A/B knob of the measurement build
#endif
    const size_t table_bytes = tsdf_host::launch_table_bytes(*cfg, v->geo.tile, v->geo.fine);
    if ((e = tsdf_store::store_ref(cfg->device, (size_t)cfg->im_height * cfg->im_width, table_bytes, &v->store)) != hipSuccess ||
        (e = event_create(v->flush_done[0])) != hipSuccess ||
        (e = event_create(v->flush_done[1])) != hipSuccess ||
        (e = event_create(v->pend_copied)) != hipSuccess)
        return cleanup(fail(TSDF_ERR_HIP, "tsdf_create: frame store: %s", hipGetErrorString(e)));
    v->copy_stream = v->store->copy_stream;   // the store's: shared by its handles (thread-safe; copies share one PCIe pipe anyway)
    if ((rc = fill(v)) != TSDF_OK) return cleanup(rc);
    *out = v;
    return TSDF_OK;
}

int tsdf_create(const tsdf_config *cfg, tsdf_volume **out)
{
    if (!cfg || !out) return fail(TSDF_ERR_INVALID, "tsdf_create: NULL argument");
    return create_volume(cfg, false, out);
}

int tsdf_destroy(tsdf_volume *v)
{
    if (!v) return TSDF_OK;
    (void)hipSetDevice(v->cfg.device);
    if (v->own_stream) (void)hipStreamSynchronize(v->own_stream);
    if (v->stream && v->stream != v->own_stream) (void)hipStreamSynchronize(v->stream);
    if (v->copy_stream) (void)hipStreamSynchronize(v->copy_stream);
    if (v->pre_stream) (void)hipStreamSynchronize(v->pre_stream);
    if (v->rb_stream) (void)hipStreamSynchronize(v->rb_stream);
    v->pend_count = 0;   // frames collected but never observed: nothing can tell whether they were applied
    if (v->store) {      // (the streams are idle: whatever this handle held, or others were waiting on its events for, is free)
        tsdf_store::slots_drop_owner(v->store, v);   // before the events the store's slots point at (flush_done) go
        tsdf_store::store_unref(v->store);
        v->store = nullptr;
    }
    delete v;            // the owners release the handle's memory, events and streams (its device is current)
    return TSDF_OK;
}

int tsdf_reset(tsdf_volume *v)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_reset: NULL handle");
    int rc = bind_device(v);
    if (rc) return rc;
    return fill(v);
}

int tsdf_integrate(tsdf_volume *v, const float *depth_host, const float cam2world[16])
{
    if (!v || !depth_host || !cam2world) return fail(TSDF_ERR_INVALID, "tsdf_integrate: NULL argument");
    const bool defer = v->defer_n > 1;
    int rc = bind_device(v, !defer);
    if (rc) return rc;
    const size_t img = (size_t)v->cfg.im_height * v->cfg.im_width * sizeof(float);
    StoreSlot frame;
    rc = stage_frame(v, img, [&](float *pinned) { tsdf_host::copy_to_pinned(pinned, depth_host, img); }, frame);
    if (rc) return rc;
    return apply_host_frame(v, frame, cam2world, defer, false);
}

int tsdf_set_deferral(tsdf_volume *v, int32_t n_frames)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_set_deferral: NULL handle");
    if (n_frames < 0 || n_frames > tsdfk::kMaxFramesPerLaunch)
        return fail(TSDF_ERR_INVALID, "tsdf_set_deferral: n_frames must be in [0, %d]", tsdfk::kMaxFramesPerLaunch);
    int rc = bind_device(v);   // applies what has been collected under the old setting
    if (rc) return rc;
    v->defer_n = n_frames;
    return TSDF_OK;
}

int tsdf_convert_depth_u16(tsdf_volume *v, const uint16_t *raw_dev, float *depth_dev, float depth_factor,
                           int32_t row_step, int32_t col_step)
{
    if (!v || !raw_dev || !depth_dev) return fail(TSDF_ERR_INVALID, "tsdf_convert_depth_u16: NULL argument");
    if (!(depth_factor > 0.0f) || row_step < 1 || col_step < 1)
        return fail(TSDF_ERR_INVALID, "tsdf_convert_depth_u16: depth_factor must be > 0 and steps >= 1");
    int rc = bind_device(v);
    if (rc) return rc;
    const int n = v->cfg.im_height * v->cfg.im_width;
    const float scale = 1.0f / depth_factor;  // ref: examples/label_instance_rgbd.cpp:99-100 (fp32 reciprocal)
    hipLaunchKernelGGL(tsdfk::depth_u16_to_f32, dim3((n + 255) / 256), dim3(256), 0, v->stream, raw_dev, depth_dev,
                       v->cfg.im_height, v->cfg.im_width, scale, row_step, col_step);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

int tsdf_integrate_u16(tsdf_volume *v, const uint16_t *raw_host, float depth_factor, int32_t row_step,
                       int32_t col_step, const float cam2world[16])
{
    if (!v || !raw_host || !cam2world) return fail(TSDF_ERR_INVALID, "tsdf_integrate_u16: NULL argument");
    if (!(depth_factor > 0.0f) || row_step < 1 || col_step < 1)
        return fail(TSDF_ERR_INVALID, "tsdf_integrate_u16: depth_factor must be > 0 and steps >= 1");
    const bool defer = v->defer_n > 1;
    int rc = bind_device(v, !defer);
    if (rc) return rc;
    StoreSlot frame;
    rc = stage_frame_u16(v, raw_host, depth_factor, row_step, col_step, frame);
    if (rc) return rc;
    return apply_host_frame(v, frame, cam2world, defer, true);
}

int tsdf_integrate_device(tsdf_volume *v, const float *depth_dev, const float cam2world[16])
{
    return integrate_device_frame("tsdf_integrate_device", v, depth_dev, nullptr, false, cam2world, nullptr);
}

int tsdf_integrate_cam2base(tsdf_volume *v, const float *depth_dev, const float cam2base[16])
{
    return integrate_device_frame("tsdf_integrate_cam2base", v, depth_dev, nullptr, false, nullptr, cam2base);
}

int tsdf_integrate_masked_device(tsdf_volume *v, const float *depth_dev, const uint8_t *mask_dev,
                                 const float cam2world[16])
{
    return integrate_device_frame("tsdf_integrate_masked_device", v, depth_dev, mask_dev, true, cam2world, nullptr);
}

int tsdf_integrate_frames_device(tsdf_volume *v, const float *const *depth_dev, const uint8_t *const *masks_dev,
                                 const float *cam2world, int32_t n_frames)
{
    if (!v || !depth_dev || !cam2world || n_frames < 0)
        return fail(TSDF_ERR_INVALID, "tsdf_integrate_frames_device: bad argument");
    for (int k = 0; k < n_frames; ++k)
        if (!depth_dev[k]) return fail(TSDF_ERR_INVALID, "tsdf_integrate_frames_device: depth_dev[%d] is NULL", k);
    int rc = bind_device(v);
    if (rc) return rc;
    return integrate_frames(v, depth_dev, masks_dev, cam2world, n_frames);
}

int tsdf_integrate_frames_labels_device(tsdf_volume *v, const float *const *depth_dev, const uint16_t *const *label_im_dev,
                                        const float *const *score_im_dev, const float *cam2world, int32_t n_frames)
{
    if (!v || !depth_dev || !label_im_dev || !score_im_dev || !cam2world || n_frames < 0)
        return fail(TSDF_ERR_INVALID, "tsdf_integrate_frames_labels_device: bad argument");
    if (!v->d_label) return fail(TSDF_ERR_INVALID, "tsdf_integrate_frames_labels_device: call tsdf_labels_enable first");
    for (int k = 0; k < n_frames; ++k)
        if (!depth_dev[k] || !label_im_dev[k] || !score_im_dev[k])
            return fail(TSDF_ERR_INVALID, "tsdf_integrate_frames_labels_device: frame %d has a NULL image", k);
    int rc = bind_device(v);
    if (rc) return rc;
    return integrate_frames(v, depth_dev, nullptr, cam2world, n_frames, label_im_dev, score_im_dev);   // (always through launch_multi)
}

int tsdf_sync(tsdf_volume *v)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_sync: NULL handle");
    int rc = bind_device(v);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(v->stream));
    return TSDF_OK;
}

int tsdf_download(tsdf_volume *v, float *tsdf_host, float *weight_host)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_download: NULL handle");
    int rc = bind_device(v);
    if (rc) return rc;
    size_t bytes = (size_t)v->geo.n_vox * sizeof(float);
    HIP_TRY(hipStreamSynchronize(v->stream));
    if (bytes == 0) return TSDF_OK;
    if (tsdf_host) HIP_TRY(hipMemcpy(tsdf_host, v->d_tsdf, bytes, hipMemcpyDeviceToHost));
    if (weight_host) HIP_TRY(hipMemcpy(weight_host, v->d_weight, bytes, hipMemcpyDeviceToHost));
    return TSDF_OK;
}

int tsdf_copy_slices(tsdf_volume *v, int32_t z_local, int32_t n_slices, void *tsdf_dst, void *weight_dst)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_copy_slices: NULL handle");
    const int nz = v->cfg.z_end - v->cfg.z_begin;
    if (z_local < 0 || n_slices < 0 || z_local + n_slices > nz)
        return fail(TSDF_ERR_INVALID, "tsdf_copy_slices: slices [%d,%d) outside the slab's %d", z_local, z_local + n_slices, nz);
    int rc = bind_device(v);
    if (rc) return rc;
    const size_t slice = (size_t)v->cfg.dim_x * v->cfg.dim_y;
    const size_t bytes = slice * (size_t)n_slices * sizeof(float);
    if (bytes == 0) return TSDF_OK;
    if (tsdf_dst) HIP_TRY(hipMemcpyAsync(tsdf_dst, v->d_tsdf + slice * z_local, bytes, hipMemcpyDefault, v->stream));
    if (weight_dst) HIP_TRY(hipMemcpyAsync(weight_dst, v->d_weight + slice * z_local, bytes, hipMemcpyDefault, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    return TSDF_OK;
}

int tsdf_upload(tsdf_volume *v, const float *tsdf_host, const float *weight_host)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_upload: NULL handle");
    int rc = bind_device(v);
    if (rc) return rc;
    size_t bytes = (size_t)v->geo.n_vox * sizeof(float);
    HIP_TRY(hipStreamSynchronize(v->stream));
    if (bytes == 0) return TSDF_OK;
    if (tsdf_host) HIP_TRY(hipMemcpy(v->d_tsdf, tsdf_host, bytes, hipMemcpyHostToDevice));
    if (weight_host) HIP_TRY(hipMemcpy(v->d_weight, weight_host, bytes, hipMemcpyHostToDevice));
    return rebuild_summary(v);
}

int tsdf_refresh_summary(tsdf_volume *v)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_refresh_summary: NULL handle");
    int rc = bind_device(v);
    if (rc) return rc;
    return rebuild_summary(v);
}

int tsdf_device_ptrs(tsdf_volume *v, float **tsdf_dev, float **weight_dev)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_device_ptrs: NULL handle");
    int rc = bind_device(v);   // what the caller reads through the pointers must include every frame handed over so far
    if (rc) return rc;
    if (tsdf_dev) *tsdf_dev = v->d_tsdf;
    if (weight_dev) *weight_dev = v->d_weight;
    return TSDF_OK;
}

int64_t tsdf_slab_voxels(const tsdf_volume *v) { return v ? v->geo.n_vox : 0; }

int tsdf_get_config(const tsdf_volume *v, tsdf_config *out)
{
    if (!v || !out) return fail(TSDF_ERR_INVALID, "tsdf_get_config: NULL argument");
    *out = v->cfg;
    return TSDF_OK;
}

int tsdf_set_stream(tsdf_volume *v, void *hip_stream)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_set_stream: NULL handle");
    int rc = bind_device(v);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(v->stream));  // do not reorder against work already queued
    v->stream = hip_stream ? (hipStream_t)hip_stream : v->own_stream;
    return TSDF_OK;
}

int tsdf_get_stream(tsdf_volume *v, void **hip_stream)
{
    if (!v || !hip_stream) return fail(TSDF_ERR_INVALID, "tsdf_get_stream: NULL argument");
    *hip_stream = (void *)v->stream;
    return TSDF_OK;
}

int tsdf_object_origin(int32_t device, const float *depth_dev, const uint8_t *mask_dev, int32_t im_height,
                       int32_t im_width, const float cam_K[9], float origin_out[3])
{
    if (!depth_dev || !cam_K || !origin_out || im_height <= 0 || im_width <= 0)
        return fail(TSDF_ERR_INVALID, "tsdf_object_origin: bad argument");
    HIP_TRY(hipSetDevice(device));
    // the frame may have been produced on a handle's (non-blocking) stream, which the null stream does not order against
    HIP_TRY(hipDeviceSynchronize());
    DevPtr<float> d_out;
    const float init[3] = {1000.0f, 1000.0f, 1000.0f};   // ref: src/Object.cpp:37
    HIP_TRY(dev_alloc(d_out, sizeof init));
    hipError_t e = hipMemcpy(d_out, init, sizeof init, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const int n = im_height * im_width;
        hipLaunchKernelGGL(tsdfk::object_origin, dim3(std::min((n + 255) / 256, 1024)), dim3(256), 0, 0, depth_dev, mask_dev,
                           im_height, im_width, cam_K[0], cam_K[4], cam_K[2], cam_K[5], d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(origin_out, d_out, sizeof init, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(TSDF_ERR_HIP, "tsdf_object_origin: %s", hipGetErrorString(e));
    return TSDF_OK;
}

// ---------------------------------------------------------------------------------------------
// per-voxel label fusion (csrc/tsdf_labels.hip.h)
// ---------------------------------------------------------------------------------------------
int tsdf_labels_enable(tsdf_volume *v, float prob_threshold)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_labels_enable: NULL handle");
    if (!v->geo.quad_rows) return fail(TSDF_ERR_INVALID, "tsdf_labels_enable: dim_x must be a multiple of 4");
    int rc = bind_device(v);
    if (rc) return rc;
    v->prob_thd = prob_threshold;
    const size_t n = (size_t)(v->geo.n_vox > 0 ? v->geo.n_vox : 1);
    if (!v->d_label) {      // all three or none: the other entry points test d_label alone
        DevPtr<uint16_t> label;
        DevPtr<float> fp, bp;
        HIP_TRY(dev_alloc(label, n * sizeof(uint16_t)));
        HIP_TRY(dev_alloc(fp, n * sizeof(float)));
        HIP_TRY(dev_alloc(bp, n * sizeof(float)));
        v->d_label = std::move(label); v->d_fp = std::move(fp); v->d_bp = std::move(bp);
    }
    HIP_TRY(hipMemsetAsync(v->d_label, 0, n * sizeof(uint16_t), v->stream));
    HIP_TRY(hipMemsetAsync(v->d_fp, 0, n * sizeof(float), v->stream));
    HIP_TRY(hipMemsetAsync(v->d_bp, 0, n * sizeof(float), v->stream));
    return TSDF_OK;
}

int tsdf_integrate_labels_device(tsdf_volume *v, const float *depth_dev, const uint16_t *label_im_dev,
                                 const float *score_im_dev, const float cam2world[16])
{
    if (!v || !depth_dev || !label_im_dev || !score_im_dev || !cam2world)
        return fail(TSDF_ERR_INVALID, "tsdf_integrate_labels_device: NULL argument");
    if (!v->d_label) return fail(TSDF_ERR_INVALID, "tsdf_integrate_labels_device: call tsdf_labels_enable first");
    int rc = bind_device(v);
    if (rc) return rc;
    if (v->geo.nz == 0) return TSDF_OK;
    float c2b[16];
    compose_cam2base(v, cam2world, c2b);
    tsdfk::LabelParams lp;
    lp.g = make_params(v, depth_dev, nullptr, c2b, 4);
    lp.label_im = label_im_dev; lp.score_im = score_im_dev;
    lp.label = v->d_label; lp.fp = v->d_fp; lp.bp = v->d_bp; lp.prob_thd = v->prob_thd;
    hipLaunchKernelGGL(tsdfk::integrate_labels, to_dim3(tsdf_host::grid_quad_rows(v->geo, 4)), dim3(64, 4, 1), 0, v->stream, lp);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

int tsdf_download_labels(tsdf_volume *v, uint16_t *label_host, float *fp_host, float *bp_host)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_download_labels: NULL handle");
    if (!v->d_label) return fail(TSDF_ERR_INVALID, "tsdf_download_labels: labels not enabled");
    int rc = bind_device(v);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(v->stream));
    const size_t n = (size_t)v->geo.n_vox;
    if (n == 0) return TSDF_OK;
    if (label_host) HIP_TRY(hipMemcpy(label_host, v->d_label, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (fp_host) HIP_TRY(hipMemcpy(fp_host, v->d_fp, n * sizeof(float), hipMemcpyDeviceToHost));
    if (bp_host) HIP_TRY(hipMemcpy(bp_host, v->d_bp, n * sizeof(float), hipMemcpyDeviceToHost));
    return TSDF_OK;
}

int tsdf_upload_labels(tsdf_volume *v, const uint16_t *label_host, const float *fp_host, const float *bp_host)
{
    if (!v || !label_host || !fp_host || !bp_host) return fail(TSDF_ERR_INVALID, "tsdf_upload_labels: NULL argument");
    if (!v->d_label) return fail(TSDF_ERR_INVALID, "tsdf_upload_labels: labels not enabled");
    int rc = bind_device(v);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(v->stream));
    const size_t n = (size_t)v->geo.n_vox;
    if (n == 0) return TSDF_OK;
    HIP_TRY(hipMemcpy(v->d_label, label_host, n * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v->d_fp, fp_host, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v->d_bp, bp_host, n * sizeof(float), hipMemcpyHostToDevice));
    return TSDF_OK;
}

int tsdf_compose_labels(tsdf_volume *v, const uint8_t *masks_dev, const uint16_t *labels_host, const float *scores_host,
                        int32_t k, uint16_t *label_im_dev, float *score_im_dev)
{
    if (!v || !label_im_dev || !score_im_dev || k < 0 || (k > 0 && (!masks_dev || !labels_host || !scores_host)))
        return fail(TSDF_ERR_INVALID, "tsdf_compose_labels: bad argument");
    if (k > tsdfk::kMaxInstances) return fail(TSDF_ERR_INVALID, "tsdf_compose_labels: at most %d instances per frame", tsdfk::kMaxInstances);
    int rc = bind_device(v);
    if (rc) return rc;
    tsdfk::ComposeParams c;
    c.masks = masks_dev; c.label_im = label_im_dev; c.score_im = score_im_dev; c.k = k;
    c.n_pixels = v->cfg.im_height * v->cfg.im_width;
    for (int i = 0; i < tsdfk::kMaxInstances; ++i) { c.labels[i] = i < k ? labels_host[i] : 0; c.scores[i] = i < k ? scores_host[i] : 0.0f; }
    hipLaunchKernelGGL(tsdfk::compose_labels, dim3((c.n_pixels + 255) / 256), dim3(256), 0, v->stream, c);
    HIP_TRY(hipGetLastError());
    return TSDF_OK;
}

// ---------------------------------------------------------------------------------------------
// per-voxel colour fusion (csrc/tsdf_colour.hip.h)
// ---------------------------------------------------------------------------------------------
int tsdf_colour_enable(tsdf_volume *v)
{
    if (!v) return fail(TSDF_ERR_INVALID, "tsdf_colour_enable: NULL handle");
    if (!v->geo.quad_rows) return fail(TSDF_ERR_INVALID, "tsdf_colour_enable: dim_x must be a multiple of 4");
    int rc = bind_device(v);
    if (rc) return rc;
    const size_t n = (size_t)(v->geo.n_vox > 0 ? v->geo.n_vox : 1);
    if (!v->d_colour) HIP_TRY(dev_alloc(v->d_colour, n * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(v->d_colour, 0, n * sizeof(uint32_t), v->stream));
    return TSDF_OK;
}

int tsdf_integrate_colour_device(tsdf_volume *v, const float *depth_dev, const uint8_t *rgb_dev, const float cam2world[16])
{
    if (!v || !depth_dev || !rgb_dev || !cam2world) return fail(TSDF_ERR_INVALID, "tsdf_integrate_colour_device: NULL argument");
    if (!v->d_colour) return fail(TSDF_ERR_INVALID, "tsdf_integrate_colour_device: call tsdf_colour_enable first");
    int rc = bind_device(v);
    if (rc) return rc;
    float c2b[16];
    compose_cam2base(v, cam2world, c2b);
    return launch_colour(v, depth_dev, rgb_dev, c2b);
}

int tsdf_integrate_rgbd(tsdf_volume *v, const float *depth_host, const uint8_t *rgb_host, const float cam2world[16])
{
    if (!v || !depth_host || !rgb_host || !cam2world) return fail(TSDF_ERR_INVALID, "tsdf_integrate_rgbd: NULL argument");
    if (!v->d_colour) return fail(TSDF_ERR_INVALID, "tsdf_integrate_rgbd: call tsdf_colour_enable first");
    int rc = bind_device(v);
    if (rc) return rc;
    const size_t px = (size_t)v->cfg.im_height * v->cfg.im_width, img = px * sizeof(float);
    // the colour image has a small ring of its own (pinned + HBM, allocated on first use; one event per slot: the colour
    // kernel that read it), the depth frame goes through the shared store like any other host frame
    decltype(v->rgb)::Slot *s = nullptr;
    HIP_TRY(v->rgb.take(&s));
    if (!s->dev) HIP_TRY(staged_alloc(*s, s->done, px * 3));
    std::memcpy(s->host, rgb_host, px * 3);           // the caller may free both images after we return
    {
        StoreSlot frame;
        rc = stage_frame(v, img, [&](float *pinned) { tsdf_host::copy_to_pinned(pinned, depth_host, img); }, frame);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(s->dev, s->host, px * 3, hipMemcpyHostToDevice, v->copy_stream));
        rc = apply_host_frame(v, frame, cam2world, false, false, s->dev);
    }
    // a copy out of the colour image's slot has been queued: after a failure too (the frame's holder has then made the handle's
    // stream wait for the copy stream) its last reader is in front of this point of the handle's stream
    const hipError_t ce = v->rgb.consumed(s, v->stream);
    if (rc == TSDF_OK && ce != hipSuccess) rc = fail(TSDF_ERR_HIP, "tsdf_integrate_rgbd: hipEventRecord failed: %s", hipGetErrorString(ce));
    return rc;
}

int tsdf_download_colour(tsdf_volume *v, uint32_t *colour_host)
{
    if (!v || !colour_host) return fail(TSDF_ERR_INVALID, "tsdf_download_colour: NULL argument");
    if (!v->d_colour) return fail(TSDF_ERR_INVALID, "tsdf_download_colour: colour not enabled");
    int rc = bind_device(v);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(v->stream));
    if (v->geo.n_vox > 0) HIP_TRY(hipMemcpy(colour_host, v->d_colour, (size_t)v->geo.n_vox * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return TSDF_OK;
}

int tsdf_upload_colour(tsdf_volume *v, const uint32_t *colour_host)
{
    if (!v || !colour_host) return fail(TSDF_ERR_INVALID, "tsdf_upload_colour: NULL argument");
    if (!v->d_colour) return fail(TSDF_ERR_INVALID, "tsdf_upload_colour: colour not enabled");
    int rc = bind_device(v);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(v->stream));
    if (v->geo.n_vox > 0) HIP_TRY(hipMemcpy(v->d_colour, colour_host, (size_t)v->geo.n_vox * sizeof(uint32_t), hipMemcpyHostToDevice));
    return TSDF_OK;
}

}  // extern "C"

#include "tsdf_batch_host.hip.h"
#include "tsdf_raycast_host.hip.h"
#include "tsdf_track_host.hip.h"
#include "tsdf_photo_host.hip.h"
#include "tsdf_fuse_host.hip.h"
#include "tsdf_align_host.hip.h"
#include "tsdf_extent_host.hip.h"
#include "tsdf_associate_host.hip.h"
#include "tsdf_batch_track_host.hip.h"
#include "tsdf_segment_host.hip.h"
#include "tsdf_scan_host.hip.h"
#include "tsdf_scan_fill_host.hip.h"
#include "tsdf_scan_ground_host.hip.h"
#include "tsdf_scan_track_host.hip.h"
#include "tsdf_extract_host.hip.h"
#include "tsdf_group.hip.h"
#include "tsdf_diag.hip.h"
