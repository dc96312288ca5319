// tsdf_batch_track.hip.h -- joint tracking against the members of a batch: one camera pose from all the objects a caller trusts,
// and one system of normal equations per object at that pose (tsdf_batch_track, tsdf_batch_track_system,
// tsdf_track_member_systems).
//
// THE RULE is tsdf_track's (tsdf_track.hip.h, restated in tests/track_spec.py) with three changes and nothing else;
// tests/batch_track_spec.py restates them as a layer over track_spec, DESIGN.md ("N6 -- tracking") describes them.
//
//   Frame    The members have base frames of their own, so the rule works in the frame of the reference camera: C_ref is the
//            float32 ref_cam2world itself (the guess for tsdf_batch_track) and C_cur the float32 cam2world, with no
//            compose_cam2base.  M = C_ref^-1 * C_cur as tsdf_track computes it.  The result is cam2world = C_ref * M (4 x 4,
//            double, sums over k left to right), each entry rounded to float32: tsdf_track's result with an identity
//            base2world, whose products are exact.
//   Model    The batch's render at C_ref: depth t, normal nm and member index per pixel, what tsdf_batch_raycast_device writes
//            bit for bit.  At the model-pixel gate a pair is rejected unless t > 0, nm != (0, 0, 0) and
//            0 <= member[pixel] < n_members; for the joint system also unless member_use[member[pixel]] != 0.  A pair belongs
//            to member m = member[(ui, vi)].
//   Systems  S[m], 29 doubles, is the sum of the 29 float32 terms over member m's pairs.  The joint system of an iteration is
//            the sum over the pairs of the used members; the solve, the lost test, the step, the level state machine, status,
//            iters_run, inliers and rmse are tsdf_track's, applied to the joint system.  After the last iteration ONE MORE
//            association pass evaluates S[m] for every member, used or not, at the final estimate (the state after the last
//            step) and at the finest level that has iters > 0 (level 0 when none has).  Entry 28 of S[m] is the member's pair
//            count, entry 27 its sum r^2: these are counts of a later pass than the one out->inliers and out->rmse report, at
//            a pose one step further.  On a lost track every S[m] is all +0.0 and the pose is the guess's own bits.
//
// So the joint track is tsdf_track's on the render with depth 0 wherever the member is outside [0, n_members) or is not used,
// and S[m] is tsdf_track_system's on the render with depth 0 everywhere but at member m.
//
// MAPPING.  The joint iterations run track_pairs / track_solve unchanged on a copy of the render's depth that track_mask_model
// has zeroed where a member is out.  The member pass, track_member_pairs, is a reduction keyed by member: one live sample per
// lane, a grid-stride loop over at most kTrackMaxBlocks 256-lane workgroups on blockIdx.x, and on blockIdx.y one tile of
// kTrackMemberTile members (any number of members fits: a workgroup keeps one LDS row of 29 doubles per wave and member of
// its tile, 32 480 bytes, and sees only the pairs of its tile).  A wave works on one member at a time: per trip it takes the
// member of its lowest pending lane, the lanes that hold that member add their 29 terms into double registers of their own,
// and the rest wait their turn, until no lane is pending.  Only when the wave moves on to another member (and at the end) are
// the registers summed across the wave (track_wave_sum, 64 lanes) and added into the wave's own LDS row of the member they
// belonged to.  Neighbouring samples nearly always share a member, so a trip usually takes one round and the cross-lane sums
// are as rare as the member changes; a different member on every pixel costs one sum per round.  A member index addresses
// LDS only after 0 <= m - m0 < tile has been tested.  After a barrier the four waves' rows are added in wave order and
// stored with plain stores as the workgroup's partial row of every member of the tile; track_member_sum, one workgroup per
// member, adds a member's partial rows in the fixed order track_solve uses.  No atomics anywhere: the same inputs give the
// same bits, and a system of one pair is the double value of its float32 terms (every other addend is +0.0).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tsdf_track.hip.h"

namespace tsdfk {

constexpr int kTrackMemberTile = 35;         // members per workgroup: 4 waves x 35 rows x 29 doubles = 32 480 bytes of LDS
constexpr int kTrackMemberMaxRows = 65536;   // partial rows of a member pass (members x workgroups per tile), about

struct TrackMemberParams {
    TrackPairsParams pp;         // the pass as track_pairs sees it (its partials are not used)
    const int32_t *member;       // the render's member image, H*W
    double *rows;                // n_members x gridDim.x partial rows of kTrackTerms
    int n_members;
};

// depth with 0 where the member is outside [0, n_members) or not used: the model of the joint iterations.
__global__ __launch_bounds__(256) void track_mask_model(const float *depth, const int32_t *member, const uint8_t *use,
                                                        int n_members, float *out, int64_t n_px)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_px; i += (int64_t)gridDim.x * 256) {
        const int32_t m = member[i];
        const bool in = m >= 0 && m < n_members && use[m] != 0;
        out[i] = in ? depth[i] : 0.0f;
    }
}

// The wave's sums of acc into its LDS row `row` (lane k adds entry k), and acc back to zero.
__device__ __forceinline__ void track_member_flush(double acc[kTrackTerms], double *row, int lane)
{
    double add = 0.0;
#pragma unroll
    for (int k = 0; k < kTrackTerms; ++k) {
        const double x = track_wave_sum(acc[k]);
        if (lane == k) add = x;
        acc[k] = 0.0;
    }
    if (lane < kTrackTerms) row[lane] += add;
}

__global__ __launch_bounds__(256) void track_member_pairs(TrackMemberParams q)
{
    const TrackPairsParams &p = q.pp;
    const TrackState *st = p.state;
    if (st->lost) return;                    // track_member_sum writes the zeros
    __shared__ double rows[4][kTrackMemberTile][kTrackTerms];
    const int m0 = blockIdx.y * kTrackMemberTile;
    const int mt = min(kTrackMemberTile, q.n_members - m0);
    for (int i = threadIdx.x; i < 4 * kTrackMemberTile * kTrackTerms; i += 256) (&rows[0][0][0])[i] = 0.0;
    __syncthreads();
    float Rm[9], tm[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rm[k] = st->Rm[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tm[k] = st->tm[k];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[kTrackTerms];                 // per lane, of the pairs of member `cur` since the last flush
#pragma unroll
    for (int k = 0; k < kTrackTerms; ++k) acc[k] = 0.0;
    int cur = -1;                            // the same in every lane of the wave; in [0, mt) once set
    const unsigned n = (unsigned)p.ni * (unsigned)p.nj;     // < 2^30: the image size is checked on the host
    // every lane of a wave runs the same number of trips (the wave operations below need the whole wave): the bound is rounded
    // up to a multiple of the stride and a lane past the last sample holds no pair
    const unsigned stride = gridDim.x * 256, n_end = (n + stride - 1) / stride * stride;
    for (unsigned idx = blockIdx.x * 256 + threadIdx.x; idx < n_end; idx += stride) {
        float term[kTrackTerms] = {};
        int loc = -1;                        // the pair's member within the tile, or -1: no pair of this tile
        if (idx < n) {
            const int j = (int)(idx / (unsigned)p.ni), i = (int)(idx - (unsigned)j * (unsigned)p.ni);
            float J[6], r;
            int64_t mp;
            if (track_pair_at(p, Rm, tm, i, j, J, r, mp)) {
                const int32_t m = q.member[mp];
                if (m >= m0 && m < m0 + mt) {
                    loc = m - m0;
                    int k = 0;
#pragma unroll
                    for (int a = 0; a < 6; ++a)
#pragma unroll
                        for (int b = a; b < 6; ++b) term[k++] = J[a] * J[b];
#pragma unroll
                    for (int a = 0; a < 6; ++a) term[21 + a] = J[a] * r;
                    term[27] = r * r;
                    term[28] = 1.0f;
                }
            }
        }
        unsigned long long pend = __ballot(loc >= 0);
        while (pend) {
            const int leader = __ffsll(pend) - 1;
            const int key = __builtin_amdgcn_readfirstlane(__shfl(loc, leader, 64));     // in [0, mt): tested above
            if (key != cur) {                // the wave moves on to another member
                if (cur >= 0) track_member_flush(acc, rows[wave][cur], lane);
                cur = key;
            }
            const bool mine = loc == key;
            if (mine) {
#pragma unroll
                for (int k = 0; k < kTrackTerms; ++k) acc[k] += (double)term[k];
            }
            pend &= ~__ballot(mine);
        }
    }
    if (cur >= 0) track_member_flush(acc, rows[wave][cur], lane);
    __syncthreads();
    for (int i = threadIdx.x; i < mt * kTrackTerms; i += 256) {
        const int ml = i / kTrackTerms, k = i - ml * kTrackTerms;
        q.rows[((int64_t)(m0 + ml) * gridDim.x + blockIdx.x) * kTrackTerms + k] =
            ((rows[0][ml][k] + rows[1][ml][k]) + rows[2][ml][k]) + rows[3][ml][k];
    }
}

// S[m][k]: the partial rows of member m = blockIdx.x in a fixed order (32-lane column groups over strided rows, then the
// eight groups in order, as track_solve sums); all +0.0 on a lost track.
__global__ __launch_bounds__(256) void track_member_sum(const TrackState *state, const double *rows, int n_rows, double *systems)
{
    __shared__ double grp[8][32];
    const int m = blockIdx.x, col = threadIdx.x & 31, g = threadIdx.x >> 5;
    const bool lost = state->lost != 0;
    if (col < kTrackTerms) {
        double x = 0.0;
        if (!lost) {
            const double *mine = rows + (int64_t)m * n_rows * kTrackTerms + col;
#pragma unroll 8
            for (int row = g; row < n_rows; row += 8) x += mine[(int64_t)row * kTrackTerms];
        }
        grp[g][col] = x;
    }
    __syncthreads();
    if (threadIdx.x < kTrackTerms) {
        const int k = threadIdx.x;
        double x = grp[0][k];
        for (int c = 1; c < 8; ++c) x += grp[c][k];
        systems[(int64_t)m * kTrackTerms + k] = x;
    }
}

}  // namespace tsdfk
