"""Joint tracking against a batch on the device (tsdf_batch_track, tsdf_batch_track_system, tsdf_track_member_systems;
csrc/tsdf_batch_track.hip.h) held to its restatement (tests/batch_track_spec.py over tests/track_spec.py):

  1. the member pass on crafted member images over a device render of the track_cases scene volume: M = 1, 7 and 300 (nine
     member tiles), one constant member, a different member on every neighbouring pixel, 16 x 16 blocks, 2 % ids no member has,
     levels 0..2, with and without a live mask; per member the count is exact and every entry within n_m * 2^-52 * sum |term|;
  2. single pairs (a mask on one sample's three pixels): the pair's member row equals the double value of the restatement's
     float32 terms, every other row is all +0.0, at the places where what the kernel iterates over changes (BOUNDARIES below);
  3. the product call on synth.ObjectScene at 640 x 480, four members of different grids, one with a base frame of its own:
     every result field and every member system against the restatement run on tsdf_batch_raycast_device's own render;
  4. member_use on a frame in which one object was moved; every member out loses the track;
  5. a one-member batch with an identity base2world returns what tsdf_track returns on the borrowed handle, byte for byte;
  6. collected frames are applied first, nothing the calls read is changed, identical calls give identical bytes, images made
     on a caller's stream are waited for;
  7. the refusals of the C ABI.

BOUNDARIES of track_member_pairs (csrc/tsdf_batch_track.hip.h): a wave is 64 lanes, a workgroup 256 (4 waves, each with LDS
rows of its own), a member tile TILE = 35 members (blockIdx.y), and level 0 has at most BLOCKS(M) = min(256, 65536 // M)
workgroups per tile, so the second trip of the grid-stride loop begins at sample 256 * BLOCKS(M): 65536 up to 256 members,
55808 for the 300 of these tests."""
import ctypes as C

import numpy as np
import pytest

import batch_track_cases as bc
import batch_track_spec as bts
import track_cases as tc
import track_spec as ts
from test_gpu_associate import member_config
from test_gpu_track import fused_volume
from semantic_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

f32 = np.float32
TILE = 35
N = len(synth.OBJECTS)
ZERO_ROW = np.zeros(29).tobytes()                 # 29 times +0.0
_torch = None


@pytest.fixture(autouse=True)
def _bind_torch(cuda):
    global _torch
    _torch = cuda


def blocks(M):
    return min(256, 65536 // M)


def dev(a):
    return None if a is None else _torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: renders are read-only


def ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------------------------
# the member pass over caller images
# ------------------------------------------------------------------------------------------------------------------------
class Rig:
    """The track_cases scene volume and a World over the device's renders of it."""

    def __init__(self, torch):
        self.vol, self.cfg, origin = fused_volume(torch, tc.DIMS, tc.VS, z0=tc.Z0, poses_k=tc.FUSED_POSES)
        self.world = tc.World(tc.DIMS, tc.VS, origin, self.render)

    def render(self, volume, ray, pose):
        assert volume == "scene"
        o = self.vol.raycast(pose, params=ray, normals=True)
        return o["depth"], o["normal"]

    def model(self, case, member):
        d, n = self.world.model(case)
        return d, n, np.ascontiguousarray(member, np.int32)

    def systems(self, case, member, M, mask=None):
        """tsdf_track_member_systems of a system Case over the scene's render and a crafted member image."""
        d, n, member = self.model(case, member)
        keep = [dev(d), dev(n), dev(member), dev(case.live), dev(mask)]
        return capi.track_member_systems(case.params(), ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), M, ptr(keep[3]), case.ref,
                                         case.cur, level=case.level, mask_ptr=ptr(keep[4]))

    def spec(self, case, member, M, mask=None):
        """(terms, owner, info) of the restatement."""
        return bts.member_terms((case.live, mask), self.model(case, member), M, case.level, ts.relative(case.ref, case.cur),
                                case.P())


@pytest.fixture(scope="module")
def rig(cuda):
    r = Rig(cuda)
    yield r
    r.vol.close()


def crafted_case(world, hw, level):
    K = tc.k_for(hw)
    scene = world.scene(K, hw)
    true = scene.pose(9)
    return tc.Case(f"{hw[1]}x{hw[0]} level {level}", scene.depth(true, quantize=True), None, tc.guess_of(scene, true, 80, False),
                   true, level, K=K, hw=hw)


def member_images(rng, hw, M):
    H, W = hw
    v, u = np.mgrid[0:H, 0:W]
    every = ((u + 3 * v) % M).astype(np.int32)                       # the neighbours of a pixel all differ from it (M >= 4)
    bh, bw = (H + 15) // 16, (W + 15) // 16
    blocky = np.kron(rng.integers(0, M, (bh, bw)), np.ones((16, 16), np.int64))[:H, :W].astype(np.int32)
    stray = every.copy()
    at = rng.choice(H * W, H * W // 50, replace=False)
    stray.ravel()[at] = rng.choice(np.array([-7, -1, M, M + 3], np.int32), at.size)
    return {"constant": np.full(hw, M - 1, np.int32), "every pixel": every, "blocks": blocky, "stray ids": stray}


def check_member_systems(got, terms, owner, M, what):
    """Per member: the count exact, every entry within n_m * 2^-52 * sum |term| (tc.system_bound)."""
    assert got.shape == (M, 29)
    seen = 0
    for m in range(M):
        sel = terms[owner == m]
        want, bound = tc.system_bound(sel) if len(sel) else (np.zeros(29), np.zeros(29))
        assert got[m, 28] == len(sel), f"{what}: member {m} has {got[m, 28]} pairs, spec {len(sel)}"
        bad = ~(np.abs(got[m] - want) <= bound)
        assert not bad.any(), f"{what}: member {m} entries {np.nonzero(bad)[0].tolist()}: {got[m][bad]} vs {want[bad]}"
        seen += len(sel) > 0
    return seen


@pytest.mark.parametrize("M", [1, 7, 300])
def test_member_pass_on_crafted_member_images(rig, M):
    rng = np.random.default_rng(20 + M)
    calls = pairs = 0
    for hw in ((97, 161), (237, 331)):
        images = member_images(rng, hw, M)
        mask = rng.choice(np.array([0, 127, 128, 255], np.uint8), hw, p=[0.1, 0.1, 0.4, 0.4])
        for level in range(3):
            c = crafted_case(rig.world, hw, level)
            for name, member in images.items():
                for m in (None, mask):
                    what = f"M {M} {c} {name} mask {m is not None}"
                    terms, owner, _ = rig.spec(c, member, M, m)
                    assert len(terms) >= 20, what
                    seen = check_member_systems(rig.systems(c, member, M, m), terms, owner, M, what)
                    if name == "constant":
                        assert seen == 1, (what, seen)
                    if name == "every pixel" and m is None and level == 0:
                        assert seen == M if M <= 7 else seen > 250, (what, seen)      # every member tile has work
                    calls, pairs = calls + 1, pairs + len(terms)
    print(f"M {M}: {calls} member passes, {pairs} pairs")


# (H, W), M, the two members that alternate from pixel to pixel, further sample indices to pick pairs at
SINGLE = [(hw, 2 * TILE, (TILE - 1, TILE), ()) for hw in tc.REDUCTION] + \
         [((257, 258), 300, (8 * TILE - 1, 8 * TILE), (256 * blocks(300) - 1, 256 * blocks(300)))]


@pytest.mark.parametrize("hw, M, pair, more", SINGLE, ids=[f"{hw[1]}x{hw[0]}-M{M}" for hw, M, _, _ in SINGLE])
def test_single_pairs_at_the_boundaries(rig, hw, M, pair, more):
    """Lanes 0 and 63 of a wave, the waves' and the workgroup's edges (63 | 64, 127 | 128, 191 | 192, 255 | 256), the last
    sample, either side of the second trip of the grid-stride loop, and members on either side of a tile boundary."""
    c = tc.reduction_case(rig.world, hw, close=True)
    n = (hw[0] - 1) * (hw[1] - 1)
    v, u = np.mgrid[0:hw[0], 0:hw[1]]
    terms, _, info = rig.spec(c, np.full(hw, pair[0], np.int32), M)          # the terms do not depend on which member it is
    targets = sorted(t for t in set(tc.reduction_targets(hw)) | {127, 128, 191, 192} | set(more) if 0 <= t < n)
    picks = tc.nearest_pairs(info["idx"], targets)
    assert len(picks) >= 4, picks
    for i, idx in enumerate(picks):
        k = int(np.searchsorted(info["idx"], idx))
        want = terms[k].astype(np.float64)
        assert want[28] == 1.0
        # the two members alternate from pixel to pixel, and from pick to pick the pair's model pixel shows one or the other
        m, other = pair[i % 2], pair[1 - i % 2]
        ui, vi = int(info["model_px"][0][k]), int(info["model_px"][1][k])
        member = np.where((u + v) % 2 == (ui + vi) % 2, m, other).astype(np.int32)
        got = rig.systems(c, member, M, tc.single_mask(hw, 0, idx))
        assert np.all(got[m] == want), f"{c} sample {idx} member {m}: {np.nonzero(got[m] != want)[0].tolist()}: {got[m]} vs {want}"
        rest = np.delete(got, m, axis=0)
        assert rest.tobytes() == ZERO_ROW * (M - 1), f"{c} sample {idx}: rows {np.nonzero(rest.any(axis=1))[0].tolist()} are not +0.0"
    if more:
        assert max(picks) >= more[1], (picks, more)                           # a pair of the second trip was picked
    print(f"{c} M {M}: {len(picks)} single pairs at {picks}")


def test_images_made_on_a_caller_stream_are_waited_for(rig):
    """tsdf_track_member_systems waits for all work queued on the device: images that work on a caller's (non-blocking) stream
    is still producing when the call is made give the result of images that were ready."""
    c = crafted_case(rig.world, (237, 331), 0)
    M = 7
    member = member_images(np.random.default_rng(5), c.hw, M)["blocks"]
    want = rig.systems(c, member, M)
    d, n, member = rig.model(c, member)
    host = [_torch.from_numpy(np.array(a, order="C")).pin_memory() for a in (d, n, member, c.live)]
    s = _torch.cuda.Stream()
    with _torch.cuda.stream(s):
        big = _torch.ones(64 << 20, device="cuda")
        for _ in range(8):
            big = big * 1.0001                                      # work ahead of the copies on s
        keep = [h.to("cuda", non_blocking=True) for h in host]
        keep[0] = keep[0] * 1.0
        got = capi.track_member_systems(c.params(), ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), M, ptr(keep[3]), c.ref, c.cur)
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------------------------------
# the product calls on the object scene
# ------------------------------------------------------------------------------------------------------------------------
FUSED_POSES = range(0, 16, 2)
BASE_SHIFT = np.array([0.25, -0.125, 0.5], f32)      # member 2 has a base frame of its own: a pure translation


def object_configs(scene):
    cfgs = [member_config(scene, o) for o in range(N)]
    c = cfgs[2]
    base = np.eye(4, dtype=f32)
    base[:3, 3] = BASE_SHIFT
    c.base2world[:] = [float(x) for x in base.ravel()]
    c.origin[:] = [float(f32(o) - s) for o, s in zip(c.origin, BASE_SHIFT)]       # the grid stays where the object is
    return cfgs


def fuse(batch, scene, objects=range(N), poses=FUSED_POSES, sync=True):
    """Frames of `scene` at `poses`, each member fed depth x its object's mask; returns the device frames (they must stay
    allocated until the batch's stream has copied them)."""
    keep = []
    for k in poses:
        c = scene.pose(k)
        ids = scene.ids(c)
        d = dev(scene.depth(c))
        ms = [dev(np.where(ids == o, 255, 0).astype(np.uint8)) for o in objects]
        _torch.cuda.synchronize()
        batch.integrate_device(d.data_ptr(), [m.data_ptr() for m in ms], c)
        keep.append((d, ms))
        if sync:
            _torch.cuda.synchronize()
    return keep


def track_params(cfg):
    p = capi.track_params_default(cfg)
    p.cos_normal_thresh, p.min_inliers = bc.COS_WIDE, bc.MIN_INLIERS
    return p


class Objects:
    def __init__(self):
        self.scene, self.true, self.live, self.moved = bc.frames(1)
        self.cfgs = object_configs(self.scene)
        self.batch = capi.Batch(self.cfgs)
        fuse(self.batch, self.scene)
        self.batch.sync()
        self.p = track_params(self.cfgs[0])
        self.P = ts.from_ctypes(self.p)
        self._models, self._specs = {}, {}

    def model(self, pose):
        """tsdf_batch_raycast_device's own render at pose: (depth, normal, member)."""
        key = np.asarray(pose, f32).tobytes()
        if key not in self._models:
            d = _torch.empty(480 * 640, dtype=_torch.float32, device="cuda")             # written on the batch's stream
            n = _torch.empty(480 * 640 * 3, dtype=_torch.float32, device="cuda")
            m = _torch.empty(480 * 640, dtype=_torch.int32, device="cuda")
            _torch.cuda.synchronize()
            self.batch.raycast_device(pose, d.data_ptr(), n.data_ptr(), m.data_ptr(), params=self.p.ray)
            self.batch.sync()
            self._models[key] = (d.cpu().numpy().reshape(480, 640), n.cpu().numpy().reshape(480, 640, 3),
                                 m.cpu().numpy().reshape(480, 640))
        return self._models[key]

    def spec(self, live, use, guess):
        """(the restatement's track on the device's render at guess, its breaches of track_cases.preconditions)."""
        key = (live.tobytes(), repr(use), np.asarray(guess, f32).tobytes())
        if key not in self._specs:
            hist = []
            r = bts.track((live, None), self.model(guess), N, use, self.P, hist)
            self._specs[key] = (r, tc.preconditions(hist, self.P))
        return self._specs[key]

    def guesses(self, live, uses, want, what):
        taken, passed = bc.clear_seeds(self.true, lambda g: sum((self.spec(live, u, g)[1] for u in uses), []), want)
        print(f"{what}: guesses of seeds {taken}; passed over {passed}")
        return [bc.guess_of(self.true, s) for s in taken]


@pytest.fixture(scope="module")
def objects(cuda):
    o = Objects()
    yield o
    o.batch.close()


def check_batch_track(o, live, use, guess, what):
    """Every result field and every member system of tsdf_batch_track against the restatement; returns (pose, stats, systems,
    the restatement's result)."""
    want, breaches = o.spec(live, use, guess)
    assert breaches == [], what
    d = dev(live)
    _torch.cuda.synchronize()
    pose, st, systems = o.batch.track(d.data_ptr(), guess, params=o.p, use=use)
    assert (st["status"], st["iters_run"], st["inliers"]) == (want["status"], want["iters_run"], want["inliers"]), \
        f"{what}: {st} vs {want}"
    assert tc.ulps32(st["rmse"], f32(want["rmse"])) <= 1.0, f"{what}: rmse {st['rmse']!r} vs {want['rmse']!r}"
    if want["lost"]:
        assert pose.tobytes() == np.asarray(guess, f32).tobytes(), f"{what}: a lost track returns the guess's own bits"
        assert systems.tobytes() == ZERO_ROW * N, what
        return pose, st, systems, want
    u = tc.ulps32(pose.ravel(), bts.result_pose(guess, want["M"]))
    assert u.max() <= 1.0, f"{what}: pose entries {np.nonzero(u > 1.0)[0].tolist()} off by {u[u > 1.0]} float32 ulps"
    assert systems[:, 28].tolist() == want["counts"].tolist(), f"{what}: counts {systems[:, 28]} vs {want['counts']}"
    bound = want["counts"][:, None] * 2.0 ** -52 * want["abs_systems"]
    bad = ~(np.abs(systems - want["systems"]) <= bound)
    assert not bad.any(), f"{what}: member systems differ at {np.argwhere(bad).tolist()}"
    return pose, st, systems, want


def test_product_track_on_the_object_scene(objects):
    o = objects
    member = o.model(o.true)[2]
    assert all((member == m).sum() > 2000 for m in range(N)), [(member == m).sum() for m in range(N)]
    for guess in o.guesses(o.live, [None], bc.N_PRODUCT_GUESSES, "product"):
        pose, st, systems, want = check_batch_track(o, o.live, None, guess, "product")
        assert st["status"] != 2 and (systems[:, 28] > 1000).all(), (st, systems[:, 28])
        e, g = ts.pose_error(pose, o.true), ts.pose_error(guess, o.true)
        print(f"product: {e[0]:.2e} m, {e[1]:.2e} rad from the truth (the guess {g[0]:.2e} m, {g[1]:.2e} rad); {st}; "
              f"member rmse {bts.member_rmse(systems)}, member pairs {systems[:, 28].astype(int).tolist()}")
        assert e[0] < g[0] and e[1] < g[1], (e, g)


def test_product_member_systems_per_level(objects):
    o = objects
    guess = bc.guess_of(o.true, bc.CANDIDATE_SEEDS[0])
    d = dev(o.live)
    _torch.cuda.synchronize()
    for level in range(3):
        terms, owner, _ = bts.member_terms((o.live, None), o.model(guess), N, level, ts.relative(guess, o.true), o.P)
        got = o.batch.track_system(d.data_ptr(), guess, o.true, level=level, params=o.p)
        assert check_member_systems(got, terms, owner, N, f"level {level}") == N


def test_member_use_and_a_moved_object(objects):
    o = objects
    out = bc.all_but(bc.MOVED)
    guess, = o.guesses(o.moved, [None, out], 1, "moved")
    p_all, st_all, s_all, _ = check_batch_track(o, o.moved, None, guess, "moved, all members")
    p_out, st_out, s_out, _ = check_batch_track(o, o.moved, out, guess, f"moved, member {bc.MOVED} out")
    e_all, e_out = ts.pose_error(p_all, o.true), ts.pose_error(p_out, o.true)
    rm_all, rm_out = bts.member_rmse(s_all), bts.member_rmse(s_out)
    print(f"moved box, all members: {e_all[0]:.2e} m, {e_all[1]:.2e} rad, member rmse {rm_all}")
    print(f"moved box, member {bc.MOVED} out: {e_out[0]:.2e} m, {e_out[1]:.2e} rad, member rmse {rm_out}")
    assert st_all["status"] != 2 and st_out["status"] != 2
    assert e_out[0] < e_all[0] and e_out[1] < e_all[1], (e_all, e_out)
    assert int(np.argmax(rm_out)) == bc.MOVED, rm_out
    _, st, systems, want = check_batch_track(o, o.moved, [0] * N, guess, "every member out")
    assert want["lost"] and st["status"] == 2 and st["inliers"] == 0


# ------------------------------------------------------------------------------------------------------------------------
# one member, lifecycle, refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_one_member_batch_is_tsdf_track_on_the_borrowed_handle(cuda):
    origin = synth.surf_volume(max(tc.DIMS), tc.VS, tc.Z0)
    cfg = capi.make_config(tc.DIMS, tc.VS, origin)                   # base2world is the identity
    scene = synth.TrackScene(tc.DIMS, tc.VS, origin)
    true = scene.pose(9)
    guess = ts.perturb(true, np.random.default_rng(6), 1.0, 0.01)
    live = dev(scene.depth(true, quantize=True))
    mask = np.zeros((480, 640), np.uint8)
    mask[60:420, 80:600] = 255
    mask = dev(mask)
    with capi.Batch([cfg]) as batch:
        keep = []
        for k in tc.FUSED_POSES:
            c = scene.pose(k)
            keep.append(dev(scene.depth(c, quantize=True)))
            _torch.cuda.synchronize()
            batch.integrate_device(keep[-1].data_ptr(), None, c)
        p = capi.track_params_default(cfg)
        for m in (None, mask):
            for iters in ((10, 5, 4), (0, 0, 0), (0, 3, 0)):
                p.iters[:] = iters
                want = batch.volumes[0].track(live.data_ptr(), guess, params=p, mask_ptr=ptr(m))
                pose, st, systems = batch.track(live.data_ptr(), guess, params=p, mask_ptr=ptr(m))
                assert pose.tobytes() == want[0].tobytes() and st == want[1], (iters, st, want[1])
                assert f32(st["rmse"]).tobytes() == f32(want[1]["rmse"]).tobytes()
                assert st["status"] == (0 if iters == (10, 5, 4) else 1), (iters, st)
                if iters == (0, 0, 0):
                    # no step was taken: the member pass is tsdf_track_system's at the guess (another order of summation)
                    A, b, r2, n = batch.volumes[0].track_system(live.data_ptr(), guess, guess, level=0, params=p, mask_ptr=ptr(m))
                    one = np.concatenate([A[np.triu_indices(6)], b, [r2, float(n)]])
                    assert systems[0, 28] == n and n > 1000
                    assert np.all(np.abs(systems[0] - one) <= n * 2.0 ** -52 * np.abs(one).max() * n), (systems[0], one)
                else:
                    assert systems[0, 28] > 1000


def test_collected_frames_read_only_and_repeatable(cuda):
    scene, true, live, _ = bc.frames(1)
    cfgs = object_configs(scene)[:3]
    objs = range(3)
    guess = bc.guess_of(true, 8)
    d_live = dev(live)
    with capi.Batch(cfgs) as ref:
        ref.volumes[0].set_deferral(0)
        fuse(ref, scene, objs)
        ref.sync()
        p = track_params(cfgs[0])
        want = ref.track(d_live.data_ptr(), guess, params=p)
        want_sys = ref.track_system(d_live.data_ptr(), guess, true, level=1, params=p)
    with capi.Batch(cfgs) as plain:                  # never tracked: the same frames in the same launches
        plain.volumes[0].set_deferral(32)
        keep = fuse(plain, scene, objs, sync=False)
        plain.sync()
        keep += fuse(plain, scene, objs, poses=[1])
        plain.sync()
        want_state = [v.download() for v in plain.volumes]
    assert want[1]["status"] != 2 and (want[2][:, 28] > 1000).all()
    with capi.Batch(cfgs) as b:
        b.volumes[0].set_deferral(32)                # frames are collected, and the call applies them first
        keep = fuse(b, scene, objs, sync=False)
        got = b.track(d_live.data_ptr(), guess, params=p)
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2].tobytes() == want[2].tobytes()
        before = [v.download() for v in b.volumes]
        again = b.track(d_live.data_ptr(), guess, params=p)
        sys1 = b.track_system(d_live.data_ptr(), guess, true, level=1, params=p)
        sys2 = b.track_system(d_live.data_ptr(), guess, true, level=1, params=p)
        none = b.track(d_live.data_ptr(), guess, params=p, want_systems=False)
        after = [v.download() for v in b.volumes]
        for (t0, w0), (t1, w1) in zip(before, after):
            assert t0.tobytes() == t1.tobytes() and w0.tobytes() == w1.tobytes()
        assert again[0].tobytes() == got[0].tobytes() and again[1] == got[1] and again[2].tobytes() == got[2].tobytes()
        assert sys1.tobytes() == sys2.tobytes() == want_sys.tobytes()
        assert none[2] is None and none[0].tobytes() == got[0].tobytes() and none[1] == got[1]
        # the free-space summaries were not touched either: one more frame lands as it does in a batch that was never tracked
        keep += fuse(b, scene, objs, poses=[1])
        b.sync()
        for (t0, w0), v in zip(want_state, b.volumes):
            t1, w1 = v.download()
            assert t0.tobytes() == t1.tobytes() and w0.tobytes() == w1.tobytes()
    del keep


def test_refusals(cuda):
    lib = capi.load()
    cfg = capi.make_config((32, 32, 32), 0.01, [-0.16, -0.16, 1.0])
    depth = _torch.zeros(480 * 640, dtype=_torch.float32, device="cuda")
    _torch.cuda.synchronize()
    eye = np.eye(4, dtype=f32).ravel()
    res, sysbuf = capi.TrackResult(), np.zeros((2, 29))
    use = np.ones(2, np.uint8)

    def track(b, p, d=depth.data_ptr(), guess=eye, out=True):
        return lib.tsdf_batch_track(b, C.byref(p) if p is not None else None, d, None, use.ctypes.data,
                                    guess.ctypes.data if guess is not None else None, C.byref(res) if out else None,
                                    sysbuf.ctypes.data)

    def system(b, p, d=depth.data_ptr(), guess=eye, out=True, level=0, cur=eye):
        return lib.tsdf_batch_track_system(b, C.byref(p) if p is not None else None, d, None,
                                           guess.ctypes.data if guess is not None else None,
                                           cur.ctypes.data if cur is not None else None, level,
                                           sysbuf.ctypes.data if out else None)

    def refused(rc, what):
        msg = lib.tsdf_last_error().decode()
        assert rc == -1 and what in msg, (rc, msg)

    with capi.Batch([cfg, cfg]) as batch:
        good = capi.track_params_default(cfg)
        for call in (track, system):
            refused(call(None, good), "NULL")
            refused(call(batch._h, None), "NULL parameters")
            refused(call(batch._h, good, d=None), "NULL depth")
            refused(call(batch._h, good, guess=None), "NULL")
            refused(call(batch._h, good, out=False), "NULL result")
            for field, value, what in (("n_levels", 0, "n_levels"), ("n_levels", 4, "n_levels"),
                                       ("cos_normal_thresh", 1.5, "cos_normal_thresh"),
                                       ("cos_normal_thresh", float("nan"), "cos_normal_thresh"),
                                       ("eps_rot", 0.0, "eps_rot"), ("eps_trans", float("inf"), "eps_rot"),
                                       ("min_inliers", -1, "min_inliers")):
                p = capi.track_params_default(cfg)
                setattr(p, field, value)
                refused(call(batch._h, p), what)
            for arr, i, value, what in (("iters", 2, -1, "iters[2]"), ("dist_thresh", 0, 0.0, "dist_thresh[0]"),
                                        ("dist_thresh", 1, float("nan"), "dist_thresh[1]")):
                p = capi.track_params_default(cfg)
                getattr(p, arr)[i] = value
                refused(call(batch._h, p), what)
            for field, value, what in (("near_m", -1.0, "near"), ("im_height", 240, "render is"), ("im_width", 320, "render is"),
                                       ("im_height", 0, "image size")):
                p = capi.track_params_default(cfg)
                setattr(p.ray, field, value)
                refused(call(batch._h, p), what)
        refused(system(batch._h, good, cur=None), "NULL")
        p = capi.track_params_default(cfg)
        p.n_levels = 2
        refused(system(batch._h, p, level=2), "level 2 is outside")
        refused(system(batch._h, p, level=-1), "level -1 is outside")
        pose, st, systems = batch.track(depth.data_ptr(), eye)                 # and a good call still works: an empty batch
        assert st["status"] == 2 and pose.tobytes() == eye.tobytes() and not systems.any()
        assert not batch.track_system(depth.data_ptr(), eye, eye).any()
    slab = capi.make_config((32, 32, 32), 0.01, [-0.16, -0.16, 1.0], z_begin=4, z_end=12)
    with capi.Batch([cfg, slab]) as batch:
        refused(track(batch._h, good), "z-slab")
        refused(system(batch._h, good), "z-slab")
    # the pass over caller images
    p = capi.track_params_default(capi.default_config(48, 64))
    buf = _torch.zeros(48 * 64 * 3, dtype=_torch.float32, device="cuda")
    mem = _torch.zeros(48 * 64, dtype=_torch.int32, device="cuda")
    b, m = buf.data_ptr(), mem.data_ptr()
    out = np.zeros((3, 29))

    def images(args, level=0, n=3, q=p, ref=eye, o=out):
        return lib.tsdf_track_member_systems(0, C.byref(q) if q is not None else None, args[0], args[1], args[2], n, args[3], None,
                                             ref.ctypes.data if ref is not None else None, eye.ctypes.data, level,
                                             o.ctypes.data if o is not None else None)

    for k in range(4):
        args = [b, b, m, b]
        args[k] = None
        refused(images(args), "NULL")
    refused(images([b, b, m, b], ref=None), "NULL")
    refused(images([b, b, m, b], o=None), "NULL")
    refused(images([b, b, m, b], q=None), "NULL parameters")
    refused(images([b, b, m, b], n=0), "n_members = 0")
    refused(images([b, b, m, b], n=65537), "n_members = 65537")
    refused(images([b, b, m, b], level=3), "level 3 is outside")
    bad = capi.track_params_default(capi.default_config(48, 64))
    bad.dist_thresh[1] = -1.0
    refused(images([b, b, m, b], q=bad), "dist_thresh[1]")
    assert images([b, b, m, b]) == 0 and not out.any()                         # and a good call still works
