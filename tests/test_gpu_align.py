"""Volume-to-volume registration on the device (csrc/tsdf_align.hip.h: tsdf_align_volume, tsdf_align_system) and the merge at a
pose (tsdf_fuse_volume_at) against their float32 restatement (tests/align_spec.py) over the cases of tests/align_cases.py:

  * a system of n pairs is within n * 2^-52 * sum |term| per entry of the restatement's, its count exact (two double sums of
    the same float32 terms); the system of a single pair equals the double value of its float32 terms;
  * a run's status, iters_run and pairs are the restatement's, its rmse and every entry of its pose within one float32 ulp
    (track_cases.ulps32), a lost run returns the start's own bits -- in the cases tests/test_align_spec.py shows clear of the
    restatement's own thresholds;
  * the calls read: not one bit of either volume changes, and two calls give the same bytes;
  * tsdf_fuse_volume_at equals tsdf_fuse_volume at the default pose and the restatement at any other, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import align_cases as ac
import align_spec as asp
import fuse_cases as fc
import fuse_spec as fs
import track_cases as tc
from semantic_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

f32 = np.float32


def same(got, want, what):
    bad = fs.differs(got, want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.flatnonzero(bad)[:5].tolist()}"


def fuse_params(thr=0.9, tol=0.4, write=1):
    p = capi.FuseParams()
    p.weight_thresh, p.agree_tol, p.write = thr, tol, write
    return p


def volumes(case):
    dst, src = capi.Volume(case.dcfg), capi.Volume(case.scfg)
    dst.upload(case.arrays[0], case.arrays[1])
    src.upload(case.arrays[2], case.arrays[3])
    return dst, src


def device_system(case, dst, src):
    return ac.system_vector(*dst.align_system(src, case.dst2src, level=case.level, params=ac.align_params(case.P)))


def check_system(case, dst=None, src=None):
    own = dst is None
    if own:
        dst, src = volumes(case)
    try:
        got = device_system(case, dst, src)
    finally:
        if own:
            dst.close()
            src.close()
    want, bound = case.want()
    assert got[28] == len(case.terms), f"{case}: {got[28]} pairs, restatement {len(case.terms)}"
    bad = ~(np.abs(got - want) <= bound)
    assert not bad.any(), f"{case}: entries {np.nonzero(bad)[0].tolist()} differ: {got[bad]} vs {want[bad]} (bound {bound[bad]})"
    return got


# ------------------------------------------------------------------------------------------------------------------------
# the system against the restatement
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ac.STATES)
@pytest.mark.parametrize("pose", range(ac.N_POSES))
@pytest.mark.parametrize("dst_dims", ac.DST_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_system_parity(cuda, dst_dims, pose, state):
    first = ac.parity_case(dst_dims, pose, state, 0)
    dst, src = volumes(first)
    with dst, src:
        for level in ac.LEVELS:
            c = ac.parity_case(dst_dims, pose, state, level)
            assert len(c.terms) >= 0.10 * c.info["lattice"]
            got = check_system(c, dst, src)
            print(f"{c}: {int(got[28])} pairs of {c.info['lattice']} lattice points, rejected {c.info['rejected']}")
        t, w = dst.download()
        st, sw = src.download()
    for got, want in zip((t, w, st, sw), first.arrays):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_single_pair(cuda):
    pts = ac.interior_points()
    for k in (0, 777, 40000, pts.size - 1):
        c = ac.picked_case(f"one pair at lattice point {k}", pts[[k]])
        assert len(c.terms) == 1
        dst, src = volumes(c)
        with dst, src:
            got = device_system(c, dst, src)
        want = c.terms[0].astype(np.float64)
        assert np.all(got == want), f"{c}: entries {np.nonzero(got != want)[0].tolist()}: {got} vs {want}"


@pytest.mark.parametrize("n", ac.EXACT_COUNTS)
def test_reduction_boundaries(cuda, n):
    c = ac.reduction_case(n)
    assert len(c.terms) == n
    check_system(c)


def test_candidates_only_in_the_last_trip_of_the_last_workgroup(cuda):
    c, first = ac.last_trip_case()
    lane, _, _ = ac.device_lanes(ac.BIG, 0)
    assert lane[c.info["idx"]].min() >= first and len(c.terms) >= 8
    check_system(c)


# ------------------------------------------------------------------------------------------------------------------------
# the state machine
# ------------------------------------------------------------------------------------------------------------------------
def check_run(case, dst, src):
    """Every result field of tsdf_align_volume against the restatement's run; returns (pose entries that differ at all, worst
    difference in float32 ulps)."""
    want = case.want()
    assert ac.preconditions(want["history"], case.P) == [], case
    got, st = dst.align_to(src, params=ac.align_params(case.P), guess=case.guess)
    assert (st["status"], st["iters_run"], st["pairs"]) == (want["status"], want["iters_run"], want["pairs"]), f"{case}: {st} vs {want}"
    assert tc.ulps32(st["rmse"], want["rmse32"]) <= 1.0, f"{case}: rmse {st['rmse']!r} vs {want['rmse32']!r}"
    if want["lost"]:
        start = capi.fuse_pose_default(case.dcfg, case.scfg) if case.guess is None else case.guess
        assert got.tobytes() == start.tobytes(), f"{case}: a lost run returns the start's own bits"
        return 0, 0.0
    assert got.ravel()[12:].tolist() == [0.0, 0.0, 0.0, 1.0]
    u = tc.ulps32(got.ravel(), want["dst2src"])
    assert u.max() <= 1.0, f"{case}: pose entries {np.nonzero(u > 1.0)[0].tolist()} off by {u[u > 1.0]} float32 ulps"
    return int((u > 0).sum()), float(u.max())


def test_state_machine(cuda):
    cases = ac.state_machine_cases()
    dcfg, scfg, arrays, _ = ac.run_world()
    differ = worst = 0
    with capi.Volume(dcfg) as dst:
        dst.upload(arrays[0], arrays[1])
        srcs = {}
        try:
            for c in cases:
                key = bytes(c.scfg)
                if key not in srcs:
                    srcs[key] = capi.Volume(c.scfg)
                    srcs[key].upload(arrays[2], arrays[3])
                n, u = check_run(c, dst, srcs[key])
                differ, worst = differ + n, max(worst, u)
        finally:
            for v in srcs.values():
                v.close()
    print(f"{len(cases)} runs, {differ} pose entries differ from the restatement's at all (worst {worst:.2f} ulp)")


@pytest.mark.parametrize("with_guess", [False, True])
def test_empty_source_is_lost_with_the_starts_own_bits(cuda, with_guess):
    dcfg, scfg, _, truth = ac.run_world()
    guess = ac.moved(truth, ac.centre_of(dcfg), 1.0, 0.003, 5) if with_guess else None
    c = ac.empty_source_case(guess)
    dst, src = volumes(c)
    with dst, src:
        got, st = dst.align_to(src, params=ac.align_params(c.P), guess=guess)
    assert (st["status"], st["iters_run"], st["pairs"], st["rmse"]) == (2, [0, 0, 1], 0, 0.0), st
    start = capi.fuse_pose_default(dcfg, scfg) if guess is None else guess
    assert got.tobytes() == start.tobytes()
    check = c.want()
    assert (check["status"], check["iters_run"]) == (2, [0, 0, 1])


def test_one_destination_against_sources_of_different_sizes_in_turn(cuda):
    """The scratch block knows no size: a used destination handle answers as the restatement and as a fresh handle do."""
    dcfg, _, arrays, _ = ac.run_world()
    run = [c for c in ac.state_machine_cases() if c.name.startswith("default schedule from 2.0")][0]
    _, ecfg = ac.exact_grids()
    et, ew = ac.exact_source()
    small_cfg = fc.config((9, 8, 7), 0.02, np.asarray(dcfg.origin, f32))
    P = asp.params(n_levels=3)
    pose = lambda scfg: asp.pose_default((fs.grid_of(dcfg), fs.grid_of(scfg)))
    sys_run = ac.SystemCase("the run's source, level 1", dcfg, run.scfg, arrays, pose(run.scfg), 1, P)
    sys_exact = ac.SystemCase("a (72, 56, 48) source, level 0", dcfg, ecfg, (arrays[0], arrays[1], et, ew), pose(ecfg), 0, P)
    assert len(sys_run.terms) > 1000 and len(sys_exact.terms) > 1000
    with capi.Volume(dcfg) as used, capi.Volume(run.scfg) as s_run, capi.Volume(ecfg) as s_exact, \
            capi.Volume(small_cfg) as s_small:
        used.upload(arrays[0], arrays[1])
        s_run.upload(arrays[2], arrays[3])
        s_exact.upload(et, ew)
        answers = []
        for case, src in ((sys_run, s_run), (sys_exact, s_exact), (sys_run, s_run)):
            answers.append(check_system(case, used, src).tobytes())
            _, st = used.align_to(s_small)                    # an untouched source of another size: lost
            assert st["status"] == 2
        assert answers[0] == answers[2]
        check_run(run, used, s_run)
        with capi.Volume(dcfg) as fresh:
            fresh.upload(arrays[0], arrays[1])
            assert device_system(sys_exact, fresh, s_exact).tobytes() == answers[1]


# ------------------------------------------------------------------------------------------------------------------------
# determinism, read-only
# ------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes_and_nothing_is_written(cuda):
    dcfg, _, arrays, _ = ac.run_world()
    run = [c for c in ac.state_machine_cases() if c.name.startswith("default schedule from 4.0")][0]
    h, w = fc.IM_HW
    scene = synth.TrackScene(ac.BIG, fc.DST_VS, np.asarray(dcfg.origin, f32), K=fc.K_SMALL, h=h, w=w)
    c2w = scene.pose(3)
    depth = cuda.from_numpy(scene.depth(c2w, quantize=True)).cuda()
    lab = cuda.full((h, w), 3, dtype=cuda.int16, device="cuda")
    sc = cuda.full((h, w), 0.8, dtype=cuda.float32, device="cuda")
    rgb = cuda.full((h, w, 3), 90, dtype=cuda.uint8, device="cuda")

    def everything(v):
        return [a.tobytes() for a in (*v.download(), *v.download_labels(), v.download_colour())]

    with capi.Volume(dcfg) as dst, capi.Volume(run.scfg) as src:
        dst.upload(arrays[0], arrays[1])
        src.upload(arrays[2], arrays[3])
        for v in (dst, src):
            v.labels_enable()
            v.colour_enable()
            v.integrate_device(depth.data_ptr(), c2w)
            v.integrate_colour_device(depth.data_ptr(), rgb.data_ptr(), c2w)
            v.integrate_labels_device(depth.data_ptr(), lab.data_ptr(), sc.data_ptr(), c2w)
        before = everything(dst), everything(src)
        assert any(np.frombuffer(before[0][2], np.uint16)) and any(np.frombuffer(before[0][5], np.uint32))
        p = ac.align_params(run.P)
        a, sa = dst.align_to(src, params=p)
        b, sb = dst.align_to(src, params=p)
        assert sa["status"] != 2 and sa["pairs"] > 1000 and a.tobytes() == b.tobytes() and sa == sb
        s1 = ac.system_vector(*dst.align_system(src, a, level=1, params=p))
        s2 = ac.system_vector(*dst.align_system(src, a, level=1, params=p))
        assert s1.tobytes() == s2.tobytes() and s1[28] > 1000
        assert (everything(dst), everything(src)) == before


def test_summary_words_are_untouched(cuda):
    """Fused Integrate launches trust the free-space summary: four frames as one sequence after an align call give the bits
    they give without it, on both handles (row-mapped kernels, 256-voxel rows)."""
    dims, vs = (256, 16, 12), 0.004
    origin = np.array([-0.512, -0.032, 0.9], f32)
    cfg = fc.config(dims, vs, origin)
    scene = synth.SurfScene(dims, vs, origin, K=fc.K_SMALL, h=fc.IM_HW[0], w=fc.IM_HW[1])
    poses = [scene.pose(k, n=8) for k in range(6)]
    d_dev = [cuda.from_numpy(scene.depth(c, quantize=True)).cuda() for c in poses]
    ptrs = [d.data_ptr() for d in d_dev]

    def run(align):
        with capi.Volume(cfg) as a, capi.Volume(cfg) as b:
            for v in (a, b):
                v.integrate_frames_device(ptrs[:2], np.stack(poses[:2]))
            if align:
                _, st = a.align_to(b)
                assert st["status"] != 2 and st["pairs"] > 300
            for v in (a, b):
                v.integrate_frames_device(ptrs[2:], np.stack(poses[2:]))
            return [x.tobytes() for v in (a, b) for x in v.download()]

    assert run(True) == run(False)


# ------------------------------------------------------------------------------------------------------------------------
# the merge at a pose
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_dims", fc.DST_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_merge_at_the_default_pose_is_the_merge(cuda, dst_dims):
    dcfg, scfg, (dt, dw, st, sw), (want_t, want_w, want_counts), _ = fc.parity_case(dst_dims, 2, "edges")
    m = capi.fuse_pose_default(dcfg, scfg)
    out = []
    for pose in (None, m):
        with capi.Volume(dcfg) as dst, capi.Volume(scfg) as src:
            dst.upload(dt, dw)
            src.upload(st, sw)
            counts = dst.fuse_from(src, fuse_params(fc.WEIGHT_THRESH, 0.4, 1), dst2src=pose)
            out.append((counts, *dst.download()))
    assert out[0][0] == out[1][0] == want_counts
    assert out[0][1].tobytes() == out[1][1].tobytes() and out[0][2].tobytes() == out[1][2].tobytes()
    same(out[1][2], want_w, "weight")
    same(out[1][1], want_t, "tsdf")


@pytest.mark.parametrize("dst_dims", fc.DST_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_merge_at_another_pose_against_the_restatement(cuda, dst_dims):
    dcfg, scfg, (dt, dw, st, sw), (_, _, default_counts), _ = fc.parity_case(dst_dims, 0, "surf")
    dg, sg = fs.grid_of(dcfg), fs.grid_of(scfg)
    m = ac.moved(asp.pose_default((dg, sg)), ac.centre_of(dcfg), 3.0, 0.006, 9)
    want_t, want_w, want_counts = asp.fuse_at(dt, dw, dg, st, sw, sg, m, weight_thresh=fc.WEIGHT_THRESH, agree_tol=0.4, write=1)
    assert want_counts != default_counts and want_counts["sampled"] > 0.1 * dt.size and want_counts["both_band"] > 0
    with capi.Volume(dcfg) as dst, capi.Volume(scfg) as src:
        dst.upload(dt, dw)
        src.upload(st, sw)
        dry = dst.fuse_from(src, fuse_params(fc.WEIGHT_THRESH, 0.4, 0), dst2src=m)
        t0, w0 = dst.download()
        assert t0.tobytes() == dt.tobytes() and w0.tobytes() == dw.tobytes(), "a dry run wrote"
        wet = dst.fuse_from(src, fuse_params(fc.WEIGHT_THRESH, 0.4, 1), dst2src=m)
        got_t, got_w = dst.download()
    assert dry == wet == want_counts
    same(got_w, want_w, "weight")
    same(got_t, want_t, "tsdf")


def test_summary_is_rebuilt_after_a_merge_at_a_pose(cuda, oracle):
    """tests/test_gpu_fuse.py's test_summary_is_rebuilt_before_later_fused_integration through tsdf_fuse_volume_at, at a pose
    that shifts the source by two voxels along x."""
    ddims, sdims, vs = (256, 16, 12), (40, 16, 12), 0.004
    d_origin = np.array([-0.512, -0.032, 0.9], f32)
    s_origin = np.array([-0.08, -0.032, 0.9], f32)
    dcfg, scfg = fc.config(ddims, vs, d_origin), fc.config(sdims, vs, s_origin)
    rng = np.random.default_rng(5)
    st = rng.uniform(-0.9, 0.9, int(np.prod(sdims))).astype(f32)
    sw = rng.choice(np.array([1.0, 2.0, 3.0], f32), st.size)
    dgrid = fs.grid_of(dcfg)
    m = np.eye(4, dtype=f32)
    m[0, 3] = 0.008
    dt0, dw0 = oracle.init_grid(ddims)
    want_t, want_w, want_counts = asp.fuse_at(dt0, dw0, dgrid, st, sw, fs.grid_of(scfg), m.ravel())
    merged = want_w > 0
    assert merged.sum() > 0.5 * st.size
    scene = synth.SurfScene(ddims, vs, d_origin, K=fc.K_SMALL, h=fc.IM_HW[0], w=fc.IM_HW[1])
    poses = [scene.pose(k, n=8) for k in range(4)]
    depths = [scene.depth(c, quantize=True) for c in poses]
    before = want_t.copy()
    for c2w, d in zip(poses, depths):
        oracle.integrate(fc.K_SMALL, oracle.cam2base(dgrid[4], c2w), d, ddims, d_origin, vs, dcfg.trunc_margin, want_t, want_w)
    assert ((want_t != before) & merged).sum() > 0.25 * merged.sum(), "the frames must update merged voxels"
    d_dev = [cuda.from_numpy(d).cuda() for d in depths]
    with capi.Volume(dcfg) as dst, capi.Volume(scfg) as src:
        src.upload(st, sw)
        assert dst.fuse_from(src, dst2src=m.ravel()) == want_counts
        dst.integrate_frames_device([d.data_ptr() for d in d_dev], np.stack(poses))
        got_t, got_w = dst.download()
    same(got_w, want_w, "weight after merge + frames")
    same(got_t, want_t, "tsdf after merge + frames")


def test_end_to_end(cuda):
    """A source whose base2world is off by 4 deg / 10 mm: align_to, then the write = 0 comparison at the result."""
    dcfg, _, arrays, truth = ac.run_world()
    cfg, _ = ac.perturbed_source(*ac.MAGNITUDES[2])
    with capi.Volume(dcfg) as dst, capi.Volume(cfg) as src:
        dst.upload(arrays[0], arrays[1])
        src.upload(arrays[2], arrays[3])
        before = dst.fuse_from(src, fuse_params(write=0))
        pose, st = dst.align_to(src)
        after = dst.fuse_from(src, fuse_params(write=0), dst2src=pose)
        t, w = dst.download()
    r0, r1 = ac.band_ratio(before), ac.band_ratio(after)
    e = asp.motion_error(pose, truth, ac.centre_of(dcfg))
    print(f"agree_band / both_band {r0:.4f} at the perturbed default pose, {r1:.4f} at the aligned one; status {st}; "
          f"{e[0]:.3f} deg {1e3 * e[1]:.3f} mm from the true motion")
    assert st["status"] == 0 and r1 > r0
    assert t.tobytes() == arrays[0].tobytes() and w.tobytes() == arrays[1].tobytes()


# ------------------------------------------------------------------------------------------------------------------------
# ordering
# ------------------------------------------------------------------------------------------------------------------------
def test_batch_members_with_collected_frames(cuda):
    """Member 0 aligned against member 1 through the borrowed handles while the batch still holds collected frames: the
    answer is that of flushing first (tests/test_gpu_fuse.py's case: two small members defer, set_deferral(32) asks for it)."""
    dims, vs = (48, 40, 36), 2.0 ** -8
    origin = np.array([-24 * vs, -20 * vs, 230 * vs], f32)
    cfgs = [fc.config(dims, vs, origin), fc.config(dims, vs, origin)]
    scene = synth.SurfScene(dims, vs, origin, K=fc.K_SMALL, h=fc.IM_HW[0], w=fc.IM_HW[1])
    poses = [scene.pose(k, n=8) for k in range(3)]
    d_dev = [cuda.from_numpy(scene.depth(c, quantize=True)).cuda() for c in poses]
    masks = np.zeros((2,) + fc.IM_HW, np.uint8)
    masks[0, :, :100] = 255
    masks[1, :, 60:] = 255
    m_dev = cuda.from_numpy(masks).cuda()
    m_ptrs = [m_dev[0].data_ptr(), m_dev[1].data_ptr()]
    guess = ac.moved(np.eye(4, dtype=f32).ravel(), ac.centre_of(cfgs[0]), 0.5, 0.001, 3)
    p = ac.align_params(asp.params(min_pairs=50))

    def feed(batch):
        batch.volumes[0].set_deferral(32)
        for c2w, d in zip(poses, d_dev):
            batch.integrate_device(d.data_ptr(), m_ptrs, c2w)

    def answers(batch):
        a, b = batch.volumes
        pose, st = a.align_to(b, params=p, guess=guess)
        return pose.tobytes(), st, ac.system_vector(*a.align_system(b, guess, level=0, params=p)).tobytes()

    with capi.Batch(cfgs) as flushed:
        feed(flushed)
        flushed.sync()
        want = answers(flushed)
        state = [v.download() for v in flushed.volumes]
    assert want[1]["status"] != 2 and want[1]["pairs"] > 1000
    with capi.Batch(cfgs) as batch:
        feed(batch)                                           # collected, not flushed
        got_sys = ac.system_vector(*batch.volumes[0].align_system(batch.volumes[1], guess, level=0, params=p)).tobytes()
        after = [v.download() for v in batch.volumes]
    assert got_sys == want[2]
    with capi.Batch(cfgs) as batch:
        feed(batch)
        pose, st = batch.volumes[0].align_to(batch.volumes[1], params=p, guess=guess)
    assert (pose.tobytes(), st) == want[:2]
    for (t, w), (t0, w0) in zip(after, state):
        assert t.tobytes() == t0.tobytes() and w.tobytes() == w0.tobytes()


def test_source_frames_queued_on_a_caller_stream_order_the_call(cuda):
    """src on a caller's stream with its frames queued just before the call and no sync, dst with collected host frames: the
    bytes of the flushed-and-synchronised run."""
    dcfg, scfg = ac.configs(ac.BIG, 0, thick=False)
    scene = synth.TrackScene(ac.BIG, fc.DST_VS, np.asarray(dcfg.origin, f32), K=fc.K_SMALL, h=fc.IM_HW[0], w=fc.IM_HW[1])
    poses = [scene.pose(k) for k in ac.TRACK_VIEWS]
    depths = [scene.depth(c, quantize=True) for c in poses]
    guess = ac.moved(capi.fuse_pose_default(dcfg, scfg), ac.centre_of(dcfg), 2.0, 0.005, 4)

    def answers(dst, src):
        pose, st = dst.align_to(src, guess=guess)
        return pose.tobytes(), st

    with capi.Volume(dcfg) as dst, capi.Volume(scfg) as src:
        for v in (dst, src):
            v.set_deferral(0)
            for c, d in zip(poses, depths):
                v.integrate(d, c)
            v.sync()
        want = answers(dst, src)
    assert want[1]["status"] == 0 and want[1]["pairs"] > 10000
    with capi.Volume(dcfg) as dst, capi.Volume(scfg) as src:
        for c, d in zip(poses, depths):
            dst.integrate(d, c)                               # collected host frames, no sync
        s = cuda.cuda.Stream()
        src.set_stream(s.cuda_stream)
        host = [cuda.from_numpy(d).pin_memory() for d in depths]
        with cuda.cuda.stream(s):
            dev = [x.to("cuda", non_blocking=True) * 1.0 for x in host]     # produced by work queued on s
            for c, d in zip(poses, dev):
                src.integrate_device(d.data_ptr(), c)
            got = answers(dst, src)
        src.set_stream(None)
    assert got == want


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_refusals(cuda):
    lib = capi.load()
    dims, vs, origin = (16, 12, 8), 0.004, np.zeros(3, f32)
    cfg = fc.config(dims, vs, origin)
    flat = fc.config((16, 12, 1), vs, origin)
    slab_cfg = capi.make_config(dims, vs, origin, z_begin=0, z_end=4, K=fc.K_SMALL, im_height=fc.IM_HW[0], im_width=fc.IM_HW[1])
    eye = np.eye(4, dtype=f32).ravel()
    res, sys_out, counts = capi.AlignResult(), np.zeros(29), capi.FuseCounts()

    def params(**kw):
        p = capi.align_params_default(cfg)
        for k, v in kw.items():
            if k == "iters":
                p.iters[:] = v
            else:
                setattr(p, k, v)
        return p

    h = lambda v: v._h if v is not None else None
    ptr = lambda a: None if a is None else a.ctypes.data

    def volume(dst, src, p, guess=eye, out=res):
        return "tsdf_align_volume", lib.tsdf_align_volume(h(dst), h(src), C.byref(p) if p is not None else None, ptr(guess),
                                                          C.byref(out) if out is not None else None)

    def system(dst, src, p, pose=eye, level=0, out=sys_out):
        return "tsdf_align_system", lib.tsdf_align_system(h(dst), h(src), C.byref(p) if p is not None else None, ptr(pose), level,
                                                          ptr(out))

    def fuse_at(dst, src, p, pose=eye):
        return "tsdf_fuse_volume_at", lib.tsdf_fuse_volume_at(h(dst), h(src), C.byref(p) if p is not None else None, ptr(pose),
                                                              C.byref(counts))

    def refused(call, word):
        name, rc = call
        msg = lib.tsdf_last_error().decode()
        assert rc == -1 and name in msg and word in msg, (name, rc, msg, word)

    ok, fok = params(), fuse_params()
    with capi.Volume(cfg) as a, capi.Volume(cfg) as b, capi.Volume(slab_cfg) as slab, capi.Volume(flat) as thin, \
            capi.Group(cfg, [0, 0]) as group:
        for f, good in ((volume, ok), (system, ok), (fuse_at, fok)):
            refused(f(None, b, good), "NULL")
            refused(f(a, None, good), "NULL")
            refused(f(a, b, None), "NULL")
            refused(f(a, a, good), "same handle")
            refused(f(slab, b, good), "z-slab")
            refused(f(a, slab, good), "z-slab")
            refused(f(group.slabs[0], b, good), "tsdf_group")
            refused(f(a, group.slabs[1], good), "tsdf_group")
            for bad in (float("nan"), float("inf"), float("-inf")):
                pose = eye.copy()
                pose[7] = bad
                refused(f(a, b, good, pose), "[7]")
            pose = eye.copy()
            pose[13] = float("nan")                           # the last row is not read
            assert f(a, b, good, pose)[1] == 0
        refused(system(a, b, ok, None), "dst2src")
        refused(fuse_at(a, b, fok, None), "dst2src")
        assert volume(a, b, ok, None)[1] == 0                 # the guess is optional
        refused(volume(a, b, ok, out=None), "NULL")
        refused(system(a, b, ok, out=None), "NULL")
        for f in (volume, system):
            refused(f(a, thin, ok), "dim")
            for thr in (float("nan"), float("inf"), float("-inf")):
                refused(f(a, b, params(weight_thresh=thr)), "weight_thresh")
            for r in (float("nan"), float("inf"), 0.0, -0.5):
                refused(f(a, b, params(resid_thresh=r)), "resid_thresh")
            for n in (0, 4, -1):
                refused(f(a, b, params(n_levels=n)), "n_levels")
            refused(f(a, b, params(iters=[3, -1, 0])), "iters[1]")
            assert f(a, b, params(iters=[3, 3, -1]))[1] == 0  # beyond n_levels: not read
            refused(f(a, b, params(min_pairs=-1)), "min_pairs")
            for e in (float("nan"), float("inf"), 0.0, -1e-5):
                refused(f(a, b, params(eps_rot=e)), "eps_rot")
                refused(f(a, b, params(eps_trans=e)), "eps_trans")
        for level in (-1, 2, 3):
            refused(system(a, b, ok, level=level), "level")
        for thr in (float("nan"), float("inf")):
            refused(fuse_at(a, b, fuse_params(thr=thr)), "weight_thresh")
        refused(fuse_at(a, b, fuse_params(tol=0.0)), "agree_tol")
        refused(fuse_at(a, b, fuse_params(write=2)), "write")
        if cuda.cuda.device_count() > 1:                      # a volume on a second device cannot be created without one
            other = fc.config(dims, vs, origin)
            other.device = 1
            with capi.Volume(other) as c:
                for f, good in ((volume, ok), (system, ok), (fuse_at, fok)):
                    refused(f(a, c, good), "device")
        else:
            print("NOT CHECKED: the refusal of volumes on different devices needs a second device; this machine shows one")
        t, w = a.download()                                   # nothing was touched
        assert np.all(t == 1.0) and np.all(w == 0.0)
        pose, st = a.align_to(b)                              # and the handles still work: two empty volumes are lost
        assert st["status"] == 2 and st["iters_run"] == [0, 1, 0] and np.array_equal(pose.ravel(), eye)
        assert a.fuse_from(b, dst2src=eye) == {"sampled": 0, "both": 0, "both_band": 0, "agree_band": 0}
