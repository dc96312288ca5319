"""Randomised parity of the colour pass (csrc/tsdf_colour.hip.h) and of label composition and fusion
(csrc/tsdf_labels.hip.h) against the CPU oracle, bit for bit: grid shapes with rows of a multiple of 4 voxels (row-mapped,
flat, less than one chunk), z-slabs, image sizes, intrinsics and base poses from tests/fuzz_cases.py, and cameras outside
the volume, on its boundary, inside it and facing away from it.  The colour pass re-derives which voxels Integrate updated
with its own copy of the projection, so besides parity a one-frame case checks that it coloured exactly those voxels."""
import numpy as np
import pytest

from fuzz_cases import random_case
from semantic_slam_amd import capi, synth

pytestmark = pytest.mark.gpu

f32 = np.float32


def case(seed):
    """random_case with the row width rounded up to a multiple of 4, a random z-slab of the grid and a base pose."""
    rng, dims, h, w, K, vs, origin, trunc, max_depth = random_case(seed)
    dims = ((dims[0] + 3) // 4 * 4, dims[1], dims[2])
    z0 = int(rng.integers(0, dims[2]))
    z1 = int(rng.integers(z0 + 1, dims[2] + 1)) if seed % 3 else dims[2]
    base = synth.random_pose(rng, 0.5, 0.5) if seed % 2 else synth.identity_pose()
    cfg = capi.make_config(dims, vs, origin, trunc=trunc, K=K, base2world=base, im_height=h, im_width=w,
                           max_depth=max_depth, z_begin=z0, z_end=z1)
    return rng, dims, h, w, K, vs, origin, trunc, max_depth, z0, z1, base, cfg


def camera(rng, oracle, dims, vs, origin, base, max_depth, z0, z1, kind):
    """(cam2world, cam2base, distance) of a camera outside the volume (0), on its boundary (1), inside it (2), looking at
    the centre of the slab [z0, z1) from within max_depth, or in front of the volume and facing away from it (3): every
    voxel then lies behind the camera."""
    centre = origin.astype(np.float64) + np.array([dims[0] / 2.0, dims[1] / 2.0, (z0 + z1) / 2.0]) * vs
    ext = float(max(dims) * vs)
    dist = [1.5 * ext + 0.2, 0.5 * ext, 0.05 * ext, 2.0 * ext + 0.2][kind]
    if kind != 3:
        dist = min(dist, 0.8 * max_depth)
    c2b = synth.look_at_pose(rng, centre, dist, jitter=0.02).reshape(4, 4).copy()
    if kind == 3:
        c2b[:3, :3] = c2b[:3, :3] @ np.diag([-1.0, 1.0, -1.0]).astype(f32)
    c2w = oracle.multiply(base, c2b.ravel())
    return c2w, oracle.cam2base(base, c2w), dist


def depth_image(rng, scene, c2b, dist, h, w, max_depth, k):
    """Frame k's depth: a plane through the slab's centre (k = 0: the voxels there are in the band), the scene, a plane at
    exactly max_depth (the last valid depth), or noise including invalid values."""
    mode = 0 if k == 0 else 1 + k % 3
    if mode == 0:
        return np.full((h, w), dist, f32)
    if mode == 1:
        return scene.depth(c2b, quantize=True)
    if mode == 2:
        return np.full((h, w), max_depth, f32)
    return rng.uniform(-0.5, max_depth * 1.2, (h, w)).astype(f32)


@pytest.mark.parametrize("seed", range(16))
def test_colour_matches_oracle(cuda, oracle, seed):
    rng, dims, h, w, K, vs, origin, trunc, max_depth, z0, z1, base, cfg = case(seed)
    scene = synth.SurfScene(dims, vs, origin, K=K, h=h, w=w)
    ref_t, ref_w = oracle.init_grid(dims, z0, z1)
    ref_c = np.zeros(ref_t.size, np.uint32)
    kw = dict(z_begin=z0, z_end=z1, max_depth=max_depth)
    with capi.Volume(cfg) as vol:
        vol.colour_enable()
        for k in range(int(rng.integers(3, 7))):
            c2w, c2b, dist = camera(rng, oracle, dims, vs, origin, base, max_depth, z0, z1, k % 4)
            depth = depth_image(rng, scene, c2b, dist, h, w, max_depth, k)
            rgb = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
            oracle.integrate(K, c2b, depth, dims, origin, vs, trunc, ref_t, ref_w, **kw)
            oracle.integrate_colour(K, c2b, depth, rgb, dims, origin, vs, trunc, ref_w, ref_c, **kw)
            if (seed + k) % 2 == 0:      # host images, deferred
                vol.integrate_rgbd(depth, rgb, c2w)
            else:                        # device images: Integrate, then the colour pass of the same frame
                d_dev, c_dev = cuda.from_numpy(depth).cuda(), cuda.from_numpy(rgb).cuda()
                vol.integrate_device(d_dev.data_ptr(), c2w)
                vol.integrate_colour_device(d_dev.data_ptr(), c_dev.data_ptr(), c2w)
                vol.sync()
        t, wt = vol.download()
        c = vol.download_colour()
    what = f"seed {seed} dims {dims} slab {z0}:{z1} image {h}x{w}"
    assert np.array_equal(wt, ref_w) and np.array_equal(t.view(np.uint32), ref_t.view(np.uint32)), what
    assert np.array_equal(c, ref_c), f"{what}: {np.count_nonzero(c != ref_c)} packed colours differ"
    assert np.all(c[ref_w == 0] == 0), what
    assert np.count_nonzero(ref_c) > 0, f"{what}: no voxel was coloured"


@pytest.mark.parametrize("seed", range(16))
def test_colour_touches_exactly_the_voxels_integrate_updated(cuda, oracle, seed):
    """One frame into a fresh volume, every colour channel >= 1: colour != 0 exactly where the weight became 1."""
    rng, dims, h, w, K, vs, origin, trunc, max_depth, z0, z1, base, cfg = case(seed)
    kind = seed % 4
    c2w, c2b, dist = camera(rng, oracle, dims, vs, origin, base, max_depth, z0, z1, kind)
    far = min(dist + float(rng.uniform(0.0, 0.5)) * float(max(dims) * vs), max_depth)
    depth = np.full((h, w), dist if kind == 3 else (max_depth if seed % 8 < 4 else far), f32)    # max_depth itself is valid
    depth[::7, ::5] = 0.0
    rgb = rng.integers(1, 256, (h, w, 3)).astype(np.uint8)
    with capi.Volume(cfg) as vol:
        vol.colour_enable()
        vol.set_deferral(0)
        d_dev, c_dev = cuda.from_numpy(depth).cuda(), cuda.from_numpy(rgb).cuda()
        vol.integrate_device(d_dev.data_ptr(), c2w)
        vol.integrate_colour_device(d_dev.data_ptr(), c_dev.data_ptr(), c2w)
        _, wt = vol.download()
        c = vol.download_colour()
    rt, rw = oracle.init_grid(dims, z0, z1)
    oracle.integrate(K, c2b, depth, dims, origin, vs, trunc, rt, rw, z_begin=z0, z_end=z1, max_depth=max_depth)
    rc = np.zeros(rt.size, np.uint32)
    oracle.integrate_colour(K, c2b, depth, rgb, dims, origin, vs, trunc, rw, rc, z_begin=z0, z_end=z1, max_depth=max_depth)
    what = f"seed {seed} camera {kind} dims {dims} slab {z0}:{z1}"
    assert np.array_equal(wt, rw), what
    assert (np.count_nonzero(rw) == 0) if kind == 3 else (np.count_nonzero(rw) > 0), what
    assert np.array_equal(c != 0, wt == 1.0), \
        f"{what}: {np.count_nonzero((c != 0) != (wt == 1.0))} voxels coloured without an update or updated without a colour"
    assert np.array_equal(c, rc), what


def masks_for(rng, k, h, w):
    """k overlapping rectangles in MaskRCNN's output format: uint8 {0,255}, label 1..80, scores with ties."""
    masks = np.zeros((k, h, w), np.uint8)
    for m in range(k):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        masks[m, y0:y0 + int(rng.integers(1, h + 1)), x0:x0 + int(rng.integers(1, w + 1))] = 255
    labels = rng.integers(1, 81, k).astype(np.uint16)
    scores = rng.choice(np.array([0.55, 0.7, 0.9, 0.95], f32), k)
    return masks, labels, scores


def run_labels(cuda, oracle, seed, n_frames, fused):
    rng, dims, h, w, K, vs, origin, trunc, max_depth, z0, z1, base, cfg = case(seed)
    scene = synth.SurfScene(dims, vs, origin, K=K, h=h, w=w)
    prob = float(rng.choice([0.3, 0.5, 0.8]))
    n = dims[0] * dims[1] * (z1 - z0)
    ref_l, ref_f, ref_b = np.zeros(n, np.uint16), np.zeros(n, f32), np.zeros(n, f32)
    ref_t, ref_w = oracle.init_grid(dims, z0, z1)
    kw = dict(z_begin=z0, z_end=z1, max_depth=max_depth)
    frames = []
    for k in range(n_frames):
        c2w, c2b, dist = camera(rng, oracle, dims, vs, origin, base, max_depth, z0, z1, [0, 1, 2, 0, 3][k % 5])
        depth = depth_image(rng, scene, c2b, dist, h, w, max_depth, k)
        masks, labels, scores = masks_for(rng, int(rng.integers(1, 6)), h, w)
        masks[0, h // 4:h - h // 4, w // 4:w - w // 4] = 255         # the image centre: the slab's centre voxels
        if k % 3 == 2:
            labels[:] = labels[::-1]
        frames.append((c2w, c2b, depth, masks, labels, scores))
    with capi.Volume(cfg) as vol:
        vol.labels_enable(prob)
        keep = []
        for c2w, c2b, depth, masks, labels, scores in frames:
            lab_dev = cuda.empty((h, w), dtype=cuda.uint16, device="cuda")
            sc_dev = cuda.empty((h, w), dtype=cuda.float32, device="cuda")
            m_dev, d_dev = cuda.from_numpy(masks).cuda(), cuda.from_numpy(depth).cuda()
            vol.compose_labels(m_dev.data_ptr(), labels, scores, lab_dev.data_ptr(), sc_dev.data_ptr())
            want_lab, want_sc = oracle.compose_labels(masks, labels, scores)
            if not fused:
                vol.integrate_labels_device(d_dev.data_ptr(), lab_dev.data_ptr(), sc_dev.data_ptr(), c2w)
                vol.integrate_device(d_dev.data_ptr(), c2w)
            vol.sync()
            assert np.array_equal(lab_dev.cpu().numpy(), want_lab) and np.array_equal(sc_dev.cpu().numpy(), want_sc)
            keep.append((d_dev, lab_dev, sc_dev))
            oracle.integrate_labels(K, c2b, depth, want_lab, want_sc, dims, origin, vs, trunc, ref_l, ref_f, ref_b,
                                    prob_thd=prob, **kw)
            oracle.integrate(K, c2b, depth, dims, origin, vs, trunc, ref_t, ref_w, **kw)
        if fused:
            vol.integrate_frames_labels_device([d.data_ptr() for d, _, _ in keep], [l.data_ptr() for _, l, _ in keep],
                                               [s.data_ptr() for _, _, s in keep], np.stack([f[0] for f in frames]))
        lab, fp, bp = vol.download_labels()
        t, wt = vol.download()
    what = f"seed {seed} dims {dims} slab {z0}:{z1} image {h}x{w} frames {n_frames}"
    assert np.array_equal(wt, ref_w) and np.array_equal(t.view(np.uint32), ref_t.view(np.uint32)), what
    assert np.array_equal(lab, ref_l), f"{what}: {np.count_nonzero(lab != ref_l)} labels differ"
    assert np.array_equal(fp.view(np.uint32), ref_f.view(np.uint32)), what
    assert np.array_equal(bp.view(np.uint32), ref_b.view(np.uint32)), what
    assert np.all(wt[lab != 0] > 0), f"{what}: a label on a voxel the TSDF never saw"
    assert np.count_nonzero(ref_l) > 0, f"{what}: no voxel was labelled"


@pytest.mark.parametrize("seed", range(16))
def test_labels_match_oracle(cuda, oracle, seed):
    run_labels(cuda, oracle, seed, 6, fused=False)


@pytest.mark.parametrize("seed", [1, 4, 8])
def test_fused_labelled_sequences_longer_than_one_pass(cuda, oracle, seed):
    """More than 32 frames through tsdf_integrate_frames_labels_device: several passes over the same label state."""
    run_labels(cuda, oracle, seed, 33 + seed, fused=True)


@pytest.mark.parametrize("dim_x", [1, 6, 37, 258])
def test_rows_not_a_multiple_of_4_are_refused(cuda, dim_x):
    cfg = capi.make_config((dim_x, 5, 3), 0.01, [0, 0, 1])
    with capi.Volume(cfg) as vol:
        with pytest.raises(capi.TsdfError, match="tsdf_colour_enable: dim_x must be a multiple of 4"):
            vol.colour_enable()
        with pytest.raises(capi.TsdfError, match="tsdf_labels_enable: dim_x must be a multiple of 4"):
            vol.labels_enable(0.5)
