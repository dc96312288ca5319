"""Entry points that take caller device pointers, held to include/tsdf_hip.h's contract: a pointer needs its element's
alignment only, and exactly the stated elements are read or written.

Every case runs five times.  Once with plain torch tensors: that run is held to the entry point's own reference by the
comparison its existing test uses (the oracle bit for bit, raycast_spec, associate_spec, segment_spec, track_spec's bound).
Then with EVERY caller buffer inside a tests/guarded.py allocation -- [front band | payload | back band], both bands holding a
live value of the buffer's role -- for the two fills and for the payload at a 16-byte boundary and at an address aligned to
its element only.  Each guarded run must equal the plain run bit for bit in every output and in the downloaded volume; after
the call and a sync no band byte has changed, no input payload has changed, and every output element the header says is
written either left its prefill or equals the reference.  The exception to bit equality is the tracking systems: their
existing tests hold double sums of float terms to a bound, not to bits, so each guarded run is held to the spec by that bound.

Nothing here can fault: every stray access the net is made for lands inside the test's own allocation.  The image sizes and
volumes are tests/caller_buffer_cases.py's; tests/test_caller_buffer_cases.py shows on the CPU that the first and the last
element of every image are consumed.  At 32 x 24 the depth tile tables (float4 / uchar4) and associate_count<VEC> take their
vector path at residue 0 and must leave it at the element residue."""
import numpy as np
import pytest

import associate_spec as asp
import batch_track_spec as bts
import caller_buffer_cases as cb
import raycast_spec as rs
import segment_spec as ss
import test_gpu_associate as t_assoc
import test_gpu_batch_track as t_btrack
import test_gpu_raycast as t_ray
import test_gpu_segment as t_seg
import test_gpu_track as t_track
import track_cases as tc
import track_spec as ts
from guarded import Guarded, element_residue
from semantic_slam_amd import capi
from walk_cases import same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
MODES = [(fill, res) for fill in "AB" for res in (0, "element")]
PAIRS4 = [p for p in cb.PAIRS if cb.four_wide(p[1])]
pairs = pytest.mark.parametrize("pair", cb.PAIRS, ids=cb.pair_id)
pairs4 = pytest.mark.parametrize("pair", PAIRS4, ids=cb.pair_id)         # labels, colour and batches refuse the scalar rows
sizes = pytest.mark.parametrize("hw", cb.SIZES, ids=lambda hw: f"{hw[1]}x{hw[0]}")


# ------------------------------------------------------------------------------------------------------------------------
# buffers of one run: plain tensors, or guarded allocations of one (fill, residue) mode
# ------------------------------------------------------------------------------------------------------------------------
class Plain:
    def __init__(self, torch, array=None, dtype=None, n=0):
        self.dtype = np.dtype(dtype if array is None else array.dtype)
        if array is None:
            self.t = torch.zeros(n * self.dtype.itemsize, dtype=torch.uint8, device="cuda")
        else:
            self.t = torch.from_numpy(np.ascontiguousarray(array).reshape(-1).view(np.uint8).copy()).cuda()
        self.ptr = self.t.data_ptr()

    def read(self):
        return self.t.cpu().numpy().view(self.dtype)


class Bufs:
    def __init__(self, torch, mode, row_elems, median):
        self.torch, self.mode, self.row, self.median = torch, mode, row_elems, median
        self.inputs, self.outputs = [], []

    def _residue(self, dtype):
        return 0 if self.mode[1] == 0 else element_residue(dtype)

    def inp(self, array, role, per_pixel=1):
        array = np.ascontiguousarray(array)
        if self.mode is None:
            return Plain(self.torch, array)
        g = Guarded(self.torch, "cuda", array.dtype, array.size, role, self.mode[0], self._residue(array.dtype),
                    row_bytes=self.row * per_pixel * array.dtype.itemsize, value=self.median)
        self.inputs.append((role, g.write(array)))
        return g

    def out(self, name, dtype, n, per_pixel=1):
        if self.mode is None:
            return Plain(self.torch, dtype=dtype, n=n)
        g = Guarded(self.torch, "cuda", dtype, n, "out", self.mode[0], self._residue(dtype),
                    row_bytes=self.row * per_pixel * np.dtype(dtype).itemsize)
        self.outputs.append((name, g))
        return g

    def verify(self, reference, what):
        """After the call and a sync: bands intact, inputs unchanged, outputs written or equal to the reference."""
        self.torch.cuda.synchronize()
        for name, g in self.inputs + self.outputs:
            bad = g.bands_intact()
            assert bad.size == 0, f"{what}: {name}: {bad.size} band bytes changed, at {bad[:8].tolist()} from the payload's start"
        for name, g in self.inputs:
            assert g.payload_unchanged(), f"{what}: the {name} input was written"
        for name, g in self.outputs:
            got, pre, want = g.read(), g.prefill(), np.ascontiguousarray(reference[name]).ravel()
            left = (got.view(np.uint8).reshape(got.size, -1) == pre.view(np.uint8).reshape(pre.size, -1)).all(axis=1)
            differ = (got.view(np.uint8).reshape(got.size, -1) != want.view(np.uint8).reshape(want.size, -1)).any(axis=1)
            assert not (left & differ).any(), f"{what}: {name}: elements {np.flatnonzero(left & differ)[:8].tolist()} were not written"


def hold(torch, hw, median, run, check, what, equal=None):
    """The case grid of one call sequence.  run(bufs) -> {name: array}; check(plain results) holds the plain run to its
    reference; equal(got, plain results, what) replaces bit equality where an entry point's own tests do not establish it."""
    plain = run(Bufs(torch, None, hw[1], median))
    check(plain)
    for mode in MODES:
        where = f"{what}, fill {mode[0]}, residue {mode[1]}"
        bufs = Bufs(torch, mode, hw[1], median)
        got = run(bufs)
        if equal is not None:
            equal(got, plain, where)
        else:
            assert got.keys() == plain.keys()
            for name in plain:
                same_bits(got[name], plain[name], f"{where}: {name}")
        bufs.verify(plain, where)


def against(want):
    def check(plain):
        for name, w in want.items():
            same_bits(plain[name], np.ascontiguousarray(w).ravel(), f"plain run vs reference: {name}")
    return check


def downloaded(vol, res=None):
    res = {} if res is None else res
    res["tsdf"], res["weight"] = vol.download()
    return res


def ref_frames(oracle, cfg, frames, share=0.10):
    """The oracle's state after (depth, mask or None) frames at the identity pose."""
    state = None
    for depth, mask in frames:
        state = cb.integrate(oracle, cfg, depth, state, mask)
    assert (state[1] > 0).mean() >= share
    return {"tsdf": state[0], "weight": state[1]}


# ------------------------------------------------------------------------------------------------------------------------
# the net itself, on the device (tests/test_caller_buffer_cases.py holds the helper on the CPU)
# ------------------------------------------------------------------------------------------------------------------------
def test_the_net_is_live_on_the_device(cuda):
    """Stand-ins made of torch operations on the test's own allocation: a store of one byte next to the payload is reported
    with its offset, and a consumer that reads one element past the payload answers differently under the two fills."""
    data = np.linspace(1.0, 2.0, 24 * 32).astype(f32)
    sums = []
    for fill in "AB":
        g = Guarded(cuda, "cuda", f32, data.size, "depth", fill, 4, row_bytes=4 * 32, value=1.5).write(data)
        assert g.ptr % 16 == 4 and g.ptr == g.buf.data_ptr() + g.off and g.bands_intact().size == 0 and g.payload_unchanged()
        past = g.buf[g.off:g.off + g.nbytes + 4].clone().view(cuda.float32)         # one element too many
        sums.append(float(cuda.nan_to_num(past, nan=-1.0).sum()))
        g.buf[g.off + g.nbytes] ^= 0xFF
        g.buf[g.off - 1] ^= 0xFF
        assert g.bands_intact().tolist() == [-1, g.nbytes] and g.payload_unchanged()
    assert sums[0] != sums[1]


# ------------------------------------------------------------------------------------------------------------------------
# the Integrate family
# ------------------------------------------------------------------------------------------------------------------------
@pairs
@pytest.mark.parametrize("deferral", [0, None], ids=["kernel-reads-caller", "library-copies"])
@pytest.mark.parametrize("entry", ["integrate_device", "integrate_cam2base"])
def test_integrate_one_frame(cuda, oracle, pair, entry, deferral):
    c = cb.case(*pair)
    want = ref_frames(oracle, c.cfg, [(c.depths[0], None), (c.depths[1], None)])

    def run(b):
        with capi.Volume(c.cfg) as vol:
            if deferral is not None:
                vol.set_deferral(deferral)
            keep = [b.inp(d, "depth") for d in c.depths[:2]]
            for d in keep:
                getattr(vol, entry)(d.ptr, c.pose)
            vol.sync()
            return downloaded(vol)

    hold(cuda, c.hw, c.median, run, against(want), f"{entry} {cb.pair_id(pair)}")


@pairs
@pytest.mark.parametrize("deferral", [0, None], ids=["kernel-reads-caller", "library-copies"])
@pytest.mark.parametrize("variant", [7, 8])
def test_integrate_masked(cuda, oracle, pair, variant, deferral):
    """Variant 7: integrate_tile<2, true>; variant 8: the tile tables read depth x mask, then the masked bricks."""
    c = cb.case(*pair)
    want = ref_frames(oracle, c.cfg, [(c.depths[0], c.masks[0]), (c.depths[1], c.masks[1])])

    def run(b):
        with capi.Volume(c.cfg) as vol:
            vol.set_kernel_variant(variant)
            if deferral is not None:
                vol.set_deferral(deferral)
            keep = [(b.inp(c.depths[k], "depth"), b.inp(c.masks[k], "mask")) for k in range(2)]
            for d, m in keep:
                vol.integrate_masked_device(d.ptr, m.ptr, c.pose)
            vol.sync()
            return downloaded(vol)

    hold(cuda, c.hw, c.median, run, against(want), f"masked v{variant} {cb.pair_id(pair)}")


@pairs
@pytest.mark.parametrize("variant", [0, 7, 8])
def test_integrate_frames(cuda, oracle, pair, variant):
    """Three frames, each in a buffer of its own; masks [guarded, None, guarded]."""
    c = cb.case(*pair)
    masks = [c.masks[0], None, c.masks[1]]
    want = ref_frames(oracle, c.cfg, list(zip(c.depths, masks)))

    def run(b):
        with capi.Volume(c.cfg) as vol:
            vol.set_kernel_variant(variant)
            d = [b.inp(x, "depth") for x in c.depths]
            m = [None if x is None else b.inp(x, "mask") for x in masks]
            vol.integrate_frames_device([x.ptr for x in d], np.stack([c.pose] * 3), [None if x is None else x.ptr for x in m])
            vol.sync()
            return downloaded(vol)

    hold(cuda, c.hw, c.median, run, against(want), f"frames v{variant} {cb.pair_id(pair)}")


@pairs4
@pytest.mark.parametrize("deferred", [False, True], ids=["per-frame", "deferred"])
@pytest.mark.parametrize("classified", [True, False], ids=["classified", "unclassified"])
def test_batch_integrate(cuda, oracle, pair, classified, deferred):
    """Three members, per-member masks with one None; variants as tests/test_gpu_batch.py selects them."""
    c = cb.case(*pair)
    cfgs = cb.batch_configs(c)
    masks = [c.masks[0], None, c.masks[1]]
    want = {}
    for i, (cfg, mask) in enumerate(zip(cfgs, masks)):
        r = ref_frames(oracle, cfg, [(c.depths[0], mask), (c.depths[1], mask)])
        want[f"tsdf{i}"], want[f"weight{i}"] = r["tsdf"], r["weight"]

    def run(b):
        with capi.Batch(cfgs) as batch:
            for vol in batch.volumes:
                vol.set_kernel_variant(8 if classified else 7)
            batch.volumes[0].set_deferral(32 if deferred else 0)
            m = [None if x is None else b.inp(x, "mask") for x in masks]
            d = [b.inp(x, "depth") for x in c.depths[:2]]
            for x in d:
                batch.integrate_device(x.ptr, [None if y is None else y.ptr for y in m], c.pose)
                if not deferred:
                    batch.sync()
            batch.sync()
            res = {}
            for i, vol in enumerate(batch.volumes):
                res[f"tsdf{i}"], res[f"weight{i}"] = vol.download()
            return res

    hold(cuda, c.hw, c.median, run, against(want), f"batch {cb.pair_id(pair)}")


# ------------------------------------------------------------------------------------------------------------------------
# conversion, labels, colour, origin
# ------------------------------------------------------------------------------------------------------------------------
@pairs
@pytest.mark.parametrize("steps", [(1, 1), (4, 3)], ids=["1x1", "4x3"])
def test_convert_depth_u16_then_integrate(cuda, oracle, pair, steps):
    """Raw in, depth OUT; the output is then the input of integrate_device, read by the kernel itself."""
    c = cb.case(*pair)
    raw = c.raws[0]
    depth = oracle.depth_prep(raw, 5000.0) if steps == (4, 3) else (raw.astype(f32) * (f32(1.0) / f32(5000.0))).astype(f32)
    want = ref_frames(oracle, c.cfg, [(depth, None)], share=0.10 if steps == (1, 1) else 0.01)   # (4, 3) keeps a pixel in 12
    want["depth"] = depth

    def run(b):
        with capi.Volume(c.cfg) as vol:
            vol.set_deferral(0)
            r, d = b.inp(raw, "raw"), b.out("depth", f32, raw.size)
            vol.convert_depth_u16(r.ptr, d.ptr, 5000.0, *steps)
            vol.integrate_device(d.ptr, c.pose)
            vol.sync()
            return downloaded(vol, {"depth": d.read()})

    hold(cuda, c.hw, c.median, run, against(want), f"convert {steps} {cb.pair_id(pair)}")


@pairs
def test_compose_labels(cuda, oracle, pair):
    """K = 3 masks in one buffer, label and score images OUT."""
    c = cb.case(*pair)
    lab, sc = oracle.compose_labels(c.mask_stack, c.labels, c.scores)
    assert len(np.unique(lab)) >= 3

    def run(b):
        with capi.Volume(c.cfg) as vol:
            m = b.inp(c.mask_stack, "mask")
            l, s = b.out("label_im", np.uint16, lab.size), b.out("score_im", f32, sc.size)
            vol.compose_labels(m.ptr, c.labels, c.scores, l.ptr, s.ptr)
            vol.sync()
            return {"label_im": l.read(), "score_im": s.read()}

    hold(cuda, c.hw, c.median, run, against({"label_im": lab, "score_im": sc}), f"compose {cb.pair_id(pair)}")


@pairs4
def test_integrate_labels(cuda, oracle, pair):
    c = cb.case(*pair)
    labels = None
    for k in range(2):
        labels = cb.integrate_labels(oracle, c.cfg, c.depths[k], c.label_ims[k], c.score_ims[k], labels)
    assert np.count_nonzero(labels[1]) > 0
    want = dict(zip(("label", "fp", "bp"), labels))

    def run(b):
        with capi.Volume(c.cfg) as vol:
            vol.labels_enable(0.5)
            keep = [(b.inp(c.depths[k], "depth"), b.inp(c.label_ims[k], "label"), b.inp(c.score_ims[k], "score")) for k in range(2)]
            for d, l, s in keep:
                vol.integrate_labels_device(d.ptr, l.ptr, s.ptr, c.pose)
            vol.sync()
            return downloaded(vol, dict(zip(("label", "fp", "bp"), vol.download_labels())))

    hold(cuda, c.hw, c.median, run, against(want), f"labels {cb.pair_id(pair)}")


@pairs4
@pytest.mark.parametrize("variant", [0, 8])
def test_integrate_frames_labels(cuda, oracle, pair, variant):
    """The fused call: three frames, each with a depth, a label and a score buffer of its own."""
    c = cb.case(*pair)
    state = labels = None
    for k in range(3):
        state = cb.integrate(oracle, c.cfg, c.depths[k], state)
        labels = cb.integrate_labels(oracle, c.cfg, c.depths[k], c.label_ims[k], c.score_ims[k], labels)
    want = dict(zip(("tsdf", "weight", "label", "fp", "bp"), state + labels))

    def run(b):
        with capi.Volume(c.cfg) as vol:
            vol.set_kernel_variant(variant)
            vol.labels_enable(0.5)
            d = [b.inp(x, "depth") for x in c.depths]
            l = [b.inp(x, "label") for x in c.label_ims]
            s = [b.inp(x, "score") for x in c.score_ims]
            vol.integrate_frames_labels_device([x.ptr for x in d], [x.ptr for x in l], [x.ptr for x in s], np.stack([c.pose] * 3))
            vol.sync()
            return downloaded(vol, dict(zip(("label", "fp", "bp"), vol.download_labels())))

    hold(cuda, c.hw, c.median, run, against(want), f"frames+labels v{variant} {cb.pair_id(pair)}")


@pairs4
def test_integrate_colour(cuda, oracle, pair):
    """The rgb payload sits at byte residue 1 in the element-residue runs."""
    c = cb.case(*pair)
    state = cb.integrate(oracle, c.cfg, c.depths[0])
    colour = cb.integrate_colour(oracle, c.cfg, c.depths[0], c.rgb, state)
    want = {"tsdf": state[0], "weight": state[1], "colour": colour}

    def run(b):
        with capi.Volume(c.cfg) as vol:
            vol.colour_enable()
            d, rgb = b.inp(c.depths[0], "depth"), b.inp(c.rgb, "rgb", per_pixel=3)
            vol.integrate_device(d.ptr, c.pose)
            vol.integrate_colour_device(d.ptr, rgb.ptr, c.pose)
            vol.sync()
            return downloaded(vol, {"colour": vol.download_colour()})

    hold(cuda, c.hw, c.median, run, against(want), f"colour {cb.pair_id(pair)}")


@sizes
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_object_origin(cuda, oracle, hw, masked):
    c = cb.case(hw, "flat")
    mask = c.masks[2] if masked else None
    want = oracle.object_origin(c.origin_depth if mask is None else oracle.mask_depth(c.origin_depth, mask), c.K)

    def run(b):
        d = b.inp(c.origin_depth, "depth")
        m = None if mask is None else b.inp(mask, "mask")
        return {"origin": capi.object_origin(d.ptr, None if m is None else m.ptr, hw[0], hw[1], c.K)}

    hold(cuda, hw, c.median, run, against({"origin": want}), f"object_origin {hw}")


# ------------------------------------------------------------------------------------------------------------------------
# raycasts: every output image is the caller's
# ------------------------------------------------------------------------------------------------------------------------
def fused(vol, c, cuda, extras):
    """The case's three frames into vol from plain tensors (library-owned state), with labels and colour where asked."""
    if extras:
        vol.labels_enable(0.5)
        vol.colour_enable()
    for k in range(3):
        d = Plain(cuda, c.depths[k])
        vol.integrate_device(d.ptr, c.pose)
        if extras:
            rgb, l, s = Plain(cuda, c.rgb), Plain(cuda, c.label_ims[k]), Plain(cuda, c.score_ims[k])
            vol.integrate_colour_device(d.ptr, rgb.ptr, c.pose)
            vol.integrate_labels_device(d.ptr, l.ptr, s.ptr, c.pose)
        vol.sync()


@pairs
def test_volume_raycast(cuda, pair):
    """All four outputs (depth, normal, label, colour); the scalar rows have no labels or colour: depth and normal."""
    c = cb.case(*pair)
    n, extras = c.hw[0] * c.hw[1], cb.four_wide(c.cls)
    with capi.Volume(c.cfg) as vol:
        fused(vol, c, cuda, extras)
        p = capi.raycast_params_default(c.cfg)
        t, w = vol.download()
        label = vol.download_labels()[0] if extras else None
        colour = vol.download_colour() if extras else None
        want = t_ray.spec(vol, t, w, p, c.pose, label=label, colour=colour)
        assert want["hit"].mean() > 0.5

        def run(b):
            outs = {"depth": b.out("depth", f32, n), "normal": b.out("normal", f32, 3 * n, per_pixel=3)}
            if extras:
                outs["label"], outs["colour"] = b.out("label", np.uint16, n), b.out("colour", np.uint32, n)
            vol.raycast_device(c.pose, outs["depth"].ptr, outs["normal"].ptr, outs["label"].ptr if extras else None,
                               outs["colour"].ptr if extras else None, params=p)
            vol.sync()
            return {k: o.read() for k, o in outs.items()}

        def check(plain):
            for name in plain:
                t_ray.same_bits(plain[name], want[name].ravel(), f"plain render vs raycast_spec: {name}")

        hold(cuda, c.hw, c.median, run, check, f"raycast {cb.pair_id(pair)}")


def batch_render_spec(batch, cfgs, p, pose):
    members = []
    for vol, cfg in zip(batch.volumes, cfgs):
        t, w = vol.download()
        members.append(dict(tsdf=t, weight=w, dims=(cfg.dim_x, cfg.dim_y, cfg.dim_z), origin=np.asarray(cfg.origin, f32),
                            vs=cfg.voxel_size, trunc=cfg.trunc_margin, cam2base=pose))
    return rs.render_batch(members, np.asarray(p.cam_K, f32), (p.im_height, p.im_width), p.near_m, p.far_m, p.weight_thresh)


def fused_batch(batch, c, cuda):
    masks = [None, Plain(cuda, c.masks[0]), Plain(cuda, c.masks[1])]        # members that differ in what they hold
    for k in range(3):
        d = Plain(cuda, c.depths[k])
        batch.integrate_device(d.ptr, [None if m is None else m.ptr for m in masks], c.pose)
        batch.sync()


@pairs4
def test_batch_raycast(cuda, pair):
    """Depth, normal and member OUT."""
    c = cb.case(*pair)
    cfgs, n = cb.batch_configs(c), c.hw[0] * c.hw[1]
    with capi.Batch(cfgs) as batch:
        fused_batch(batch, c, cuda)
        p = capi.raycast_params_default(cfgs[0])
        want = batch_render_spec(batch, cfgs, p, c.pose)
        assert len(np.unique(want["member"])) >= 2

        def run(b):
            outs = {"depth": b.out("depth", f32, n), "normal": b.out("normal", f32, 3 * n, per_pixel=3),
                    "member": b.out("member", np.int32, n)}
            batch.raycast_device(c.pose, outs["depth"].ptr, outs["normal"].ptr, outs["member"].ptr, params=p)
            batch.sync()
            return {k: o.read() for k, o in outs.items()}

        def check(plain):
            for name in plain:
                t_ray.same_bits(plain[name], want[name].ravel(), f"plain batch render vs raycast_spec: {name}")

        hold(cuda, c.hw, c.median, run, check, f"batch raycast {cb.pair_id(pair)}")


# ------------------------------------------------------------------------------------------------------------------------
# association: counts exact
# ------------------------------------------------------------------------------------------------------------------------
@sizes
def test_associate_count(cuda, hw):
    """Member, render depth, live depth and K = 3 masks, all the caller's.  At 32 x 24 the host picks associate_count<true> at
    residue 0 (W % 4 == 0, 16-byte aligned images, 4-byte aligned masks) and associate_count<false> at the element residue."""
    rng = np.random.default_rng(hw[0] * 100 + hw[1])
    p = t_assoc.count_params(hw)
    member, rd, d, masks = t_assoc.crafted(rng, hw[0], hw[1], cb.K_MASKS, 5, p, False)
    want = asp.counts(member, rd, d, masks, 5, asp.from_ctypes(p))
    assert asp.split(want, cb.K_MASKS, 5)[0].sum() > 0

    def run(b):
        bm, br, bd, bk = b.inp(member, "member"), b.inp(rd, "depth"), b.inp(d, "depth"), b.inp(masks, "mask")
        return {"counts": capi.associate_count(p, bm.ptr, br.ptr, 5, bd.ptr, bk.ptr, cb.K_MASKS)[0]}

    hold(cuda, hw, 1.5, run, against({"counts": want}), f"associate_count {hw}")


@pairs4
def test_batch_associate(cuda, pair):
    """The product call: the live frame and the K = 3 masks are the caller's; the counts equal the spec applied to the
    batch's own render, the assignment the spec's."""
    c = cb.case(*pair)
    cfgs, n = cb.batch_configs(c), c.hw[0] * c.hw[1]
    live = c.depths[1]
    with capi.Batch(cfgs) as batch:
        fused_batch(batch, c, cuda)
        p = capi.associate_params_default(cfgs[0])
        p.min_pixels = 5
        rd, rm = Plain(cuda, dtype=f32, n=n), Plain(cuda, dtype=np.int32, n=n)
        batch.raycast_device(c.pose, rd.ptr, None, rm.ptr, params=p.ray)
        batch.sync()
        sp = asp.from_ctypes(p)
        want = asp.counts(rm.read().reshape(c.hw), rd.read().reshape(c.hw), live, c.mask_stack, 3, sp)
        want_assign, want_iou = asp.assign(want, cb.K_MASKS, 3, sp)
        assert asp.split(want, cb.K_MASKS, 3)[0][:, :, 0].sum() > 0

        def run(b):
            d, m = b.inp(live, "depth"), b.inp(c.mask_stack, "mask")
            out = batch.associate(c.pose, d.ptr, m.ptr, cb.K_MASKS, params=p)
            return {"counts": out["counts"], "assign": out["assign"], "iou": out["iou"]}

        hold(cuda, c.hw, c.median, run, against({"counts": want, "assign": want_assign, "iou": want_iou}),
             f"batch associate {cb.pair_id(pair)}")


# ------------------------------------------------------------------------------------------------------------------------
# segmentation
# ------------------------------------------------------------------------------------------------------------------------
def segment_inputs(hw):
    """A wall with two raised boxes (one touching the first pixel's corner, one the last's), seen by a pinhole of the image's
    size: DoN responds along the boxes' edges and the corners' pixels are valid points other pixels' normals take in."""
    h, w = hw
    K = t_seg.camera(640.0 / w)
    depth = np.full(hw, 1.2, f32)
    depth[: h // 3, : w // 3] = 1.1
    depth[h // 2:, w // 2:] = 1.0
    depth += (np.arange(w, dtype=f32) * f32(0.0005))[None, :]
    masks = np.zeros((cb.K_MASKS, h, w), np.uint8)                    # bytes around the threshold of 128
    masks[0, : h // 2 + 2, : w // 2 + 2] = 255
    masks[1, h // 3:, w // 3:] = 200
    masks[2] = np.where(np.random.default_rng(h * w).random(hw) < 0.02, 127, 128)
    masks[2].flat[0], masks[2].flat[-1] = 0, 255
    return t_seg.lib_params(hw, K, min_cluster=3, small_radius_m=0.05, large_radius_m=0.3, inset=1), depth, masks


@sizes
@pytest.mark.parametrize("with_don", [True, False], ids=["don", "don-NULL"])
def test_segment_depth(cuda, hw, with_don):
    """Depth in; cluster and, unless NULL, DoN OUT."""
    p, depth, _ = segment_inputs(hw)
    sp = ss.from_ctypes(p)
    want_don, want_cl, want_n = ss.segment_depth(depth, sp, t_seg.spec_values(("caller", hw), depth, sp))
    assert want_n >= 3
    n = hw[0] * hw[1]
    with capi.Segmenter(*hw) as seg:
        def run(b):
            d, cl = b.inp(depth, "depth"), b.out("cluster", np.int32, n)
            don = b.out("don", f32, n) if with_don else None
            res = {"n": np.array([seg.segment_depth(p, d.ptr, cl.ptr, None if don is None else don.ptr)]), "cluster": cl.read()}
            if with_don:
                res["don"] = don.read()
            return res

        def check(plain):
            assert plain["n"][0] == want_n
            t_seg.differ("clusters", plain["cluster"], want_cl.ravel())
            if with_don:
                t_seg.differ("DoN", plain["don"], want_don.ravel())

        hold(cuda, hw, 1.2, run, check, f"segment_depth {hw}")


@sizes
def test_segment_refine_and_frame(cuda, hw):
    """refine_masks: cluster image and masks in, masks OUT; segment_frame: depth and masks in, masks and clusters OUT."""
    p, depth, masks = segment_inputs(hw)
    sp = ss.from_ctypes(p)
    _, want_cl, want_n = ss.segment_depth(depth, sp, t_seg.spec_values(("caller", hw), depth, sp))
    want_out, want_counts = ss.refine(want_cl, want_n, masks, sp)
    assert want_out.any()
    n = hw[0] * hw[1]
    with capi.Segmenter(*hw) as seg:
        def refine(b):
            cl, m = b.inp(want_cl.astype(np.int32), "cluster"), b.inp(masks, "mask")
            out = b.out("masks", np.uint8, masks.size)
            size, inside = seg.refine_masks(p, cl.ptr, want_n, m.ptr, cb.K_MASKS, out.ptr)
            return {"masks": out.read(), "counts": np.concatenate([size, inside.ravel()])}

        def check_refine(plain):
            t_seg.differ("counts", plain["counts"], want_counts)
            t_seg.differ("refined masks", plain["masks"], want_out.ravel())

        hold(cuda, hw, 1.2, refine, check_refine, f"refine_masks {hw}")

        def frame(b):
            d, m = b.inp(depth, "depth"), b.inp(masks, "mask")
            out, cl = b.out("masks", np.uint8, masks.size), b.out("cluster", np.int32, n)
            k = seg.segment_frame(p, d.ptr, m.ptr, cb.K_MASKS, out.ptr, cl.ptr)
            return {"masks": out.read(), "cluster": cl.read(), "n": np.array([k])}

        def check_frame(plain):
            assert plain["n"][0] == want_n
            t_seg.differ("clusters", plain["cluster"], want_cl.ravel())
            t_seg.differ("refined masks", plain["masks"], want_out.ravel())

        hold(cuda, hw, 1.2, frame, check_frame, f"segment_frame {hw}")


# ------------------------------------------------------------------------------------------------------------------------
# slices out, a device halo in
# ------------------------------------------------------------------------------------------------------------------------
@pairs
def test_copy_slices_to_device(cuda, pair):
    """Two whole z-slices of TSDF and weights into caller buffers."""
    c = cb.case(*pair)
    n = 2 * c.dims[0] * c.dims[1]
    with capi.Volume(c.cfg) as vol:
        fused(vol, c, cuda, False)
        want = dict(zip(("tsdf", "weight"), vol.copy_slices(5, 2)))
        assert (want["weight"] > 0).any()

        def run(b):
            t, w = b.out("tsdf", f32, n), b.out("weight", f32, n)
            vol.copy_slices_to_device(5, 2, t.ptr, w.ptr)
            return {"tsdf": t.read(), "weight": w.read()}

        hold(cuda, (c.dims[1], c.dims[0]), 0.99, run, against(want), f"copy_slices {cb.pair_id(pair)}")


@pairs
def test_extraction_with_a_device_halo(cuda, oracle, pair):
    """Crossings and mesh of the lower half slab with the upper half's first slice handed over in device memory.  The halo
    arrays take the score role's fills: a NaN, or 0.99, which as a weight passes the 0.9 threshold."""
    c = cb.case(*pair)
    dims, cut = c.dims, c.dims[2] // 2
    state = None
    for k in range(3):
        state = cb.integrate(oracle, c.cfg, c.depths[k], state)
    slice_n = dims[0] * dims[1]
    lo = (state[0][:cut * slice_n], state[1][:cut * slice_n])
    halo = (state[0][cut * slice_n:(cut + 1) * slice_n], state[1][cut * slice_n:(cut + 1) * slice_n])
    want = {"crossings": oracle.zero_crossings(lo[0], lo[1], dims[:2], 0, cut, c.vs, c.origin, halo=halo),
            "mesh": oracle.mesh_triangles(lo[0], lo[1], dims[:2], 0, cut, c.vs, c.origin, halo=halo)}
    assert len(want["crossings"]) > len(oracle.zero_crossings(lo[0], lo[1], dims[:2], 0, cut, c.vs, c.origin)), \
        "the halo must add crossings"
    cfg = capi.make_config(dims, c.vs, c.origin, K=c.K, im_height=c.hw[0], im_width=c.hw[1], z_begin=0, z_end=cut)
    with capi.Volume(cfg) as vol:
        vol.upload(*lo)

        def run(b):
            ht, hw_ = b.inp(halo[0], "score"), b.inp(halo[1], "score")
            return {"crossings": vol.extract_crossings((ht.ptr, hw_.ptr)).ravel(), "mesh": vol.extract_mesh((ht.ptr, hw_.ptr)).ravel()}

        hold(cuda, (dims[1], dims[0]), 0.99, run, against(want), f"halo {cb.pair_id(pair)}")


# ------------------------------------------------------------------------------------------------------------------------
# tracking: every image the calls take
# ------------------------------------------------------------------------------------------------------------------------
def track_setup(c, cfg):
    p = capi.track_params_default(cfg)
    p.n_levels, p.min_inliers, p.cos_normal_thresh = 2, 20, t_track.COS_WIDE
    p.iters[:] = [2, 2, 0]
    shift = np.eye(4, dtype=f32)
    shift[2, 3] = 0.3 * c.vs                        # the camera a third of a voxel nearer than where the live frame was taken
    return p, shift.ravel()


def within_bound(got, terms, what):
    """tests/test_gpu_track_exact.py's rule for a system: the pair count exact, every entry within track_cases.system_bound."""
    want, bound = tc.system_bound(terms)
    assert got[28] == len(terms), f"{what}: {got[28]} pairs, spec {len(terms)}"
    bad = ~(np.abs(got - want) <= bound)
    assert not bad.any(), f"{what}: entries {np.nonzero(bad)[0].tolist()} differ: {got[bad]} vs {want[bad]}"


@pairs
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_volume_track_and_system(cuda, pair, masked):
    """The live frame and its mask are the caller's.  Systems are held by the existing bound (their tests do not establish
    bit equality between runs); tsdf_track's result is compared field by field, as tests/test_gpu_track.py's determinism test."""
    c = cb.case(*pair)
    live, mask = c.depths[0], c.masks[2] if masked else None
    with capi.Volume(c.cfg) as vol:
        fused(vol, c, cuda, False)
        p, guess = track_setup(c, c.cfg)
        model = t_track.device_model(vol, p, guess)
        M = ts.relative(t_track.c2b(c.cfg, guess), t_track.c2b(c.cfg, c.pose))
        terms, _ = ts.pair_terms((live, mask), model, 0, M[:, :3].astype(f32), M[:, 3].astype(f32), ts.from_ctypes(p))
        assert len(terms) > 50
        t_track._torch = cuda                          # its own check of the call on buffers it makes itself
        t_track.check_system(vol, c.cfg, p, live, mask, guess, c.pose, 0, f"track_system {cb.pair_id(pair)}")

        def run(b):
            d = b.inp(live, "depth")
            m = None if mask is None else b.inp(mask, "mask")
            mp = None if m is None else m.ptr
            A, bb, r2, n = vol.track_system(d.ptr, guess, c.pose, level=0, params=p, mask_ptr=mp)
            pose, stats = vol.track(d.ptr, guess, params=p, mask_ptr=mp)
            return {"system": np.concatenate([A[np.triu_indices(6)], bb, [r2, n]]), "pose": pose.ravel(),
                    "stats": np.array([stats["status"], stats["inliers"]] + stats["iters_run"], np.float64),
                    "rmse": np.array([stats["rmse"]], f32)}

        def check(plain):
            within_bound(plain["system"], terms, "plain track_system vs track_spec")

        def equal(got, plain, what):
            within_bound(got["system"], terms, f"{what}: track_system vs track_spec")
            for name in ("pose", "stats", "rmse"):
                same_bits(got[name], plain[name], f"{what}: track {name}")

        hold(cuda, c.hw, c.median, run, check, f"track {cb.pair_id(pair)}", equal=equal)


@pairs4
def test_batch_track_systems_and_member_systems(cuda, pair):
    """Batch.track_system and Batch.track take the live frame and a mask; track_member_systems also the model's depth, normal
    and member images.  The member systems are held to batch_track_spec through the bound, as their own tests do."""
    c = cb.case(*pair)
    cfgs, n = cb.batch_configs(c), c.hw[0] * c.hw[1]
    live, mask = c.depths[0], c.masks[2]
    with capi.Batch(cfgs) as batch:
        fused_batch(batch, c, cuda)
        p, guess = track_setup(c, cfgs[0])
        rd, rn, rm = Plain(cuda, dtype=f32, n=n), Plain(cuda, dtype=f32, n=3 * n), Plain(cuda, dtype=np.int32, n=n)
        batch.raycast_device(guess, rd.ptr, rn.ptr, rm.ptr, params=p.ray)
        batch.sync()
        model = (rd.read().reshape(c.hw), rn.read().reshape(c.hw + (3,)), rm.read().reshape(c.hw))
        M = ts.relative(guess, c.pose)
        terms, owner, _ = bts.member_terms((live, mask), model, 3, 0, M, ts.from_ctypes(p))
        assert len(terms) > 50

        def run(b):
            d, m = b.inp(live, "depth"), b.inp(mask, "mask")
            md, mn, mm = b.inp(model[0], "depth"), b.inp(model[1], "normal", per_pixel=3), b.inp(model[2], "member")
            res = {"batch_system": batch.track_system(d.ptr, guess, c.pose, level=0, params=p, mask_ptr=m.ptr),
                   "member_systems": capi.track_member_systems(p, md.ptr, mn.ptr, mm.ptr, 3, d.ptr, guess, c.pose, level=0,
                                                               mask_ptr=m.ptr)}
            pose, stats, _ = batch.track(d.ptr, guess, params=p, mask_ptr=m.ptr, want_systems=False)
            res["pose"] = pose.ravel()
            res["stats"] = np.array([stats["status"], stats["inliers"]] + stats["iters_run"], np.float64)
            return res

        def held(res, what):
            for name in ("batch_system", "member_systems"):
                t_btrack.check_member_systems(res[name], terms, owner, 3, f"{what}: {name} vs batch_track_spec")

        def equal(got, plain, what):
            held(got, what)
            for name in ("pose", "stats"):
                same_bits(got[name], plain[name], f"{what}: batch track {name}")

        hold(cuda, c.hw, c.median, run, lambda plain: held(plain, "plain"), f"batch track {cb.pair_id(pair)}", equal=equal)
