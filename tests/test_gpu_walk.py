"""Random call sequences on one volume handle, and on one batch, against a CPU model of the whole handle
(tests/walk_cases.py; tests/test_walk_spec.py holds the scripts themselves to conditions): every step of a seeded script runs
on the device and in the model, and every observing step -- download, labels, colour, surface count, extent, raycast, the
counts of a merge -- is compared at once, bit for bit and field for field.  Deferral, kernel variants, brick shapes and
streams change between the steps and must change no result.  A failure names the seed, the step and the last five ops; the
case's id replays it alone.

The summary words (tests/summary_spec.py) are read at every download and must be sound for the arrays just downloaded:
no word may say more than its segment bears out, whatever launched.  The "runs" class keeps the one-frame kernel's weight
runs alive under every op and holds bit 2 and the count of every word to the prediction after every mutating step (the whole
word after reset and after a rebuild); test_walk_batch_runs does the same for a batch with a row-mapped member.  A failure
there names the segment and the word in hex as well."""
import ctypes as C

import numpy as np
import pytest

import summary_spec as ss
import walk_cases as wc
from semantic_slam_amd import capi

pytestmark = pytest.mark.gpu

f32 = np.float32
H, W = wc.IM_HW


def fuse_params(write):
    p = capi.FuseParams()
    p.weight_thresh, p.agree_tol, p.write = wc.WEIGHT_THRESH, 0.4, write
    return p


def extent_params(band, margin):
    p = capi.ExtentParams()
    p.weight_thresh, p.band, p.margin = wc.WEIGHT_THRESH, band, margin
    return p


def raycast_params(cfg):
    p = capi.RaycastParams()
    p.cam_K[:] = [float(x) for x in wc.K_SMALL]
    p.im_height, p.im_width = H, W
    p.near_m, p.far_m, p.weight_thresh = 0.0, cfg.max_depth, wc.WEIGHT_THRESH
    return p


def at_pixels(images, px):
    return {k: v[px[:, 1], px[:, 0]] for k, v in images.items()}


class DeviceArray:
    """n float32 values at a device address, for torch.as_tensor."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 2}


def sound_download(vol, lay):
    """The arrays, with the summary words read beside them held to what the arrays bear out."""
    words = vol.summary_words()
    t, w = vol.download()
    ss.assert_sound(lay, words, t, w, "summary words at a download")
    return t, w


class Inputs:
    """The script's arrays on the device, uploaded and synchronised before the walk starts, and the output images of device
    renders."""

    def __init__(self, cuda, inp):
        dev = lambda a: cuda.from_numpy(np.array(a)).cuda()                    # (a copy: shared frames are read-only)
        self.depth = [dev(f["depth"]) for f in inp["frames"]]
        self.masks = [dev(m) for m in inp["masks"]]
        self.labels = [(dev(l.view(np.int16)), dev(s)) for l, s in inp.get("labels", [])]
        self.rgb = [dev(c) for c in inp.get("rgb", [])]
        self.out = {"depth": cuda.empty((H, W), dtype=cuda.float32, device="cuda"),
                    "normal": cuda.empty((H, W, 3), dtype=cuda.float32, device="cuda"),
                    "label": cuda.empty((H, W), dtype=cuda.int16, device="cuda"),
                    "colour": cuda.empty((H, W), dtype=cuda.int32, device="cuda"),
                    "member": cuda.empty((H, W), dtype=cuda.int32, device="cuda")}
        cuda.cuda.synchronize()

    def read(self, names):
        views = {"label": np.uint16, "colour": np.uint32}                # torch has no arithmetic on them; the bits are theirs
        host = {k: self.out[k].cpu().numpy() for k in names}
        return {k: a.view(views[k]) if k in views else a for k, a in host.items()}


class DeviceWalk:
    """The script's steps on the device: apply(op, arguments) returns what an observing step answers."""

    def __init__(self, cuda, inputs, tmp_path):
        self.inp, self.dev = inputs, Inputs(cuda, inputs)
        self.streams = [cuda.cuda.Stream(), cuda.cuda.Stream()]    # the caller's streams: the handle's and the partner's
        self.on_caller_stream = False
        self.labels = self.colour = False
        self.path = str(tmp_path / "state.bin")
        self.vol, self.partner = capi.Volume(inputs["cfg"]), capi.Volume(inputs["partner_cfg"])
        self.ray = raycast_params(inputs["cfg"])
        self.cuda = cuda
        self.lay = ss.Layout((inputs["cfg"].dim_x, inputs["cfg"].dim_y, inputs["cfg"].dim_z))

    def close(self):
        self.vol.close()
        self.partner.close()

    def apply(self, op, a):
        v, inp, dev = self.vol, self.inp, self.dev
        fr = inp["frames"][a["frame"]] if "frame" in a else None
        d_ptr = dev.depth[a["frame"]].data_ptr() if "frame" in a else None
        if op == "integrate":
            buf = fr["depth"].copy()
            v.integrate(buf, fr["pose"])
            buf[:] = -7.0                                   # the caller's buffer is free again when the call returns
        elif op == "integrate_u16":
            buf = fr["raw"].copy()
            v.integrate_u16(buf, fr["pose"], 5000.0, *a["steps"])
            buf[:] = 12345
        elif op == "integrate_rgbd":
            v.integrate_rgbd(fr["depth"], inp["rgb"][a["rgb"]], fr["pose"])
        elif op == "integrate_device":
            v.integrate_device(d_ptr, fr["pose"])
        elif op == "integrate_cam2base":
            v.integrate_cam2base(d_ptr, fr["pose"])
        elif op == "integrate_masked_device":
            v.integrate_masked_device(d_ptr, dev.masks[a["mask"]].data_ptr(), fr["pose"])
        elif op == "integrate_colour_device":
            v.integrate_device(d_ptr, fr["pose"])
            v.integrate_colour_device(d_ptr, dev.rgb[a["rgb"]].data_ptr(), fr["pose"])
        elif op == "integrate_labels_device":
            lab, sc = dev.labels[a["label"]]
            v.integrate_labels_device(d_ptr, lab.data_ptr(), sc.data_ptr(), fr["pose"])
        elif op == "integrate_frames_device":
            masks = None if a["masks"] is None else [None if k is None else dev.masks[k].data_ptr() for k in a["masks"]]
            v.integrate_frames_device([dev.depth[i].data_ptr() for i in a["frames"]],
                                      np.stack([inp["frames"][i]["pose"] for i in a["frames"]]), masks)
        elif op == "integrate_frames_labels_device":
            v.integrate_frames_labels_device([dev.depth[i].data_ptr() for i in a["frames"]],
                                             [dev.labels[j][0].data_ptr() for j in a["labels"]],
                                             [dev.labels[j][1].data_ptr() for j in a["labels"]],
                                             np.stack([inp["frames"][i]["pose"] for i in a["frames"]]))
        elif op == "reset":
            v.reset()
        elif op == "upload":
            v.upload(*inp["states"][a["state"]])
        elif op == "save_state":
            v.save_state(self.path)
        elif op == "load_state":
            v.load_state(self.path)
        elif op == "fuse_from":
            return v.fuse_from(self.partner, fuse_params(1))
        elif op == "fuse_into":
            return self.partner.fuse_from(v, fuse_params(1))
        elif op == "fuse_dry":
            return v.fuse_from(self.partner, fuse_params(0))
        elif op == "set_deferral":
            v.set_deferral(a["n"])
        elif op == "set_kernel_variant":
            v.set_kernel_variant(a["variant"])
        elif op == "set_brick_shape":
            v.set_brick_shape(*a["shape"])
        elif op == "set_stream":
            v.set_stream(self.streams[0].cuda_stream if a["caller"] else None)
            self.on_caller_stream = a["caller"]
        elif op == "sync":
            v.sync()
        elif op == "labels_enable":
            v.labels_enable(0.5)
            self.labels = True
        elif op == "colour_enable":
            v.colour_enable()
            self.colour = True
        elif op == "download":
            return sound_download(v, self.lay)
        elif op == "summary_words":                         # (the words first: the download must not be what makes them right)
            return (v.summary_words(),) + v.download()
        elif op == "refresh_external":
            self.refresh_external(a["patch"])
        elif op == "download_labels":
            return v.download_labels()
        elif op == "download_colour":
            return v.download_colour()
        elif op == "count_surface":
            return v.count_surface(wc.WEIGHT_THRESH)
        elif op == "extent":
            return v.extent(extent_params(a["band"], a["margin"])).as_dict()
        elif op == "raycast":
            return self.raycast(inp["views"][a["view"]], a["device"])
        elif op == "partner":
            return self.apply_partner(a)
        else:
            raise AssertionError(f"no such op: {op}")
        return None

    def refresh_external(self, patch):
        """The header's contract for external writes: the arrays through tsdf_device_ptrs, written on the handle's stream,
        then tsdf_refresh_summary."""
        v, torch = self.vol, self.cuda
        idx, t, w = wc.external_patch(self.lay, patch)
        n = v.n_voxels
        assert idx.dtype == np.int64 and 0 <= idx.min() and idx.max() < n == self.lay.n_vox and t.size == w.size == idx.size
        t_ptr, w_ptr = v.device_ptrs()
        stream = C.c_void_p()
        capi.check(v.lib.tsdf_get_stream(v._h, C.byref(stream)), "tsdf_get_stream")
        with torch.cuda.stream(torch.cuda.ExternalStream(stream.value)):
            i = torch.from_numpy(idx).cuda()
            for ptr, values in ((t_ptr, t), (w_ptr, w)):
                torch.as_tensor(DeviceArray(ptr, n), device="cuda").index_put_((i,), torch.from_numpy(values).cuda())
        capi.check(v.lib.tsdf_refresh_summary(v._h), "tsdf_refresh_summary")

    def raycast(self, view, device):
        v, out = self.vol, self.dev.out
        names = ["depth", "normal"] + ["label"] * self.labels + ["colour"] * self.colour
        if device:
            v.raycast_device(view, out["depth"].data_ptr(), out["normal"].data_ptr(), out["label"].data_ptr() if self.labels else None,
                             out["colour"].data_ptr() if self.colour else None, params=self.ray)
            if self.on_caller_stream:                       # the images are written in the order of the caller's stream
                self.streams[0].synchronize()
            else:
                v.sync()
            images = self.dev.read(names)
        else:
            images = v.raycast(view, params=self.ray, normals=True, labels=self.labels, colour=self.colour)
        return at_pixels(images, self.inp["pixels"])

    def apply_partner(self, a):
        p, sub = self.partner, a["op"]
        if sub == "integrate":
            fr = self.inp["frames"][a["frame"]]
            p.integrate(fr["depth"], fr["pose"])
        elif sub == "integrate_device":
            p.integrate_device(self.dev.depth[a["frame"]].data_ptr(), self.inp["frames"][a["frame"]]["pose"])
        elif sub == "upload":
            p.upload(*self.inp["partner_states"][a["state"]])
        elif sub == "reset":
            p.reset()
        elif sub == "set_deferral":
            p.set_deferral(a["n"])
        elif sub == "set_stream":
            p.set_stream(self.streams[1].cuda_stream if a["caller"] else None)
        elif sub == "download":
            return p.download()
        return None


def walk(steps, device, model, compare, what):
    """Every step on the device and in the model; what a step answers is compared at once."""
    for i, (op, a) in enumerate(steps):
        try:
            got = device.apply(op, a)
            want = model.apply(op, a)
            assert (got is None) == (want is None), f"the device answers {type(got).__name__}, the model {type(want).__name__}"
            if want is not None:
                compare(op, got, want)
            if op == "fuse_from":                           # a merge leaves its source's bits as they were
                wc.compare("partner", device.partner.download(), (model.partner.t, model.partner.w))
        except Exception as e:
            last = ", ".join(f"{j}:{o}" for j, (o, _) in list(enumerate(steps))[max(0, i - 4):i + 1])
            raise AssertionError(f"{what}, step {i} of {len(steps)}: {op} {a}: {e}\nlast ops: {last}") from e


@pytest.mark.parametrize("seed,cls", [(s, c) for c in wc.CLASSES for s in wc.SEEDS[c]], ids=lambda x: str(x))
def test_walk_volume(cuda, oracle, tmp_path, seed, cls):
    steps = wc.script(seed, cls)
    device = DeviceWalk(cuda, steps.inputs, tmp_path)
    try:
        walk(steps, device, wc.Walk(oracle, steps.inputs, predict=cls == "runs"), wc.compare, f"walk seed {seed} on the {cls} grid")
    finally:
        device.close()


class DeviceBatchWalk:
    def __init__(self, cuda, inputs):
        self.inp, self.dev = inputs, Inputs(cuda, inputs)
        self.batch = capi.Batch(inputs["cfgs"])
        self.batch.volumes[0].set_deferral(32)              # the batch collects frames (tests/test_gpu_fuse.py)
        self.ray = raycast_params(inputs["cfgs"][0])

    def close(self):
        self.batch.close()

    def apply(self, op, a):
        b, inp, dev = self.batch, self.inp, self.dev
        m = b.volumes[a["member"]] if "member" in a else None
        if op == "integrate":
            b.integrate_device(dev.depth[a["frame"]].data_ptr(), [None if k is None else dev.masks[k].data_ptr() for k in a["masks"]],
                               inp["frames"][a["frame"]]["pose"])
        elif op == "fuse":
            return b.volumes[a["dst"]].fuse_from(b.volumes[a["src"]], fuse_params(a["write"]))
        elif op == "extent":
            return m.extent(extent_params(a["band"], a["margin"])).as_dict()
        elif op == "extents":
            return [e.as_dict() for e in b.extents(extent_params(a["band"], a["margin"]))]
        elif op == "raycast":
            return at_pixels(m.raycast(inp["views"][a["view"]], params=self.ray), inp["pixels"])
        elif op == "batch_raycast":
            out = dev.out
            b.raycast_device(inp["views"][a["view"]], out["depth"].data_ptr(), out["normal"].data_ptr(), out["member"].data_ptr(),
                             params=self.ray)
            b.sync()
            return at_pixels(dev.read(["depth", "normal", "member"]), inp["pixels"])
        elif op == "download":
            return m.download()
        elif op == "upload":
            m.upload(*inp["states"][a["member"]])
        elif op == "reset":
            m.reset()
        else:
            raise AssertionError(f"no such op: {op}")
        return None


@pytest.mark.parametrize("seed", wc.BATCH_SEEDS)
def test_walk_batch(cuda, oracle, seed):
    steps = wc.batch_script(seed)
    device = DeviceBatchWalk(cuda, steps.inputs)
    try:
        walk(steps, device, wc.BatchWalk(oracle, steps.inputs), wc.compare_batch, f"batch walk seed {seed}")
    finally:
        device.close()


class DeviceBatchRunsWalk:
    """walk_cases.batch_runs_script on the device: every member handle launches one frame per call, so the batch applies every
    frame at once with its batched kernel."""

    def __init__(self, cuda, inputs):
        self.inp, self.dev = inputs, Inputs(cuda, inputs)
        self.batch = capi.Batch(inputs["cfgs"])
        for v in self.batch.volumes:
            v.set_deferral(0)
        self.lays = [ss.Layout((c.dim_x, c.dim_y, c.dim_z)) for c in inputs["cfgs"]]

    def close(self):
        self.batch.close()

    def apply(self, op, a):
        b, inp, dev = self.batch, self.inp, self.dev
        i = a.get("member")
        m = b.volumes[i] if i is not None else None
        if op == "integrate":
            b.integrate_device(dev.depth[a["frame"]].data_ptr(), [None if k is None else dev.masks[k].data_ptr() for k in a["masks"]],
                               inp["frames"][a["frame"]]["pose"])
        elif op == "member_integrate":
            m.integrate_device(dev.depth[a["frame"]].data_ptr(), inp["frames"][a["frame"]]["pose"])
        elif op == "upload":
            m.upload(*inp["states"][i][a["state"]])
        elif op == "reset":
            m.reset()
        elif op == "fuse":
            return b.volumes[a["dst"]].fuse_from(b.volumes[a["src"]], fuse_params(a["write"]))
        elif op == "summary_words":
            return (m.summary_words(),) + m.download()
        elif op == "download":
            return sound_download(m, self.lays[i])
        else:
            raise AssertionError(f"no such op: {op}")
        return None


@pytest.mark.parametrize("seed", wc.BATCH_RUNS_SEEDS)
def test_walk_batch_runs(cuda, oracle, seed):
    steps = wc.batch_runs_script(seed)
    device = DeviceBatchRunsWalk(cuda, steps.inputs)
    try:
        walk(steps, device, wc.BatchRunsWalk(oracle, steps.inputs), wc.compare_batch_runs, f"batch runs walk seed {seed}")
    finally:
        device.close()
