"""Seeded random walks over the C ABI of one volume handle, and of one batch (test infrastructure, no GPU): script() and
batch_script() make the steps and every input array from a seed, Tracker restates what the host code does with a step as far
as a script has to know it (which frames are collected, which launches a step queues), and Walk / BatchWalk apply the steps
to a CPU model assembled from the oracle and the restatements (fuse_spec, extent_spec, raycast_spec).  The model is frame by
frame: it knows nothing of deferral, kernel variants, brick shapes or streams, none of which may change a result.
tests/test_walk_spec.py holds the scripts to conditions on the CPU; tests/test_gpu_walk.py runs them on the device.

A step is (op, arguments); arguments name input arrays by their index in script.inputs.  Ops of the handle under test:

  mutating   integrate (host frame, deferred), integrate_u16, integrate_rgbd, integrate_device, integrate_cam2base,
             integrate_masked_device, integrate_frames_device, integrate_labels_device, integrate_frames_labels_device,
             integrate_colour_device (integrate_device and the colour pass of the same frame, as the header asks), reset,
             upload, load_state (the state the last save_state wrote), fuse_from (the partner merged into the handle),
             fuse_into (the handle merged into the partner)
  policy     set_deferral, set_kernel_variant, set_brick_shape, set_stream, sync, labels_enable, colour_enable, save_state
  observing  download, download_labels, download_colour, count_surface, extent, raycast, fuse_dry (fuse_from with write = 0)
  partner    a step of the second, smaller volume: integrate, integrate_device, upload, reset, set_deferral, set_stream,
             download

The fourth class, "runs", keeps the weight runs of the one-frame kernel alive (csrc/host_derive.h, "the summary word"): a grid
the camera sees whole, frames that update whole segments, uploaded states whose weights are counts, deferral 0 or 1 and
variants 0, 3 and 7 most of the time, so that most frames are integrate_tile launches that take weights from the words.  It adds

  mutating   refresh_external (a seeded patch written into the device arrays through tsdf_device_ptrs, then tsdf_refresh_summary)
  observing  summary_words (tsdf_summary_words: held to summary_spec.unsound against the download of the same step and, for
             bit 2 and the count, to summary_spec.Predictor)

and follows every mutating step with summary_words and download.  batch_runs_script() does the same for a batch with one
row-mapped member.
"""
import functools

import numpy as np

import extent_spec as es
import fuse_spec as fs
import raycast_spec as rs
import summary_spec as ss
from fuse_cases import IM_HW, K_SMALL
from semantic_slam_amd import capi, synth

f32 = np.float32

# the three shape classes of tests/test_gpu_deferral.py.  The grids are wider than any camera of the walk sees (about 1.4 m
# at the near face), so a strip at both x ends stays fresh whatever is integrated; the partner is centred on the grid's centre.
# "runs" is the grid of tests/test_gpu_weight_runs.py on synth.sband_volume's origin: two segments per row, an odd dim_y, and
# every voxel inside the camera's view and the truncation band; its partner covers a tenth of the x range.
CLASSES = {
    "row": dict(dims=(256, 24, 12), vs=0.006, partner=(32, 20, 12), partner_vs=0.0075),       # dim_x % 256 == 0
    "flat": dict(dims=(200, 24, 12), vs=0.008, partner=(28, 22, 10), partner_vs=0.01),        # dim_x % 4 == 0 only
    "scalar": dict(dims=(37, 20, 12), vs=0.05, partner=(25, 13, 9), partner_vs=0.0625),       # dim_x % 4 != 0
    "runs": dict(dims=(512, 9, 6), vs=0.005, partner=(40, 8, 6), partner_vs=0.00625, trunc=synth.SBAND_TRUNC),
}
SEEDS = {"row": range(48), "flat": range(48), "scalar": range(24), "runs": range(32)}
BATCH_SEEDS = range(6)
BATCH_RUNS_SEEDS = range(4)

FRAME_OPS = ["integrate", "integrate_u16", "integrate_rgbd", "integrate_device", "integrate_cam2base",
             "integrate_masked_device", "integrate_frames_device", "integrate_labels_device", "integrate_frames_labels_device",
             "integrate_colour_device"]
MUTATING = FRAME_OPS + ["reset", "upload", "load_state", "fuse_from", "fuse_into"]
# tsdf_labels_enable and tsdf_colour_enable refuse rows that are no multiple of 4 voxels; nothing else of the walk does
NEEDS_LABELS = {"integrate_labels_device", "integrate_frames_labels_device", "download_labels"}
NEEDS_COLOUR = {"integrate_rgbd", "integrate_colour_device", "download_colour"}
POLICY = ["set_deferral", "set_kernel_variant", "set_brick_shape", "set_stream", "sync", "labels_enable", "colour_enable",
          "save_state"]
OBSERVING = ["download", "download_labels", "download_colour", "count_surface", "extent", "raycast", "fuse_dry"]
VARIANTS = (0, 1, 3, 7, 8)           # capi.SHIPPED_VARIANTS: both builds know them
FUSING = (0, 7, 8)                   # csrc/host_derive.h, decode_variant: sequences and collected frames go through fused launches
DEFERRALS = (0, 1, 5, 32)
MAX_FRAMES_PER_LAUNCH = 32           # kMaxFramesPerLaunch
N_FRAMES, N_MASKS, N_LABELS, N_RGB, N_STATES = 8, 3, 2, 2, 2
N_PIXELS = 240
WEIGHT_THRESH = 0.9


RUNS_ONLY = {"refresh_external", "summary_words"}      # the ops of the "runs" class alone
RUNS_VARIANTS = (0, 3, 7)            # one-frame launches under them are integrate_tile launches on rows of 256 voxels
RUNS_DEFERRALS = (0, 1)
WHOLE, BROKEN = (0, 2, 4, 6), (3, 7)  # frames of the "runs" class by kind (make_runs_inputs)


def legal(op, cls):
    if op in RUNS_ONLY:
        return cls == "runs"
    return cls != "scalar" or (op not in NEEDS_LABELS and op not in NEEDS_COLOUR)


def mutating_kinds(cls):
    return [op for op in MUTATING + ["refresh_external"] if legal(op, cls)]


def observing_kinds(cls):
    return [op for op in OBSERVING + ["summary_words"] if legal(op, cls)]


# ------------------------------------------------------------------------------------------------------------------------
# geometry and inputs
# ------------------------------------------------------------------------------------------------------------------------
def config(dims, vs, origin, base2world=None, trunc=None):
    return capi.make_config(dims, vs, origin, trunc=trunc, K=K_SMALL, base2world=base2world, im_height=IM_HW[0], im_width=IM_HW[1])


def origin_of(dims, vs):
    """The grid centred on the optical axis, its near face 0.9 m in front of the base camera."""
    return np.array([-dims[0] * vs / 2, -dims[1] * vs / 2, 0.9], f32)


def configs(seed, cls):
    """(main config, partner config): the partner has its own voxel size (ratio 1.2 to 1.25) and a seeded rigid offset."""
    c = CLASSES[cls]
    dims, vs, pdims, pvs = c["dims"], c["vs"], c["partner"], c["partner_vs"]
    origin = synth.sband_volume(dims, vs) if cls == "runs" else origin_of(dims, vs)
    centre = origin.astype(np.float64) + np.array(dims) * vs / 2
    rng = np.random.default_rng([7, seed, list(CLASSES).index(cls)])
    ax, ay, az = rng.uniform(-0.2, 0.2, 3)
    R = synth.rot_z(az) @ synth.rot_y(ay) @ synth.rot_x(ax)
    b2w = fs.pose_about(R, centre, rng.uniform(-0.5, 0.5, 3) * vs)
    p_origin = (centre - np.array(pdims) * pvs / 2).astype(f32)
    return config(dims, vs, origin, trunc=c.get("trunc")), config(pdims, pvs, p_origin, base2world=b2w, trunc=c.get("trunc"))


def scene_of(dims, vs):
    """synth.SurfScene with its back wall two and a half voxels inside the grid's far face, where a ray can hit it."""
    return synth.SurfScene(dims, vs, origin_of(dims, vs) - np.array([0.0, 0.0, 2.5 * vs], f32), K=K_SMALL, h=IM_HW[0], w=IM_HW[1])


@functools.lru_cache(maxsize=None)
def scene_frame(dims, vs, k, quantize):
    """(pose, depth) of the scene from the k-th of 16 poses on its orbit; shared between the seeds that draw it, read-only."""
    scene = scene_of(dims, vs)
    c2w = np.asarray(scene.pose(k, n=16), f32).ravel()
    depth = scene.depth(c2w, quantize=quantize)
    c2w.setflags(write=False)
    depth.setflags(write=False)
    return c2w, depth


def random_state(rng, n):
    """Finite values only (a NaN's payload is not the oracle's to restate): values inside the band, a fifth of the voxels
    fresh (1, 0), a few observed free space (t = 1) and a few with a weight at the threshold."""
    t = rng.uniform(-1.0, 1.0, n).astype(f32)
    w = rng.choice(np.array([1.0, 2.0, 3.0, 7.0], f32), n)
    u = rng.uniform(0, 1, n)
    t[u < 0.2], w[u < 0.2] = 1.0, 0.0
    t[(u >= 0.2) & (u < 0.23)] = 1.0
    w[(u >= 0.23) & (u < 0.26)] = f32(0.9)
    return t, w


def make_inputs(seed, cls, rng):
    if cls == "runs":
        return make_runs_inputs(seed, rng)
    cfg, pcfg = configs(seed, cls)
    dims, vs = CLASSES[cls]["dims"], CLASSES[cls]["vs"]
    h, w = IM_HW
    frames = []
    for k in range(N_FRAMES):
        c2w, depth = scene_frame(dims, vs, int(rng.integers(0, 16)), k % 2 == 0)
        kind = ["noise", "constant", "invalid"][k - 1] if 1 <= k <= 3 else "scene"
        if kind == "noise":                                 # as tests/test_gpu_fuzz.py makes them: invalid values included
            depth = rng.uniform(-0.5, 6.0 * 1.2, (h, w)).astype(f32)
        elif kind == "constant":                            # a plane behind the grid's near face
            depth = np.full((h, w), float(rng.uniform(0.95, 2.0)), f32)
        elif kind == "invalid":
            depth = depth.copy()
            depth[rng.integers(0, h, 20), rng.integers(0, w, 20)] = 0.0
        raw = np.clip(np.round(np.clip(depth, 0, 13).astype(np.float64) * 5000.0), 0, 65535).astype(np.uint16)
        frames.append({"pose": c2w, "depth": depth, "raw": raw, "kind": kind})
    masks = [np.zeros((h, w), np.uint8) for _ in range(N_MASKS)]
    masks[0][20:100, 30:130] = 255
    masks[1][:] = (rng.uniform(0, 1, (h, w)) < 0.7).astype(np.uint8) * 255
    masks[2][:, :int(0.55 * w)] = 255
    labels = [(np.repeat(np.repeat(rng.integers(1, 50, (h // 8, w // 8)), 8, 0), 8, 1).astype(np.uint16),
               rng.uniform(0.3, 1.0, (h, w)).astype(f32)) for _ in range(N_LABELS)]
    rgb = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(N_RGB)]
    n, pn = int(np.prod(dims)), int(np.prod(CLASSES[cls]["partner"]))
    views = [scene_frame(dims, vs, int(rng.integers(0, 16)), True)[0] for _ in range(4)]
    # pixels of a render: three in four in the rows that see the (flat) grids, the rest anywhere
    px = np.stack([rng.integers(0, w, N_PIXELS), np.where(np.arange(N_PIXELS) % 4 == 0, rng.integers(0, h, N_PIXELS),
                                                            rng.integers(h // 2 - 8, h // 2 + 8, N_PIXELS))], 1).astype(np.int64)
    return {"cfg": cfg, "partner_cfg": pcfg, "frames": frames, "masks": masks, "labels": labels, "rgb": rgb,
            "states": [random_state(rng, n) for _ in range(N_STATES)], "partner_states": [random_state(rng, pn)],
            "views": views, "pixels": px}


def runs_state(rng, lay, kind):
    """An uploaded state of the "runs" class: random finite TSDF with a quarter of the segments all ones, and weights of the
    given kind (what a rebuild must make of each: tests/test_gpu_weight_runs.py, UPLOADS)."""
    n, nw = lay.n_vox, lay.n_words
    t = rng.uniform(-0.9, 0.9, n).astype(f32)
    t[(rng.random(nw) < 0.25)[lay.word_of]] = 1.0
    if kind == "uniform":                                   # one count everywhere: a run in every segment
        w = np.full(n, 3.0, f32)
    elif kind == "per_segment":                             # a run in every segment, of four counts; 2^24 - 2 is two launches below the limit
        w = rng.choice(np.array([0.0, 1.0, 5.0, 16777214.0], f32), nw)[lay.word_of]
    elif kind == "one_differs":                             # a run in every segment but one
        w = np.full(n, 3.0, f32)
        w[256 * int(rng.integers(0, nw)) + int(rng.integers(0, 256))] = 4.0
    elif kind == "fraction":                                # no count: no run
        w = np.full(n, 2.5, f32)
    else:                                                   # -0.0 is not the count 0
        assert kind == "minus_zero"
        w = np.full(n, -0.0, f32)
    return t, w


RUNS_STATES = ("uniform", "per_segment", "one_differs", "fraction", "minus_zero")
RUNS_FRAME_KINDS = ("whole", "noise", "whole", "broken", "whole", "nothing", "whole", "broken")


def make_runs_inputs(seed, rng):
    """The inputs of the "runs" class: poses synth.sband_pose(k); "whole" frames of one depth (behind the grid: frames 0 and 4;
    on a plane inside the grid's 3 cm of z, so that there is a surface to count, measure and render: 2 and 6) update every
    voxel, "broken" ones (a zero rectangle) leave segments untouched, wholly and partly updated, one frame touches nothing
    and one is noise; masks: all 255, blocks of 2 x 64 pixels, half the image."""
    cls = "runs"
    cfg, pcfg = configs(seed, cls)
    dims, vs = CLASSES[cls]["dims"], CLASSES[cls]["vs"]
    h, w = IM_HW
    lay = ss.Layout(dims)
    z_mid = float(cfg.origin[2]) + 0.5 * dims[2] * vs
    frames = []
    for k, kind in enumerate(RUNS_FRAME_KINDS):
        # (a broken frame under a pose with next to no roll, so that its rectangle's edge runs along the voxel rows)
        c2w = np.asarray(synth.sband_pose(int(rng.integers(0, 8)) % (2 if kind == "broken" else 8)), f32).ravel()
        inside = k in (2, 6, 7)
        depth = np.full((h, w), z_mid - float(c2w[11]) + float(rng.uniform(-1.0, 1.0)) * vs if inside else synth.SFULL_DEPTH, f32)
        if kind == "noise":
            depth = rng.uniform(-0.5, 6.0 * 1.2, (h, w)).astype(f32)
        elif kind == "nothing":
            depth[:] = 0.0
        elif kind == "broken":
            if k == 3:
                depth[:62, :83] = 0.0
            else:
                depth[62:, int(rng.integers(74, 79)):] = 0.0          # the other corner: the lower voxel rows' second segment sees nothing
        raw = np.clip(np.round(np.clip(depth, 0, 13).astype(np.float64) * 5000.0), 0, 65535).astype(np.uint16)
        frames.append({"pose": c2w, "depth": depth, "raw": raw, "kind": kind})
    masks = [np.full((h, w), 255, np.uint8),
             np.repeat(np.repeat(np.where(rng.random((h // 2, -(-w // 64))) < 0.7, 255, 0).astype(np.uint8), 2, axis=0), 64, axis=1)[:, :w].copy(),
             np.zeros((h, w), np.uint8)]
    masks[2][:, :int(0.55 * w)] = 255
    labels = [(np.repeat(np.repeat(rng.integers(1, 50, (h // 8, w // 8)), 8, 0), 8, 1).astype(np.uint16),
               rng.uniform(0.3, 1.0, (h, w)).astype(f32)) for _ in range(N_LABELS)]
    rgb = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(N_RGB)]
    pn = int(np.prod(CLASSES[cls]["partner"]))
    views = [np.asarray(synth.sband_pose(int(rng.integers(0, 8))), f32).ravel() for _ in range(4)]
    # pixels of a render: three in four in the four image rows that see the grid (45 mm of y at 3.2 m), the rest anywhere
    px = np.stack([rng.integers(0, w, N_PIXELS), np.where(np.arange(N_PIXELS) % 4 == 0, rng.integers(0, h, N_PIXELS),
                                                            rng.integers(60, 64, N_PIXELS))], 1).astype(np.int64)
    return {"cfg": cfg, "partner_cfg": pcfg, "frames": frames, "masks": masks, "labels": labels, "rgb": rgb,
            "states": [runs_state(rng, lay, kind) for kind in RUNS_STATES], "partner_states": [random_state(rng, pn)],
            "views": views, "pixels": px}


def external_patch(lay, seed):
    """What refresh_external writes: (voxel indices, TSDF values, weights) of one to four whole segments given one count
    (a new run where there may have been none) and a stretch of up to 300 voxels anywhere given another weight (runs end)."""
    rng = np.random.default_rng([13, seed])
    idx, t, w = [], [], []
    for s in rng.choice(lay.n_words, int(rng.integers(1, 5)), replace=False):
        i = np.arange(lay.starts[s], lay.starts[s] + lay.sizes[s])
        idx.append(i)
        t.append(np.full(i.size, 1.0, f32) if rng.integers(0, 2) else rng.uniform(-0.9, 0.9, i.size).astype(f32))
        w.append(np.full(i.size, float(rng.choice([0.0, 2.0, 9.0])), f32))
    n = int(rng.integers(1, 301))
    i = np.arange(n) + int(rng.integers(0, lay.n_vox - n))
    idx.append(i)
    t.append(rng.uniform(-0.9, 0.9, n).astype(f32))
    w.append(np.full(n, float(rng.choice([4.0, 0.5])), f32))
    idx = np.concatenate(idx)
    _, keep = np.unique(idx[::-1], return_index=True)       # a voxel named twice takes the later value
    keep = idx.size - 1 - keep
    return idx[keep], np.concatenate(t)[keep], np.concatenate(w)[keep]


# ------------------------------------------------------------------------------------------------------------------------
# what a script has to know of the host code
# ------------------------------------------------------------------------------------------------------------------------
class Tracker:
    """The handle's hidden state as far as tsdf_capi.hip decides it from the calls alone: frames collected (every entry point
    but the collecting ones, set_kernel_variant and set_brick_shape applies them first), and the launches a step queues:
    ("fused", variant, frames) for a fused sequence launch (launch_multi; a labelled sequence of one frame too), ("one",
    variant) for a one-frame launch (launch_integrate; info["masked"][k] says whether launch k brings an instance mask, which
    with the variant and the grid decides its kernel: summary_spec.one_frame_kind), ("label", variant) for the label kernel
    of tsdf_integrate_labels_device, which writes neither weights nor summary words."""

    def __init__(self, cls, partner_fuses):
        self.cls, self.partner_fuses = cls, partner_fuses
        self.defer_n, self.variant, self.pend, self.caller_stream = 32, 0, 0, False
        self.labels = self.colour = self.saved = False
        self.p_defer_n, self.p_pend = 32, 0
        self.pend_masked, self.masked = [], []

    def _queue(self, out, launch, masked=None):
        out.append(launch)
        self.masked.append(masked)

    def can_fuse(self):
        return self.variant in FUSING and self.cls != "scalar"

    def _flush(self, out):
        n, self.pend = self.pend, 0
        masked, self.pend_masked = self.pend_masked, []
        if n > 1 and self.can_fuse():
            self._queue(out, ("fused", self.variant, n))
        else:
            for m in masked:
                self._queue(out, ("one", self.variant), m)

    def _frame(self, out, host, masked=False):
        if self.defer_n > 1 and (host or self.can_fuse()):
            self.pend += 1
            self.pend_masked.append(masked)
            if self.pend >= min(self.defer_n, MAX_FRAMES_PER_LAUNCH):
                self._flush(out)
        else:
            self._flush(out)
            self._queue(out, ("one", self.variant), masked)

    def _p_flush(self):
        self.p_pend = 0

    def apply(self, op, a):
        """Returns what the step meets and does: frames collected on the handle and on the partner before it, the launches
        it queues on the handle, and whether it waits for the handle's stream."""
        info = {"pend": self.pend, "p_pend": self.p_pend, "variant": self.variant, "defer_n": self.defer_n}
        out, self.masked = [], []
        waits = op in OBSERVING or op == "summary_words" or op in ("sync", "set_stream", "upload", "load_state", "save_state", "fuse_from", "fuse_into")
        if op == "partner":
            sub = a["op"]
            if sub == "integrate" or (sub == "integrate_device" and self.partner_fuses):
                if self.p_defer_n > 1:
                    self.p_pend += 1
                    if self.p_pend >= self.p_defer_n:
                        self._p_flush()
            else:
                self._p_flush()
                if sub == "set_deferral":
                    self.p_defer_n = a["n"]
        elif op in ("set_kernel_variant", "set_brick_shape"):
            if op == "set_kernel_variant":
                self.variant = a["variant"]
        elif op in ("integrate", "integrate_u16"):
            self._frame(out, True)
        elif op in ("integrate_device", "integrate_cam2base", "integrate_masked_device"):
            self._frame(out, False, op == "integrate_masked_device")
        elif op == "integrate_colour_device":
            self._frame(out, False)
            self._flush(out)
        else:
            self._flush(out)
            if op == "integrate_rgbd":
                self._queue(out, ("one", self.variant), False)
            elif op == "integrate_labels_device":
                self._queue(out, ("label", self.variant))
            elif op == "integrate_frames_device":
                n = len(a["frames"])
                if self.can_fuse():
                    for k in range(0, n, MAX_FRAMES_PER_LAUNCH):
                        self._queue(out, ("fused", self.variant, min(MAX_FRAMES_PER_LAUNCH, n - k)))
                else:
                    for k in range(n):
                        self._queue(out, ("one", self.variant), a["masks"] is not None and a["masks"][k] is not None)
            elif op == "integrate_frames_labels_device":
                n = len(a["frames"])
                for k in range(0, n, MAX_FRAMES_PER_LAUNCH):
                    self._queue(out, ("fused", self.variant, min(MAX_FRAMES_PER_LAUNCH, n - k)))
            elif op == "set_deferral":
                self.defer_n = a["n"]
            elif op == "set_stream":
                self.caller_stream = a["caller"]
            elif op == "labels_enable":
                self.labels = True
            elif op == "colour_enable":
                self.colour = True
            elif op == "save_state":
                self.saved = True
            elif op in ("fuse_from", "fuse_into", "fuse_dry"):
                self._p_flush()
        info.update(launches=out, masked=self.masked, waits=waits)
        return info


def trace(steps, cls):
    """Tracker.apply's record of every step of a script."""
    tr = Tracker(cls, CLASSES[cls]["partner"][0] % 4 == 0)
    return [tr.apply(op, a) for op, a in steps]


# ------------------------------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------------------------------
class Script(list):
    """The steps; .inputs holds the arrays they name, .seed and .cls what made them."""


def dealt_pairs(cls):
    """Every ordered pair of mutating kinds legal on the class, shuffled once and dealt out to the class's seeds: plain random
    drawing leaves some of the 225 pairs out of any affordable number of walks."""
    kinds = mutating_kinds(cls)
    pairs = [(a, b) for a in kinds for b in kinds]
    order = np.random.default_rng(11 + list(CLASSES).index(cls)).permutation(len(pairs))
    n = len(SEEDS[cls])
    return [[pairs[i] for i in order[s::n]] for s in range(n)]


def situations(cls):
    """The named situations tests/test_walk_spec.py asks for, one list entry each; entry k goes to seed k of the class."""
    out = [("stream_collected",), ("merge_collected", "partner"), ("merge_collected", "handle")]
    out += [("observe_collected", kind) for kind in observing_kinds(cls)]
    if cls != "scalar":
        out += [("trusting", after) for after in ("upload", "load_state", "fuse_from", "reset", "scalar")]
    if cls == "runs":       # (a seed may hold two: entry k goes to seed k % 32)
        return ([("run_handover", kind) for kind in mutating_kinds(cls)] + [("count_limit",)] +
                [("masked_handover", v) for v in (8, 1)] + out)
    if cls != "scalar":
        out += [("ten_fused", v) for v in (0, 8, 7)]
        out += [("brick_between",)]
    assert len(out) <= len(SEEDS[cls])
    return out


class Generator:
    def __init__(self, seed, cls):
        self.seed, self.cls = seed, cls
        self.rng = np.random.default_rng([3, seed, list(CLASSES).index(cls)])
        self.inputs = make_inputs(seed, cls, self.rng)
        self.dims = CLASSES[cls]["dims"]
        self.tr = Tracker(cls, CLASSES[cls]["partner"][0] % 4 == 0)
        self.steps = Script()
        self.n_long = self.n_raycast = 0
        self.runs = cls == "runs"
        self.only_whole = False
        self.follow = self.runs         # the "runs" class looks at the words and the arrays after every mutating step

    # -- single steps -------------------------------------------------------------------------------------------------
    def emit(self, step, **a):
        self.steps.append((step, a))
        self.tr.apply(step, a)
        if self.follow and step in MUTATING + ["refresh_external"]:
            for obs in ("summary_words", "download"):
                self.steps.append((obs, {}))
                self.tr.apply(obs, {})

    def pick(self, n):
        return int(self.rng.integers(0, n))

    def frame(self):
        """A frame of the inputs; the "runs" class takes a whole frame three times in five."""
        if self.runs and (self.only_whole or self.rng.uniform() < 0.6):
            return WHOLE[self.pick(len(WHOLE))]
        return self.pick(N_FRAMES)

    def frames_list(self, lo, hi):
        return [self.frame() for _ in range(int(self.rng.integers(lo, hi + 1)))]

    def brick_shape(self):
        """A random valid shape as tests/test_gpu_fuzz.py draws it, or the library's own choice."""
        if self.cls == "scalar" or self.rng.integers(0, 3) == 0:
            return 0, 0, 0
        quads = self.dims[0] // 4
        q = int(self.rng.choice([d for d in range(1, min(quads, 64) + 1) if quads % d == 0]))
        r = int(self.rng.integers(1, 64 // q + 1))
        return q, r, int(self.rng.integers(1, 64 // (q * r) + 1))

    def policy(self, op=None):
        tr = self.tr
        if op is None:
            ops = ["set_deferral", "set_kernel_variant", "set_brick_shape", "set_stream", "sync", "save_state"]
            if self.cls != "scalar":
                ops += [o for o, on in (("labels_enable", tr.labels), ("colour_enable", tr.colour)) if not on]
            op = ops[self.pick(len(ops))]
        live = self.runs and self.rng.uniform() < 0.7        # keep the one-frame launches on integrate_tile most of the time
        if op == "set_deferral":
            self.emit(op, n=int(self.rng.choice(RUNS_DEFERRALS if live else DEFERRALS)))
        elif op == "set_kernel_variant":
            self.emit(op, variant=int(self.rng.choice(RUNS_VARIANTS if live else VARIANTS)))
        elif op == "set_brick_shape":
            self.emit(op, shape=self.brick_shape())
        elif op == "set_stream":
            self.emit(op, caller=not tr.caller_stream)
        else:
            self.emit(op)

    def maybe_policy(self, p):
        if self.rng.uniform() < p:
            self.policy()

    def prepare(self, op):
        """What the op needs the walk to have done once: labels or colour enabled, a state saved."""
        if op in NEEDS_LABELS and not self.tr.labels:
            self.emit("labels_enable")
        if op in NEEDS_COLOUR and not self.tr.colour:
            self.emit("colour_enable")
        if op == "load_state" and not self.tr.saved:
            self.emit("save_state")

    def mutate(self, op, short=False):
        if op in ("integrate", "integrate_device", "integrate_cam2base"):
            self.emit(op, frame=self.frame())
        elif op == "integrate_u16":                         # every pixel, or the labeller's every 4th row and 3rd column
            self.emit(op, frame=self.frame(), steps=(4, 3) if self.rng.integers(0, 2) else (1, 1))
        elif op == "integrate_rgbd" or op == "integrate_colour_device":
            self.emit(op, frame=self.frame(), rgb=self.pick(N_RGB))
        elif op == "integrate_masked_device":
            self.emit(op, frame=self.frame(), mask=self.pick(N_MASKS))
        elif op == "integrate_labels_device":
            self.emit(op, frame=self.frame(), label=self.pick(N_LABELS))
        elif op == "integrate_frames_device":
            long = not short and self.n_long < 1 and self.rng.integers(0, 4) == 0     # more than one launch holds: 33..40 frames
            self.n_long += long
            frames = self.frames_list(33, 40) if long else self.frames_list(1, 5)
            masks = None
            if self.rng.integers(0, 2):
                masks = [self.pick(N_MASKS) if self.rng.integers(0, 2) else None for _ in frames]
            self.emit(op, frames=frames, masks=masks)
        elif op == "integrate_frames_labels_device":
            frames = self.frames_list(1, 4)
            self.emit(op, frames=frames, labels=[self.pick(N_LABELS) for _ in frames])
        elif op == "upload":
            self.emit(op, state=self.pick(len(self.inputs["states"])))
        elif op == "refresh_external":
            self.emit(op, patch=int(self.rng.integers(0, 1 << 30)))
        else:                                              # reset, load_state, fuse_from, fuse_into
            self.emit(op)

    def observe(self, op=None):
        if op is None:
            ops = ["download", "download", "download", "count_surface", "extent", "fuse_dry"]
            ops += ["raycast"] if self.n_raycast < 2 else []
            ops += ["download_labels"] if self.tr.labels else []
            ops += ["download_colour"] if self.tr.colour else []
            ops += ["summary_words"] if self.runs else []
            op = ops[self.pick(len(ops))]
        if op == "extent":
            band = float(self.rng.choice([1.0, 0.25, float(f32(self.rng.uniform(0.1, 1.0)))]))
            self.emit(op, band=band, margin=int(self.rng.integers(0, 7)))
        elif op == "raycast":
            self.n_raycast += 1
            self.emit(op, view=self.pick(4), device=bool(self.rng.integers(0, 2)))
        else:
            self.emit(op)

    def partner(self, sub=None):
        if sub is None:
            sub = ["integrate", "integrate", "integrate_device", "upload", "reset", "set_deferral", "set_stream"][self.pick(7)]
        if sub in ("integrate", "integrate_device"):
            self.emit("partner", op=sub, frame=self.frame())
        elif sub == "upload":
            self.emit("partner", op=sub, state=0)
        elif sub == "set_deferral":
            self.emit("partner", op=sub, n=int(self.rng.choice(DEFERRALS)))
        elif sub == "set_stream":
            self.emit("partner", op=sub, caller=bool(self.rng.integers(0, 2)))
        else:
            self.emit("partner", op=sub)

    # -- blocks -------------------------------------------------------------------------------------------------------
    def pair(self, a, b):
        """a, then b, with nothing but policy steps between them, then an observation."""
        self.prepare(a)
        self.prepare(b)
        if self.runs and self.rng.uniform() < 0.5:          # runs end at the first fused launch: start them again
            self.live_runs()
        self.maybe_policy(0.6)
        self.mutate(a)
        self.maybe_policy(0.3)
        self.mutate(b)
        self.maybe_policy(0.2)
        self.observe()
        if self.rng.uniform() < 0.3:
            self.partner()

    def collect(self, n=2):
        """Leaves n frames collected on the handle."""
        self.emit("set_deferral", n=32)
        follow, self.follow = self.follow, False            # (an observation would apply them)
        for _ in range(n):
            self.mutate("integrate" if self.rng.integers(0, 2) or not self.tr.can_fuse() else "integrate_device")
        self.follow = follow
        assert self.tr.pend == n

    def live_runs(self):
        """Leaves the handle launching one frame per call through integrate_tile, with a run of a count >= 1 in at least
        three segments of four."""
        self.emit("set_deferral", n=int(self.rng.choice(RUNS_DEFERRALS)))
        self.emit("set_kernel_variant", variant=int(self.rng.choice(RUNS_VARIANTS)))
        how = self.pick(3)
        if how < 2:
            self.emit("upload", state=how)                  # "uniform" or "per_segment"
        else:
            self.emit("reset")
            for _ in range(2):
                self.emit("integrate_device", frame=WHOLE[self.pick(len(WHOLE))])

    def fusing_variant(self, v=None):
        self.emit("set_kernel_variant", variant=int(self.rng.choice(FUSING)) if v is None else v)

    def situation(self, name, arg=None):
        if name == "stream_collected":
            self.collect()
            self.policy("set_stream")
            self.observe("download")
        elif name == "merge_collected":
            if arg == "partner":                            # the source holds collected frames when it is merged
                self.emit("partner", op="set_deferral", n=32)
                self.partner("integrate")
                self.partner("integrate")
                assert self.tr.p_pend == 2
                self.emit("fuse_from")
            else:
                self.collect()
                self.emit("fuse_into")
            self.emit("partner", op="download")
            self.observe("download")
        elif name == "observe_collected":
            self.prepare(arg)
            self.collect()
            self.observe(arg)
        elif name == "trusting":                            # launches that trust the free-space summary words
            self.fusing_variant()
            self.emit("integrate_device", frame=0)          # a scene frame: values other than 1 in the band
            if arg == "load_state":
                self.emit("save_state")
            elif arg == "fuse_from":                        # the partner holds a surface to merge
                self.emit("partner", op="integrate", frame=0)
            self.emit("reset")
            if arg in ("upload", "load_state", "fuse_from"):
                self.mutate(arg)
            elif arg == "scalar":
                v = self.tr.variant
                self.emit("set_kernel_variant", variant=1)
                self.emit("integrate_device", frame=0)      # a scene frame
                self.fusing_variant(v)
            self.emit("integrate_frames_device", frames=self.frames_list(2, 4), masks=None)
            self.observe("download")
        elif name == "ten_fused":
            self.fusing_variant(arg)
            for k in range(10):
                self.emit("integrate_frames_device", frames=self.frames_list(2, 3), masks=None)
                if k in (3, 7):
                    self.policy("set_brick_shape")
            self.observe("download")
        elif name == "run_handover":                        # a writer of weights meets live runs; a whole one-frame launch follows
            self.prepare(arg)
            self.live_runs()
            self.only_whole = True
            self.mutate(arg, short=True)
            self.only_whole = False
            self.emit("integrate_device", frame=WHOLE[self.pick(len(WHOLE))])
        elif name == "masked_handover":                     # a masked frame under variant 8 (wavefront bricks) or 1 (the scalar kernel)
            self.live_runs()
            back = self.tr.variant
            self.emit("set_kernel_variant", variant=arg)
            self.emit("integrate_masked_device", frame=WHOLE[self.pick(len(WHOLE))], mask=self.pick(N_MASKS))
            self.emit("set_kernel_variant", variant=back)
            self.emit("integrate_device", frame=WHOLE[self.pick(len(WHOLE))])
        elif name == "count_limit":                         # segments at 2^24 - 2: one more count, then the run ends
            self.emit("set_deferral", n=0)
            self.emit("set_kernel_variant", variant=int(self.rng.choice(RUNS_VARIANTS)))
            self.emit("upload", state=RUNS_STATES.index("per_segment"))
            for _ in range(3):
                self.emit("integrate_device", frame=WHOLE[self.pick(len(WHOLE))])
        elif name == "brick_between":
            self.fusing_variant()
            self.mutate("integrate_frames_device", short=True)
            self.emit("set_brick_shape", shape=self.brick_shape())
            self.mutate("integrate_frames_device", short=True)
            self.observe("download")

    def build(self):
        if self.seed % 2:
            self.emit("partner", op="set_stream", caller=True)
        for _ in range(2):                                  # the partner holds something before the first merge
            self.partner("integrate")
        sits = situations(self.cls)
        blocks = [("pair", p) for p in dealt_pairs(self.cls)[self.seed]]
        if self.runs:
            self.emit("set_deferral", n=int(self.rng.choice(RUNS_DEFERRALS)))
            blocks += [("situation", sit) for sit in sits[self.seed::len(SEEDS[self.cls])]]
        elif self.seed < len(sits):
            blocks.append(("situation", sits[self.seed]))
        for i in self.rng.permutation(len(blocks)):
            kind, what = blocks[i]
            if kind == "pair":
                self.pair(*what)
            else:
                self.situation(*what)
        if self.runs:                                       # ... nor on words that are all alike: a broken frame ends some runs
            self.live_runs()
            for _ in range(3):
                self.emit("integrate_device", frame=WHOLE[self.pick(len(WHOLE))])
            self.emit("integrate_device", frame=BROKEN[self.pick(len(BROKEN))])
        self.emit("integrate_device", frame=0)              # a scene frame: the walk does not end on an empty volume
        self.observe("download")
        self.steps.inputs, self.steps.seed, self.steps.cls = self.inputs, self.seed, self.cls
        return self.steps


def script(seed, cls):
    """The walk of one seed on one shape class: a Script (list of (op, arguments)) with its input arrays in .inputs."""
    return Generator(seed, cls).build()


@functools.lru_cache(maxsize=None)
def cached_script(seed, cls):
    return script(seed, cls)


# ------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------
class Model:
    """One volume on the CPU: float32 TSDF and weights and, once enabled, label / fp / bp and colour, with one method per op
    that applies the existing restatement."""

    def __init__(self, oracle, cfg):
        self.oracle, self.cfg = oracle, cfg
        self.grid = fs.grid_of(cfg)
        self.dims, self.origin, self.vs, self.trunc, self.b2w = self.grid
        self.vs, self.trunc = float(self.vs), float(self.trunc)
        self.K = np.asarray(cfg.cam_K, f32)
        self.t, self.w = oracle.init_grid(self.dims)
        self.label = self.fp = self.bp = self.colour = self.saved = None
        self.prob = 0.5
        self.watch = None               # called with the arrays before and after every frame (summary_spec.Predictor.frame)

    def cam2base(self, c2w):
        return self.oracle.cam2base(self.b2w, c2w)

    def integrate(self, depth, c2w=None, c2b=None, mask=None):
        c2b = self.cam2base(c2w) if c2b is None else c2b
        d = depth if mask is None else self.oracle.mask_depth(depth, mask)
        before = (self.t.copy(), self.w.copy()) if self.watch else None
        self.oracle.integrate(self.K, c2b, d, self.dims, self.origin, self.vs, self.trunc, self.t, self.w,
                              max_depth=self.cfg.max_depth)
        if self.watch:
            self.watch(*before, self.t, self.w)

    def integrate_u16(self, raw, c2w, steps):
        """steps (4, 3): the labeller's preparation (oracle.depth_prep); (1, 1): every pixel times the fp32 reciprocal."""
        assert steps in ((4, 3), (1, 1))
        depth = self.oracle.depth_prep(raw, 5000.0) if steps == (4, 3) else (raw.astype(f32) * (f32(1.0) / f32(5000.0))).astype(f32)
        self.integrate(depth, c2w)

    def integrate_labels(self, depth, label_im, score_im, c2w):
        self.oracle.integrate_labels(self.K, self.cam2base(c2w), depth, label_im, score_im, self.dims, self.origin, self.vs,
                                     self.trunc, self.label, self.fp, self.bp, max_depth=self.cfg.max_depth, prob_thd=self.prob)

    def integrate_colour(self, depth, rgb, c2w):
        """The colour pass of a frame that integrate() has just applied."""
        self.oracle.integrate_colour(self.K, self.cam2base(c2w), depth, rgb, self.dims, self.origin, self.vs, self.trunc,
                                     self.w, self.colour, max_depth=self.cfg.max_depth)

    def labels_enable(self, prob=0.5):
        n = self.t.size
        self.prob = prob
        self.label, self.fp, self.bp = np.zeros(n, np.uint16), np.zeros(n, f32), np.zeros(n, f32)

    def colour_enable(self):
        self.colour = np.zeros(self.t.size, np.uint32)

    def reset(self):
        self.t, self.w = self.oracle.init_grid(self.dims)

    def upload(self, t, w):
        self.t, self.w = t.copy(), w.copy()

    def save_state(self):
        self.saved = (self.t.copy(), self.w.copy())

    def load_state(self):
        self.upload(*self.saved)

    def refresh_external(self, idx, t, w):
        self.t[idx], self.w[idx] = t, w

    def fuse_from(self, src, write=1):
        t, w, counts = fs.fuse(self.t, self.w, self.grid, src.t, src.w, src.grid, weight_thresh=WEIGHT_THRESH, agree_tol=0.4,
                               write=write)
        if write:
            self.t, self.w = t, w
        return counts

    def count_surface(self):
        return len(self.oracle.surface_points(self.t, self.w, self.dims, self.vs, self.origin))

    def extent(self, band, margin):
        return es.extent(self.t, self.w, self.dims, weight_thresh=WEIGHT_THRESH, band=band, margin=margin)

    def render_args(self, c2w):
        c2b = capi.multiply_matrix(capi.invert_matrix(self.b2w)[1], c2w)
        return dict(tsdf=self.t, weight=self.w, dims=self.dims, origin=self.origin, vs=self.cfg.voxel_size,
                    trunc=self.cfg.trunc_margin, cam2base=c2b)

    def raycast(self, c2w, pixels):
        a = self.render_args(c2w)
        return rs.render(a["tsdf"], a["weight"], a["dims"], a["origin"], a["vs"], a["trunc"], K_SMALL, IM_HW, 0.0,
                         self.cfg.max_depth, WEIGHT_THRESH, a["cam2base"], pixels=pixels, label=self.label, colour=self.colour)


class Walk:
    """The model of a script: apply(op, arguments) returns what the device must answer to the step (None where the step
    returns nothing to compare)."""

    def __init__(self, oracle, inputs, predict=False):
        self.inp = inputs
        self.main, self.partner = Model(oracle, inputs["cfg"]), Model(oracle, inputs["partner_cfg"])
        self.lay = ss.Layout(self.main.dims)
        self.pred = self.tr = None
        if predict:             # the summary words beside the arrays: Tracker names the launches, the model's frames feed them
            cls = next(k for k, c in CLASSES.items() if tuple(c["dims"]) == tuple(self.main.dims))
            self.tr = Tracker(cls, self.partner.dims[0] % 4 == 0)
            self.pred = ss.Predictor(self.lay)
            self.main.watch = self.pred.frame

    def apply(self, op, a):
        if self.pred is None:
            return self.apply_model(op, a)
        info = self.tr.apply(op, a)
        out = self.apply_model(op, a)
        self.pred.launches(info["launches"], info["masked"])
        if op == "reset":
            self.pred.reset()
        elif op in ("upload", "load_state", "fuse_from", "refresh_external"):
            self.pred.rebuild(self.main.t, self.main.w)
        assert len(self.pred.frames) == self.tr.pend, "the frames that wait in the model are those the handle has collected"
        return out

    def apply_model(self, op, a):
        m, inp = self.main, self.inp
        fr = inp["frames"][a["frame"]] if "frame" in a else None
        if op in ("integrate", "integrate_device"):
            m.integrate(fr["depth"], fr["pose"])
        elif op == "integrate_u16":
            m.integrate_u16(fr["raw"], fr["pose"], a["steps"])
        elif op == "integrate_cam2base":                    # the handle's base frame is the world: the pose as it is
            m.integrate(fr["depth"], c2b=fr["pose"])
        elif op == "integrate_masked_device":
            m.integrate(fr["depth"], fr["pose"], mask=inp["masks"][a["mask"]])
        elif op in ("integrate_rgbd", "integrate_colour_device"):
            m.integrate(fr["depth"], fr["pose"])
            m.integrate_colour(fr["depth"], inp["rgb"][a["rgb"]], fr["pose"])
        elif op == "integrate_labels_device":
            m.integrate_labels(fr["depth"], *inp["labels"][a["label"]], fr["pose"])
        elif op == "integrate_frames_device":
            for k, i in enumerate(a["frames"]):
                mask = None if a["masks"] is None or a["masks"][k] is None else inp["masks"][a["masks"][k]]
                m.integrate(inp["frames"][i]["depth"], inp["frames"][i]["pose"], mask=mask)
        elif op == "integrate_frames_labels_device":
            for i, j in zip(a["frames"], a["labels"]):
                f = inp["frames"][i]
                m.integrate(f["depth"], f["pose"])
                m.integrate_labels(f["depth"], *inp["labels"][j], f["pose"])
        elif op == "reset":
            m.reset()
        elif op == "upload":
            m.upload(*inp["states"][a["state"]])
        elif op == "save_state":
            m.save_state()
        elif op == "load_state":
            m.load_state()
        elif op == "fuse_from":
            return m.fuse_from(self.partner)
        elif op == "fuse_into":
            return self.partner.fuse_from(m)
        elif op == "fuse_dry":
            return m.fuse_from(self.partner, write=0)
        elif op == "labels_enable":
            m.labels_enable()
        elif op == "colour_enable":
            m.colour_enable()
        elif op == "refresh_external":
            m.refresh_external(*external_patch(self.lay, a["patch"]))
        elif op == "summary_words":
            return {"lay": self.lay, "pred": self.pred, "t": m.t, "w": m.w}
        elif op == "download":
            return m.t, m.w
        elif op == "download_labels":
            return m.label, m.fp, m.bp
        elif op == "download_colour":
            return m.colour
        elif op == "count_surface":
            return m.count_surface()
        elif op == "extent":
            return m.extent(a["band"], a["margin"])
        elif op == "raycast":
            return m.raycast(inp["views"][a["view"]], inp["pixels"])
        elif op == "partner":
            return self.apply_partner(a)
        else:
            assert op in ("set_deferral", "set_kernel_variant", "set_brick_shape", "set_stream", "sync"), op
        return None

    def apply_partner(self, a):
        p, sub = self.partner, a["op"]
        if sub in ("integrate", "integrate_device"):
            fr = self.inp["frames"][a["frame"]]
            p.integrate(fr["depth"], fr["pose"])
        elif sub == "upload":
            p.upload(*self.inp["partner_states"][a["state"]])
        elif sub == "reset":
            p.reset()
        elif sub == "download":
            return p.t, p.w
        return None


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} for {want.dtype}{want.shape}"
    bad = got.view(np.uint8).reshape(got.size, -1) != want.view(np.uint8).reshape(want.size, -1)
    bad = bad.any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.flatnonzero(bad)[:5].tolist()}"


def compare(op, got, want):
    """The device's answer to an observing step against the model's: every bit of every array, every field of every record."""
    if op in ("download", "partner"):
        same_bits(got[1], want[1], "weight")
        same_bits(got[0], want[0], "tsdf")
    elif op == "summary_words":                             # (words, the device's own download of the same step)
        words, t, w = got
        ss.assert_sound(want["lay"], words, t, w, "summary words against the device's arrays")
        if want["pred"] is not None:
            want["pred"].check(words, "summary words")
        same_bits(w, want["w"], "weight")
        same_bits(t, want["t"], "tsdf")
    elif op == "download_labels":
        for g, w, name in zip(got, want, ("label", "fp", "bp")):
            same_bits(g, w, name)
    elif op == "download_colour":
        same_bits(got, want, "colour")
    elif op == "raycast":
        for name in ("depth", "normal", "label", "colour"):
            assert (name in got) == (name in want), name
            if name in want:
                same_bits(got[name], want[name], name)
    else:                                                   # count_surface, extent, the counts of a merge
        assert got == want, f"device {got}, model {want}"


# ------------------------------------------------------------------------------------------------------------------------
# the batch walk
# ------------------------------------------------------------------------------------------------------------------------
BATCH_DIMS = [(40, 28, 16), (24, 36, 12), (64, 16, 20)]
BATCH_VS = 0.0075
BATCH_OPS = ["integrate", "fuse", "extent", "raycast", "download", "upload", "reset", "extents", "batch_raycast"]


def batch_configs():
    """Three members of different dims centred on one optical axis, so that they overlap: merges between them sample."""
    return [config(d, BATCH_VS, origin_of(d, BATCH_VS)) for d in BATCH_DIMS]


def batch_script(seed):
    """The walk of one seed over a batch of three: ("integrate", depth, per-member masks, pose) of the batch mixed with calls
    on the borrowed member handles -- fuse (member j merged into member i), extent, raycast, download, upload, reset -- and the
    batch's own extents and raycast."""
    rng = np.random.default_rng([5, seed])
    cfgs = batch_configs()
    h, w = IM_HW
    scene = scene_of(BATCH_DIMS[0], BATCH_VS)
    frames = []
    for k in range(6):
        c2w = scene.pose(int(rng.integers(0, 16)), n=16)
        depth = scene.depth(c2w, quantize=True)
        if k == 1:
            depth = rng.uniform(-0.5, 7.2, (h, w)).astype(f32)
        frames.append({"pose": np.asarray(c2w, f32).ravel(), "depth": depth})
    masks = [np.zeros((h, w), np.uint8) for _ in range(3)]
    masks[0][:, :90] = 255
    masks[1][:, 70:] = 255
    masks[2][:] = (rng.uniform(0, 1, (h, w)) < 0.7).astype(np.uint8) * 255
    views = [np.asarray(scene.pose(int(rng.integers(0, 16)), n=16), f32).ravel() for _ in range(3)]
    px = np.stack([rng.integers(w // 2 - 22, w // 2 + 22, N_PIXELS), rng.integers(h // 2 - 13, h // 2 + 13, N_PIXELS)], 1).astype(np.int64)
    states = [random_state(rng, int(np.prod(d))) for d in BATCH_DIMS]
    steps = Script()
    emit = lambda step, **a: steps.append((step, a))
    member = lambda: int(rng.integers(0, 3))

    def integrate(n):
        for _ in range(n):
            emit("integrate", frame=int(rng.integers(0, 6)), masks=[int(rng.integers(0, 3)) if rng.integers(0, 3) else None for _ in range(3)])

    integrate(3)
    for _ in range(14):
        integrate(int(rng.integers(1, 4)))                  # collected by the batch when the next call comes
        op = BATCH_OPS[1 + int(rng.integers(0, len(BATCH_OPS) - 1))]
        if op == "fuse":
            i = member()
            emit(op, dst=i, src=(i + 1 + int(rng.integers(0, 2))) % 3, write=int(rng.integers(0, 4) > 0))
            emit("download", member=i)
        elif op in ("extent", "extents"):
            emit(op, member=member(), band=float(rng.choice([1.0, 0.25])), margin=int(rng.integers(0, 5)))
        elif op in ("raycast", "batch_raycast"):
            emit(op, member=member(), view=int(rng.integers(0, 3)))
        elif op == "upload":
            emit(op, member=member())
        else:
            emit(op, member=member())
    emit("integrate", frame=0, masks=[None, 0, None])       # a scene frame: the walk does not end on an empty member
    for i in range(3):
        emit("download", member=i)
    steps.inputs = {"cfgs": cfgs, "frames": frames, "masks": masks, "views": views, "pixels": px, "states": states}
    steps.seed, steps.cls = seed, "batch"
    return steps


class BatchWalk:
    """One Model per member, each fed mask_depth(depth, mask_i)."""

    def __init__(self, oracle, inputs):
        self.inp = inputs
        self.members = [Model(oracle, c) for c in inputs["cfgs"]]

    def apply(self, op, a):
        inp = self.inp
        m = self.members[a["member"]] if "member" in a else None
        if op == "integrate":
            fr = inp["frames"][a["frame"]]
            for mod, k in zip(self.members, a["masks"]):
                mod.integrate(fr["depth"], fr["pose"], mask=None if k is None else inp["masks"][k])
        elif op == "fuse":
            return self.members[a["dst"]].fuse_from(self.members[a["src"]], write=a["write"])
        elif op == "extent":
            return m.extent(a["band"], a["margin"])
        elif op == "extents":
            return [mod.extent(a["band"], a["margin"]) for mod in self.members]
        elif op == "raycast":
            return m.raycast(inp["views"][a["view"]], inp["pixels"])
        elif op == "batch_raycast":                         # the nearest member's hit, ties to the lower index
            c = inp["cfgs"][0]
            return rs.render_batch([mod.render_args(inp["views"][a["view"]]) for mod in self.members], K_SMALL, IM_HW, 0.0,
                                   c.max_depth, WEIGHT_THRESH, pixels=inp["pixels"])
        elif op == "download":
            return m.t, m.w
        elif op == "upload":
            m.upload(*inp["states"][a["member"]])
        elif op == "reset":
            m.reset()
        return None


def compare_batch(op, got, want):
    if op == "download":
        compare("download", got, want)
    elif op == "raycast":
        compare("raycast", got, want)
    elif op == "batch_raycast":
        for name in ("member", "depth", "normal"):
            same_bits(got[name], want[name], name)
    else:
        assert got == want, f"device {got}, model {want}"


# ------------------------------------------------------------------------------------------------------------------------
# the batch walk with weight runs alive
# ------------------------------------------------------------------------------------------------------------------------
BATCH_RUNS_DIMS = [(40, 12, 6), (256, 10, 6), (72, 10, 8)]      # member 1 is row-mapped: one segment per row; the others are flat
BATCH_RUNS_VS = 0.01
ROW_MEMBER = 1
BATCH_RUNS_SITUATIONS = ("upload", "block_mask", "reset", "merge")


def batch_runs_configs():
    """Three members on synth.sband_volume's origin for their own dims: whole frames update all of each."""
    return [config(d, BATCH_RUNS_VS, synth.sband_volume(d, BATCH_RUNS_VS), trunc=synth.SBAND_TRUNC) for d in BATCH_RUNS_DIMS]


def batch_runs_script(seed):
    """The walk of one seed over a batch whose member handles launch one frame per call (set_deferral(0): the batch then
    applies every frame with its batched kernel, which keeps bits 0 and 1 of the summary words only).  Every mutating step
    is followed by summary_words and download of the members it wrote.  Each of the four situations occurs, in a seeded order:
    the row member holds runs of a count -- from an upload, or from reset, or with a written merge on top of the upload --
    then a batch integrate with an all-255 mask (or a mask of blocks) for it, then integrate_device on its own handle, a
    one-frame launch of integrate_tile that must not meet the runs the batched kernel outdated."""
    rng = np.random.default_rng([17, seed])
    cfgs = batch_runs_configs()
    h, w = IM_HW
    frames = []
    for k in range(5):                                      # whole (behind the grids), whole, broken, noise, whole
        c2w = np.asarray(synth.sband_pose(int(rng.integers(0, 8))), f32).ravel()
        depth = np.full((h, w), synth.SFULL_DEPTH, f32)
        if k == 2:
            depth[:62, :83] = 0.0
        elif k == 3:
            depth = rng.uniform(-0.5, 7.2, (h, w)).astype(f32)
        frames.append({"pose": c2w, "depth": depth, "kind": ("whole", "whole", "broken", "noise", "whole")[k]})
    masks = [np.full((h, w), 255, np.uint8),
             np.repeat(np.repeat(np.where(rng.random((h // 2, -(-w // 64))) < 0.7, 255, 0).astype(np.uint8), 2, axis=0), 64, axis=1)[:, :w].copy(),
             np.zeros((h, w), np.uint8)]
    masks[2][:, :int(0.55 * w)] = 255
    lays = [ss.Layout(d) for d in BATCH_RUNS_DIMS]
    states = [[runs_state(rng, lay, kind) for kind in ("uniform", "per_segment")] for lay in lays]
    steps = Script()

    def emit(step, **a):
        steps.append((step, a))
        wrote = {"integrate": range(3), "fuse": [a.get("dst")] if a.get("write") else []}.get(step, [a.get("member")])
        if step in ("integrate", "member_integrate", "upload", "reset", "fuse"):
            for m in wrote:
                steps.append(("summary_words", {"member": m}))
                steps.append(("download", {"member": m}))

    whole = lambda: (0, 1, 4)[int(rng.integers(0, 3))]
    other = lambda: (0, 2)[int(rng.integers(0, 2))]

    def situation(name):
        emit("upload", member=ROW_MEMBER, state=0)          # the count 3 in every segment
        if name == "reset":
            emit("reset", member=ROW_MEMBER)                # ... the count 0
        elif name == "merge":
            emit("upload", member=0, state=1)
            emit("fuse", dst=ROW_MEMBER, src=0, write=1)
        mask = 1 if name == "block_mask" else 0
        emit("integrate", frame=whole(), masks=[None if rng.integers(0, 2) else int(rng.integers(0, 3)), mask, int(rng.integers(0, 3))], situation=name)
        emit("member_integrate", member=ROW_MEMBER, frame=whole())

    for name in rng.permutation(BATCH_RUNS_SITUATIONS):
        for _ in range(int(rng.integers(1, 3))):            # something else in between
            op = ("integrate", "member_integrate", "upload", "reset", "fuse")[int(rng.integers(0, 5))]
            if op == "integrate":
                emit(op, frame=int(rng.integers(0, 5)), masks=[int(rng.integers(0, 3)) if rng.integers(0, 3) else None for _ in range(3)])
            elif op == "member_integrate":
                emit(op, member=int(rng.integers(0, 3)), frame=int(rng.integers(0, 5)))
            elif op == "upload":
                emit(op, member=int(rng.integers(0, 3)), state=int(rng.integers(0, 2)))
            elif op == "reset":
                emit(op, member=int(rng.integers(0, 3)))
            else:
                i = int(rng.integers(0, 3))
                emit(op, dst=i, src=(i + 1 + int(rng.integers(0, 2))) % 3, write=int(rng.integers(0, 4) > 0))
        situation(str(name))
    emit("integrate", frame=0, masks=[None, 0, None])
    steps.inputs = {"cfgs": cfgs, "frames": frames, "masks": masks, "states": states}
    steps.seed, steps.cls = seed, "batch_runs"
    return steps


class BatchRunsWalk:
    """One Model and one summary_spec.Predictor per member.  What the host does is fixed by the set-up: the batch does not
    collect, so "integrate" is the batched kernel (runs forgotten in every member) and a member's own frame is one launch of
    launch_integrate under variant 0, unmasked."""

    def __init__(self, oracle, inputs):
        self.inp = inputs
        self.members = [Model(oracle, c) for c in inputs["cfgs"]]
        self.lays = [ss.Layout(m.dims) for m in self.members]
        self.preds = [ss.Predictor(lay) for lay in self.lays]
        for m, p in zip(self.members, self.preds):
            m.watch = p.frame

    def apply(self, op, a):
        inp = self.inp
        i = a.get("member")
        m, p = (self.members[i], self.preds[i]) if i is not None else (None, None)
        if op == "integrate":
            fr = inp["frames"][a["frame"]]
            for mod, pred, k in zip(self.members, self.preds, a["masks"]):
                mod.integrate(fr["depth"], fr["pose"], mask=None if k is None else inp["masks"][k])
                pred.frames.clear()
                pred.forget()
        elif op == "member_integrate":
            fr = inp["frames"][a["frame"]]
            m.integrate(fr["depth"], fr["pose"])
            p.launches([("one", 0)], [False])
        elif op == "upload":
            m.upload(*inp["states"][i][a["state"]])
            p.rebuild(m.t, m.w)
        elif op == "reset":
            m.reset()
            p.reset()
        elif op == "fuse":
            dst = self.members[a["dst"]]
            out = dst.fuse_from(self.members[a["src"]], write=a["write"])
            if a["write"]:
                self.preds[a["dst"]].rebuild(dst.t, dst.w)
            return out
        elif op == "summary_words":
            return {"lay": self.lays[i], "pred": p, "t": m.t, "w": m.w}
        elif op == "download":
            return m.t, m.w
        else:
            raise AssertionError(f"no such op: {op}")
        return None


def compare_batch_runs(op, got, want):
    if op in ("download", "summary_words"):
        compare(op, got, want)
    else:
        assert got == want, f"device {got}, model {want}"
