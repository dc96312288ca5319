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
"""
import functools

import numpy as np

import extent_spec as es
import fuse_spec as fs
import raycast_spec as rs
from fuse_cases import IM_HW, K_SMALL
from semantic_slam_amd import capi, synth

f32 = np.float32

# the three shape classes of tests/test_gpu_deferral.py.  The grids are wider than any camera of the walk sees (about 1.4 m
# at the near face), so a strip at both x ends stays fresh whatever is integrated; the partner is centred on the grid's centre.
CLASSES = {
    "row": dict(dims=(256, 24, 12), vs=0.006, partner=(32, 20, 12), partner_vs=0.0075),       # dim_x % 256 == 0
    "flat": dict(dims=(200, 24, 12), vs=0.008, partner=(28, 22, 10), partner_vs=0.01),        # dim_x % 4 == 0 only
    "scalar": dict(dims=(37, 20, 12), vs=0.05, partner=(25, 13, 9), partner_vs=0.0625),       # dim_x % 4 != 0
}
SEEDS = {"row": range(48), "flat": range(48), "scalar": range(24)}
BATCH_SEEDS = range(6)

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


def legal(op, cls):
    return cls != "scalar" or (op not in NEEDS_LABELS and op not in NEEDS_COLOUR)


def mutating_kinds(cls):
    return [op for op in MUTATING if legal(op, cls)]


def observing_kinds(cls):
    return [op for op in OBSERVING if legal(op, cls)]


# ------------------------------------------------------------------------------------------------------------------------
# geometry and inputs
# ------------------------------------------------------------------------------------------------------------------------
def config(dims, vs, origin, base2world=None):
    return capi.make_config(dims, vs, origin, K=K_SMALL, base2world=base2world, im_height=IM_HW[0], im_width=IM_HW[1])


def origin_of(dims, vs):
    """The grid centred on the optical axis, its near face 0.9 m in front of the base camera."""
    return np.array([-dims[0] * vs / 2, -dims[1] * vs / 2, 0.9], f32)


def configs(seed, cls):
    """(main config, partner config): the partner has its own voxel size (ratio 1.2 to 1.25) and a seeded rigid offset."""
    c = CLASSES[cls]
    dims, vs, pdims, pvs = c["dims"], c["vs"], c["partner"], c["partner_vs"]
    origin = origin_of(dims, vs)
    centre = origin.astype(np.float64) + np.array(dims) * vs / 2
    rng = np.random.default_rng([7, seed, list(CLASSES).index(cls)])
    ax, ay, az = rng.uniform(-0.2, 0.2, 3)
    R = synth.rot_z(az) @ synth.rot_y(ay) @ synth.rot_x(ax)
    b2w = fs.pose_about(R, centre, rng.uniform(-0.5, 0.5, 3) * vs)
    p_origin = (centre - np.array(pdims) * pvs / 2).astype(f32)
    return config(dims, vs, origin), config(pdims, pvs, p_origin, base2world=b2w)


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


# ------------------------------------------------------------------------------------------------------------------------
# what a script has to know of the host code
# ------------------------------------------------------------------------------------------------------------------------
class Tracker:
    """The handle's hidden state as far as tsdf_capi.hip decides it from the calls alone: frames collected (every entry point
    but the collecting ones, set_kernel_variant and set_brick_shape applies them first), and the launches a step queues:
    ("fused", variant, frames) for a fused sequence launch, ("one", variant) for a one-frame launch."""

    def __init__(self, cls, partner_fuses):
        self.cls, self.partner_fuses = cls, partner_fuses
        self.defer_n, self.variant, self.pend, self.caller_stream = 32, 0, 0, False
        self.labels = self.colour = self.saved = False
        self.p_defer_n, self.p_pend = 32, 0

    def can_fuse(self):
        return self.variant in FUSING and self.cls != "scalar"

    def _flush(self, out):
        n, self.pend = self.pend, 0
        if n > 1 and self.can_fuse():
            out.append(("fused", self.variant, n))
        else:
            out.extend([("one", self.variant)] * n)

    def _frame(self, out, host):
        if self.defer_n > 1 and (host or self.can_fuse()):
            self.pend += 1
            if self.pend >= min(self.defer_n, MAX_FRAMES_PER_LAUNCH):
                self._flush(out)
        else:
            self._flush(out)
            out.append(("one", self.variant))

    def _p_flush(self):
        self.p_pend = 0

    def apply(self, op, a):
        """Returns what the step meets and does: frames collected on the handle and on the partner before it, the launches
        it queues on the handle, and whether it waits for the handle's stream."""
        info = {"pend": self.pend, "p_pend": self.p_pend, "variant": self.variant, "defer_n": self.defer_n}
        out = []
        waits = op in OBSERVING or op in ("sync", "set_stream", "upload", "load_state", "save_state", "fuse_from", "fuse_into")
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
            self._frame(out, False)
        elif op == "integrate_colour_device":
            self._frame(out, False)
            self._flush(out)
        else:
            self._flush(out)
            if op == "integrate_rgbd":
                out.append(("one", self.variant))
            elif op == "integrate_frames_device":
                n = len(a["frames"])
                if self.can_fuse():
                    out.extend(("fused", self.variant, min(MAX_FRAMES_PER_LAUNCH, n - k)) for k in range(0, n, MAX_FRAMES_PER_LAUNCH))
                else:
                    out.extend([("one", self.variant)] * n)
            elif op == "integrate_frames_labels_device":
                n = len(a["frames"])
                out.extend(("fused", self.variant, min(MAX_FRAMES_PER_LAUNCH, n - k)) for k in range(0, n, MAX_FRAMES_PER_LAUNCH))
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
        info.update(launches=out, waits=waits)
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

    # -- single steps -------------------------------------------------------------------------------------------------
    def emit(self, step, **a):
        self.steps.append((step, a))
        self.tr.apply(step, a)

    def pick(self, n):
        return int(self.rng.integers(0, n))

    def frames_list(self, lo, hi):
        return [self.pick(N_FRAMES) for _ in range(int(self.rng.integers(lo, hi + 1)))]

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
        if op == "set_deferral":
            self.emit(op, n=int(self.rng.choice(DEFERRALS)))
        elif op == "set_kernel_variant":
            self.emit(op, variant=int(self.rng.choice(VARIANTS)))
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
            self.emit(op, frame=self.pick(N_FRAMES))
        elif op == "integrate_u16":                         # every pixel, or the labeller's every 4th row and 3rd column
            self.emit(op, frame=self.pick(N_FRAMES), steps=(4, 3) if self.rng.integers(0, 2) else (1, 1))
        elif op == "integrate_rgbd" or op == "integrate_colour_device":
            self.emit(op, frame=self.pick(N_FRAMES), rgb=self.pick(N_RGB))
        elif op == "integrate_masked_device":
            self.emit(op, frame=self.pick(N_FRAMES), mask=self.pick(N_MASKS))
        elif op == "integrate_labels_device":
            self.emit(op, frame=self.pick(N_FRAMES), label=self.pick(N_LABELS))
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
            self.emit(op, state=self.pick(N_STATES))
        else:                                              # reset, load_state, fuse_from, fuse_into
            self.emit(op)

    def observe(self, op=None):
        if op is None:
            ops = ["download", "download", "download", "count_surface", "extent", "fuse_dry"]
            ops += ["raycast"] if self.n_raycast < 2 else []
            ops += ["download_labels"] if self.tr.labels else []
            ops += ["download_colour"] if self.tr.colour else []
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
            self.emit("partner", op=sub, frame=self.pick(N_FRAMES))
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
        for _ in range(n):
            self.mutate("integrate" if self.rng.integers(0, 2) or not self.tr.can_fuse() else "integrate_device")
        assert self.tr.pend == n

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
        if self.seed < len(sits):
            blocks.append(("situation", sits[self.seed]))
        for i in self.rng.permutation(len(blocks)):
            kind, what = blocks[i]
            if kind == "pair":
                self.pair(*what)
            else:
                self.situation(*what)
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

    def cam2base(self, c2w):
        return self.oracle.cam2base(self.b2w, c2w)

    def integrate(self, depth, c2w=None, c2b=None, mask=None):
        c2b = self.cam2base(c2w) if c2b is None else c2b
        d = depth if mask is None else self.oracle.mask_depth(depth, mask)
        self.oracle.integrate(self.K, c2b, d, self.dims, self.origin, self.vs, self.trunc, self.t, self.w,
                              max_depth=self.cfg.max_depth)

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

    def __init__(self, oracle, inputs):
        self.inp = inputs
        self.main, self.partner = Model(oracle, inputs["cfg"]), Model(oracle, inputs["partner_cfg"])

    def apply(self, op, a):
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
