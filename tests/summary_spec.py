"""The summary words of a volume, restated in numpy (test infrastructure, no GPU): where the words lie, what a word may say
about its segment at any moment (sound), what a rebuild makes of the arrays (rebuilt), how a word moves under a one-frame
launch of integrate_tile (after_update) and under every other writer of weights (Predictor).  Restated from
csrc/host_derive.h ("the summary word", word_after_update), csrc/tsdf_kernels.hip.h (IntegrateParams::flags, recompute_flags,
forget_runs), csrc/launch_geometry.h ("the summary duty": Keeps and SummaryRecord, whose actions are Predictor.drop and
Predictor.forget; one_frame, restated as one_frame_kind) and csrc/tsdf_capi.hip (fill, rebuild_summary, summary_before and its
callers); nothing here calls the library, and tests/test_summary_duty.py holds one_frame_kind and the Predictor's step to
one_frame without a device.  tsdf_summary_words (include/tsdf_hip_diag.h) reads the words this file speaks about.

  bit 0       every TSDF value of the segment has the bit pattern of 1.0f
  bit 1       every weight of the segment is finite and >= 0
  bit 2       every weight of the segment has the bit pattern of float32(c), c = word >> 8 <= 2^24 - 1 (implies bit 1)
  bits 3..7   zero; bits 8..31 zero where bit 2 is clear
"""
import numpy as np

ONES, SANE, RUN = 1, 2, 4
COUNT_SHIFT = 8
MAX_COUNT = 2 ** 24 - 1
FRESH = ONES | SANE | RUN                     # create / reset: TSDF 1, weight 0 = the count 0
ONE_BITS = 0x3F800000
SANE_BELOW = np.float32(3.0e38)               # recompute_flags takes "finite" as below this
CLASSIFY_MIN_VOXELS = 48_000_000              # host_derive.h, kClassifyMinVoxels
u32 = np.uint32


# ------------------------------------------------------------------------------------------------------------------------
# where the words lie
# ------------------------------------------------------------------------------------------------------------------------
class Layout:
    """Segments of a slab of nz slices of dims = (dim_x, dim_y, .): kind "row" (rows of a multiple of 256 voxels: one word per
    row segment, index (lz * dim_y + y) * nseg + seg), "flat" (other rows of a multiple of 4 voxels: one word per 256-voxel
    chunk of a slice's linear view, ceil(dim_x * dim_y / 256) per slice, the last one partial) or "none" (no summary)."""

    def __init__(self, dims, nz=None):
        dx, dy = int(dims[0]), int(dims[1])
        nz = int(dims[2]) if nz is None else int(nz)
        self.dims, self.nz, self.n_vox = (dx, dy, nz), nz, dx * dy * nz
        self.kind = "none" if dx % 4 else "row" if dx % 256 == 0 else "flat"
        z, y, x = np.meshgrid(np.arange(nz), np.arange(dy), np.arange(dx), indexing="ij")
        if self.kind == "row":
            nseg = dx // 256
            self.per_slice = dy * nseg
            word = (z * dy + y) * nseg + x // 256
        elif self.kind == "flat":
            self.per_slice = -(-(dx * dy) // 256)
            word = z * self.per_slice + (y * dx + x) // 256
        else:
            self.per_slice, word = 0, np.zeros((0,), np.int64)
        self.n_words = self.per_slice * nz
        self.word_of = word.ravel()                 # the word of every voxel, voxels in memory order (x fastest)
        if self.n_words:
            assert np.all(np.diff(self.word_of) >= 0), "a segment is a run of consecutive voxels"
            self.starts = np.flatnonzero(np.diff(self.word_of, prepend=-1))
            assert len(self.starts) == self.n_words
            self.sizes = np.diff(np.append(self.starts, self.n_vox))
            assert self.sizes.max() == 256 and (self.kind == "flat" or self.sizes.min() == 256)

    def every(self, cond):
        """Per segment: cond holds for every voxel of it."""
        return np.logical_and.reduceat(np.asarray(cond, bool), self.starts)

    def some(self, cond):
        return np.logical_or.reduceat(np.asarray(cond, bool), self.starts)

    def first(self, a):
        return np.asarray(a)[self.starts]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(u32)


def count_bits(c):
    """The bit pattern of float32(c) for counts c <= 2^24 - 1 (exact)."""
    return np.asarray(c, np.int64).astype(np.float32).view(u32)


def has_run(words):
    return (np.asarray(words, u32) & u32(RUN)) != 0


def run_count(words):
    return np.asarray(words, u32) >> u32(COUNT_SHIFT)


def weights_sane(w):
    w = np.asarray(w, np.float32)
    with np.errstate(invalid="ignore"):
        return (w >= 0) & (w < SANE_BELOW)


# ------------------------------------------------------------------------------------------------------------------------
# what a word may say
# ------------------------------------------------------------------------------------------------------------------------
def unsound(lay, words, t, w):
    """[(segment, word, why)] for every word that says something its segment does not bear out, whatever launched."""
    words = np.asarray(words)
    assert words.dtype == u32 and words.shape == (lay.n_words,), f"{words.dtype}{words.shape} for {lay.n_words} words"
    if lay.n_words == 0:
        return []
    tb, wb = bits(t), bits(w)
    assert tb.size == lay.n_vox == wb.size
    w = np.ascontiguousarray(w, np.float32)
    with np.errstate(invalid="ignore"):
        finite_nonneg = np.isfinite(w) & (w >= 0)
    c = run_count(words)
    run = has_run(words)
    want = count_bits(np.minimum(c, MAX_COUNT))
    checks = [
        ("bit 0 over a TSDF value that is not 1.0f", ((words & ONES) != 0) & ~lay.every(tb == ONE_BITS)),
        ("bit 1 over a weight that is negative or not finite", ((words & SANE) != 0) & ~lay.every(finite_nonneg)),
        ("bit 2 without bit 1", run & ((words & SANE) == 0)),
        ("a count above 2^24 - 1", run & (c > MAX_COUNT)),
        ("bit 2 over a weight that is not float32(count)", run & ~lay.every(wb == want[lay.word_of])),
        ("a count without bit 2", ~run & (c != 0)),
        ("bits 3..7", (words & u32(0xF8)) != 0),
    ]
    return [(int(s), int(words[s]), why) for why, bad in checks for s in np.flatnonzero(bad)]


def assert_sound(lay, words, t, w, what):
    bad = unsound(lay, words, t, w)
    assert not bad, f"{what}: {len(bad)} unsound words, first: " + "; ".join(f"segment {s} word {x:#010x}: {why}" for s, x, why in bad[:4])


def sound(lay, words, t, w):
    return not unsound(lay, words, t, w)


# ------------------------------------------------------------------------------------------------------------------------
# the writers of words
# ------------------------------------------------------------------------------------------------------------------------
def rebuilt(lay, t, w):
    """recompute_flags: the words a rebuild makes of the arrays, every bit."""
    tb, wb = bits(t), bits(w)
    ones, sane = lay.every(tb == ONE_BITS), lay.every(weights_sane(w))
    lead = lay.first(wb)
    same = lay.every(wb == lead[lay.word_of])
    wl = lead.view(np.float32)
    with np.errstate(invalid="ignore"):
        small = wl <= np.float32(MAX_COUNT)
    c = np.where(small & sane, wl, 0).astype(np.int64)              # (sane: finite and >= 0, so the conversion is defined)
    run = sane & same & small & (count_bits(c) == lead)             # an integer, and not -0
    words = ones.astype(u32) * u32(ONES) | sane.astype(u32) * u32(SANE)
    return np.where(run, words | u32(RUN) | (c.astype(u32) << u32(COUNT_SHIFT)), words).astype(u32)


def after_update(words, touched, all_updated, left_not_one):
    """word_after_update over arrays: the words after a one-frame launch of integrate_tile."""
    words = np.asarray(words, u32)
    out = np.where(left_not_one, words & ~u32(ONES), words)
    c = run_count(out)
    goes_on = has_run(out) & all_updated & (c < MAX_COUNT)
    out = np.where(has_run(out), np.where(goes_on, (out & u32(ONES | SANE | RUN)) | ((c + u32(1)) << u32(COUNT_SHIFT)), out & u32(ONES | SANE)), out)
    return np.where(touched, out, words).astype(u32)


def frame_effect(lay, t0, w0, t1, w1):
    """(touched, all_updated, left_not_one) per segment of one frame, from the arrays before and after it.  A voxel was
    updated iff its weight changed (w + 1 != w below 2^24; a segment whose weights have reached 2^24 carries no run, and no
    word without a run depends on the first two)."""
    upd = bits(w0) != bits(w1)
    return lay.some(upd), lay.every(upd), lay.some(upd & (bits(t1) != ONE_BITS))


def stale_run_errors(lay, stale, upd, w1):
    """Voxels a one-frame launch of integrate_tile would get wrong if it met the words `stale` instead of the true ones: those
    it updates in a segment whose stale word carries a run, where float32(count + 1) is not the weight `w1` the model has
    after the frame (the kernel takes the weights of such a segment from the word)."""
    would_store = count_bits(np.minimum(run_count(stale).astype(np.int64) + 1, 2 ** 24))
    return int((upd & has_run(stale)[lay.word_of] & (would_store[lay.word_of] != bits(w1))).sum())


def one_frame_kind(lay, variant, masked, n_vox):
    """What launch_integrate queues for one frame (csrc/launch_geometry.h, one_frame): "scalar" (variant 1, or rows of no multiple of 4 voxels), "multi" (the flat
    mapping: launch_multi with one frame), "bricks" (a masked frame that is classified: variant 8 always, 7 never, else from
    48 M voxels: classify_one_frame) or "tile" (integrate_tile).  Frames of the walks have tile tables that fit and every
    grid with rows of a multiple of 4 voxels has a brick view."""
    assert variant in (0, 1, 3, 7, 8)
    if variant == 1 or lay.kind == "none":
        return "scalar"
    if lay.kind == "flat":
        return "multi"
    classify = variant == 8 or (variant != 7 and n_vox >= CLASSIFY_MIN_VOXELS)
    return "bricks" if masked and classify else "tile"


class Predictor:
    """Bit 2 and the count of every word through the steps of a walk, exactly.  .words holds the prediction, .claim where it
    claims anything, .exact whether bits 0 and 1 are predicted too (right after reset, a rebuild or a drop).  Frames reach
    it as they reach the model -- at the call -- and wait in .frames until the step that launches them."""

    def __init__(self, lay, n_vox=None):
        self.lay = lay
        self.n_vox = lay.n_vox if n_vox is None else n_vox
        self.frames = []
        self.no_claims = self.tile_launches = 0
        self.events = None                          # a list: every change is recorded there, tile launches with what they met
        self.reset()

    def note(self, *event):
        if self.events is not None:
            self.events.append(event)

    def reset(self):                                # fill: every word fresh
        self.note("reset")
        self.words = np.full(self.lay.n_words, FRESH, u32)
        self.claim = np.ones(self.lay.n_words, bool)
        self.exact = True

    def rebuild(self, t, w):                        # upload, load_state, a written merge, refresh_summary
        self.note("rebuild")
        self.words = rebuilt(self.lay, t, w) if self.lay.n_words else np.zeros(0, u32)
        self.claim = np.ones(self.lay.n_words, bool)
        self.exact = True

    def forget(self):                               # summary_before, bits 0 and 1 kept: launch_multi, masked bricks, the batched kernel
        self.note("forget")
        self.words = self.words & u32(ONES | SANE)
        self.claim[:] = True
        self.exact = False

    def drop(self):                                 # summary_before, nothing kept: the scalar kernel
        self.note("drop")
        self.words = np.zeros(self.lay.n_words, u32)
        self.claim[:] = True
        self.exact = True

    def frame(self, t0, w0, t1, w1):
        """One frame as the model applies it: (touched, all_updated, left_not_one, voxels updated, weights after it)."""
        self.frames.append(frame_effect(self.lay, t0, w0, t1, w1) + (bits(w0) != bits(w1), w1.copy()) if self.lay.n_words else None)

    def tile(self, effect):
        self.note("tile", effect, self.words.copy())
        self.tile_launches += 1
        self.words = after_update(self.words, *effect[:3])
        self.exact = False

    def unknown(self, effect):
        """A one-frame launch whose kernel the script cannot know: no claim for the segments it touched."""
        self.note("unknown")
        self.no_claims += 1
        self.claim &= ~effect[0]
        self.exact = False

    def launches(self, launches, masked):
        """Tracker's launches of one step, with masked[k] for the one-frame ones."""
        for launch, m in zip(launches, masked):
            if launch[0] == "label":                # the label kernel writes neither weights nor words
                continue
            if launch[0] == "fused":
                del self.frames[:launch[2]]
                self.forget()
                continue
            effect = self.frames.pop(0)
            kind = one_frame_kind(self.lay, launch[1], m, self.n_vox)
            if kind == "scalar":
                self.drop()
            elif kind == "tile":
                self.tile(effect)
            else:
                self.forget()

    def mismatches(self, words):
        """[(segment, got, predicted, what)]: bit 2 and the count wherever a claim stands; the whole word where exact."""
        words = np.asarray(words, u32)
        mask = u32(0xFFFFFFFF) if self.exact else u32(RUN | 0xFFFFFF00)
        bad = self.claim & ((words & mask) != (self.words & mask))
        return [(int(s), int(words[s]), int(self.words[s]), "whole word" if self.exact else "bit 2 and count") for s in np.flatnonzero(bad)]

    def check(self, words, what):
        bad = self.mismatches(words)
        assert not bad, f"{what}: {len(bad)} words differ from the prediction, first: " + "; ".join(
            f"segment {s} word {g:#010x} predicted {p:#010x} ({k})" for s, g, p, k in bad[:4])
