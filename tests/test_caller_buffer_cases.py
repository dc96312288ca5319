"""Conditions on the cases of tests/test_gpu_caller_buffers.py and on its buffer helper, on the CPU: the first and the last
element of every caller image is really consumed (changing it alone changes voxels under the oracle), the masks cover both
corner patterns, every case updates a tenth of its voxels, and tests/guarded.py places, fills and watches its bands as
documented -- including that an over-read whose value is used shows as a difference between the two fills.  These are
conditions on inputs, not measurements."""
import numpy as np
import pytest

import caller_buffer_cases as cb
import guarded

f32 = np.float32


@pytest.fixture(scope="module")
def torch_cpu():
    import torch
    return torch


# ------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------
def test_the_sizes_are_the_residues_of_a_four_wide_access():
    assert sorted((h * w) % 4 for h, w in cb.SIZES) == [0, 1, 2, 3]
    assert all(w % 2 == 1 for h, w in cb.SIZES if (h * w) % 4) and [w % 4 for h, w in cb.SIZES if (h * w) % 4 == 0] == [0]
    assert max(int(np.prod(cb.CLASSES[cls]["dims"])) for cls in cb.VOLUMES) <= 74000


def poked(a, at, value):
    """A copy of `a` with the flat element `at` alone changed."""
    b = np.array(a)
    assert b.flat[at] != value
    b.flat[at] = value
    return b


@pytest.mark.parametrize("pair", cb.PAIRS, ids=cb.pair_id)
def test_first_and_last_depth_pixel_are_consumed(oracle, pair):
    c = cb.case(*pair)
    for k, depth in enumerate(c.depths):
        base = cb.integrate(oracle, c.cfg, depth)
        assert (base[1] > 0).mean() >= 0.10, f"frame {k} updates {100 * (base[1] > 0).mean():.1f} % of the voxels"
        for at in (0, -1):
            for value in (0.0, float(depth.flat[at]) + 1.5 * c.cfg.trunc_margin):       # dropped; moved along its ray
                other = cb.integrate(oracle, c.cfg, poked(depth, at, f32(value)))
                assert cb.differs(base, other) >= 1, f"frame {k} pixel {at} -> {value} changes nothing"


@pytest.mark.parametrize("pair", cb.PAIRS, ids=cb.pair_id)
def test_first_and_last_mask_byte_are_consumed(oracle, pair):
    c = cb.case(*pair)
    assert (c.masks[0].flat[0], c.masks[0].flat[-1]) == (0, 255) and (c.masks[1].flat[0], c.masks[1].flat[-1]) == (255, 0)
    for i, mask in enumerate(c.masks):
        assert set(np.unique(mask)) == {0, 255}
        base = cb.integrate(oracle, c.cfg, c.depths[0], mask=mask)
        assert (base[1] > 0).mean() >= 0.10
        for at in (0, -1):
            other = cb.integrate(oracle, c.cfg, c.depths[0], mask=poked(mask, at, 255 - mask.flat[at]))
            assert cb.differs(base, other) >= 1, f"mask {i} byte {at} changes nothing"


@pytest.mark.parametrize("pair", [p for p in cb.PAIRS if cb.four_wide(p[1])], ids=cb.pair_id)
def test_first_and_last_rgb_label_and_score_element_are_consumed(oracle, pair):
    c = cb.case(*pair)
    state = cb.integrate(oracle, c.cfg, c.depths[0])
    colour = cb.integrate_colour(oracle, c.cfg, c.depths[0], c.rgb, state)
    assert np.count_nonzero(colour) >= 0.10 * colour.size
    labels = cb.integrate_labels(oracle, c.cfg, c.depths[0], c.label_ims[0], c.score_ims[0])
    assert np.count_nonzero(labels[1]) > 0
    for at in (0, -1):
        other = cb.integrate_colour(oracle, c.cfg, c.depths[0], poked(c.rgb, at, c.rgb.flat[at] ^ 0x80), state)
        assert cb.differs(colour, other) >= 1, f"rgb byte {at} changes nothing"
        other = cb.integrate_labels(oracle, c.cfg, c.depths[0], poked(c.label_ims[0], at, 60), c.score_ims[0])
        assert cb.differs(labels, other) >= 1, f"label element {at} changes nothing"
        other = cb.integrate_labels(oracle, c.cfg, c.depths[0], c.label_ims[0], poked(c.score_ims[0], at, f32(0.123)))
        assert cb.differs(labels, other) >= 1, f"score element {at} changes nothing"


@pytest.mark.parametrize("hw", cb.SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_compose_and_origin_consume_the_corners(oracle, hw):
    c = cb.case(hw, "flat")
    masks = c.mask_stack
    base = oracle.compose_labels(masks, c.labels, c.scores)
    for at in (0, -1):
        m = poked(masks, at, 255 - masks.flat[at])
        assert cb.differs(base, oracle.compose_labels(m, c.labels, c.scores)) >= 1, f"compose: mask byte {at} changes nothing"
    # object_origin, with and without the mask that is set on both corners: each corner holds one axis' minimum
    for mask in (None, c.masks[2]):
        prep = (lambda d: d) if mask is None else (lambda d: oracle.mask_depth(d, mask))
        origin = oracle.object_origin(prep(c.origin_depth), c.K)
        for at in (0, -1):
            other = oracle.object_origin(prep(poked(c.origin_depth, at, f32(0.0))), c.K)
            assert cb.differs(origin, other) >= 1, f"origin: pixel {at} changes nothing"


def test_batch_members_differ_and_are_four_wide():
    for pair in cb.PAIRS:
        if cb.four_wide(pair[1]):
            cfgs = cb.batch_configs(cb.case(*pair))
            assert len(cfgs) == 3 and len({tuple(cfg.origin) for cfg in cfgs}) == 3 and all(cfg.dim_x % 4 == 0 for cfg in cfgs)


# ------------------------------------------------------------------------------------------------------------------------
# the helper
# ------------------------------------------------------------------------------------------------------------------------
TYPED = [  # role, dtype, fill, value the element next to the payload reads as
    ("depth", np.float32, "A", None), ("depth", np.float32, "B", 1.25), ("mask", np.uint8, "A", 255), ("mask", np.uint8, "B", 0),
    ("rgb", np.uint8, "A", 255), ("rgb", np.uint8, "B", 0), ("raw", np.uint16, "A", 0xFFFF), ("raw", np.uint16, "B", 0),
    ("label", np.uint16, "A", 0xFFFF), ("label", np.uint16, "B", 1), ("score", np.float32, "A", None),
    ("score", np.float32, "B", f32(0.99)), ("member", np.int32, "A", 0), ("member", np.int32, "B", -1),
    ("cluster", np.int32, "A", 0), ("cluster", np.int32, "B", -1),
]


@pytest.mark.parametrize("role,dtype,fill,want", TYPED)
def test_layout_residue_and_typed_fill(torch_cpu, role, dtype, fill, want):
    es = np.dtype(dtype).itemsize
    for residue in (0, guarded.element_residue(dtype)):
        for n in (1, 7, 24 * 32):
            g = guarded.Guarded(torch_cpu, "cpu", dtype, n, role, fill, residue, row_bytes=es * 600, value=1.25)
            assert g.ptr % 16 == residue and g.ptr == g.buf.data_ptr() + g.off
            raw = g.buf.numpy()
            front, back = raw[:g.off], raw[g.off + g.nbytes:]
            assert front.size >= max(4096, 4 * es * 600) and back.size >= max(4096, 4 * es * 600)
            before = raw[g.off - es:g.off].copy().view(dtype)[0]
            after = raw[g.off + g.nbytes:g.off + g.nbytes + es].copy().view(dtype)[0]
            for got in (before, after):
                if want is None:
                    assert np.isnan(got) and np.array([got]).view(np.uint32)[0] == 0x7FC00BAD
                else:
                    assert got == np.dtype(dtype).type(want)
            data = (np.arange(n) % 251).astype(dtype)
            g.write(data)
            assert np.array_equal(g.read(), data) and g.payload_unchanged() and g.bands_intact().size == 0


def test_normal_and_output_fills(torch_cpu):
    for fill, want in (("A", None), ("B", (0.0, 0.0, 1.0))):
        g = guarded.Guarded(torch_cpu, "cpu", np.float32, 3 * 35, "normal", fill, 4)
        raw = g.buf.numpy()
        for at in (g.off - 12, g.off + g.nbytes):
            got = raw[at:at + 12].copy().view(f32)
            assert np.isnan(got).all() if want is None else tuple(got) == want
    for fill, byte in (("A", 0xA5), ("B", 0x5A)):
        g = guarded.Guarded(torch_cpu, "cpu", np.int32, 11, "out", fill, 4)
        assert (g.buf.numpy()[:g.off + g.nbytes + 4096] == byte).all() and (g.prefill().view(np.uint8) == byte).all()
        assert g.bands_intact().size == 0


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_a_one_byte_write_next_to_the_payload_is_reported(torch_cpu, dtype):
    g = guarded.Guarded(torch_cpu, "cpu", dtype, 33 * 45, "out", "A", guarded.element_residue(dtype))
    g.buf[g.off - 1] = 0
    assert g.bands_intact().tolist() == [-1]
    g.buf[g.off + g.nbytes] = 0
    assert g.bands_intact().tolist() == [-1, g.nbytes]
    g.buf[g.off + 3] = 0                                   # the payload is the callee's to write
    assert g.bands_intact().tolist() == [-1, g.nbytes]
    d = guarded.Guarded(torch_cpu, "cpu", np.float32, 8, "depth", "A").write(np.ones(8, f32))
    d.buf[d.off + 4] = 7
    assert not d.payload_unchanged() and d.bands_intact().size == 0


def test_an_over_read_whose_value_is_used_differs_between_the_fills(torch_cpu):
    """A stand-in consumer that sums one element too many: the net catches it because the two fills give other results."""
    def consumer(g, n):
        a = g.buf.numpy()[g.off:g.off + 4 * (n + 1)].copy().view(f32)        # one element past the payload
        return float(np.nansum(a)), bool(np.isnan(a).any())

    data = np.linspace(1.0, 2.0, 24 * 32).astype(f32)
    out = [consumer(guarded.Guarded(torch_cpu, "cpu", f32, data.size, "depth", fill, 4, value=1.5).write(data), data.size)
           for fill in "AB"]
    assert out[0] != out[1]
    honest = [float(guarded.Guarded(torch_cpu, "cpu", f32, data.size, "depth", fill, 4, value=1.5).write(data).read().sum())
              for fill in "AB"]
    assert honest[0] == honest[1]
