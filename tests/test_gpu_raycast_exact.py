"""Raycasting on the device held to its rule (csrc/tsdf_raycast.hip.h) at ray, box, march, value, normal, label-voxel, base-frame
and batch edges: every case of tests/raycast_cases.py is uploaded, rendered through tsdf_raycast / tsdf_raycast_device /
tsdf_batch_raycast_device and compared with the restatement (tests/raycast_spec.py) on all 32 bits of depth, normal, label,
colour and member.  tests/test_raycast_cases.py proves on the CPU that each case reaches the branch it is named for and ends
within max_steps (the cap and the stall cases are bounded by the rule's own termination guarantees)."""
import ctypes as C

import numpy as np
import pytest

import raycast_cases as rc
import raycast_spec as rs
from test_gpu_raycast import params, same_bits
from semantic_slam_amd import capi

pytestmark = pytest.mark.gpu

f32 = np.float32

SINGLES = rc.single_cases()
BATCHES = rc.batch_cases()


def groups():
    """Cases that share a grid (dims, vs, origin, trunc, base2world), in the order of SINGLES: one volume each."""
    out = {}
    for c in SINGLES:
        out.setdefault(rc.grid_key(c), []).append(c)
    return list(out.values())


GROUPS = groups()


def group_id(g):
    c = g[0]
    frame = c["name"].split("[")[1].rstrip("]") if "[" in c["name"] else "identity base frame"
    return f"{'x'.join(map(str, c['dims']))} vs {c['vs']:g} trunc {c['trunc']:g} {frame}"


def config(c, vol_id=0):
    return capi.make_config(c["dims"], c["vs"], c["origin"], trunc=c["trunc"], base2world=c["base2world"], vol_id=vol_id)


def want_of(c):
    return rs.render(c["tsdf"], c["weight"], c["dims"], c["origin"], c["vs"], c["trunc"], c["K"], c["hw"], c["near"], c["far"],
                     c["thr"], rc.cam2base(c, capi), pixels=c["pixels"], label=c["label"], colour=c["colour"])


def case_params(c):
    return params(c["K"], c["hw"], near=c["near"], far=c["far"], thr=c["thr"])


class Loaded:
    """A volume and the state it holds: a case's arrays are uploaded only when they differ from the last ones."""

    def __init__(self, vol, dims, with_ids):
        self.vol, self.state = vol, None
        if with_ids:
            vol.labels_enable(0.5)
            vol.colour_enable()
            n = vol.n_voxels
            label, colour = rc.ids(dims)
            vol.upload_labels(label, np.zeros(n, f32), np.zeros(n, f32))
            vol.upload_colour(colour)

    def load(self, c):
        key = (c["tsdf"].tobytes(), c["weight"].tobytes())
        if key != self.state:
            self.vol.upload(c["tsdf"], c["weight"])
            self.state = key


def check_case(vol, c):
    h, w = c["hw"]
    want = want_of(c)
    with_ids = c["label"] is not None
    got = vol.raycast(c["cam2world"], params=case_params(c), normals=True, labels=with_ids, colour=with_ids)
    what = f"case '{c['name']}'"
    same_bits(got["depth"].reshape(-1), want["depth"], f"{what} depth")
    same_bits(got["normal"].reshape(-1, 3), want["normal"], f"{what} normal")
    if with_ids:
        same_bits(got["label"].reshape(-1), want["label"], f"{what} label")
        same_bits(got["colour"].reshape(-1), want["colour"], f"{what} colour")
    assert got["depth"].shape == (h, w)
    return got, want


@pytest.mark.parametrize("group", GROUPS, ids=[group_id(g) for g in GROUPS])
def test_cases_bit_for_bit(cuda, group):
    with_ids = group[0]["dims"][0] % 4 == 0
    assert all((c["label"] is not None) <= with_ids for c in group)
    with capi.Volume(config(group[0])) as vol:
        held = Loaded(vol, group[0]["dims"], with_ids)
        for c in group:
            held.load(c)
            check_case(vol, c)


def pick(name):
    return next(c for c in SINGLES if c["name"] == name)


def test_device_outputs_one_at_a_time(cuda):
    """tsdf_raycast_device with depth NULL and only the normal asked for, then with only the label: the image asked for is the
    full render's, and a buffer that was not passed is not written (a guard value behind each survives)."""
    c = pick("hits beside the side faces, plane near the middle [tilted base frame]")
    h, w = c["hw"]
    want = want_of(c)
    assert want["hit"].sum() > 100
    with capi.Volume(config(c)) as vol:
        Loaded(vol, c["dims"], True).load(c)
        normal = cuda.full((h * w * 3 + 1,), -7.0, dtype=cuda.float32, device="cuda")
        vol.raycast_device(c["cam2world"], None, normal_ptr=normal.data_ptr(), params=case_params(c))
        vol.sync()
        n = normal.cpu().numpy()
        same_bits(n[:-1].reshape(-1, 3), want["normal"], "normal alone")
        assert n[-1] == -7.0
        label = cuda.full((h * w + 1,), 9, dtype=cuda.int16, device="cuda")
        vol.raycast_device(c["cam2world"], None, label_ptr=label.data_ptr(), params=case_params(c))
        vol.sync()
        lab = label.cpu().numpy().view(np.uint16)
        same_bits(lab[:-1], want["label"], "label alone")
        assert lab[-1] == 9
        assert len(np.unique(want["label"])) > 50


# ------------------------------------------------------------------------------------------------------------------------
# batch
# ------------------------------------------------------------------------------------------------------------------------
def batch_want(b):
    members = [dict(m, cam2base=capi.multiply_matrix(capi.invert_matrix(m["base2world"])[1], b["cam2world"]))
               for m in b["members"]]
    return rs.render_batch(members, b["K"], b["hw"], b["near"], b["far"], b["thr"])


@pytest.mark.parametrize("b", BATCHES, ids=[b["name"] for b in BATCHES])
def test_batch_cases_bit_for_bit(cuda, b):
    h, w = b["hw"]
    p = params(b["K"], b["hw"], near=b["near"], far=b["far"], thr=b["thr"])
    want = batch_want(b)
    cfgs = [config(m, vol_id=i) for i, m in enumerate(b["members"])]
    with capi.Batch(cfgs) as batch:
        for v, m in zip(batch.volumes, b["members"]):
            v.upload(m["tsdf"], m["weight"])
        d = cuda.full((h, w), -7.0, dtype=cuda.float32, device="cuda")
        nrm = cuda.full((h, w, 3), -7.0, dtype=cuda.float32, device="cuda")
        who = cuda.full((h, w), -7, dtype=cuda.int32, device="cuda")
        batch.raycast_device(b["cam2world"], d.data_ptr(), nrm.data_ptr(), who.data_ptr(), params=p)
        batch.sync()
        got_d, got_n, got_who = d.cpu().numpy(), nrm.cpu().numpy(), who.cpu().numpy()
        what = f"batch case '{b['name']}'"
        same_bits(got_who.reshape(-1), want["member"], f"{what} member")
        same_bits(got_d.reshape(-1), want["depth"], f"{what} depth")
        same_bits(got_n.reshape(-1, 3), want["normal"], f"{what} normal")
        # each output NULL in turn: the other two are unchanged
        for drop in range(3):
            bufs = [cuda.full((h, w), -7.0, dtype=cuda.float32, device="cuda"),
                    cuda.full((h, w, 3), -7.0, dtype=cuda.float32, device="cuda"),
                    cuda.full((h, w), -7, dtype=cuda.int32, device="cuda")]
            ptrs = [None if k == drop else x.data_ptr() for k, x in enumerate(bufs)]
            batch.raycast_device(b["cam2world"], ptrs[0], ptrs[1], ptrs[2], params=p)
            batch.sync()
            for k, (x, full) in enumerate(zip(bufs, (got_d, got_n, got_who))):
                if k != drop:
                    same_bits(x.cpu().numpy(), full, f"{what} output {k} with output {drop} NULL")
        # every member's own render is the batch's image where that member wins
        for i, v in enumerate(batch.volumes):
            single = v.raycast(b["cam2world"], params=p)
            mine = got_who == i
            if not mine.any():
                continue
            same_bits(single["depth"][mine], got_d[mine], f"{what} member {i} depth")
            same_bits(single["normal"][mine], got_n[mine], f"{what} member {i} normal")
            assert np.all(single["depth"][mine] > 0)


def test_labels_and_colour_refuse_rows_that_are_no_quads(cuda):
    """Why label and colour ride on raycast_cases.LABEL_GRIDS and the cases on the other grids render depth and normal alone."""
    c = pick("shape (9, 7, 5) 16x16 look x")
    assert c["label"] is None
    with capi.Volume(config(c)) as vol:
        for enable, what in ((lambda: vol.labels_enable(0.5), "tsdf_labels_enable"), (vol.colour_enable, "tsdf_colour_enable")):
            with pytest.raises(capi.TsdfError, match=f"{what}: dim_x must be a multiple of 4"):
                enable()
        held = Loaded(vol, c["dims"], False)
        held.load(c)
        check_case(vol, c)                                              # and the handle still renders


def test_batch_refuses_a_member_whose_rows_are_no_quads(cuda):
    """Why the batch cases use dim_x = 8, 16, 4, 32 where the single-volume cases use 9, 17, 2, 33."""
    cfgs = [capi.make_config((8, 7, 5), 0.0625, [0, 0, 0.5]), capi.make_config((9, 7, 5), 0.0625, [0, 0, 0.5], vol_id=1)]
    arr = (capi.TsdfConfig * 2)(*cfgs)
    h = C.c_void_p()
    lib = capi.load()
    assert lib.tsdf_batch_create(arr, 2, C.byref(h)) == -1
    assert "volume 1: dim_x must be a multiple of 4" in lib.tsdf_last_error().decode()
