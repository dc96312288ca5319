"""The random walks of tests/test_gpu_walk.py (tests/walk_cases.py), held to conditions without a GPU, so that the GPU test
cannot be vacuous: the scripts are deterministic and end on a download; over a class's seeds every ordered pair of mutating
ops occurs back to back and is observed, and every named situation of the handle's hidden state occurs (an observation, a
merge, a stream change while frames are collected; fused launches that trust the free-space summary right after the calls
that must rebuild or drop it; ten fused launches in a row under each classification mode; a brick shape change between two
fused launches); and the model alone, run over every script, is not idle."""
import ctypes as C
import functools

import numpy as np
import pytest

import walk_cases as wc

ROWS_OF_4 = [cls for cls in wc.CLASSES if cls != "scalar"]


def equal(a, b):
    """Deep equality of steps and inputs: arrays by dtype, shape and bytes, configs by their bytes."""
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, C.Structure):
        return bytes(a) == bytes(b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("cls", list(wc.CLASSES))
def test_scripts_are_deterministic_and_end_on_a_download(cls):
    for seed in list(wc.SEEDS[cls])[:3]:
        a, b = wc.script(seed, cls), wc.script(seed, cls)
        assert equal(list(a), list(b)) and equal(a.inputs, b.inputs)
        assert not equal(list(a), list(wc.cached_script(seed + 3, cls)))
    for seed in wc.SEEDS[cls]:
        s = wc.cached_script(seed, cls)
        assert s[-1][0] == "download"
        assert 15 <= len(s) <= 50, (seed, len(s))
        assert all(op in wc.MUTATING + wc.POLICY + wc.OBSERVING + ["partner"] and wc.legal(op, cls) for op, _ in s)
    a, b = wc.batch_script(1), wc.batch_script(1)
    assert equal(list(a), list(b)) and equal(a.inputs, b.inputs)
    assert all(wc.batch_script(seed)[-1][0] == "download" for seed in wc.BATCH_SEEDS)


def test_the_class_grids_are_what_they_are_named_for():
    for cls, c in wc.CLASSES.items():
        dx = c["dims"][0]
        assert {"row": dx % 256 == 0, "flat": dx % 4 == 0 and dx % 256 != 0, "scalar": dx % 4 != 0}[cls]
        assert int(np.prod(c["dims"])) <= 250000 and np.prod(c["partner"]) < np.prod(c["dims"])
        cfg, pcfg = wc.configs(0, cls)
        assert pcfg.voxel_size != cfg.voxel_size and list(pcfg.base2world) != list(cfg.base2world)
    assert set(wc.VARIANTS) == set(wc.capi.SHIPPED_VARIANTS)


# ------------------------------------------------------------------------------------------------------------------------
# what the scripts cover
# ------------------------------------------------------------------------------------------------------------------------
def observed_pairs(steps):
    """(a, b) for every two mutating steps with nothing but policy steps between them and an observation of the handle after
    them, before the next mutating step."""
    tokens = [op if op in wc.MUTATING else "observed" if op in wc.OBSERVING else "partner"
              for op, _ in steps if op not in wc.POLICY]
    return {(a, b) for a, b, c in zip(tokens, tokens[1:], tokens[2:]) if a in wc.MUTATING and b in wc.MUTATING and c == "observed"}


@pytest.mark.parametrize("cls", list(wc.CLASSES))
def test_every_ordered_pair_of_mutating_ops_occurs_and_is_observed(cls):
    kinds = wc.mutating_kinds(cls)
    assert len(kinds) == (15 if cls != "scalar" else 11)
    seen = set()
    for seed in wc.SEEDS[cls]:
        seen |= observed_pairs(wc.cached_script(seed, cls))
    missing = [(a, b) for a in kinds for b in kinds if (a, b) not in seen]
    assert not missing, missing


def fused_runs(steps, infos):
    """{variant: the longest run of fused launches under it with no other launch and no wait for the GPU before the run's
    last launch}."""
    best, run, at = {}, 0, None
    for info in infos:
        for launch in info["launches"]:
            run = run + 1 if launch[0] == "fused" and launch[1] == at else (1 if launch[0] == "fused" else 0)
            at = launch[1]
            if launch[0] == "fused":
                best[at] = max(best.get(at, 0), run)
        if info["waits"]:
            run = 0
    return best


def brick_shape_between_fused_launches(steps, infos):
    state = 0                       # 1: a fused launch is the last thing queued; 2: and the brick shape was set since
    for (op, _), info in zip(steps, infos):
        for launch in info["launches"]:
            if launch[0] == "fused" and state == 2:
                return True
            state = 1 if launch[0] == "fused" else 0
        if op == "set_brick_shape" and state >= 1:
            state = 2
        elif info["waits"]:
            state = 0
    return False


@pytest.mark.parametrize("cls", list(wc.CLASSES))
def test_the_named_situations_occur(cls):
    seen = set()
    runs = {}
    for seed in wc.SEEDS[cls]:
        steps = wc.cached_script(seed, cls)
        infos = wc.trace(steps, cls)
        for (op, a), info in zip(steps, infos):
            if op in wc.OBSERVING and info["pend"] > 0:
                assert info["defer_n"] > 1 and info["pend"] < info["defer_n"]
                seen.add(("observed while collected", op))
            if (op == "fuse_from" and info["p_pend"] > 0) or (op == "fuse_into" and info["pend"] > 0):
                seen.add(("merge of a source with collected frames", op))
            if op == "set_stream" and info["pend"] > 0:
                seen.add("set_stream while collected")
            if op == "partner" and a["op"] == "set_stream" and a["caller"]:
                seen.add("partner on a caller's stream")
            if op == "integrate_frames_device" and len(a["frames"]) > wc.MAX_FRAMES_PER_LAUNCH:
                seen.add("a sequence longer than one launch holds")
            if op == "integrate_frames_device" and a["masks"] is not None and None in a["masks"] and len(set(a["masks"])) > 1:
                seen.add("a sequence with masks on some frames")
            if op == "set_brick_shape" and a["shape"] == (0, 0, 0):
                seen.add("the library's own brick shape")
        for v, n in fused_runs(steps, infos).items():
            runs[v] = max(runs.get(v, 0), n)
        if brick_shape_between_fused_launches(steps, infos):
            seen.add("set_brick_shape between two fused launches")
        kinds = {s["kind"] for s in steps.inputs["frames"]}
        assert kinds == {"scene", "noise", "constant", "invalid"}
    want = {("observed while collected", op) for op in wc.observing_kinds(cls)}
    want |= {("merge of a source with collected frames", op) for op in ("fuse_from", "fuse_into")}
    want |= {"set_stream while collected", "partner on a caller's stream", "a sequence longer than one launch holds",
             "a sequence with masks on some frames", "the library's own brick shape"}
    if cls in ROWS_OF_4:
        want.add("set_brick_shape between two fused launches")
        assert all(runs.get(v, 0) >= 10 for v in (0, 7, 8)), runs
    else:
        assert not runs, "a grid whose rows are no multiple of 4 voxels has no fused launches"
    assert want <= seen, want - seen


# ------------------------------------------------------------------------------------------------------------------------
# the model alone
# ------------------------------------------------------------------------------------------------------------------------
TRUSTED_AFTER = ("upload", "load_state", "fuse_from", "reset", "scalar")


@functools.lru_cache(maxsize=None)
def model_run(seed, cls):
    """The model over one script: what every observing op saw, the final shares of observed and fresh voxels, and for every
    fused sequence directly after a call that must rebuild or drop the summary the number of voxels a stale "all ones" word
    would get wrong: TSDF 1 before that call, another value after it, updated by the sequence."""
    from oracle.oracle import Oracle
    steps = wc.cached_script(seed, cls)
    infos = wc.trace(steps, cls)
    walk = wc.Walk(Oracle(), steps.inputs)
    saw = {}
    trusted = {}
    last = None                     # (trigger, t before it, t after it, w after it) of the last mutating step, not observed since
    for (op, a), info in zip(steps, infos):
        m = walk.main
        before = m.t.copy() if op in wc.MUTATING else None
        out = walk.apply(op, a)
        if op in wc.MUTATING:
            fused = op == "integrate_frames_device" and info["launches"] and all(l[0] == "fused" for l in info["launches"])
            if fused and last is not None:
                trigger, t0, t1, w1 = last
                wrong = int(((t0 == 1) & (t1 != 1) & (walk.main.w != w1)).sum())
                trusted[trigger] = max(trusted.get(trigger, -1), wrong)
            trigger = op if op in TRUSTED_AFTER else "scalar" if info["launches"] == [("one", 1)] else None
            last = (trigger, before, walk.main.t.copy(), walk.main.w.copy()) if trigger and op != "fuse_into" else None
        elif op in wc.OBSERVING or op == "partner":
            last = None
        if op in ("fuse_from", "fuse_into", "fuse_dry"):
            saw[op] = max(saw.get(op, 0), out["sampled"])
        elif op == "download":
            saw[op] = max(saw.get(op, 0), int((out[1] > 0).sum()))
        elif op == "download_labels":
            saw[op] = max(saw.get(op, 0), int(np.count_nonzero(out[0])))
        elif op == "download_colour":
            saw[op] = max(saw.get(op, 0), int(np.count_nonzero(out)))
        elif op == "count_surface":
            saw[op] = max(saw.get(op, 0), out)
        elif op == "extent":
            saw[op] = max(saw.get(op, 0), out["n_surface"])
        elif op == "raycast":
            saw[op] = max(saw.get(op, 0), int(out["hit"].sum()))
            for name in ("label", "colour"):
                if name in out:
                    saw["raycast " + name] = max(saw.get("raycast " + name, 0), int(np.count_nonzero(out[name])))
    w = walk.main.w
    return {"saw": saw, "trusted": trusted, "observed": float((w > 0).mean()), "fresh": float((w == 0).mean()),
            "partner_observed": float((walk.partner.w > 0).mean())}


@pytest.mark.parametrize("cls", list(wc.CLASSES))
def test_the_model_is_not_idle(cls):
    saw, trusted = {}, {}
    for seed in wc.SEEDS[cls]:
        r = model_run(seed, cls)
        assert r["observed"] >= 0.10 and r["fresh"] >= 0.01, (seed, r["observed"], r["fresh"])
        for k, v in r["saw"].items():
            saw[k] = max(saw.get(k, 0), v)
        for k, v in r["trusted"].items():
            trusted[k] = max(trusted.get(k, -1), v)
    print(cls, saw, trusted)
    for op in wc.observing_kinds(cls) + ["fuse_from", "fuse_into"]:
        assert saw.get(op, 0) >= (100 if op == "raycast" else 1), (op, saw)
    if cls in ROWS_OF_4:
        assert saw["raycast label"] > 0 and saw["raycast colour"] > 0
        # a fused sequence directly after each of the calls that leave the summary words to be trusted; but for reset (after
        # which "all ones" is the truth) stale words would change what the sequence computes
        assert set(trusted) == set(TRUSTED_AFTER), trusted
        assert all(trusted[k] > 0 for k in TRUSTED_AFTER if k != "reset"), trusted


# ------------------------------------------------------------------------------------------------------------------------
# the batch walk
# ------------------------------------------------------------------------------------------------------------------------
def test_the_batch_walk_covers_its_ops_and_its_model_is_not_idle():
    from oracle.oracle import Oracle
    oracle = Oracle()
    dims = [(c.dim_x, c.dim_y, c.dim_z) for c in wc.batch_configs()]
    assert len(set(dims)) == 3 and all(d[0] % 4 == 0 for d in dims)
    ops, saw = set(), {}
    some_masks_missing = merges_written = 0
    for seed in wc.BATCH_SEEDS:
        steps = wc.batch_script(seed)
        assert 30 <= len(steps) <= 75, len(steps)
        walk = wc.BatchWalk(oracle, steps.inputs)
        for op, a in steps:
            ops.add(op)
            out = walk.apply(op, a)
            if op == "integrate":
                some_masks_missing += None in a["masks"] and any(k is not None for k in a["masks"])
            elif op == "fuse":
                merges_written += a["write"]
                saw[op] = max(saw.get(op, 0), out["sampled"])
            elif op == "extent":
                saw[op] = max(saw.get(op, 0), out["n_surface"])
            elif op == "extents":
                saw[op] = max(saw.get(op, 0), min(e["n_surface"] for e in out))
            elif op == "raycast":
                saw[op] = max(saw.get(op, 0), int(out["hit"].sum()))
            elif op == "batch_raycast":
                saw[op] = max(saw.get(op, 0), len(set(out["member"][out["member"] >= 0].tolist())))
        for m in walk.members:
            assert (m.w > 0).mean() >= 0.10, seed
    print(saw)
    assert ops == set(wc.BATCH_OPS)
    assert some_masks_missing > 0 and merges_written > 0
    assert saw["fuse"] > 0 and saw["extent"] > 0 and saw["extents"] > 0 and saw["raycast"] >= 100
    assert saw["batch_raycast"] >= 2, "no render in which two members win pixels"
