"""The random walks of tests/test_gpu_walk.py (tests/walk_cases.py), held to conditions without a GPU, so that the GPU test
cannot be vacuous: the scripts are deterministic and end on a download; over a class's seeds every ordered pair of mutating
ops occurs back to back and is observed, and every named situation of the handle's hidden state occurs (an observation, a
merge, a stream change while frames are collected; fused launches that trust the free-space summary right after the calls
that must rebuild or drop it; ten fused launches in a row under each classification mode; a brick shape change between two
fused launches); and the model alone, run over every script, is not idle.

The fourth class, "runs", and the batch walk with a row-mapped member have conditions of their own (second half of this file):
the grid and its frames are what they are named for, weight runs are alive when every mutating kind arrives and a one-frame
launch of integrate_tile follows that a stale summary word would lead astray, some walk crosses the count limit, the predictor
(tests/summary_spec.py) makes a claim for every launch, and the restated rule rejects what is wrong."""
import ctypes as C
import functools

import numpy as np
import pytest

import summary_spec as ss
import walk_cases as wc

OLD_CLASSES = ["row", "flat", "scalar"]     # the classes the conditions below were written for; "runs" has its own further down
ROWS_OF_4 = ["row", "flat"]


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
        assert (15 <= len(s) <= 50) if cls != "runs" else (60 <= len(s) <= 200), (seed, len(s))   # (runs: two observations per mutating step)
        assert all(op in wc.mutating_kinds(cls) + wc.POLICY + wc.observing_kinds(cls) + ["partner"] for op, _ in s)
        assert cls == "runs" or not any(op in wc.RUNS_ONLY for op, _ in s)
    a, b = wc.batch_script(1), wc.batch_script(1)
    assert equal(list(a), list(b)) and equal(a.inputs, b.inputs)
    assert all(wc.batch_script(seed)[-1][0] == "download" for seed in wc.BATCH_SEEDS)


def test_the_class_grids_are_what_they_are_named_for():
    for cls, c in wc.CLASSES.items():
        dx = c["dims"][0]
        assert {"row": dx % 256 == 0, "flat": dx % 4 == 0 and dx % 256 != 0, "scalar": dx % 4 != 0, "runs": dx % 256 == 0}[cls]
        assert int(np.prod(c["dims"])) <= 250000 and np.prod(c["partner"]) < np.prod(c["dims"])
        cfg, pcfg = wc.configs(0, cls)
        assert pcfg.voxel_size != cfg.voxel_size and list(pcfg.base2world) != list(cfg.base2world)
    assert set(wc.VARIANTS) == set(wc.capi.SHIPPED_VARIANTS)


# ------------------------------------------------------------------------------------------------------------------------
# what the scripts cover
# ------------------------------------------------------------------------------------------------------------------------
def observed_pairs(steps):
    """(a, b) for every two mutating steps with nothing but policy steps between them and an observation of the handle after
    them, before the next mutating step.  (The "runs" class looks at the words and the arrays after every mutating step: there
    observations may stand between the two as well.)"""
    mutating = wc.mutating_kinds(steps.cls)
    tokens = [op if op in mutating else "observed" if op in wc.observing_kinds(steps.cls) else "partner"
              for op, _ in steps if op not in wc.POLICY]
    if steps.cls == "runs":                                 # (every mutating step is observed at once)
        tokens = [t for t in tokens if t != "observed"]
        return {(a, b) for a, b in zip(tokens, tokens[1:]) if a in mutating and b in mutating}
    return {(a, b) for a, b, c in zip(tokens, tokens[1:], tokens[2:]) if a in mutating and b in mutating and c == "observed"}


@pytest.mark.parametrize("cls", list(wc.CLASSES))
def test_every_ordered_pair_of_mutating_ops_occurs_and_is_observed(cls):
    kinds = wc.mutating_kinds(cls)
    assert len(kinds) == {"row": 15, "flat": 15, "scalar": 11, "runs": 16}[cls]
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


@pytest.mark.parametrize("cls", OLD_CLASSES)
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


@pytest.mark.parametrize("cls", OLD_CLASSES)
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


# ------------------------------------------------------------------------------------------------------------------------
# the "runs" class: weight runs alive under every op, every summary word checked
# ------------------------------------------------------------------------------------------------------------------------
REBUILDS = ("upload", "load_state", "fuse_from", "refresh_external")
# the two mutating kinds that write no weight of the handle: the label kernel writes labels, fuse_into writes the partner.
# A word they left stale is the true word, so no launch after them can go wrong over it; they must leave every word as it is.
WRITES_NO_WEIGHT = ("integrate_labels_device", "fuse_into")


def test_the_runs_grid_is_what_it_is_named_for():
    from oracle.oracle import Oracle
    oracle = Oracle()
    c = wc.CLASSES["runs"]
    dims, vs = c["dims"], c["vs"]
    lay = ss.Layout(dims)
    assert dims[0] % 256 == 0 and dims[1] % 2 == 1 and lay.kind == "row" and lay.n_words == 2 * dims[1] * dims[2] == 108
    cfg, pcfg = wc.configs(0, "runs")
    assert cfg.trunc_margin == wc.synth.SBAND_TRUNC == pcfg.trunc_margin
    # every "whole" frame of every seed, under every pose the class draws, updates every voxel and leaves no value at 1
    depths = {}
    for seed in wc.SEEDS["runs"]:
        for f in wc.cached_script(seed, "runs").inputs["frames"]:
            if f["kind"] == "whole":
                depths[float(f["depth"][0, 0])] = f["depth"]
                assert np.all(f["depth"] == f["depth"][0, 0])
    assert len(depths) > 32
    some = list(depths.values())
    for k in range(8):
        for depth in some[k::8][:6] + [wc.synth.sfull_depth(*wc.IM_HW)]:
            m = wc.Model(oracle, cfg)
            m.integrate(depth, np.asarray(wc.synth.sband_pose(k), np.float32).ravel())
            assert np.all(m.w == 1.0) and np.all(m.t < 1.0), (k, float(depth[0, 0]))
    # each broken frame leaves segments untouched, wholly updated and partly updated, all three; one frame touches nothing
    inside = 0
    for seed in wc.SEEDS["runs"]:
        inp = wc.cached_script(seed, "runs").inputs
        assert tuple(f["kind"] for f in inp["frames"]) == wc.RUNS_FRAME_KINDS
        assert all(inp["frames"][k]["kind"] == "whole" for k in wc.WHOLE) and all(inp["frames"][k]["kind"] == "broken" for k in wc.BROKEN)
        for f in inp["frames"]:
            m = wc.Model(oracle, cfg)
            m.integrate(f["depth"], f["pose"])
            lo, hi = lay.every(m.w == 1.0), lay.some(m.w == 1.0)
            if f["kind"] == "broken":
                assert (~hi).sum() > 0 and lo.sum() > 0 and (hi & ~lo).sum() > 0, (seed, int((~hi).sum()), int(lo.sum()))
            elif f["kind"] == "nothing":
                assert not hi.any()
            elif f["kind"] == "whole":
                inside += bool((m.t < 0).any() and (m.t > 0).any())        # a zero crossing inside the grid
        kinds = [ss.rebuilt(lay, *st) for st in inp["states"]]
        runs = [int(ss.has_run(wd).sum()) for wd in kinds]
        assert runs == [108, 108, 107, 0, 0], runs
        assert len(set(ss.run_count(kinds[1]).tolist())) == 4 and (ss.run_count(kinds[1]) == 2 ** 24 - 2).any()
        assert all(0 < int((wd & 1).sum()) < 108 for wd in kinds), "a quarter of the segments all ones"
        assert inp["masks"][0].min() == 255 and 0 < (inp["masks"][1] == 255).mean() < 1
        blocks = inp["masks"][1][:, :128].reshape(60, 2, 2, 64)
        assert np.all(blocks == blocks[:, :1, :, :1]), "blocks of 2 x 64 pixels"
    assert inside >= 32, "whole frames with a surface inside the grid"
    # the library's own restatement of the layout: the words of a 200 x 24 x 12 grid lie by 256-voxel chunks of a slice
    flat = ss.Layout(wc.CLASSES["flat"]["dims"])
    assert flat.kind == "flat" and flat.per_slice == 19 and flat.n_words == 19 * 12 and flat.sizes[18] == 200 * 24 - 18 * 256
    assert ss.Layout(wc.CLASSES["scalar"]["dims"]).n_words == 0 and ss.Layout(wc.CLASSES["row"]["dims"]).n_words == 24 * 12


@functools.lru_cache(maxsize=None)
def runs_model_run(seed):
    """The model and the predictor over one script of the "runs" class: per step the predicted words before and after, the
    predictor's events (tile launches with their frame's effect, forgets, drops, resets, rebuilds), what observing ops saw."""
    from oracle.oracle import Oracle
    steps = wc.cached_script(seed, "runs")
    walk = wc.Walk(Oracle(), steps.inputs, predict=True)
    pred, lay = walk.pred, walk.lay
    pred.events = []
    rows, saw = [], {}
    for op, a in steps:
        before, n0 = pred.words.copy(), len(pred.events)
        t0, w0 = walk.main.t.copy(), walk.main.w.copy()
        out = walk.apply(op, a)
        rows.append({"op": op, "before": before, "after": pred.words.copy(), "events": pred.events[n0:],
                     "same_arrays": np.array_equal(ss.bits(t0), ss.bits(walk.main.t)) and np.array_equal(ss.bits(w0), ss.bits(walk.main.w))})
        assert pred.claim.all()
        shown = pred.words if pred.exact else pred.words & ~np.uint32(1)      # (bit 0 is predicted after reset and rebuilds only)
        assert not ss.unsound(lay, shown, walk.main.t, walk.main.w) or pred.frames, \
            "the prediction itself is sound for the model's arrays whenever no frame waits"
        if op == "count_surface":
            saw[op] = max(saw.get(op, 0), out)
        elif op == "extent":
            saw[op] = max(saw.get(op, 0), out["n_surface"])
        elif op == "raycast":
            saw[op] = max(saw.get(op, 0), int(out["hit"].sum()))
        elif op in ("fuse_from", "fuse_into", "fuse_dry"):
            saw[op] = max(saw.get(op, 0), out["sampled"])
    return {"rows": rows, "saw": saw, "final": pred.words.copy(), "tiles": pred.tile_launches, "no_claims": pred.no_claims, "lay": lay}


def live(words):
    """Segments whose word carries a run of a count >= 1."""
    return ss.has_run(words) & (ss.run_count(words) >= 1)


def stale_errors(rows, i, lay):
    """For the mutating step i: (voxels that one-frame launches after it would get wrong had the step left the words as it
    found them, whether such a launch wholly updated a segment that carried a live run before the step); up to the next
    reset or rebuild.  The stale words move as the kernels would move them: summary_spec.after_update, forget, drop."""
    stale, was_live = rows[i]["before"].copy(), live(rows[i]["before"])
    wrong, whole = 0, False
    for row in rows[i + 1:]:
        for ev in row["events"]:
            if ev[0] in ("reset", "rebuild"):
                return wrong, whole
            if ev[0] == "forget":
                stale &= np.uint32(3)
            elif ev[0] == "drop":
                stale[:] = 0
            elif ev[0] == "tile":
                effect = ev[1]
                wrong += ss.stale_run_errors(lay, stale, effect[3], effect[4])
                whole = whole or bool((effect[1] & was_live).any())
                stale = ss.after_update(stale, *effect[:3])
    return wrong, whole


def test_the_runs_walks_keep_runs_alive_under_every_op():
    kinds = wc.mutating_kinds("runs")
    assert "refresh_external" in kinds and len(kinds) == 16
    met = {}                        # kind -> the most voxels a stale run would get wrong after an occurrence that met live runs
    tiles = no_claims = crossed = 0
    saw = {}
    for seed in wc.SEEDS["runs"]:
        r = runs_model_run(seed)
        rows, lay = r["rows"], r["lay"]
        tiles += r["tiles"]
        no_claims += r["no_claims"]
        for k, v in r["saw"].items():
            saw[k] = max(saw.get(k, 0), v)
        met_live = sum(bool((live(ev[2]) & ev[1][0]).any()) for row in rows for ev in row["events"] if ev[0] == "tile")
        assert met_live >= 5, (seed, met_live)
        assert 0 < int(ss.has_run(r["final"]).sum()) < lay.n_words, (seed, int(ss.has_run(r["final"]).sum()))
        for i, row in enumerate(rows):
            if row["op"] in kinds and live(row["before"]).mean() >= 0.25:
                wrong, whole = stale_errors(rows, i, lay)
                if row["op"] in WRITES_NO_WEIGHT:
                    assert wrong == 0 and row["same_arrays"] and np.array_equal(row["before"], row["after"]), (seed, i, row["op"])
                if whole:
                    met[row["op"]] = max(met.get(row["op"], -1), wrong)
        # the count limit: a segment at 2^24 - 2, then 2^24 - 1, then without a run
        for s in range(lay.n_words):
            c = [int(ss.run_count(row["after"][s])) if ss.has_run(row["after"][s]) else -1 for row in rows if row["op"] in kinds]
            c = [x for j, x in enumerate(c) if j == 0 or x != c[j - 1]]
            crossed += any(c[j:j + 3] == [2 ** 24 - 2, 2 ** 24 - 1, -1] for j in range(len(c)))
    share = no_claims / tiles
    print(f"runs: {tiles} one-frame tile launches, {no_claims} without a claim ({share:.1%}); stale-run errors per kind {met}; "
          f"{crossed} segments crossed the count limit; saw {saw}")
    assert share <= 0.10
    assert set(met) == set(kinds), set(kinds) - set(met)
    assert all((met[k] > 0) != (k in WRITES_NO_WEIGHT) for k in kinds), met
    assert crossed > 0
    assert saw["count_surface"] > 0 and saw["extent"] > 0 and saw["raycast"] >= 50 and saw["fuse_from"] > 0 and saw["fuse_into"] > 0


def test_a_written_merge_of_the_runs_class_changes_some_segments_and_leaves_others():
    hit = 0
    for seed in wc.SEEDS["runs"]:
        r = runs_model_run(seed)
        for row in r["rows"]:
            if row["op"] == "fuse_from" and not row["same_arrays"]:
                both = ss.has_run(row["before"]) & ss.has_run(row["after"]) & (row["before"] == row["after"])
                hit += bool(both.any() and (row["before"] != row["after"]).any())
    assert hit > 0


def test_the_named_situations_of_the_runs_class_occur():
    seen = set()
    one = other = 0
    lay = ss.Layout(wc.CLASSES["runs"]["dims"])
    for seed in wc.SEEDS["runs"]:
        steps = wc.cached_script(seed, "runs")
        infos = wc.trace(steps, "runs")
        for (op, a), info in zip(steps, infos):
            if op in wc.observing_kinds("runs") and info["pend"] > 0:
                seen.add(("observed while collected", op))
            if (op == "fuse_from" and info["p_pend"] > 0) or (op == "fuse_into" and info["pend"] > 0):
                seen.add(("merge of a source with collected frames", op))
            if op == "set_stream" and info["pend"] > 0:
                seen.add("set_stream while collected")
            for launch, masked in zip(info["launches"], info["masked"]):
                if launch[0] == "one":
                    kind = ss.one_frame_kind(lay, launch[1], masked, lay.n_vox)
                    seen.add((kind, bool(masked)))
                    one += kind == "tile"
                    other += kind != "tile"
                else:
                    seen.add(launch[0])
                    other += launch[0] == "fused"
    print(f"runs: {one} launches of integrate_tile, {other} other launches that write weights")
    assert one > 2 * other, "most frames go through integrate_tile"
    want = {("observed while collected", op) for op in wc.observing_kinds("runs")}
    want |= {("merge of a source with collected frames", op) for op in ("fuse_from", "fuse_into")}
    want |= {"set_stream while collected", "fused", "label", ("tile", False), ("tile", True), ("bricks", True), ("scalar", False), ("scalar", True)}
    assert want <= seen, want - seen


# ------------------------------------------------------------------------------------------------------------------------
# the rule's restatement, held to the rule
# ------------------------------------------------------------------------------------------------------------------------
def test_sound_rejects_what_is_wrong():
    lay = ss.Layout((512, 3, 2))
    n = lay.n_vox
    t, w = np.full(n, 0.5, np.float32), np.full(n, 3.0, np.float32)
    good = np.full(lay.n_words, 2 | 4 | (3 << 8), np.uint32)
    assert ss.sound(lay, good, t, w) and np.array_equal(ss.rebuilt(lay, t, w), good)

    def why(words, t=t, w=w):
        return {x[2] for x in ss.unsound(lay, words, t, w)}

    bad = good.copy()
    bad[5] = 2 | 4 | (4 << 8)
    assert why(bad) == {"bit 2 over a weight that is not float32(count)"}                     # a wrong count
    w1 = w.copy()
    w1[256 * 7 + 255] = 4.0
    assert why(good, w=w1) == {"bit 2 over a weight that is not float32(count)"}              # one voxel differs
    assert [x[0] for x in ss.unsound(lay, good, t, w1)] == [7] and not ss.has_run(ss.rebuilt(lay, t, w1)[7])
    mz = np.full(n, -0.0, np.float32)
    assert why(np.full(lay.n_words, 2 | 4, np.uint32), w=mz) == {"bit 2 over a weight that is not float32(count)"}   # -0.0 is no count
    assert ss.sound(lay, np.full(lay.n_words, 2, np.uint32), t, mz) and np.all(ss.rebuilt(lay, t, mz) == 2)
    for stray in (8, 16, 32, 64, 128):
        bad = good.copy()
        bad[0] |= stray
        assert why(bad) == {"bits 3..7"}
    assert why(good | np.uint32(1)) == {"bit 0 over a TSDF value that is not 1.0f"}
    assert why(np.full(lay.n_words, 4 | (3 << 8), np.uint32)) == {"bit 2 without bit 1"}
    assert why(np.full(lay.n_words, 2 | (3 << 8), np.uint32)) == {"a count without bit 2"}
    neg = w.copy()
    neg[3] = -1.0
    assert "bit 1 over a weight that is negative or not finite" in why(good, w=neg)
    assert ss.rebuilt(lay, t, neg)[0] == 0
    inf = w.copy()
    inf[3] = np.inf
    assert "bit 1 over a weight that is negative or not finite" in why(np.full(lay.n_words, 2, np.uint32), w=inf)
    half = np.full(n, 2.5, np.float32)
    assert np.all(ss.rebuilt(lay, t, half) == 2)
    big = np.full(n, 2.0 ** 24, np.float32)
    assert np.all(ss.rebuilt(lay, t, big) == 2), "2^24 is above the largest count"
    assert np.all(ss.rebuilt(lay, np.ones(n, np.float32), np.full(n, 2.0 ** 24 - 1, np.float32)) == (7 | ((2 ** 24 - 1) << 8)))
    # zero is sound for anything; the fresh word for a fresh grid only
    assert ss.sound(lay, np.zeros(lay.n_words, np.uint32), t, neg)
    assert ss.sound(lay, np.full(lay.n_words, 7, np.uint32), np.ones(n, np.float32), np.zeros(n, np.float32))
    assert not ss.sound(lay, np.full(lay.n_words, 7, np.uint32), t, w)


def test_after_update_follows_the_cases_of_the_stand_alone_check():
    """tests/summary_word_check.cpp's cases, restated: {bit 0} x {bit 1} x {bit 2} x counts x {untouched, partly, fully
    updated} x {value left 1, not}, the limit spelled out, and the chain from a fresh word."""
    counts = [0, 1, 2 ** 24 - 2, 2 ** 24 - 1]
    cases = 0
    for b in range(8):
        for c in counts:
            if not b & 4 and c:
                continue
            old = b | (c << 8)
            for how in range(3):
                for not_one in (False, True):
                    touched, whole = how != 0, how == 2
                    if not touched:
                        want = old
                    else:
                        b0, b1, b2, cnt = b & 1, b & 2, b & 4, c
                        if not_one:
                            b0 = 0
                        if b2:
                            if whole and c + 1 < 2 ** 24:
                                cnt = c + 1
                            else:
                                b2, cnt = 0, 0
                        want = b0 | b1 | b2 | (cnt << 8)
                    got = int(ss.after_update(np.array([old], np.uint32), np.array([touched]), np.array([whole]), np.array([not_one]))[0])
                    assert got == want, (hex(old), how, not_one, hex(got), hex(want))
                    assert got & 2 == old & 2 and (not got & 1 or old & 1) and (not got & 4 or old & 4) and (got & 4 or got >> 8 == 0) and not got & 0xF8
                    cases += 1
    assert cases == (4 * 4 + 4) * 6

    def step(word, touched, whole, not_one):
        return int(ss.after_update(np.array([word], np.uint32), np.array([touched]), np.array([whole]), np.array([not_one]))[0])

    assert step(3 | 4 | ((2 ** 24 - 2) << 8), True, True, False) == 3 | 4 | ((2 ** 24 - 1) << 8)
    assert step(3 | 4 | ((2 ** 24 - 1) << 8), True, True, False) == 3
    word = ss.FRESH
    for n in range(1, 1001):
        word = step(word, True, True, False)
        assert word == 3 | 4 | (n << 8)
    word = step(word, True, True, True)
    assert word == 2 | 4 | (1001 << 8)
    word = step(word, True, False, False)
    assert word == 2
    assert step(word, True, True, False) == 2
    # the kernel a one-frame launch runs: rows of 256 voxels, rows of 4, any row; variant 8 classifies a masked frame always
    row, flat, none = ss.Layout((512, 2, 1)), ss.Layout((200, 2, 1)), ss.Layout((37, 2, 1))
    assert [ss.one_frame_kind(row, v, False, 1000) for v in (0, 1, 3, 7, 8)] == ["tile", "scalar", "tile", "tile", "tile"]
    assert [ss.one_frame_kind(row, v, True, 1000) for v in (0, 1, 3, 7, 8)] == ["tile", "scalar", "tile", "tile", "bricks"]
    assert [ss.one_frame_kind(row, v, True, 48_000_000) for v in (0, 3, 7, 8)] == ["bricks", "bricks", "tile", "bricks"]
    assert ss.one_frame_kind(row, 0, True, 47_999_999) == "tile" and ss.one_frame_kind(row, 0, False, 48_000_000) == "tile"
    assert {ss.one_frame_kind(flat, v, m, 1000) for v in (0, 3, 7, 8) for m in (False, True)} == {"multi"}
    assert {ss.one_frame_kind(none, v, m, 1000) for v in (0, 1, 3, 7, 8) for m in (False, True)} == {"scalar"}


# ------------------------------------------------------------------------------------------------------------------------
# the batch walk with runs alive
# ------------------------------------------------------------------------------------------------------------------------
def test_the_batch_runs_walk_has_its_situations_and_its_model_is_not_idle():
    from oracle.oracle import Oracle
    oracle = Oracle()
    cfgs = wc.batch_runs_configs()
    kinds = [ss.Layout((c.dim_x, c.dim_y, c.dim_z)).kind for c in cfgs]
    assert kinds == ["flat", "row", "flat"] and kinds[wc.ROW_MEMBER] == "row"
    assert (cfgs[1].dim_x, cfgs[1].dim_y, cfgs[1].dim_z, cfgs[1].voxel_size) == (256, 10, 6, np.float32(0.01))
    for c in cfgs:                                          # whole frames update all of every member
        for k in range(8):
            m = wc.Model(oracle, c)
            m.integrate(wc.synth.sfull_depth(*wc.IM_HW), np.asarray(wc.synth.sband_pose(k), np.float32).ravel())
            assert np.all(m.w == 1.0) and np.all(m.t < 1.0)
    a, b = wc.batch_runs_script(1), wc.batch_runs_script(1)
    assert equal(list(a), list(b)) and equal(a.inputs, b.inputs)
    for seed in wc.BATCH_RUNS_SEEDS:
        steps = wc.batch_runs_script(seed)
        assert len(steps) <= 120 and steps[-1][0] == "download"
        walk = wc.BatchRunsWalk(oracle, steps.inputs)
        pred, lay = walk.preds[wc.ROW_MEMBER], walk.lays[wc.ROW_MEMBER]
        pred.events = []
        seen, stale, wrong = set(), None, 0
        for i, (op, a) in enumerate(steps):
            before = pred.words.copy()
            n0 = len(pred.events)
            walk.apply(op, a)
            if op == "integrate" and "situation" in a:
                # the row member holds a run (of the count 0 after reset) in at least a quarter of its segments when the batched kernel meets it ...
                assert ss.has_run(before).mean() >= 0.25 and not ss.has_run(pred.words).any(), (seed, i)
                assert steps[i + 1 + 6] == ("member_integrate", {"member": wc.ROW_MEMBER, "frame": steps[i + 7][1]["frame"]})
                if a["situation"] == "block_mask":
                    assert 0 < (walk.members[wc.ROW_MEMBER].w != walk.members[wc.ROW_MEMBER].w[0]).mean() < 1
                stale, name = before, a["situation"]
            elif op == "member_integrate" and stale is not None:
                # ... and the one-frame launch on its handle would store wrong weights had the runs not been forgotten
                (ev,) = [e for e in pred.events[n0:] if e[0] == "tile"]
                wrong = ss.stale_run_errors(lay, stale, ev[1][3], ev[1][4])
                assert wrong > 0 and steps.inputs["frames"][a["frame"]]["kind"] == "whole", (seed, i, wrong)
                assert steps[i + 1][0] == "summary_words" and steps[i + 2][0] == "download"
                seen.add(name)
                stale = None
        assert seen == set(wc.BATCH_RUNS_SITUATIONS), (seed, seen)
        for m in walk.members:
            assert (m.w > 0).mean() >= 0.5, seed
