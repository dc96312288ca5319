"""bench.py's --full (no GPU needed): a plain run leaves out everything beside the headline; --full puts it back, and the
--no-* options leave parts of it out again."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

LEGS = ("no_cpu_baseline", "no_extras", "no_traffic", "no_extract")


def test_a_plain_run_is_the_headline_alone():
    a = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not a.full and all(getattr(a, k) for k in LEGS)
    assert (a.steps, a.warmup, a.grid, a.workload, a.mode) == (20, 5, 512, "sband", "frame")


def test_full_runs_everything_unless_told_otherwise():
    a = bench.parse(["--full"])
    assert a.full and not any(getattr(a, k) for k in LEGS)
    a = bench.parse(["--full", "--no-traffic", "--no-cpu-baseline"])
    assert a.no_traffic and a.no_cpu_baseline and not a.no_extras and not a.no_extract

