"""The summary duty of a launch without a device: semantic_slam_amd/csrc/launch_geometry.h (Keeps, SummaryRecord -- what the
host knows of the words and what it queues ahead of a launch -- and one_frame, the kernel one frame runs) behind
tests/summary_duty_check.cpp, a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer (every finding
fatal) and run as a child process.  The record is walked through every event sequence up to length 6 beside a model of the
device, in the program; the kernel choice is printed case by case and held here to summary_spec.one_frame_kind and to the
Predictor step that goes with it, the restatement the GPU walks rest on.  Case counts are recomputed here from the rule."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import summary_spec as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

DIMS_X = (3, 4, 36, 252, 256, 260, 512)
DIMS_Y = (1, 5, 250)
DEPTHS = (0, 1, 749, 750)          # 256 x 250 x 750 is exactly CLASSIFY_MIN_VOXELS
VARIANTS = (0, 1, 3, 7, 8)
STEP_OF = {"nothing": "drop", "bits": "forget", "runs": "tile"}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "the summary duty check needs g++"
    exe = tmp_path_factory.mktemp("summary_duty") / "summary_duty_check"
    subprocess.check_call(["g++", *FLAGS, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "semantic_slam_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "summary_duty_check.cpp")])
    return str(exe)


def run(program, mode):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([program, mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and not p.stderr and "FAILED" not in out, f"rc {p.returncode}\n{out[-4000:]}\n{p.stderr.decode()[-4000:]}"
    return out.strip().splitlines()


def test_record_against_the_device_model(program):
    # the 4 x 5 single transitions, then every sequence of 1 .. 6 events over 5 from each of the 4 states
    assert run(program, "record")[-1] == f"checked {4 * 5 + 4 * sum(5 ** k for k in range(1, 7))} cases"


def predictor_step(lay, variant, masked, n_vox):
    """The step Predictor.launches takes for one one-frame launch: "drop", "forget" or "tile"."""
    p = ss.Predictor(lay, n_vox)
    p.events = []
    none = np.zeros(lay.n_words, bool)
    p.frames.append((none, none, none))
    p.launches([("frame", variant)], [masked])
    assert len(p.events) == 1 and not p.frames
    return p.events[0][0]


def test_kernel_choice_agrees_with_summary_spec(program):
    lines = run(program, "choice")
    cases = [(dx, dy, nz, v, m) for dx in DIMS_X for dy in DIMS_Y for nz in DEPTHS for v in VARIANTS for m in (0, 1)]
    assert lines[-1] == f"checked {2 * len(cases)} cases"        # each with tile tables that fit (printed) and that do not (checked there)
    assert len(lines) == len(cases) + 1
    layouts = {}
    seen = set()
    for line, (dx, dy, nz, variant, masked) in zip(lines, cases):
        *numbers, kernel, keeps = line.split()
        assert tuple(int(x) for x in numbers) == (dx, dy, nz, variant, masked), line
        # (the kind of a layout and its words per slice follow from the slice alone: no slices, no voxel tables to build)
        lay = layouts.setdefault((dx, dy), ss.Layout((dx, dy, 0)))
        kind = ss.one_frame_kind(lay, variant, bool(masked), dx * dy * nz)
        if kind == "multi":
            assert lay.kind == "flat" and kernel in ("flat", "bricks"), line      # both keep bits 0 and 1: both forget
        else:
            assert kernel == kind, f"{line}: summary_spec says {kind}"
        assert predictor_step(lay, variant, bool(masked), dx * dy * nz) == STEP_OF[keeps], line
        seen.add((kernel, keeps))
    assert seen == {("scalar", "nothing"), ("flat", "bits"), ("bricks", "bits"), ("tile", "runs")}
