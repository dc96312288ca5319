"""A slab's launch geometry without a device: semantic_slam_amd/csrc/launch_geometry.h (limits, the slab's views, the grid of
every mapping the product launches, the class table, the brick work list with list_bucket -- the function the pre-pass runs on
the device) and the table slot's layout of host_derive.h, behind tests/launch_geometry_check.cpp, a stand-alone program built
with AddressSanitizer and UndefinedBehaviorSanitizer (every finding fatal) and run as a child process.  The program states every
expectation from the rule; the number of cases it must report is counted here, again from the rule."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

DIMS_X = (1, 3, 4, 8, 36, 37, 100, 252, 256, 260, 512, 1024)
DIMS_Y = (1, 2, 3, 4, 5, 7, 8, 9, 13, 48, 200)
DEPTHS = (0, 1, 2, 3, 8, 9)
Z_BEGINS = (0, 5)


def legal_bricks(dim_x, dim_y):
    """Brick shapes (q quads, r rows, s slices) a grid accepts: q * r * s lanes of a wavefront at most, q a divisor of the row's
    quads, and a lane's byte offset within its brick a 32-bit number."""
    if dim_x % 4:
        return 0
    return sum(1 for q in range(1, 65) for r in range(1, 65) for s in range(1, 65)
               if q * r * s <= 64 and (dim_x // 4) % q == 0 and s * dim_x * dim_y < 1 << 30)


def expected_cases():
    # per shape: the slab's own views, every legal brick, the library's choice
    sweep = sum(len(DEPTHS) * len(Z_BEGINS) * (1 + legal_bricks(dx, dy) + 1) for dx in DIMS_X for dy in DIMS_Y)
    magic = 64                        # divisors 1 .. 64
    limits = 5 + 1 + 15 + 1           # admitted corners, the list too large to index, refusals (limit + 1, order), the image limit
    images = 5 * 3 + 3                # five sizes x (16, 8, 8 + fine), the three byte counts of 640 x 480
    guard = 2                         # either side of 2^31 - 1 - 1024
    return sweep + magic + limits + images + guard


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "the launch geometry check needs g++"
    exe = tmp_path_factory.mktemp("launch_geometry") / "launch_geometry_check"
    subprocess.check_call(["g++", *FLAGS, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "semantic_slam_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "launch_geometry_check.cpp")])
    return str(exe)


def test_geometry_grids_and_layouts(program):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([program], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0 and not p.stderr and "FAILED" not in out, f"rc {p.returncode}\n{out[-4000:]}\n{p.stderr.decode()[-4000:]}"
    assert out.strip().splitlines()[-1] == f"checked {expected_cases()} cases"
