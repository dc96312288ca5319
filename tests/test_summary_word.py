"""The summary word without a device: semantic_slam_amd/csrc/host_derive.h (encoding, word_after_update -- the function the
one-frame kernel runs on the device) behind tests/summary_word_check.cpp, a stand-alone program built with AddressSanitizer and
UndefinedBehaviorSanitizer (every finding fatal) and run as a child process.  The program states every expectation from the
rule: all combinations of {bit 0, bit 1, bit 2} x {untouched, partly, fully updated} x {value left 1, not} at the counts 0, 1,
2^24 - 2 and 2^24 - 1, and the encode / decode round trips."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "the summary word check needs g++"
    exe = tmp_path_factory.mktemp("summary_word") / "summary_word_check"
    subprocess.check_call(["g++", *FLAGS, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "semantic_slam_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "summary_word_check.cpp")])
    return str(exe)


def test_encoding_and_transition(program):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([program], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and not p.stderr and "FAILED" not in out, f"rc {p.returncode}\n{out[-4000:]}\n{p.stderr.decode()[-4000:]}"
    # 16 encodings + 8 bit patterns (4 counts where bit 2 is set, 1 where it is not) x 3 x 2 transitions + the chain
    assert out.strip().splitlines()[-1] == f"checked {16 + (4 * 4 + 4 * 1) * 6 + 1} cases"
