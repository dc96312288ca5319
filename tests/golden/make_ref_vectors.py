"""Regenerate tests/golden/ref_*.npz: what the reference's own functions (oracle/_ref, built by `make -C oracle ref ref_host`
where the reference repository is present) return on the inputs of tests/test_oracle_vs_ref.py, tests/test_pose_math.py and
tests/test_writers_and_adapters.py.  The inputs are built by those tests' own functions; only their digests are stored.

    make -C oracle ref ref_host && python tests/golden/make_ref_vectors.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

from oracle.oracle import Oracle, Ref, RefHost  # noqa: E402
from ref_vectors import digest, path  # noqa: E402
import test_oracle_vs_ref as ovr  # noqa: E402
import test_pose_math as pm  # noqa: E402
import test_writers_and_adapters as wa  # noqa: E402


def main():
    assert Ref.available() and RefHost.available(), "oracle/_ref not built (make -C oracle ref ref_host)"
    oracle, ref, ref_host = Oracle(), Ref(), RefHost()

    out = {}
    cases = [(f"body{s}", ovr.body_case(oracle, s), (3, 2)) for s in range(8)]
    cases += [(f"degenerate{i}", c, (0, 0)) for i, c in enumerate(ovr.degenerate_cases())]
    cases.append(("non_finite", ovr.non_finite_case(), (3, 2)))
    for key, case, threads in cases:
        out[key + "/inputs"] = np.array(digest(*ovr.case_inputs(*case)))
        out[key] = np.array(digest(*ovr._run(ref, *case, threads=threads[1])))
    np.savez_compressed(path("oracle_vs_ref"), **out)

    out = {}
    pairs = pm.multiply_inputs()
    out["multiply/inputs"] = np.array(digest(np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])))
    out["multiply/want"] = pm.reference_multiply(ref_host, pairs)
    ms = pm.invert_inputs()
    out["invert/inputs"] = np.array(digest(np.stack(ms)))
    out["invert/ok"], out["invert/want"] = pm.reference_invert(ref_host, ms)
    pairs = pm.composition_inputs()
    out["composition/inputs"] = np.array(digest(np.stack([b for b, _ in pairs]), np.stack([c for _, c in pairs])))
    out["composition/ok"], out["composition/want"] = pm.reference_composition(ref_host, pairs)
    np.savez_compressed(path("pose_math"), **out)

    out = {}
    with tempfile.TemporaryDirectory() as d:
        for k, (dims, vs, origin, t, w) in enumerate(wa.ply_cases(oracle)):
            out[f"ply{k}/inputs"] = np.array(digest(*wa.ply_case_inputs(dims, vs, origin, t, w)))
            f = os.path.join(d, f"ref{k}.ply")
            ref_host.save_ply(f, t, w, dims, vs, origin)
            raw = open(f, "rb").read()
            out[f"ply{k}"], out[f"ply{k}/len"] = np.array(digest(raw)), np.array(len(raw))
    np.savez_compressed(path("writers"), **out)
    for name in ("oracle_vs_ref", "pose_math", "writers"):
        print(path(name), os.path.getsize(path(name)), "bytes")


if __name__ == "__main__":
    main()
