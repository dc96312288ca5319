"""What the reference's own functions returned on the tests' inputs, stored under tests/golden/ref_<name>.npz.

The reference builds under oracle/_ref exist only where the reference repository was present at build time; these stored
results let the tests that compare against them run everywhere.  Large results are kept as SHA-256 digests of their
bytes (a digest that matches means the same bits), small ones as arrays.  Where oracle/_ref was built the tests also run
the reference live and check it against what is stored.  Regenerate with `python tests/golden/make_ref_vectors.py`."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def digest(*arrays):
    """SHA-256 over each array's dtype, shape and bytes (bytes objects as they are)."""
    h = hashlib.sha256()
    for a in arrays:
        if isinstance(a, (bytes, bytearray)):
            h.update(b"bytes %d:" % len(a))
            h.update(a)
            continue
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str} {a.shape}:".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def path(name):
    return os.path.join(GOLDEN, f"ref_{name}.npz")


class Stored:
    """The stored results of one test module: Stored(name)[key] -> array (digests are 0-d str arrays, read with .str())."""

    def __init__(self, name):
        self.name = name
        with np.load(path(name), allow_pickle=False) as z:
            self.d = {k: z[k] for k in z.files}

    def __getitem__(self, key):
        return self.d[key]

    def str(self, key):
        return str(self.d[key])

    def check_inputs(self, key, *arrays):
        """The inputs a stored result belongs to must be the ones the test built (same bits)."""
        assert digest(*arrays) == self.str(key + "/inputs"), \
            f"{self.name}:{key}: the test's inputs differ from those the stored reference results were made from"
