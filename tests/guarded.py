"""Guard bands round a device buffer the test owns (test infrastructure, no GPU needed, no fixtures).

include/tsdf_hip.h promises a caller that a device pointer needs its element's alignment only and that exactly the stated
elements are read or written.  A fresh torch tensor cannot show a breach: it is 512-byte aligned and sits inside a larger
block of the caching allocator, so a stray read sees mapped zeros and a stray store hits nobody's data.  Guarded makes ONE
uint8 allocation laid out [front band | payload | back band]: a stray access lands in a band, inside the same allocation,
where it is seen -- a store by bands_intact(), a load whose value is used by the result differing between the two fills of the
role -- and never on unmapped memory.

    g = Guarded(torch, "cuda", np.float32, h * w, "depth", "A", residue=4, row_bytes=4 * w, value=median)
    g.write(depth); call(g.ptr); sync; assert not g.bands_intact().size and g.payload_unchanged()
"""
import numpy as np

MIN_BAND = 4096                      # bytes; a band is at least this and at least 4 image rows
ALIGN = 16                           # the payload's address is congruent to `residue` modulo this
NAN_BITS = 0x7FC00BAD                # a quiet NaN with a payload of its own


def _nan():
    return np.array([NAN_BITS], np.uint32).view(np.float32)


# role -> (dtype, fill A, fill B): both fills are LIVE, a consumer that read the band would act on the value.  None: the value
# comes from the caller (the frame's median valid depth).
ROLES = {
    "depth": (np.float32, _nan(), None),
    "mask": (np.uint8, [255], [0]),
    "rgb": (np.uint8, [255], [0]),
    "raw": (np.uint16, [0xFFFF], [0]),
    "label": (np.uint16, [0xFFFF], [1]),
    "score": (np.float32, _nan(), [0.99]),
    "member": (np.int32, [0], [-1]),
    "cluster": (np.int32, [0], [-1]),
    "normal": (np.float32, np.repeat(_nan(), 3), [0.0, 0.0, 1.0]),
}
OUT_BYTES = {"A": 0xA5, "B": 0x5A}   # role "out": payload and bands prefilled with this byte


def fill_pattern(role, fill, dtype, value=None):
    """The bytes of one fill element (three floats for a normal), as a uint8 array."""
    assert fill in ("A", "B"), fill
    if role == "out":
        return np.full(np.dtype(dtype).itemsize, OUT_BYTES[fill], np.uint8)
    want, a, b = ROLES[role]
    assert np.dtype(dtype) == np.dtype(want), f"role {role} holds {np.dtype(want)}, not {np.dtype(dtype)}"
    v = a if fill == "A" else b
    if v is None:
        assert value is not None, f"fill B of role {role} needs the caller's value"
        v = [value]
    return np.ascontiguousarray(np.asarray(v, dtype=want)).view(np.uint8).copy()


def element_residue(dtype):
    """The payload residue at which nothing beyond element alignment holds: the element size (1 for bytes)."""
    return np.dtype(dtype).itemsize


class Guarded:
    def __init__(self, torch, device, dtype, n_elems, role, fill, residue=0, row_bytes=0, value=None):
        self.torch, self.dtype, self.n, self.role, self.fill = torch, np.dtype(dtype), int(n_elems), role, fill
        es = self.dtype.itemsize
        assert 0 <= residue < ALIGN and residue % es == 0, f"residue {residue} is not aligned to the {es}-byte element"
        self.nbytes = self.n * es
        band = max(MIN_BAND, 4 * int(row_bytes))
        self.pattern = fill_pattern(role, fill, dtype, value)
        self.buf = torch.empty(band + self.nbytes + band + 2 * ALIGN, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        self.off = band + (residue - (base + band)) % ALIGN          # front band: at least `band` bytes
        self.ptr = base + self.off
        assert self.ptr % ALIGN == residue and self.off + self.nbytes + band <= self.buf.numel()
        # the pattern is phased on the payload's first byte, so the element right before it and the one right after its last
        # both read as the fill value
        k = (np.arange(self.buf.numel()) - self.off) % self.pattern.size
        self.expected = self.pattern[k]
        if role != "out":                                             # an input's payload is whatever write() puts there
            self.expected[self.off:self.off + self.nbytes] = 0
        self.buf.copy_(torch.from_numpy(self.expected))
        self.written = None

    def write(self, array):
        a = np.ascontiguousarray(array, dtype=self.dtype).ravel()
        assert a.size == self.n, f"{a.size} elements for a payload of {self.n}"
        self.written = a.view(np.uint8).copy()
        self.buf[self.off:self.off + self.nbytes].copy_(self.torch.from_numpy(self.written))
        return self

    def _bytes(self):
        return self.buf.cpu().numpy()

    def read(self):
        return self._bytes()[self.off:self.off + self.nbytes].copy().view(self.dtype)

    def bands_intact(self):
        """Offsets of the band bytes that changed, relative to the payload's first byte (negative: front band; nbytes and
        above: back band); empty when both bands are intact."""
        bad = self._bytes() != self.expected
        bad[self.off:self.off + self.nbytes] = False
        return np.flatnonzero(bad) - self.off

    def payload_unchanged(self):
        assert self.written is not None, "payload_unchanged() is for inputs: nothing was written"
        return bool(np.array_equal(self._bytes()[self.off:self.off + self.nbytes], self.written))

    def prefill(self):
        """The typed payload an output starts from."""
        return self.expected[self.off:self.off + self.nbytes].copy().view(self.dtype)
