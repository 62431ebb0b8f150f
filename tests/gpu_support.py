"""What the GPU tests of several subjects share: the counter names, comparisons on the bit patterns, device memory without torch, and
RT_* variables set for the length of a block.  Importing this module touches no GPU: libamdhip64.so is opened when a DevBuf is made."""
import contextlib
import ctypes as C
import os

import numpy as np

F = np.float32
KEYS = ["segments", "innerSteps", "leafSteps", "triTests", "sphereTests", "modelVisits", "pixelFrames"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bits_equal(a, b):
    return a.shape == b.shape and bool(np.all(a.view(np.uint32) == b.view(np.uint32)))


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if len(bad):
        y, x, k = bad[0]
        raise AssertionError(f"{what}: {len(set(map(tuple, bad[:, :2])))} pixels differ; first at row {y}, column {x}, channel {k}: "
                             f"got {got[y, x]}, want {want[y, x]}")


class DevBuf:
    """Device memory through the HIP runtime the library already loaded (torch would bring a second runtime into this process: the
    torch tests run in a child)."""

    def __init__(self, nbytes, fill=0):
        self.hip = C.CDLL("libamdhip64.so")
        self.nbytes = nbytes
        self.p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(max(nbytes, 16))) == 0
        assert self.hip.hipMemset(self.p, fill, C.c_size_t(max(nbytes, 16))) == 0 and self.hip.hipDeviceSynchronize() == 0

    @classmethod
    def of(cls, array):
        array = np.ascontiguousarray(array)
        d = cls(array.nbytes)
        assert d.hip.hipMemcpy(d.p, C.c_void_p(array.ctypes.data), C.c_size_t(array.nbytes), C.c_int(1)) == 0
        return d

    @property
    def ptr(self):
        return self.p.value

    def upload(self, arr):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        assert self.hip.hipMemcpy(self.p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), C.c_int(1)) == 0
        return self

    def download(self, dtype, count=None):
        out = np.zeros(self.nbytes // np.dtype(dtype).itemsize if count is None else count, dtype=dtype)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.p, C.c_size_t(out.nbytes), C.c_int(2)) == 0
        return out

    def image(self, h, w):
        out = np.zeros((h, w, 4), dtype=F)
        assert out.nbytes == self.nbytes
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.p, C.c_size_t(self.nbytes), C.c_int(2)) == 0
        return out

    def records(self, pkg, h, w):
        out = np.zeros((h, w), dtype=pkg.abi.AOV_DTYPE)
        assert out.nbytes == self.nbytes
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.p, C.c_size_t(self.nbytes), C.c_int(2)) == 0
        return out

    def free(self):
        self.hip.hipFree(self.p)


@contextlib.contextmanager
def environment(env, names):
    """`names` (the RT_* variables the caller's subject reads when a context is made or a scene uploaded) cleared, then `env` set; on
    leaving, each of `names` is as it was"""
    old = {k: os.environ.get(k) for k in names}
    for k in names:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
