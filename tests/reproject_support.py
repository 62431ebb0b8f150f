"""What the tests of rt_reproject (tests/test_gpu_reproject.py) share with the tests of the passes that carry an image across a camera move."""
import ctypes as C

import numpy as np


def records_of(pkg, dev, h, w):
    out = np.zeros((h, w), dtype=pkg.abi.AOV_DTYPE)
    assert dev.hip.hipMemcpy(C.c_void_p(out.ctypes.data), dev.p, C.c_size_t(out.nbytes), C.c_int(2)) == 0
    return out


def move_camera(pkg, mgr, offset=(0.25, 0.1, 0.15), turn=(0.0, 2.0, 0.0)):
    """The manager's camera, `offset` further and `turn` degrees on; the new parameters are set (rt_set_params)."""
    t = mgr.camera.transform
    if hasattr(t, "position"):
        mgr.camera.transform = pkg.Transform(tuple(np.array(t.position) + np.array(offset)), tuple(np.array(t.euler) + np.array(turn)))
    else:  # a camera given by its matrix (scene files): the offset alone
        assert not any(turn)
        m = np.array(t.localToWorldMatrix, dtype=np.float64)
        m[:3, 3] += offset
        mgr.camera.transform = type(t)(m)
    mgr.SetShaderParams()


NEARBY = dict(offset=(0.05, 0.02, 0.03), turn=(0.0, 0.4, 0.0))
