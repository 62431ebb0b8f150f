"""oracle_math_eval and its operation numbers, for the tests of the math functions on the host and on the device."""
import numpy as np

OPS = {"log": 0, "exp": 1, "sin": 2, "cos": 3, "sqrt": 4, "pow": 5, "div": 6, "smoothstep": 7, "rsqrt": 8, "rcp": 9}


def ev(orc, op, x, y=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(np.zeros_like(x) if y is None else y, dtype=np.float32)
    out = np.empty_like(x)
    orc.math_eval(OPS[op], x.ctypes.data, y.ctypes.data, out.ctypes.data, len(x))
    return out
