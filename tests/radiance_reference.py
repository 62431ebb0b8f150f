"""What tests/test_gpu_radiance.py compares rt_radiance_trace with: RCC:15 + RC:550-576 restated — camera_rays of tests/test_gpu_aov.py,
extended so that it also returns each pixel's generator state behind the two RandomPointInCircle draws (the state Trace is handed,
RC:576) and accepts per-pixel start states (the next sample of a pixel starts from the state the previous Trace left, RC:565-578) —
and the scene set-up the cases share.  One fp32 rounding per operation, in the reference's order; the draws come from the oracle's own
generator, the divide and the normalise from oracle_math_eval.  Test infrastructure: nothing here is imported by the product."""
import ctypes as C

import numpy as np

from gpu_support import bits

F = np.float32
F3 = C.c_float * 3


def oracle_eval(orc, op, x, y=None):
    x = np.ascontiguousarray(x, dtype=F)
    y = np.ascontiguousarray(np.zeros_like(x) if y is None else np.broadcast_to(np.asarray(y, dtype=F), x.shape), dtype=F)
    out = np.zeros_like(x)
    orc.math_eval(op, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size)
    return out


def pixel_start_states(orc, p, w, h, frame):
    """RC:550-552: the generator state a pixel of frame `frame` starts with, (h, w) uint32."""
    with np.errstate(all="ignore"):
        uvx = oracle_eval(orc, 6, np.arange(w, dtype=np.uint32).astype(F), F(w) - F(1))
        uvy = oracle_eval(orc, 6, np.arange(h, dtype=np.uint32).astype(F), F(h) - F(1))
        U, V = np.broadcast_to(uvx[None, :], (h, w)), np.broadcast_to(uvy[:, None], (h, w))
        pcx = np.where(np.isnan(U), F(0), U * F(w)).astype(np.uint64)
        pcy = np.where(np.isnan(V), F(0), V * F(h)).astype(np.uint64)
    return (((pcy * w + pcx) + np.uint64(frame) * np.uint64(719393) + np.uint64(p.renderSeed & 0xffffffff)) & np.uint64(0xffffffff)).astype(np.uint32)


def camera_rays(orc, p, w, h, frame=None, start=None):
    """Origin, direction and generator state of one camera ray per pixel of a w x h image: (h, w, 3) float32, (h, w, 3) float32 and
    (h, w) uint32 — the state after the two RandomPointInCircle draws of RC:565-572, which is what Trace receives.  `start`: the
    (h, w) uint32 states the draws begin with; default: those of camera ray 0 of frame `frame` (pixel_start_states)."""
    ieee = b"RT_MATH_IEEE" in orc.version()
    start = pixel_start_states(orc, p, w, h, frame) if start is None else np.asarray(start, dtype=np.uint32).reshape(h, w)
    with np.errstate(all="ignore"):
        uvx = oracle_eval(orc, 6, np.arange(w, dtype=np.uint32).astype(F), F(w) - F(1))  # RCC:15: id.xy / (Resolution - 1.0)
        uvy = oracle_eval(orc, 6, np.arange(h, dtype=np.uint32).astype(F), F(h) - F(1))
        U, V = np.broadcast_to(uvx[None, :], (h, w)), np.broadcast_to(uvy[:, None], (h, w))
        m = np.array(list(p.camLocalToWorld), dtype=F)
        vp = np.array(list(p.viewParams), dtype=F)

        def mul_point(x, y, z):  # mul(M, float4(v, 1)).xyz, summed left to right
            return [m[r] * x + m[4 + r] * y + m[8 + r] * z + m[12 + r] * F(1) for r in range(3)]
        focus = mul_point((U - F(0.5)) * vp[0], (V - F(0.5)) * vp[1], np.full(U.shape, F(1) * vp[2], dtype=F))
        zero = np.zeros(U.shape, dtype=F)
        cam_origin = mul_point(zero, zero, zero)
        right, up = m[0:3], m[4:7]
        dj = np.zeros(U.shape + (2,), dtype=F)
        jj = np.zeros(U.shape + (2,), dtype=F)
        after = np.zeros(U.shape, dtype=np.uint32)
        out2 = (C.c_float * 2)()
        for idx in np.ndindex(U.shape):
            st = C.c_uint32(int(start[idx]))
            orc.random_point_in_circle(C.byref(st), out2)
            dj[idx] = (out2[0], out2[1])
            orc.random_point_in_circle(C.byref(st), out2)
            jj[idx] = (out2[0], out2[1])
            after[idx] = st.value
        dx = oracle_eval(orc, 6, dj[..., 0] * F(p.defocusStrength), F(w))
        dy = oracle_eval(orc, 6, dj[..., 1] * F(p.defocusStrength), F(w))
        jx = oracle_eval(orc, 6, jj[..., 0] * F(p.divergeStrength), F(w))
        jy = oracle_eval(orc, 6, jj[..., 1] * F(p.divergeStrength), F(w))
        origin = [cam_origin[k] + right[k] * dx + up[k] * dy for k in range(3)]
        jfp = [focus[k] + right[k] * jx + up[k] * jy for k in range(3)]
        d = [jfp[k] - origin[k] for k in range(3)]
        dot = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        if ieee:
            n = oracle_eval(orc, 4, dot)
            direction = [oracle_eval(orc, 6, d[k], n) for k in range(3)]
        else:
            r = oracle_eval(orc, 8, dot)  # rt_normalize = v * rt_rsqrt(dot(v, v))
            direction = [d[k] * r for k in range(3)]
    return np.stack(origin, axis=-1).astype(F), np.stack(direction, axis=-1).astype(F), after


def oracle_pixels(orc, ot, w, h, frame):
    """oracle_trace_pixel for every pixel of frame `frame`: (h, w, 3) float32."""
    out = np.zeros((h, w, 3), dtype=F)
    o3 = F3()
    for y in range(h):
        for x in range(w):
            orc.trace_pixel(ot.h, x, y, frame, o3)
            out[y, x] = o3[:]
    return out


def divide(orc, x, y):
    """x / y as the oracle divides (RC:581)."""
    return oracle_eval(orc, 6, x, y)


FRAME = 3


NO_DOF = dict(defocusStrength=0.0, divergeStrength=0.0)


def params_of(sc, api, w, h, tweak):
    """The RtParams the scene's manager would set at w x h with `tweak` applied (no tracer involved)."""
    mgr = sc.desc.make_manager(None, api, w, h)
    for k, v in tweak.items():
        assert hasattr(mgr, k), k
        setattr(mgr, k, v)
    mgr.renderSeed = 5
    p = mgr.params()
    p.frame = FRAME
    return p


def assert_rgb(got, want, what):
    a, b = bits(got).reshape(-1, 3), bits(want).reshape(-1, 3)
    bad = np.argwhere((a != b).any(axis=1)).ravel()
    assert not len(bad), f"{what}: {len(bad)} of {len(a)} rays differ; first is ray {bad[0]}: got {got.reshape(-1, 3)[bad[0]]}, want {want.reshape(-1, 3)[bad[0]]}"
