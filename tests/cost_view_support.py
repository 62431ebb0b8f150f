"""What the tests of rt_render_cost (tests/test_gpu_cost_view.py) share with the tests that check the view on other scenes: the oracle's
work log read into RtPixelCost fields, both sides' per-pixel costs and the comparison."""
import ctypes as C

import numpy as np
import pytest

from fuzz_scenes import crowded_overflow_scene


# 'R' camera ray | 'S' segment | 'A' model entered | 'B' d inner step | 'C' n d leaf with n (capped at 255) tests | 'K' / 'O' / 'G'
# the segment's outcome (miss, opaque hit, glass hit) | 'E' path ended.  Parsed token by token: d and n are bytes that may equal a tag.
_R, _S, _A, _B, _C, _E = (ord(c) for c in "RSABCE")
_OUTCOME = {ord("K"): 0, ord("O"): 1, ord("G"): 2}


def cost_of_log(log):
    """The eight RtPixelCost fields of one pixel from its work log; second value: a leaf's count was capped (255)."""
    f = [0] * 8
    capped = False
    ray, seg, primary, i = -1, 0, False, 0
    while i < len(log):
        t = log[i]
        if t == _R:
            ray, seg, i = ray + 1, 0, i + 1
        elif t == _S:
            f[0] += 1
            seg += 1
            primary = seg == 1  # the camera ray's first segment (bounce 0)
            i += 1
        elif t == _B:
            f[1] += 1
            f[4] += primary
            i += 2
        elif t == _C:
            n = log[i + 1]
            capped |= n == 255
            f[2] += 1
            f[3] += n
            if primary:
                f[5] += 1
                f[6] += n
            i += 3
        elif t in _OUTCOME:
            if primary and ray == 0:
                f[7] = _OUTCOME[t]
            primary = False
            i += 1
        elif t in (_A, _E):
            i += 1
        else:
            raise ValueError(f"unknown work-log token {t} at byte {i}")
    return f, capped


@pytest.fixture(scope="module")
def orc_log(orc):
    """The oracle with oracle_trace_pixel_schedule bound (as tools/sched_trace.py binds it)."""
    orc._bind("trace_pixel_schedule", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int])
    return orc


def scene_of(pkg, spec):
    if spec == "crowded70":  # more than 64 models: the two-level filter, candidate masks and bounce count in LDS (MANY)
        return crowded_overflow_scene(pkg, 70, 5)
    cfg, kw = spec
    return pkg.scenes.get(cfg, **kw)


def manager(pkg, lib, tracer, spec, w, h, tweak=None, seed=1):
    mgr = scene_of(pkg, spec).make_manager(tracer, lib, w, h)
    for k, v in (tweak or {}).items():
        setattr(mgr, k, v)
    mgr.OnEnable(renderSeed=seed)
    return mgr


def gpu_cost(pkg, api, spec, w, h, frame, tweak=None, seed=1):
    tr = api.create_tracer(0)
    try:
        manager(pkg, api, tr, spec, w, h, tweak, seed)
        return tr.render_cost(frame)
    finally:
        tr.close()


def oracle_cost(pkg, orc_log, spec, w, h, frame, tweak=None, seed=1):
    tr = orc_log.create_tracer(1)
    try:
        manager(pkg, orc_log, tr, spec, w, h, tweak, seed)
        buf = (C.c_uint8 * (1 << 22))()
        out = np.zeros((h, w, 8), dtype=np.uint32)
        for y in range(h):
            for x in range(w):
                n = orc_log.trace_pixel_schedule(tr.h, x, y, frame, buf, len(buf))
                assert 0 < n <= len(buf)
                f, capped = cost_of_log(bytes(buf[:n]))
                assert not capped, "a leaf with 255+ triangles: the log cannot count it (rule 2 covers such scenes)"
                out[y, x] = f
        return out
    finally:
        tr.close()


def assert_cost_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint32, (what, got.shape, want.shape)
    bad = np.argwhere(np.any(got != want, axis=-1))
    if len(bad):
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} pixels differ; first at row {y}, column {x}: got {got[y, x].tolist()}, want {want[y, x].tolist()}")
