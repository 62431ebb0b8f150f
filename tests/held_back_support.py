"""The machinery of tests/test_gpu_held_back.py that its child process needs too: device memory, the scenes, one side of a comparison, a
case with its held-back frames, the drive of a row of tests/flush_table.py and the child's main."""
import ctypes as C
import json
import os

import numpy as np

import flush_table as ft

W, H, SEED = 64, 40, 7
ENV = ("RT_HOLD_BACK", "RT_COALESCE", "RT_FUSE_CAP")
MODES = {"held": {"RT_HOLD_BACK": "1"}, "eager": {"RT_COALESCE": "0"}, "plain": {}}
_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
    return _hip


class Dev:
    def __init__(self, nbytes=None, data=None):
        if data is not None:
            data = np.ascontiguousarray(data)
            nbytes = data.nbytes
        self.nbytes = nbytes
        self.p = C.c_void_p()
        assert hip().hipMalloc(C.byref(self.p), C.c_size_t(max(nbytes, 16))) == 0
        if data is not None:
            assert hip().hipMemcpy(self.p, C.c_void_p(data.ctypes.data), C.c_size_t(nbytes), C.c_int(1)) == 0
        else:
            assert hip().hipMemset(self.p, 0, C.c_size_t(max(nbytes, 16))) == 0 and hip().hipDeviceSynchronize() == 0

    @property
    def ptr(self):
        return self.p.value

    def get(self, dtype, shape=None):
        return read_device(self.ptr, self.nbytes, dtype, shape)

    def free(self):
        hip().hipFree(self.p)


def read_device(ptr, nbytes, dtype, shape=None):
    out = np.zeros(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
    assert hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), C.c_int(2)) == 0
    return out.reshape(shape) if shape is not None else out


_DATA = {}


def scene_of(pkg, cfg):
    sc = pkg.scenes.get(cfg)
    if not sc.spheres:      # config 3 is models only: rt_update_spheres needs a sphere to move
        sc.spheres = [pkg.Sphere((0.3, 0.6, 0.2), 0.25, pkg.RayTracingMaterial(diffuseCol=(0.9, 0.5, 0.2, 1)))]
    sc.settings.update(numRaysPerPixel=2, maxBounceCount=4)
    return sc


class Side:
    """A tracer (the library's or the oracle's) behind its RayComputeManager mirror, set up as the reference's OnEnable does — with the
    BVHs of a configuration built once for all cases."""

    def __init__(self, pkg, lib, cfg):
        self.pkg, self.lib, self.cfg, self.abi = pkg, lib, cfg, pkg.abi
        self.W, self.H = W, H
        self.rows = None        # rt_set_partition: the image rows this context renders

    def setup(self):
        sc = scene_of(self.pkg, self.cfg)
        self.W, self.H = W, H
        mgr = self.mgr = sc.make_manager(self.tr, self.lib, W, H)
        if self.cfg not in _DATA:
            _DATA[self.cfg] = mgr.CreateAllMeshData(mgr.models)
        self.data = _DATA[self.cfg]
        mgr.renderSeed, mgr.numAccumulatedFrames = SEED, 1
        self.tr.resize(W, H)
        mgr._sized = mgr.hasBVH = True
        mgr.meshInfo = self.data["meshInfo"].copy()
        self.tr.upload_scene(ft.fill_models(self), self.data["triangles"], self.data["nodes"], mgr._pack_spheres())
        mgr.SetShaderParams()
        self.tr.reset_accumulation()

    def frames(self, n, one_by_one=True):
        if one_by_one:
            for _ in range(n):
                self.tr.render_frame()
        else:
            self.tr.render_frames(n)
        self.mgr.numAccumulatedFrames += n


class Env:
    """monkeypatch's setenv / delenv for the child process, which has no fixture"""

    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k, raising=False):
        os.environ.pop(k, None)


class Case(Side):
    def __init__(self, pkg, api, cfg, mode, multi, env, extra_env=None):
        super().__init__(pkg, api, cfg)
        self.api, self.mode, self.multi, self.env, self.extra_env = api, mode, multi, env, dict(extra_env or {})
        self.keep, self.devs, self.streams, self.own_stream = {}, [], [], True
        self.tr = None
        self.fresh()

    # -- contexts: the hooks are read by rt_create
    def _environment(self):
        for k in ENV:
            self.env.delenv(k, raising=False)
        for k, v in dict(MODES[self.mode], **self.extra_env).items():
            self.env.setenv(k, v)

    def make_tracer(self):
        self._environment()
        return self.api.create_tracer(0)

    def make_multi(self):
        self._environment()
        return self.api.create_multi_tracer([0, 0])

    def fresh(self):
        self.tr = self.make_multi() if self.multi else self.make_tracer()
        self.setup()
        assert self.pending() == 0 and self.frame() == 1

    def pending(self):
        return self.tr.pending_frames()

    def frame(self):
        return self.tr.context(0).frame() if self.multi else self.tr.frame()

    # -- device memory and streams of the case
    def dev(self, nbytes=None, data=None):
        d = Dev(nbytes, data)
        self.devs.append(d)
        return d

    def new_stream(self):
        s = C.c_void_p()
        assert hip().hipStreamCreate(C.byref(s)) == 0 and s.value
        self.streams.append(s)
        return s.value

    def device_synchronize(self):
        assert hip().hipDeviceSynchronize() == 0

    def read_device(self, ptr, dtype, shape):
        return read_device(ptr, int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype, shape)

    def close(self):
        if self.tr is not None and self.tr.h:
            if not self.own_stream:
                self.tr.set_stream(None)
            self.tr.close()
        for s in self.streams:
            hip().hipStreamDestroy(s)
        for d in self.devs:
            d.free()


def expected_pending(row, mode):
    if mode != "held":
        return 0
    return {ft.FLUSHES: 0, ft.LEAVES: 3, ft.HOLDS: 4, ft.CREATES: 3}[row.cls]


def drive(c, row):
    """the case on the library; every pending count on the way is asserted"""
    held = c.mode == "held"
    c.frames(2, one_by_one=False)
    c.tr.synchronize()
    assert c.pending() == 0
    if c.cfg == 2:      # the FLAT scene within the caps: the per-launch tables are in play
        first = c.tr.context(0) if c.multi else c.tr
        assert first.primary_table() == 1
    if row.prepare:
        row.prepare(c)
    assert c.pending() == 0 and c.frame() == 3
    for k in range(3):
        c.frames(1)
        assert c.pending() == (k + 1 if held else 0)
    assert c.frame() == 1 + 2 + 3
    ret = row.call(c)
    if row.gone:
        assert c.pending() == 0 and c.frame() == 1      # the fresh context
    else:
        assert c.pending() == expected_pending(row, c.mode), (row.id, c.mode)
        if row.cls in (ft.LEAVES, ft.CREATES):
            assert c.frame() == 6
    if callable(ret):
        ret = ret()
    eligible = held and c.own_stream and c.mgr.accumulate       # off the context's own stream, or without accumulation, nothing is held back
    before = c.pending()
    for k in range(2):
        c.frames(1)
        assert c.pending() == (before + k + 1 if eligible else 0)
    acc = c.tr.read_accumulated().copy()
    assert c.pending() == 0
    return {"ret": ret or {}, "accumulated": acc, "frame": c.tr.read_frame().copy(), "counters": ft.counters_of(c), "get_frame": c.frame(), "rows": c.rows}


def run_modes(pkg, api, cfg, row, env, extra=None):
    out = {}
    for mode in ("held", "eager"):
        c = Case(pkg, api, cfg, mode, row.multi, env)
        if extra:
            c.keep.update(extra)
        try:
            out[mode] = drive(c, row)
        finally:
            c.close()
    return out


def child_main(row_id, cfg, out_path):
    """rt_gather_rccl: librccl is loaded here, in a process of its own (the test process later imports torch, which brings its own RCCL)"""
    import __graft_entry__ as graft
    pkg = graft.load_package()
    api = pkg.load_library()
    row = next(r for r in ft.ROWS if r.id == row_id)
    rccl = C.CDLL("librccl.so.1")
    comm = C.c_void_p()
    assert rccl.ncclCommInitAll(C.byref(comm), 1, (C.c_int * 1)(0)) == 0
    try:
        out = run_modes(pkg, api, cfg, row, Env(), extra={"comm": comm})
    finally:
        rccl.ncclCommDestroy(comm)
    arrays, scalars = {}, {}
    for mode, res in out.items():
        for k in ("accumulated", "frame"):
            arrays[f"{mode}.{k}"] = res[k]
        for k, v in res["ret"].items():
            arrays[f"{mode}.ret.{k}"] = v
        scalars[mode] = {"counters": res["counters"], "get_frame": res["get_frame"]}
    np.savez(out_path, **arrays)
    print("RESULT " + json.dumps(scalars))
