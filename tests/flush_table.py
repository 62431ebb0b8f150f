"""The hold-back contract of the C ABI, one row per entry point.

rt_render_frame holds a frame back while the GPU is still busy: it counts it (ctx->pending, rt_get_frame) and the held frames leave later
as one fused launch, with the state the context has at that moment.  So every entry point that reads what those frames produce, or changes
what they depend on, has to launch them first.  ROWS has a row for every function declared in include/*.h that takes a context: its
first parameter is an RtContext*, an RtMulti*, or a call descriptor with such a member, as rt_mis_trace's RtMisBatch.  The two functions
that create a context have rows too.  A row says which side of the contract the function is on and how tests/test_gpu_held_back.py
calls it with three frames held back (RT_HOLD_BACK=1 forces the hold, rt_debug_pending_frames shows it):

    flushes   after the call nothing is pending (rt_debug_pending_frames == 0): the held frames were launched before the call read or
              changed anything
    leaves    the call launches nothing: pending and rt_get_frame are what they were.  Only the functions of LEAVES_ALLOWED, or a function
              whose header comment says that it "neither reads nor changes what a frame depends on"
    holds     rt_render_frame and its multi form, the calls that do the holding: pending grows by one (until the cap launches them)
    creates   rt_create, rt_create_multi: a new context holds nothing, and touches no other context

tests/test_flush_table.py (no GPU) fails when a declared function has no row, a row has no function, or a function is listed twice, so
a new pass cannot be added without deciding which side it is on.

A recipe is call(c) -> what the call hands back, as a dict of arrays / numbers (or a function that collects them once the pending count has
been checked: what a device form wrote is read after a synchronise).  c is the Case of tests/test_gpu_held_back.py: c.tr the tracer,
c.mgr its RayComputeManager mirror, c.dev() device memory, c.keep what prepare(c) left.  prepare(c) runs before the frames are held back.
oracle(o) makes the same logical step on the CPU oracle (o.tr, o.mgr), which has no hold-back; rows without one leave the image alone, and
rows the oracle cannot follow (oracle_final = False) are compared with an eager twin context (RT_COALESCE=0) only.
Test infrastructure: nothing here is imported by the product."""
import ctypes as C
import json
import os

import numpy as np

FLUSHES, LEAVES, HOLDS, CREATES = "flushes", "leaves", "holds", "creates"

# the only functions that may be `leaves` without the sentence in their header comment
LEAVES_ALLOWED = frozenset([
    "rt_last_error", "rt_get_frame", "rt_local_rows", "rt_local_to_global_row", "rt_debug_fused_frames_cap", "rt_debug_primary_table",
    "rt_debug_tile_cand", "rt_debug_tile_tri", "rt_debug_pending_frames", "rt_debug_multi_pending_frames", "rt_multi_count",
    "rt_multi_last_gather_ms", "rt_multi_peer_access"])
LEAVES_SENTENCE = "neither reads nor changes what a frame depends on"
HOLDS_ALLOWED = frozenset(["rt_render_frame", "rt_multi_render_frame"])
CREATES_ALLOWED = frozenset(["rt_create", "rt_create_multi"])


def held_at(tracer, where, forced):
    """The frames `tracer` holds back right before the call a test is about.  With the hold forced (RT_HOLD_BACK=1) there must be some: the
    test then IS about held-back frames.  With the hook off it is a race, so the count is only recorded — one JSON line per call site in the
    file RT_HELD_LOG names, if it is set: how often the timing-dependent variants meet a held frame is worth knowing."""
    n = tracer.pending_frames()
    if forced:
        assert n > 0, f"{where}: no frame is held back although RT_HOLD_BACK is set"
    path = os.environ.get("RT_HELD_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"where": where, "forced": bool(forced), "pending": n}) + "\n")
    return n


class Row:
    def __init__(self, function, cls, how, call, oracle=None, prepare=None, multi=False, oracle_final=True, oracle_counters=True, gone=False,
                 child=False, case=""):
        self.function = function      # the C symbol
        self.cls = cls
        self.how = how                # how the GPU test calls it, in words
        self.call = call
        self.oracle = oracle          # the same logical step on the oracle, or None: the image does not depend on the call
        self.prepare = prepare
        self.multi = multi            # the case runs on an RtMulti of two contexts on device 0
        self.oracle_final = oracle_final          # the final image, last frame and frame counter are the oracle's
        self.oracle_counters = oracle_counters    # ... and so are segments and pixelFrames
        self.gone = gone              # the context does not exist after the call (rt_destroy): a fresh one renders instead
        self.child = child            # runs in a child process (RCCL must not be loaded into the test process)
        self.case = case              # a second row of one function: what is different about it

    @property
    def id(self):
        return self.function + ("-" + self.case if self.case else "")


# ---------------------------------------------------------------- logical steps, the same code for the library and the oracle
def _transform(x, t, dx):
    return x.pkg.Transform((t.position[0] + dx, t.position[1] + 0.25, t.position[2]), t.euler, t.scale)


def fill_models(x):
    """RayComputeManager.UpdateModels without the call: the packed models of the manager's models as they stand"""
    from_matrix = x.pkg.manager.matrix_to_abi
    for i, model in enumerate(x.mgr.models):
        x.mgr.meshInfo[i]["worldToLocal"] = from_matrix(model.transform.worldToLocalMatrix)
        x.mgr.meshInfo[i]["localToWorld"] = from_matrix(model.transform.localToWorldMatrix)
        x.mgr.meshInfo[i]["material"] = model.material.pack()
    return x.mgr.meshInfo


def move_model(x):
    m = x.mgr.models[-1]
    m.transform = _transform(x, m.transform, 0.3)
    x.tr.update_models(fill_models(x))


def move_sphere(x):
    s = x.mgr.spheres[0]
    s.centre = (s.centre[0] + 0.4, s.centre[1] + 0.2, s.centre[2])
    x.tr.update_spheres(x.mgr._pack_spheres())


def move_camera(x):
    t = x.mgr.camera.transform
    x.mgr.camera.transform = x.pkg.Transform((t.position[0] + 0.5, t.position[1], t.position[2] + 0.3), (t.euler[0], t.euler[1] + 7.0, t.euler[2]))
    x.mgr.SetShaderParams()


def fewer_bounces(x):
    x.mgr.maxBounceCount = 2
    x.mgr.SetShaderParams()


def accumulate_off(x):
    x.mgr.accumulate = False
    x.mgr.SetShaderParams()


def another_scene(x):
    m = x.mgr.models[-1]
    m.transform = _transform(x, m.transform, -0.4)
    s = x.mgr.spheres[0]
    s.centre = (s.centre[0] - 0.3, s.centre[1] + 0.4, s.centre[2])
    s.radius *= 1.5
    x.tr.upload_scene(fill_models(x), x.data["triangles"], x.data["nodes"], x.mgr._pack_spheres())


def smaller_image(x):
    x.tr.resize(40, 24)
    x.W, x.H = 40, 24


def same_size_again(x):
    """what rt_set_partition and new render targets mean for the oracle: empty targets of the same size, the frame counter kept"""
    x.tr.resize(x.W, x.H)


def checkpoint(x):
    img = (np.arange(x.H * x.W * 4, dtype=np.float32).reshape(x.H, x.W, 4) % 97.0) / 16.0
    img[..., 3] = 5.0
    return img


def reset_accumulation(x):
    x.tr.reset_accumulation()          # (not ResetAccumulatedRender: its rt_set_params with frame 1 would be the call that flushes)
    x.mgr.numAccumulatedFrames = 1


def write_checkpoint(x):
    x.tr.write_accumulated(checkpoint(x))


def counters_of(x):
    c = x.tr.counters()
    c.pop("gpuMs")
    return c


# ---------------------------------------------------------------- what the calls take
def rays(c, n=96):
    """n rays from the camera towards the scene (a fixed fan), as abi.RAY_DTYPE"""
    rng = np.random.default_rng(11)
    o = np.tile(np.asarray(c.mgr.camera.transform.position, dtype=np.float32), (n, 1))
    d = (rng.uniform(-0.5, 0.5, (n, 3)) * [1.0, 0.6, 0.0] + [0.0, -0.1, 1.0]).astype(np.float32)
    return c.abi.make_rays(o, d)


def path_rays(c, n=96):
    r = rays(c, n)
    return c.abi.make_path_rays(r["origin"], r["dir"], (np.arange(1, n + 1, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32))


def image_bytes(c):
    return c.W * c.H * 16


def aov_bytes(c):
    return c.W * c.H * 64


def random_sum(c, seed):
    """an accumulated image as eight frames would leave it: positive colours, alpha = the frame count"""
    img = np.random.default_rng(seed).uniform(0.0, 6.0, (c.H, c.W, 4)).astype(np.float32)
    img[..., 3] = 8.0
    return img


def random_moments(c, seed):
    lum = np.random.default_rng(seed).uniform(0.1, 2.0, (c.H, c.W)).astype(np.float32)
    m = np.zeros((c.H, c.W, 4), dtype=np.float32)
    m[..., 0], m[..., 1], m[..., 3] = lum * 4, lum * lum * 5, 4.0
    return m


def aov_records(c, frame=1):
    """device records of the current view (an AOV pass of the context itself: made before the frames are held back)"""
    d = c.dev(aov_bytes(c))
    c.tr.render_aov_to_device(frame, d.ptr, d.nbytes)
    c.tr.synchronize()
    return d


def reproject_params(c):
    return c.api.reproject_params(c.mgr.params())


def motion_table(c):
    sp, md = c.mgr._pack_spheres(), fill_models(c).copy()
    moved = md.copy()
    moved["localToWorld"][:, 12] += 0.125          # every model came from 1/8 to the left
    table = c.api.motion_table(sp, sp, moved, md)
    return c.dev(data=table), len(table)


# ---------------------------------------------------------------- prepare steps
def p_stream(c):
    c.keep["stream"] = c.new_stream()


def p_targets(c):
    c.keep["old"] = c.tr.render_targets()
    c.keep["new"] = (c.dev(image_bytes(c)), c.dev(image_bytes(c)))


def p_timer(c):
    c.tr.timer_begin()


def p_prev_aov(c):
    c.keep["prev"] = aov_records(c)
    c.keep["cur"] = c.dev(aov_bytes(c))


def p_prev_aov_moving(c):
    p_prev_aov(c)
    c.keep["motion"], c.keep["n_objects"] = motion_table(c)


def p_two_aovs(c):
    c.keep["prev"], c.keep["cur"] = aov_records(c, 1), aov_records(c, 2)
    c.tr.variance_update()


def p_moments(c):
    c.tr.variance_update()


def p_tile_list(c):
    c.tr.adaptive_set_tiles([0, 3, 9, 17])


def p_selection(c):
    c.tr.variance_update()
    c.tr.adaptive_select(c.api.adaptive_params(threshold=0.0, minFrames=1))


def p_filter_inputs(c):
    c.keep["aov"] = aov_records(c)
    c.keep["in"] = c.dev(data=random_sum(c, 5))
    c.keep["moments"] = c.dev(data=random_moments(c, 6))
    c.keep["out"] = c.dev(image_bytes(c))


def p_reproject_inputs(c):
    c.keep["prev_aov"], c.keep["cur_aov"] = aov_records(c, 1), aov_records(c, 2)
    c.keep["in"] = c.dev(data=random_sum(c, 7))
    c.keep["out"] = c.dev(image_bytes(c))
    c.keep["motion"], c.keep["n_objects"] = motion_table(c)


def p_ray_buffers(record_bytes):
    def prepare(c):
        r = rays(c)
        c.keep["n"] = len(r)
        c.keep["rays"] = c.dev(data=r)
        c.keep["path_rays"] = c.dev(data=path_rays(c))
        c.keep["out"] = c.dev(len(r) * record_bytes)
    return prepare


def p_gather_target(c):
    c.keep["out"] = c.dev(image_bytes(c))


# ---------------------------------------------------------------- recipes
def image_of(buf, c):
    return lambda: {"image": buf.get(np.float32, (c.H, c.W, 4))}


def after(c, buf, dtype, shape=None, key="out"):
    """what a device form wrote, read once the stream has been waited for"""
    def collect():
        c.tr.synchronize()
        return {key: buf.get(getattr(c.abi, dtype) if isinstance(dtype, str) else dtype, shape)}
    return collect


def c_set_stream(c):
    c.tr.set_stream(c.keep["stream"])
    c.own_stream = False


def c_bind_targets(c):
    f, a = c.keep["new"]
    c.tr.bind_render_targets(f.ptr, a.ptr)
    old_f, old_a = c.keep["old"]
    return lambda: {"accumulated": c.read_device(old_a, np.float32, (c.H, c.W, 4)), "frame": c.read_device(old_f, np.float32, (c.H, c.W, 4))}


def o_bind_targets(o):
    out = {"accumulated": o.tr.read_accumulated().copy(), "frame": o.tr.read_frame().copy()}
    same_size_again(o)
    return out


def c_get_targets(c):
    f, a = c.tr.render_targets()

    def collect():
        c.device_synchronize()      # the host's own synchronise: the call has launched the frames, nothing else waits for them
        return {"accumulated": c.read_device(a, np.float32, (c.H, c.W, 4)), "frame": c.read_device(f, np.float32, (c.H, c.W, 4))}
    return collect


def o_read_both(o):
    return {"accumulated": o.tr.read_accumulated().copy(), "frame": o.tr.read_frame().copy()}


def c_set_partition(c):
    c.tr.set_partition(8, 1, 2)
    c.rows = c.tr.local_to_global_rows()


def counted(x):
    """the counters both the library and the oracle keep without statistics switched on"""
    c = counters_of(x)
    return {"segments": c["segments"], "pixelFrames": c["pixelFrames"]}


def c_reset_counters(c):
    c.tr.reset_counters()
    return {"counters": counters_of(c), "counted": counted(c)}


def o_reset_counters(o):
    o.tr.reset_counters()
    return {"counted": counted(o)}


def c_get_counters(c):
    return {"counters": counters_of(c), "counted": counted(c)}


def o_get_counters(o):
    return {"counted": counted(o)}


def c_debug_intersect(c):
    r = rays(c, 32)
    return {"hits": c.tr.debug_intersect(r["origin"], r["dir"])}


def c_math_eval(c):
    return {"values": c.tr.debug_math_eval(5, np.linspace(0.25, 9.0, 64, dtype=np.float32), np.linspace(1.0, 3.0, 64, dtype=np.float32))}


def c_aov_to_device(c):
    d = c.dev(aov_bytes(c))
    c.tr.render_aov_to_device(2, d.ptr, d.nbytes)
    return after(c, d, c.abi.AOV_DTYPE, (c.H, c.W))


def c_aov_centre_to_device(c):
    d = c.dev(aov_bytes(c))
    c.tr.render_aov_centre_to_device(d.ptr, d.nbytes)
    return after(c, d, c.abi.AOV_DTYPE, (c.H, c.W))


def c_denoise_to_device(c):
    d = c.dev(image_bytes(c))
    c.tr.denoise_to_device(d.ptr, d.nbytes, c.api.denoise_params(scale=0.2))
    return after(c, d, np.float32, (c.H, c.W, 4))


def c_denoise_buffers(c):
    k = c.keep
    c.tr.denoise_buffers(c.W, c.H, k["in"].ptr, k["aov"].ptr, k["out"].ptr, c.api.denoise_params(scale=0.125))
    return after(c, k["out"], np.float32, (c.H, c.W, 4))


def c_denoise_variance_buffers(c):
    k = c.keep
    c.tr.denoise_variance_buffers(c.W, c.H, k["in"].ptr, k["moments"].ptr, k["aov"].ptr, k["out"].ptr, c.api.variance_denoise_params(scale=0.125))
    return after(c, k["out"], np.float32, (c.H, c.W, 4))


def c_resolve_buffers(c):
    k = c.keep
    c.tr.resolve_buffers(c.W, c.H, k["in"].ptr, k["out"].ptr)
    return after(c, k["out"], np.float32, (c.H, c.W, 4))


def c_moments_update_buffers(c):
    k = c.keep
    snapshot = c.dev(image_bytes(c))
    c.tr.moments_update_buffers(c.W, c.H, k["in"].ptr, snapshot.ptr, k["moments"].ptr)

    def collect():
        c.tr.synchronize()
        return {"moments": k["moments"].get(np.float32, (c.H, c.W, 4)), "snapshot": snapshot.get(np.float32, (c.H, c.W, 4))}
    return collect


def c_reproject_buffers(c):
    k = c.keep
    c.tr.reproject_buffers(c.W, c.H, k["in"].ptr, k["prev_aov"].ptr, k["cur_aov"].ptr, k["out"].ptr, reproject_params(c))
    return after(c, k["out"], np.float32, (c.H, c.W, 4))


def c_reproject_buffers_moving(c):
    k = c.keep
    c.tr.reproject_buffers_moving(c.W, c.H, k["in"].ptr, k["prev_aov"].ptr, k["cur_aov"].ptr, k["motion"].ptr, k["n_objects"], k["out"].ptr, reproject_params(c))
    return after(c, k["out"], np.float32, (c.H, c.W, 4))


def c_reproject_accumulated(c):
    k = c.keep
    c.tr.reproject_accumulated(reproject_params(c), k["prev"].ptr, 1, k["cur"].ptr)
    return after(c, k["cur"], c.abi.AOV_DTYPE, (c.H, c.W), key="cur_aov")


def c_reproject_accumulated_moving(c):
    k = c.keep
    c.tr.reproject_accumulated_moving(reproject_params(c), k["prev"].ptr, 1, k["motion"].ptr, k["n_objects"], k["cur"].ptr)
    return after(c, k["cur"], c.abi.AOV_DTYPE, (c.H, c.W), key="cur_aov")


def c_resolve_to_device(c):
    d = c.dev(image_bytes(c))
    c.tr.resolve_to_device(d.ptr, d.nbytes)
    return after(c, d, np.float32, (c.H, c.W, 4))


def c_variance_update(c):
    c.tr.variance_update()
    return lambda: {"moments": c.tr.read_moments()}


def c_variance_reset(c):
    c.tr.variance_reset()

    def collect():      # the snapshot the reset took has the held frames: the next batch is the two later frames alone
        first = c.tr.read_moments()
        c.tr.render_frames(2)
        c.mgr.numAccumulatedFrames += 2
        c.tr.variance_update()
        return {"moments": first, "next_batch": c.tr.read_moments()}
    return collect


def o_two_more_frames(o):
    o.tr.render_frames(2)
    o.mgr.numAccumulatedFrames += 2


def c_variance_carry(c):
    k = c.keep
    c.tr.variance_carry(reproject_params(c), k["prev"].ptr, k["cur"].ptr)
    return lambda: {"moments": c.tr.read_moments()}


def c_moments_to_device(c):
    d = c.dev(image_bytes(c))
    c.tr.moments_to_device(d.ptr, d.nbytes)
    return after(c, d, np.float32, (c.H, c.W, 4))


def c_denoise_variance_to_device(c):
    d = c.dev(image_bytes(c))
    c.tr.denoise_variance_to_device(d.ptr, d.nbytes)
    return after(c, d, np.float32, (c.H, c.W, 4))


def c_adaptive_select_buffers(c):
    k = c.keep
    tiles = ((c.W + 7) // 8) * ((c.H + 7) // 8)
    err, lst, counts = c.dev(tiles * 4), c.dev(tiles * 4), c.dev(16)
    c.tr.adaptive_select_buffers(c.W, c.H, k["in"].ptr, k["moments"].ptr, err.ptr, lst.ptr, counts.ptr, c.api.adaptive_params(threshold=0.01, minFrames=1))

    def collect():
        c.tr.synchronize()
        n = counts.get(np.uint32)
        return {"errors": err.get(np.float32), "tiles": lst.get(np.uint32)[: int(n[0])], "counts": n}
    return collect


def c_adaptive_select(c):
    got = c.tr.adaptive_select(c.api.adaptive_params(threshold=0.0, minFrames=1))
    return lambda: {"result": got, "tiles": c.tr.adaptive_tiles(), "errors": c.tr.adaptive_tile_error()}


def c_adaptive_set_tiles(c):
    c.tr.adaptive_set_tiles([1, 2, 30])
    return lambda: {"tiles": c.tr.adaptive_tiles()}


def c_adaptive_render_frames(c):
    c.tr.adaptive_render_frames(2)
    c.mgr.numAccumulatedFrames += 2
    return lambda: {"accumulated": c.tr.read_accumulated().copy(), "frame": c.tr.read_frame().copy()}


def c_buffers(method, key, dtype):
    def call(c):
        k = c.keep
        getattr(c.tr, method)(k[key].ptr, k["n"], k["out"].ptr)
        return after(c, k["out"], dtype)
    return call


def c_destroy(c):
    c.tr.close()
    c.fresh()


def o_fresh(o):
    o.fresh()


def c_create(c):
    other = c.make_tracer()
    try:
        return {"pending": other.pending_frames(), "frame": other.frame(), "error": other.api.last_error(other.h)}
    finally:
        other.close()


def c_create_multi(c):
    other = c.make_multi()
    try:
        return {"pending": other.pending_frames(), "count": c.api.multi_count(other.h)}
    finally:
        other.close()


def c_pending(c):
    assert c.tr.pending_frames() == (3 if c.mode == "held" else 0)


def c_fused_cap(c):
    assert 16 <= c.tr.fused_frames_cap() <= 64


def c_multi_context(c):
    h = c.api.multi_context(c.tr.h, 1)
    return {"is_a_context": bool(h), "its_rows": c.api.local_rows(h)}


def c_peer_access(c):
    pairs, enabled = C.c_int(-1), C.c_int(-1)
    return {"answer": c.api.multi_peer_access(c.tr.h, C.byref(pairs), C.byref(enabled)), "pairs": pairs.value, "enabled": enabled.value}


def c_gather_to_device(accumulated):
    def call(c):
        d = c.keep["out"]
        (c.tr.gather_accumulated_to_device if accumulated else c.tr.gather_frame_to_device)(1, d.ptr, d.nbytes)
        return {"image": d.get(np.float32, (c.H, c.W, 4))}        # (the gather synchronises every context)
    return call


def c_gather_rccl(c):
    d = c.keep["out"]
    c.tr.gather_rccl(c.keep["comm"], 0, d.ptr, d.nbytes, accumulated=True)
    return {"accumulated": d.get(np.float32, (c.H, c.W, 4))}


def o_read_accumulated(o):
    return {"accumulated": o.tr.read_accumulated().copy()}


def o_read_frame(o):
    return {"frame": o.tr.read_frame().copy()}


def o_gather_accumulated(o):
    return {"image": o.tr.read_accumulated().copy()}


def o_gather_frame(o):
    return {"image": o.tr.read_frame().copy()}


def o_render_frames_4(o):
    o.tr.render_frames(4)
    o.mgr.numAccumulatedFrames += 4


def c_render_frames_4(c):
    c.tr.render_frames(4)
    c.mgr.numAccumulatedFrames += 4


def c_render_frame(c):
    c.tr.render_frame()
    c.mgr.numAccumulatedFrames += 1


def o_render_frame(o):
    o.tr.render_frame()
    o.mgr.numAccumulatedFrames += 1


def c_multi_resize(c):
    smaller_image(c)


R = Row
ROWS = [
    # ---- include/rt_abi.h: the context
    R("rt_create", CREATES, "a second context made while the first holds three frames: it holds none, the first keeps its three", c_create),
    R("rt_destroy", FLUSHES, "destroyed with three frames pending; a fresh context then renders the oracle's image", c_destroy, o_fresh, gone=True),
    R("rt_last_error", LEAVES, "read", lambda c: {"error": c.api.last_error(c.tr.h)}),
    R("rt_set_stream", FLUSHES, "to a caller's stream; further rt_render_frame calls are launched at once", c_set_stream, prepare=p_stream),
    R("rt_resize", FLUSHES, "to 40 x 24: the held frames go to the old targets, the later ones to empty new ones", smaller_image, smaller_image),
    R("rt_set_partition", FLUSHES, "to part 1 of 2 in strips of 8 rows: the later frames render those rows into empty targets", c_set_partition,
      same_size_again, oracle_counters=False),
    R("rt_local_rows", LEAVES, "read", lambda c: {"rows": c.tr.local_rows()}),
    R("rt_local_to_global_row", LEAVES, "read for every local row", lambda c: {"rows": c.tr.local_to_global_rows()}),
    R("rt_bind_render_targets", FLUSHES, "to two empty device images: the three held frames are in the old targets, the later ones in the new",
      c_bind_targets, o_bind_targets, prepare=p_targets),
    R("rt_get_render_targets", FLUSHES, "the targets read by the host itself after its own device synchronise", c_get_targets, o_read_both),
    R("rt_upload_scene", FLUSHES, "another scene: a model and a sphere moved, the sphere grown", another_scene, another_scene),
    R("rt_update_models", FLUSHES, "the last model moved", move_model, move_model),
    R("rt_update_spheres", FLUSHES, "the first sphere moved", move_sphere, move_sphere),
    R("rt_set_params", FLUSHES, "another camera", move_camera, move_camera),
    R("rt_set_params", FLUSHES, "maxBounceCount 4 -> 2", fewer_bounces, fewer_bounces, case="bounces"),
    R("rt_set_params", FLUSHES, "accumulate switched off with frames pending", accumulate_off, accumulate_off, case="accumulate_off"),
    R("rt_reset_accumulation", FLUSHES, "called: the held frames must not land in the emptied image", reset_accumulation, reset_accumulation),
    R("rt_render_frame", HOLDS, "a fourth frame: held like the three before it", c_render_frame, o_render_frame),
    R("rt_flush", FLUSHES, "called: no host wait; rt_synchronize then reads correct bits", lambda c: c.tr.flush()),
    R("rt_render_frames", FLUSHES, "four frames behind the three held ones: seven frames in frame order", c_render_frames_4, o_render_frames_4),
    R("rt_synchronize", FLUSHES, "called", lambda c: c.tr.synchronize()),
    R("rt_get_frame", LEAVES, "read", lambda c: {"frame": c.tr.frame()}),
    R("rt_read_frame", FLUSHES, "read", lambda c: {"frame": c.tr.read_frame().copy()}, o_read_frame),
    R("rt_read_accumulated", FLUSHES, "read", lambda c: {"accumulated": c.tr.read_accumulated().copy()}, o_read_accumulated),
    R("rt_display", FLUSHES, "the accumulated image over five frames", lambda c: {"display": c.tr.display(5, True)}, lambda o: {"display": o.tr.display(5, True)}),
    R("rt_display_srgb8", FLUSHES, "the accumulated image over five frames, flipped", lambda c: {"display": c.tr.display_srgb8(5, True, True)},
      lambda o: {"display": o.tr.display_srgb8(5, True, True)}),
    R("rt_write_accumulated", FLUSHES, "a checkpoint: the held frames must not be added to it afterwards", write_checkpoint, write_checkpoint),
    # ---- include/rt_abi.h: several contexts in one process
    R("rt_create_multi", CREATES, "a second multi-context made while the first holds three frames", c_create_multi, multi=True),
    R("rt_destroy_multi", FLUSHES, "destroyed with three frames pending in every context; a fresh one then renders the oracle's image", c_destroy, o_fresh,
      multi=True, gone=True),
    R("rt_multi_count", LEAVES, "read", lambda c: {"count": c.api.multi_count(c.tr.h)}, multi=True),
    R("rt_multi_context", LEAVES, "context 1 looked up", c_multi_context, multi=True),
    R("rt_multi_resize", FLUSHES, "to 40 x 24", c_multi_resize, smaller_image, multi=True),
    R("rt_multi_upload_scene", FLUSHES, "another scene", another_scene, another_scene, multi=True),
    R("rt_multi_update_models", FLUSHES, "the last model moved", move_model, move_model, multi=True),
    R("rt_multi_update_spheres", FLUSHES, "the first sphere moved", move_sphere, move_sphere, multi=True),
    R("rt_multi_set_params", FLUSHES, "another camera", move_camera, move_camera, multi=True),
    R("rt_multi_reset_accumulation", FLUSHES, "called", reset_accumulation, reset_accumulation, multi=True),
    R("rt_multi_render_frame", HOLDS, "a fourth frame: held in every context", c_render_frame, o_render_frame, multi=True),
    R("rt_multi_render_frames", FLUSHES, "four frames behind the three held ones", c_render_frames_4, o_render_frames_4, multi=True),
    R("rt_multi_synchronize", FLUSHES, "called", lambda c: c.tr.synchronize(), multi=True),
    R("rt_gather_accumulated", FLUSHES, "gathered to the host", lambda c: {"image": c.tr.read_accumulated().copy()}, o_gather_accumulated, multi=True),
    R("rt_gather_frame", FLUSHES, "gathered to the host", lambda c: {"image": c.tr.read_frame().copy()}, o_gather_frame, multi=True),
    R("rt_gather_accumulated_to_device", FLUSHES, "gathered into device memory of context 1's GPU", c_gather_to_device(True), o_gather_accumulated,
      prepare=p_gather_target, multi=True),
    R("rt_gather_frame_to_device", FLUSHES, "gathered into device memory of context 1's GPU", c_gather_to_device(False), o_gather_frame,
      prepare=p_gather_target, multi=True),
    R("rt_multi_last_gather_ms", LEAVES, "read", lambda c: {"positive": c.tr.last_gather_ms() >= 0}, multi=True),
    R("rt_multi_peer_access", LEAVES, "read", c_peer_access, multi=True),
    R("rt_multi_get_counters", FLUSHES, "read", c_get_counters, o_get_counters, multi=True),
    R("rt_debug_multi_pending_frames", LEAVES, "read: three with the hook on, none on the eager twin", c_pending, multi=True),
    # ---- include/rt_abi.h: timing, counters, the RCCL gather, test hooks
    R("rt_timer_begin", FLUSHES, "called: the held frames are not part of the timed stretch", lambda c: c.tr.timer_begin()),
    R("rt_timer_end", FLUSHES, "called behind an rt_timer_begin: the held frames are part of the timed stretch", lambda c: c.tr.timer_end(), prepare=p_timer),
    R("rt_enable_stats", FLUSHES, "switched on: the held frames run without statistics, the later ones with", lambda c: c.tr.enable_stats(True)),
    R("rt_reset_counters", FLUSHES, "called: the held frames' counts are gone, the later frames' are there", c_reset_counters, o_reset_counters),
    R("rt_get_counters", FLUSHES, "read", c_get_counters, o_get_counters),
    R("rt_gather_rccl", FLUSHES, "over a one-rank communicator, into device memory (a child process: RCCL stays out of the test process)", c_gather_rccl,
      o_read_accumulated, prepare=p_gather_target, child=True),
    R("rt_debug_intersect", FLUSHES, "32 rays", c_debug_intersect),
    R("rt_debug_math_eval", FLUSHES, "64 values", c_math_eval),
    R("rt_debug_phase_profile", FLUSHES, "read", lambda c: {"profile": c.tr.phase_profile()}),
    R("rt_debug_fused_frames_cap", LEAVES, "read: 16 ... 64 (scheduling: the twin's may differ)", c_fused_cap),
    R("rt_debug_pending_frames", LEAVES, "read: three with the hook on, none on the eager twin", c_pending),
    # ---- the table hooks
    R("rt_debug_primary_table", LEAVES, "read", lambda c: {"on": c.tr.primary_table()}),
    R("rt_debug_tile_cand", LEAVES, "read", lambda c: {"on": c.tr.tile_cand()}),
    R("rt_debug_tile_tri", LEAVES, "read", lambda c: {"on": c.tr.tile_tri()}),
    # ---- include/rt_cost.h, rt_aov.h, rt_motion.h
    R("rt_render_cost", FLUSHES, "frame 2", lambda c: {"cost": c.tr.render_cost(2)}),
    R("rt_render_aov", FLUSHES, "frame 2", lambda c: {"aov": c.tr.render_aov(2)}),
    R("rt_render_aov_to_device", FLUSHES, "frame 2, into device memory", c_aov_to_device),
    R("rt_render_aov_centre", FLUSHES, "read", lambda c: {"aov": c.tr.render_aov_centre()}),
    R("rt_render_aov_centre_to_device", FLUSHES, "into device memory", c_aov_centre_to_device),
    R("rt_reproject_buffers_moving", FLUSHES, "caller-owned images and records with a motion table", c_reproject_buffers_moving, prepare=p_reproject_inputs),
    R("rt_reproject_accumulated_moving", FLUSHES, "the accumulated image, held frames included, reprojected with a motion table", c_reproject_accumulated_moving,
      prepare=p_prev_aov_moving, oracle_final=False),
    # ---- include/rt_denoise.h, rt_reproject.h
    R("rt_denoise_buffers", FLUSHES, "caller-owned image and records", c_denoise_buffers, prepare=p_filter_inputs),
    R("rt_denoise", FLUSHES, "the accumulated image, scale 1/5", lambda c: {"image": c.tr.denoise(c.api.denoise_params(scale=0.2))}),
    R("rt_denoise_to_device", FLUSHES, "the accumulated image into device memory", c_denoise_to_device),
    R("rt_reproject_buffers", FLUSHES, "caller-owned images and records", c_reproject_buffers, prepare=p_reproject_inputs),
    R("rt_reproject_accumulated", FLUSHES, "the accumulated image, held frames included, reprojected into the same view", c_reproject_accumulated,
      prepare=p_prev_aov, oracle_final=False),
    R("rt_resolve_buffers", FLUSHES, "a caller-owned sum", c_resolve_buffers, prepare=p_filter_inputs),
    R("rt_resolve", FLUSHES, "read", lambda c: {"image": c.tr.resolve()}),
    R("rt_resolve_to_device", FLUSHES, "into device memory", c_resolve_to_device),
    # ---- include/rt_variance.h
    R("rt_moments_update_buffers", FLUSHES, "caller-owned sum, snapshot and moments", c_moments_update_buffers, prepare=p_filter_inputs),
    R("rt_denoise_variance_buffers", FLUSHES, "caller-owned image, moments and records", c_denoise_variance_buffers, prepare=p_filter_inputs),
    R("rt_variance_update", FLUSHES, "the batch is the three held frames", c_variance_update, prepare=p_moments),
    R("rt_variance_reset", FLUSHES, "the snapshot includes the held frames: the next batch is the later frames alone", c_variance_reset, o_two_more_frames,
      prepare=p_moments),
    R("rt_variance_carry", FLUSHES, "the moments carried into the same view", c_variance_carry, prepare=p_two_aovs),
    R("rt_variance_read_moments", FLUSHES, "read", lambda c: {"moments": c.tr.read_moments()}, prepare=p_moments),
    R("rt_variance_moments_to_device", FLUSHES, "into device memory", c_moments_to_device, prepare=p_moments),
    R("rt_denoise_variance", FLUSHES, "the accumulated image through the variance-guided filter", lambda c: {"image": c.tr.denoise_variance()}, prepare=p_moments),
    R("rt_denoise_variance_to_device", FLUSHES, "the same into device memory", c_denoise_variance_to_device, prepare=p_moments),
    # ---- include/rt_adaptive.h
    R("rt_adaptive_select_buffers", FLUSHES, "caller-owned sum and moments", c_adaptive_select_buffers, prepare=p_filter_inputs),
    R("rt_adaptive_select", FLUSHES, "the tile errors of the accumulated image, held frames included", c_adaptive_select, prepare=p_moments),
    R("rt_adaptive_set_tiles", FLUSHES, "a list of three tiles", c_adaptive_set_tiles),
    R("rt_adaptive_read_tiles", FLUSHES, "a list of four tiles read back", lambda c: {"tiles": c.tr.adaptive_tiles()}, prepare=p_tile_list),
    R("rt_adaptive_read_tile_error", FLUSHES, "the errors of a selection read back", lambda c: {"errors": c.tr.adaptive_tile_error()}, prepare=p_selection),
    R("rt_adaptive_render_frames", FLUSHES, "two frames of four tiles behind three held full frames: both targets and alpha", c_adaptive_render_frames,
      prepare=p_tile_list, oracle_final=False),
    # ---- include/rt_query.h, rt_radiance.h, rt_nee.h
    R("rt_query_closest", FLUSHES, "96 rays", lambda c: {"hits": c.tr.query_closest(rays(c))}),
    R("rt_query_closest_buffers", FLUSHES, "96 rays in device memory", c_buffers("query_closest_buffers", "rays", "RAYHIT_DTYPE"), prepare=p_ray_buffers(48)),
    R("rt_query_occluded", FLUSHES, "96 rays", lambda c: {"occluded": c.tr.query_occluded(rays(c))}),
    R("rt_query_occluded_buffers", FLUSHES, "96 rays in device memory", c_buffers("query_occluded_buffers", "rays", np.uint32), prepare=p_ray_buffers(4)),
    R("rt_radiance_trace", FLUSHES, "96 rays", lambda c: {"radiance": c.tr.radiance_trace(path_rays(c))}),
    R("rt_radiance_trace_buffers", FLUSHES, "96 rays in device memory", c_buffers("radiance_trace_buffers", "path_rays", "RADIANCE_DTYPE"),
      prepare=p_ray_buffers(16)),
    R("rt_nee_trace", FLUSHES, "96 rays", lambda c: {"radiance": c.tr.radiance_trace_nee(path_rays(c))}),
    R("rt_nee_trace_buffers", FLUSHES, "96 rays in device memory", c_buffers("radiance_trace_nee_buffers", "path_rays", "RADIANCE_DTYPE"),
      prepare=p_ray_buffers(16)),
    R("rt_nee_light_count", FLUSHES, "read", lambda c: {"lights": c.tr.nee_light_count()}),
    # ---- include/rt_mis.h: one function, which takes a call descriptor; its two forms are the descriptor's `memory`
    R("rt_mis_trace", FLUSHES, "96 rays, the host form (memory = RT_MIS_HOST)", lambda c: {"radiance": c.tr.radiance_trace_mis(path_rays(c))}),
    R("rt_mis_trace", FLUSHES, "96 rays in device memory (memory = RT_MIS_DEVICE)", c_buffers("radiance_trace_mis_buffers", "path_rays", "RADIANCE_DTYPE"),
      prepare=p_ray_buffers(16), case="device_form"),
]
