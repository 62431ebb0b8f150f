"""rt_render_cost (include/rt_cost.h) on the GPU: the per-pixel work of a frame's rays, counted by the stats build of the
trace kernel, against

  1. the oracle's per-pixel work log (oracle_trace_pixel_schedule), every field of every pixel;
  2. per 8-row strip, the oracle's counters over that row window and the reference text's own `stats` (RC:254 triangle tests,
     RC:271 box tests / 2) compiled as C++ (oracle/_ref, as tests/test_gpu_ref_pin.py loads it);
  3. over a whole 1920x1080 frame, the RtCounters delta of the same frame rendered with stats on;

and checks that the call changes nothing a caller can see (images, frame counter, counters, watchdog word), does not depend on
the device layout or the row partition, and reports its own watchdog without condemning the context's images."""
import importlib.util
import os

import numpy as np
import pytest

from cost_view_support import assert_cost_equal, gpu_cost, manager, oracle_cost, orc_log, scene_of  # noqa: F401  (orc_log: fixture)
from flush_table import held_at

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("segments", "innerSteps", "leafSteps", "triTests")

# ---------------------------------------------------------------- 1. per pixel, every field, against the oracle's work log
PIXEL_CASES = [  # name, scene, W, H, frame, manager tweaks
    ("config1_f1", (1, {}), 64, 36, 1, {}),
    ("config1_f5_spp3", (1, {}), 64, 36, 5, {"numRaysPerPixel": 3}),
    ("config2_f1_spp1", (2, {}), 64, 36, 1, {"numRaysPerPixel": 1}),
    ("config2_f5_nosky", (2, {}), 64, 36, 5, {"useSky": False}),
    ("config3_f1", (3, {}), 64, 36, 1, {}),
    ("config3_f5_spp3", (3, {}), 64, 36, 5, {"numRaysPerPixel": 3}),
    ("config3_lowq_f5", (3, {}), 48, 27, 5, {"bvhQuality": 0}),
    ("config4s3_f1", (4, {"subdivisions": 3}), 64, 36, 1, {}),
    ("config4s3_f5_spp1", (4, {"subdivisions": 3}), 64, 36, 5, {"numRaysPerPixel": 1}),
    ("glassballs_f1", (6, {}), 72, 40, 1, {}),
    ("glassballs_f5_spp3", (6, {}), 72, 40, 5, {"numRaysPerPixel": 3}),
    ("crowded70_f1", "crowded70", 64, 36, 1, {}),
    ("crowded70_f5_spp3_nosky", "crowded70", 64, 36, 5, {"numRaysPerPixel": 3, "useSky": False}),
]


@pytest.mark.parametrize("case", PIXEL_CASES, ids=[c[0] for c in PIXEL_CASES])
def test_every_pixel_equals_the_oracle_work_log(pkg, api, orc_log, case):
    name, spec, w, h, frame, tweak = case
    got = gpu_cost(pkg, api, spec, w, h, frame, tweak)
    want = oracle_cost(pkg, orc_log, spec, w, h, frame, tweak)
    assert_cost_equal(got, want, name)
    assert got[..., 0].min() >= 1  # every pixel traced at least its camera rays
    if spec != (1, {}):  # (config 1 is spheres only)
        assert got[..., 3].sum() > 0 and got[..., 6].sum() > 0
    if spec == (6, {}):
        assert (got[..., 7] == 2).any() and (got[..., 7] == 1).any()  # glass and opaque first hits
    if spec == (2, {}) and tweak.get("useSky", True):
        assert (got[..., 7] == 0).any()  # camera rays that see the sky


# ---------------------------------------------------------------- 2. per 8-row strip, against the oracle's counters and the reference text
_spec = importlib.util.spec_from_file_location("rt_ref_lib", os.path.join(ROOT, "oracle", "ref_lib.py"))
ref_lib = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_lib)


def _checked_ref(pkg, variant, name):
    """As tests/test_gpu_ref_pin.py: absent = skip, built from other inputs than oracle/REF_EXPECTED.json names = fail."""
    lib = ref_lib.load(pkg, variant)
    if lib is None:
        pytest.skip(f"oracle/_ref/{name} did not travel with the snapshot")
    why = ref_lib.stale_reason([name])
    if why:
        pytest.fail("stale reference library: " + why)
    return lib


def window_counters(pkg, lib, builder, spec, w, h, frame, rows, tweak=None, threads=16):
    """Counters of frame `frame` rendered by `lib` (oracle or reference text) over the row window [rows[0], rows[1])."""
    tr = lib.create_tracer(threads)
    try:
        mgr = manager(pkg, builder, tr, spec, w, h, tweak)
        mgr.numAccumulatedFrames = frame
        mgr.SetShaderParams()
        lib.set_row_window(tr.h, rows[0], rows[1])
        tr.reset_counters()
        tr.render_frame()
        return tr.counters()
    finally:
        tr.close()


STRIP_CASES = [  # name, scene, W, H, frame, strips (first rows), tweaks
    ("config2_1080p", (2, {}), 1920, 1080, 2, (0, 536, 1072), {}),
    ("config3_1080p", (3, {}), 1920, 1080, 2, (0, 536, 1072), {}),
    ("config4_1080p", (4, {}), 1920, 1080, 1, (0, 544), {}),
    ("config3_nobvh_48x27", (3, {}), 48, 27, 3, (0, 8, 16, 24), {"bvhQuality": 2}),  # leaves of 255+ triangles: beyond the log's reach
]


@pytest.mark.parametrize("case", STRIP_CASES, ids=[c[0] for c in STRIP_CASES])
def test_row_sums_equal_the_oracle_and_the_reference_text(pkg, api, orc, case):
    name, spec, w, h, frame, strips, tweak = case
    ref = _checked_ref(pkg, "spheres", "libref_spheres.so") if spec[0] == 2 else _checked_ref(pkg, "", "libref.so")
    cost = gpu_cost(pkg, api, spec, w, h, frame, tweak)
    assert cost.shape == (h, w, 8)
    for r0 in strips:
        rows = (r0, min(r0 + 8, h))
        got = cost[rows[0]:rows[1]].reshape(-1, 8).sum(axis=0, dtype=np.uint64)
        want = window_counters(pkg, orc, orc, spec, w, h, frame, rows, tweak)
        for k, key in enumerate(KEYS):
            assert int(got[k]) == want[key], (name, rows, key, int(got[k]), want[key])
        stats = window_counters(pkg, ref, orc, spec, w, h, frame, rows, tweak)  # the reference text has no BVH builder: the oracle's (same bytes)
        assert int(got[3]) == stats["triTests"], (name, rows, "RC:254", int(got[3]), stats)
        assert int(got[1]) == stats["innerSteps"], (name, rows, "RC:271 / 2", int(got[1]), stats)
        assert int(got[0]) == stats["segments"], (name, rows, int(got[0]), stats)


# ---------------------------------------------------------------- 3. the whole image against the stats kernel
@pytest.mark.parametrize("cfg", [2, 3])
def test_image_sum_equals_the_stats_frame(pkg, api, cfg):
    tr = api.create_tracer(0)
    try:
        tr.enable_stats(True)
        mgr = manager(pkg, api, tr, (cfg, {}), 1920, 1080, seed=7)
        tr.reset_counters()
        cost = tr.render_cost(1)
        c0 = tr.counters()
        assert all(c0[k] == 0 for k in KEYS) and c0["pixelFrames"] == 0  # the cost launch added nothing to the context's counters
        mgr.RenderFrame()  # frame 1
        c1 = tr.counters()
        total = cost.reshape(-1, 8).sum(axis=0, dtype=np.uint64)
        for k, key in enumerate(KEYS):
            assert int(total[k]) == c1[key], (cfg, key, int(total[k]), c1[key])
        assert c1["pixelFrames"] == 1920 * 1080
    finally:
        tr.close()


# ---------------------------------------------------------------- 4. no side effects
def test_cost_calls_leave_no_trace(pkg, api, orc, forced=False):
    cfg, w, h, seed = (3, {}), 96, 54, 5
    snaps = []
    costs = {}
    for with_cost in (True, False):
        tr = api.create_tracer(0)
        tr.enable_stats(True)
        mgr = manager(pkg, api, tr, cfg, w, h, seed=seed)

        def probe(tag):
            if with_cost:
                if tag.startswith("after held"):
                    held_at(tr, "test_gpu_cost_view: rt_render_cost after held-back frames", forced)
                a = tr.render_cost(tr.frame())  # the frame the context renders next
                assert np.array_equal(a, tr.render_cost(tr.frame())), tag  # the same frame twice: the same work
                costs[tr.frame()] = a
                first = tr.render_cost(1)
                assert np.array_equal(first, costs.setdefault(1, first)), tag  # and frame 1 whenever it is asked for
        mgr.RenderFrame()                       # frame 1
        probe("after rt_render_frame")
        mgr.RenderFrames(17)                    # frames 2-18: a fused launch, still running when the cost call comes
        probe("after rt_render_frames(17)")
        for _ in range(3):                      # frames 19-21: rt_render_frame may hold them back (pending)
            mgr.RenderFrame()
        probe("after held-back frames")
        mgr.RenderFrames(14)                    # frames 22-35: past the tile re-sort at 32 recorded frames
        probe("across a tile re-sort")
        snaps.append((tr.read_accumulated(), tr.read_frame(), tr.frame(), tr.counters()))
        tr.close()
    (acc_a, frame_a, n_a, c_a), (acc_b, frame_b, n_b, c_b) = snaps
    assert acc_a.tobytes() == acc_b.tobytes() and frame_a.tobytes() == frame_b.tobytes()
    assert n_a == n_b == 36 and c_a == c_b
    assert sorted(costs) == [1, 2, 19, 22, 36]
    assert all(c[..., 0].min() >= 1 for c in costs.values())
    ot = orc.create_tracer(16)
    manager(pkg, orc, ot, cfg, w, h, seed=seed).RenderFrames(35)
    acc_o = ot.read_accumulated()
    ot.close()
    assert acc_a.view(np.uint32).tobytes() == acc_o.view(np.uint32).tobytes(), "accumulated image != oracle"


def test_cost_calls_leave_no_trace_with_frames_held_back_for_certain(pkg, api, orc, monkeypatch):
    """The same with RT_HOLD_BACK=1: frames 19-21 ARE held back when the cost pass comes (asserted right before it)."""
    monkeypatch.setenv("RT_HOLD_BACK", "1")
    test_cost_calls_leave_no_trace(pkg, api, orc, forced=True)


# ---------------------------------------------------------------- 5. layout and partition independence
def test_layout_does_not_change_the_cost(pkg, api, monkeypatch):
    out = []
    for layout in ("dense", "pre,arena,cache"):
        monkeypatch.setenv("RT_LAYOUT", layout)  # read at rt_create
        out.append(gpu_cost(pkg, api, (3, {}), 96, 54, 3))
        monkeypatch.delenv("RT_LAYOUT")
    assert_cost_equal(out[0], out[1], "RT_LAYOUT dense vs pre,arena,cache")


@pytest.mark.parametrize("spec", [(3, {}), (2, {})], ids=["bvh", "flat"])
def test_partitions_and_multi_context_reassemble_the_image(pkg, api, spec):
    w, h, frame = 80, 45, 2
    full = gpu_cost(pkg, api, spec, w, h, frame)
    parts = 3
    seen = np.zeros(h, dtype=int)
    for i in range(parts):
        tr = api.create_tracer(0)
        tr.set_partition(8, i, parts)
        manager(pkg, api, tr, spec, w, h)
        local = tr.render_cost(frame)
        rows = tr.local_to_global_rows()
        assert local.shape == (len(rows), w, 8)
        assert_cost_equal(local, full[rows], f"partition {i} of {parts}")
        seen[rows] += 1
        tr.close()
    assert (seen == 1).all()
    mt = api.create_multi_tracer([0, 0, 0])
    try:
        manager(pkg, api, mt, spec, w, h)
        assert_cost_equal(mt.render_cost(frame), full, "MultiTracer.render_cost")
    finally:
        mt.close()


# ---------------------------------------------------------------- 6. errors and the watchdog
def test_errors(pkg, api):
    abi = pkg.abi
    tr = api.create_tracer(0)
    try:
        buf = np.zeros((36, 64, 8), dtype=np.uint32)
        assert api.render_cost(tr.h, 1, buf.ctypes.data, buf.nbytes) == abi.RT_ERR_STATE  # before rt_resize
        tr.resize(64, 36)
        assert api.render_cost(tr.h, 1, buf.ctypes.data, buf.nbytes) == abi.RT_ERR_STATE  # before rt_upload_scene
        manager(pkg, api, tr, (3, {}), 64, 36)
        assert api.render_cost(tr.h, 1, buf.ctypes.data, buf.nbytes - 32) == abi.RT_ERR_INVALID_ARG
        assert api.render_cost(tr.h, 1, buf.ctypes.data, buf.nbytes + 32) == abi.RT_ERR_INVALID_ARG
        assert api.render_cost(tr.h, 1, None, buf.nbytes) == abi.RT_ERR_INVALID_ARG
        assert api.render_cost(tr.h, 0, buf.ctypes.data, buf.nbytes) == abi.RT_ERR_INVALID_ARG
        assert api.render_cost(tr.h, -3, buf.ctypes.data, buf.nbytes) == abi.RT_ERR_INVALID_ARG
        assert api.render_cost(tr.h, 1, buf.ctypes.data, buf.nbytes) == abi.RT_OK and buf[..., 0].min() >= 1
    finally:
        tr.close()
    tr = api.create_tracer(0)
    try:
        tr.resize(64, 36)
        mgr = scene_of(pkg, (3, {})).make_manager(tr, api, 64, 36)
        mgr.InitTexturesAndBuffers()
        mgr.InitBVH()  # a scene, but no rt_set_params yet
        assert api.render_cost(tr.h, 1, buf.ctypes.data, buf.nbytes) == abi.RT_ERR_STATE
    finally:
        tr.close()


def test_watchdog_fails_the_call_not_the_context(pkg, api, monkeypatch):
    """RT_TRAV_LIMIT=4 (read at rt_upload_scene; the step limit is a software counter, nothing can hang): the cost launch's
    walks are cut short, the call says so — and the context's counters and images, which no frame of it touched, stay readable."""
    tr = api.create_tracer(0)
    try:
        monkeypatch.setenv("RT_TRAV_LIMIT", "4")
        manager(pkg, api, tr, (3, {}), 64, 36)
        monkeypatch.delenv("RT_TRAV_LIMIT")
        with pytest.raises(pkg.abi.RtError) as e:
            tr.render_cost(1)
        assert e.value.status == pkg.abi.RT_ERR_HIP and "watchdog" in str(e.value), str(e.value)
        c = tr.counters()  # RT_OK: the context's watchdog word was not set
        assert c["segments"] == 0
        assert not tr.read_accumulated().any()
        assert tr.frame() == 1
    finally:
        tr.close()
