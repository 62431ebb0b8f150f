"""The kernels for more than 64 models at every end of their candidate mask: the catalogue of tests/many_models.py on the GPU.
tests/test_many_models.py has checked, without a GPU, that the oracle equals the reference text on every scene, that the witness
plates and the all-candidates ray are there, that no expected image holds a NaN, and what rt_launch_plan.h plans for the LDS extreme.
Here the device renders each scene and must equal the oracle, every comparison bit for bit:

  a. crowd<n> for every n of N_EDGES, the shipped and the STATS instantiation: both render targets after a single-frame launch and after a
     fused launch of two, segments and pixelFrames, in STATS all seven counters with modelVisits == segments * n and no filter violation;
     at 1,087 and 1,300 models also as single waves (RT_HOT_KB=0), with RT_WAVES_PER_GROUP=1 and under RT_LAYOUT=pre,arena,cache.  The
     launch reports name the variants and the workgroups rt_launch_plan.h plans: 10 and 11 up to 127 models, 4 and 5 from 1,086 on (32
     extension rows leave these scenes no room for a cache; the comb scenes of (d) are the ones with 32 rows AND a cache).  (A context whose watchdog fired fails every
     pixel read and rt_get_counters: the reads succeeding is that assertion.)
  b. the staircase in both orders: the same, rt_render_aov's object per pixel against the oracle's first hit with every WITNESS index
     among them, and a whole wave of the all-candidates ray through rt_query_closest and rt_debug_intersect;
  c. always1300: models the filter cannot reject on both sides of every boundary;
  d. the height-32 comb beside 1,086 and 1,299 models, first and last: 32 stack entries under 32 extension words, launched as the one
     group of 9 waves around a 24-record cache that the CPU half computed; rt_render_cost and rt_render_aov on the same scenes;
  e. the side passes on crowd1300 and the staircase: rt_render_cost, rt_render_aov and its centre form, the ray queries with tmax at, above
     and below the hit, rt_radiance_trace, and rt_nee_trace with emitters on either side of the mask's boundaries; rt_mis_trace on the same
     scenes and on crowd96 and crowd1087, at maxBounceCount 1, 2 and 5: its bounce row lies behind 1, 2 and 32 extension words, its reverse
     lookup takes object indices up to 1,299;
  f. one context through rt_update_models steps on the staircase and through uploads of 1,300, 1,087, 64 and 1,300 models;
  g. flat1300: the FLAT kernel with 1,300 models."""
import ctypes as C
import time

import numpy as np
import pytest

import aov_support as ta
import cost_view_support as tc
import hazard_scenes as hz
import many_models as mm
import mis_reference as mr
import motion_reference as mref
import nee_reference as nr
import radiance_reference as rr
import query_support as tq
from cost_view_support import orc_log  # noqa: F401  (fixture)
from deep_trees import launches
from gpu_support import KEYS
from launch_plan_support import one, plan  # noqa: F401  (plan: the fixture that builds tests/launch_plan_driver.cpp)

pytestmark = pytest.mark.gpu
F = np.float32
MANY_VARIANTS = (4, 5, 10, 11)
ENVS = [("default", {}), ("single waves", {"RT_HOT_KB": "0"}), ("groups of one", {"RT_WAVES_PER_GROUP": "1"}), ("cache layout", {"RT_LAYOUT": "pre,arena,cache"})]


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def device(api, sc, stats):
    """mm.drive on a fresh context -> its images, counters, and in STATS the filter audit and the cache's count"""
    tr = api.create_tracer(0)
    try:
        tr.enable_stats(stats)
        single, fused, c = mm.drive(sc, tr)
        prof = tr.phase_profile() if stats else None
    finally:
        tr.close()
    return dict(single=single, fused=fused, c=c, viol=prof["filter_violations"][0] if stats else 0, hot=prof["inner_from_lds_cache"][0] if stats else None)


def assert_equals_oracle(got, want, what, stats, n):
    for part, g, o in (("a single frame", got["single"], want[0]), ("then 2 fused frames", got["fused"], want[1])):
        assert same(g[0], o[0]), f"{what}, {part}: AccumulatedRender differs from the oracle's in {int((g[0] != o[0]).any(axis=-1).sum())} pixels"
        assert same(g[1], o[1]), f"{what}, {part}: FrameRender differs from the oracle's in {int((g[1] != o[1]).any(axis=-1).sum())} pixels"
    c, oc = got["c"], want[2]
    assert (c["segments"], c["pixelFrames"]) == (oc["segments"], oc["pixelFrames"]), (what, c, oc)
    if stats:
        assert [c[k] for k in KEYS] == [oc[k] for k in KEYS], (what, c, oc)
        assert c["modelVisits"] == c["segments"] * n and got["viol"] == 0, (what, c, got["viol"])


def render_both(pkg, api, orc, name, monkeypatch, capfd, env=None):
    """the shipped and the STATS instantiation of a catalogue scene against the oracle -> the launch shapes either reported"""
    sc, want = mm.scene(pkg, api, name), mm.expected(pkg, orc, name)
    monkeypatch.setenv("RT_DEBUG_LAUNCH", "1")
    for k in ("RT_HOT_KB", "RT_WAVES_PER_GROUP", "RT_LAYOUT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    reports = {}
    for stats in (False, True):
        capfd.readouterr()
        got = device(api, sc, stats)
        reports[stats] = launches(capfd)
        assert_equals_oracle(got, want, f"{name} ({env or 'default'}, {'STATS' if stats else 'shipped'})", stats, sc.n)
        reports["hot"] = got["hot"]
    return sc, reports


def assert_many_shapes(sc, reports, what, stack=None):
    """every launch ran a > 64-model instantiation of the right build, with the LDS rt_launch_plan.h's arithmetic gives: a cache of
    `records` x 64 B and per wave (stack + 4 pixel fields + summary + extension words + bounce row) x 256 B"""
    ext = (min(sc.n, mm.FILTER_CAP) - 63 + 31) // 32
    for stats in (False, True):
        assert reports[stats], (what, "no launch was reported")
        for variant, entries, lds, threads, records in reports[stats]:
            assert variant in MANY_VARIANTS and (variant & 1) == int(stats), (what, reports)
            assert (variant >= 10) == (records > 0) and (threads > 64) <= (records > 0), (what, reports)
            assert lds == records * 64 + (threads // 64) * (entries + 4 + 2 + ext) * 256 and lds <= 160 * 1024, (what, reports)
            assert stack is None or entries == stack, (what, reports)
    return {r[0] for s in (False, True) for r in reports[s]}


def assert_planned(plan, sc, reports, what, want=12, hotkb=None):  # noqa: F811
    """the workgroups reported are rt_launch_plan.h's for the scene's tree height and model count (tests/launch_plan_driver.cpp): its
    waves per group; a cache exactly where it plans one, of at most the records it plans (a scene's trees may have fewer), and used"""
    shapes = {(r[1], r[3] // 64, r[4]) for s in (False, True) for r in reports[s]}   # (stack entries, waves per group, cache records)
    assert len(shapes) == 1, (what, reports)
    (entries, waves, records), = shapes
    g = one(plan, "groups", height=entries, models=sc.n, want=want, **({} if hotkb is None else {"hotkb": hotkb}))
    assert waves == g["wpg"] and (records > 0) == (g["records"] > 0) and records <= g["records"], (what, shapes, g)
    assert (reports["hot"] > 0) == (records > 0), (what, reports["hot"], records)
    return entries, waves, records


# ---------------------------------------------------------------- a. counts
@pytest.mark.parametrize("n", mm.N_EDGES)
def test_crowd_at_every_end_of_the_mask(pkg, api, orc, plan, n, monkeypatch, capfd):  # noqa: F811
    """The workgroup shape is rt_launch_plan.h's for the scene's tree height and model count: at 94 ... 127 models these scenes leave room
    for a top-of-tree cache (variants 10 and 11); with their 32 extension rows a wave's region leaves no whole groups with room to
    spare, and the default launch is single waves like the one RT_HOT_KB=0 asks for (variants 4 and 5).  The comb scenes below are the
    ones with 32 extension rows AND a cache."""
    name = f"crowd{n}"
    mm.expected(pkg, orc, name)   # (the oracle's render, on the CPU: not part of the time printed below)
    t0 = time.perf_counter()
    seen = {}
    for shape, env in ENVS if n in (1087, 1300) else ENVS[:1]:
        sc, reports = render_both(pkg, api, orc, name, monkeypatch, capfd, env)
        seen[shape] = assert_many_shapes(sc, reports, f"{name}, {shape}")
        assert_planned(plan, sc, reports, f"{name}, {shape}", want=1 if shape == "groups of one" else 12, hotkb=0 if shape == "single waves" else None)
        if shape == "single waves":
            assert seen[shape] == {4, 5}, (name, seen)
        if shape == "default" and n <= 127:
            assert seen[shape] == {10, 11}, (name, seen)
    print(f"{name}: variants per shape {seen}; {time.perf_counter() - t0:.2f} s on the device side")


# ---------------------------------------------------------------- b. witnesses
def _stairs_first_hits(pkg, orc, sc, ot, origins, dirs):
    """(H, W) plate index per ray from oracle_ray_collision's depth, -1 = a miss"""
    hits = tq.oracle_hits(orc, ot, origins.reshape(-1, 3), dirs.reshape(-1, 3))
    return np.where(hits[:, 0] != 0, mm.plate_of_depth(sc.order, hits[:, 8].astype(np.float64), sc.n), -1).reshape(origins.shape[:2]), hits


@pytest.mark.parametrize("order", ["near_first", "near_last"])
def test_staircase_witnesses(pkg, api, orc, plan, order, monkeypatch, capfd):  # noqa: F811
    name = f"stairs-{order}"
    sc, reports = render_both(pkg, api, orc, name, monkeypatch, capfd)
    assert_many_shapes(sc, reports, name)
    assert_planned(plan, sc, reports, name)
    tr, ot = api.create_tracer(0), orc.create_tracer(1)
    try:
        sc.upload(tr), sc.upload(ot)
        # ---- rt_render_aov_centre against the pixel-centre first hits the CPU half counted, rt_render_aov of frame 2 against its own rays'
        centre = tr.render_aov_centre()
        first = mm.first_hit_models(pkg, orc, sc)
        assert np.array_equal(centre["object"], first), f"{name}: rt_render_aov_centre: object differs in {int((centre['object'] != first).sum())} pixels"
        assert set(mm.WITNESS) <= set(np.unique(centre["object"]).tolist())
        p = sc.params(2)
        tr.set_params(p)
        aov = tr.render_aov(2)
        origins, dirs = ta.camera_rays(orc, p, sc.w, sc.h, 2)
        want, _ = _stairs_first_hits(pkg, orc, sc, ot, origins, dirs)
        assert np.array_equal(aov["object"], want), f"{name}: rt_render_aov: object differs in {int((aov['object'] != want).sum())} pixels"
        assert set(mm.WITNESS) <= set(np.unique(aov["object"]).tolist())
        # ---- a whole wave of the ray that has every candidate: every lane with every word full
        o, d = mm.pixel_centre_rays(sc)
        o64 = np.tile(o[mm.W_PIXEL[1], mm.W_PIXEL[0]], (64, 1))
        d64 = np.tile(d[mm.W_PIXEL[1], mm.W_PIXEL[0]], (64, 1))
        hits10 = tq.oracle_hits(orc, ot, o64[:1], d64[:1])
        assert hits10[0, 0] != 0 and mm.plate_of_depth(order, float(hits10[0, 8]), sc.n) == (0 if order == "near_first" else sc.n - 1)
        got = tr.query_closest(pkg.abi.make_rays(o64, d64))
        tq.assert_same_records(got, tq.records_from_oracle(pkg, None, np.tile(hits10, (64, 1)), got["object"], got["triangle"]), f"{name}: 64 x the all-candidates ray")
        assert (got["object"] == (0 if order == "near_first" else sc.n - 1)).all() and len({r.tobytes() for r in got}) == 1
        dbg = tr.debug_intersect(o64, d64)
        assert same(np.ascontiguousarray(dbg[:, :9]), np.tile(hits10[:, :9], (64, 1))), f"{name}: rt_debug_intersect on the all-candidates ray"
    finally:
        tr.close(), ot.close()


# ---------------------------------------------------------------- c. models the filter cannot reject
def test_unfilterable_models_on_both_sides_of_every_boundary(pkg, api, orc, plan, monkeypatch, capfd):  # noqa: F811
    sc, reports = render_both(pkg, api, orc, "always1300", monkeypatch, capfd)
    assert_many_shapes(sc, reports, "always1300")
    assert_planned(plan, sc, reports, "always1300")
    want, plain = mm.expected(pkg, orc, "always1300"), mm.expected(pkg, orc, "crowd1300")
    assert not same(want[1][0], plain[1][0]), "the planted models change the image"


# ---------------------------------------------------------------- d. the LDS extreme
def _side_contexts(pkg, api, orc, sc, models=None):
    tr, ot = api.create_tracer(0), orc.create_tracer(1)
    sc.upload(tr, models), sc.upload(ot, models)
    return tr, ot


def cost_of_log(log):
    """tests/cost_view_support.py::cost_of_log without the per-token loop, for logs of a million tokens.  The log's payload bytes (an
    inner step's depth, a leaf's depth and count) may equal a tag in general; where every one of them is below 'A' (65) — checked: the
    bytes below 65 must be exactly the one behind each 'B' and the two behind each 'C' — the tags are the bytes from 65 up and the fields
    are sums over masks.  Otherwise the loop does it."""
    a = np.frombuffer(log, dtype=np.uint8)
    is_b, is_c = a == ord("B"), a == ord("C")
    ib, ic = np.flatnonzero(is_b), np.flatnonzero(is_c)
    expect = np.zeros(len(a) + 2, dtype=bool)
    expect[ib + 1] = True
    expect[ic + 1] = True
    expect[ic + 2] = True
    if expect[len(a):].any() or not np.array_equal(expect[:len(a)], a < 65):
        return tc.cost_of_log(log)
    is_s, is_r = a == ord("S"), a == ord("R")
    ray = np.cumsum(is_r) - 1
    seg = np.cumsum(is_s)
    before_ray = np.concatenate([[0], seg])[np.flatnonzero(is_r)] if is_r.any() else np.zeros(0, dtype=np.int64)
    primary = (ray >= 0) & (seg - before_ray[np.maximum(ray, 0)] == 1)
    counts = a[ic + 1].astype(np.int64)
    f = [int(is_s.sum()), len(ib), len(ic), int(counts.sum()), int(primary[ib].sum()), int(primary[ic].sum()), int(counts[primary[ic]].sum()), 0]
    outcome = np.flatnonzero(((a == ord("K")) | (a == ord("O")) | (a == ord("G"))) & primary & (ray == 0))
    if len(outcome):
        f[7] = {ord("K"): 0, ord("O"): 1, ord("G"): 2}[int(a[outcome[0]])]
    return f, bool((counts == 255).any())


def assert_cost_view(pkg, tr, ot, orc_log, sc, frame, what):  # noqa: F811
    p = sc.params(frame)
    tr.set_params(p), ot.set_params(p)
    got = tr.render_cost(frame)
    buf = (C.c_uint8 * (1 << 22))()
    want = np.zeros((sc.h, sc.w, 8), dtype=np.uint32)
    for y in range(sc.h):
        for x in range(sc.w):
            n = orc_log.trace_pixel_schedule(ot.h, x, y, frame, buf, len(buf))
            assert 0 < n <= len(buf)
            log = bytes(buf[:n])
            f, capped = cost_of_log(log)
            assert not capped
            if (y * sc.w + x) % 211 == 0:   # the loop of tests/test_gpu_cost_view.py on a few pixels: the two readings of a log agree
                assert (f, capped) == tc.cost_of_log(log), (what, x, y)
            want[y, x] = f
    tc.assert_cost_equal(got, want, what)
    assert want[..., 0].sum() >= sc.w * sc.h
    return want


def assert_aov(pkg, orc, tr, ot, sc, which, frame, what):
    """every field of every pixel: tests/test_gpu_aov.py's records from the oracle's functions; the triangle inside its model's range"""
    p = sc.params(frame)
    tr.set_params(p), ot.set_params(p)
    if which == "rt_render_aov":
        aov = tr.render_aov(frame)
        origins, dirs = ta.camera_rays(orc, p, sc.w, sc.h, frame)
    else:
        aov = tr.render_aov_centre()
        origins, dirs = mref.centre_rays(orc, p, sc.w, sc.h)
    assert aov.shape == (sc.h, sc.w) and aov.dtype == pkg.abi.AOV_DTYPE
    want = ta.oracle_records(pkg, orc, ot, sc, p, origins, dirs, aov["object"])
    want["triangle"] = aov["triangle"]   # (checked below)
    ta.assert_records_equal(aov, want, f"{what}: {which}")
    hit = (aov["hit"] & 3) != 0
    assert np.array_equal(aov["object"] >= 0, hit) and np.array_equal(aov["triangle"] >= 0, hit) and hit.any()
    off = sc.models["triOffset"][np.maximum(aov["object"], 0)].astype(np.int64)
    assert ((aov["triangle"] >= off) & (aov["triangle"] < off + sc.tri_count[np.maximum(aov["object"], 0)]))[hit].all(), what
    return aov


@pytest.mark.parametrize("name", mm.COMB_SCENES)
def test_the_largest_lds_region_a_wave_can_have(pkg, api, orc, orc_log, name, monkeypatch, capfd):  # noqa: F811
    sc, reports = render_both(pkg, api, orc, name, monkeypatch, capfd)
    assert assert_many_shapes(sc, reports, name, stack=32) == {10, 11}
    waves, records, lds = mm.EXTREME_GROUP
    for stats in (False, True):
        assert {(r[2], r[3], r[4]) for r in reports[stats]} == {(lds, 64 * waves, records)}, (name, reports)
    assert reports["hot"] > 0, "the report says a cache is in use"
    # the same region as single waves (no cache)
    sc, single = render_both(pkg, api, orc, name, monkeypatch, capfd, {"RT_HOT_KB": "0"})
    assert assert_many_shapes(sc, single, name + ", single waves", stack=32) == {4, 5}
    assert {(r[2], r[3]) for s in (False, True) for r in single[s]} == {(17920, 64)}, (name, single)
    # the single-wave passes on the same scene
    for k in ("RT_HOT_KB", "RT_DEBUG_LAUNCH"):
        monkeypatch.delenv(k, raising=False)
    tr, ot = _side_contexts(pkg, api, orc_log, sc)
    try:
        cost = assert_cost_view(pkg, tr, ot, orc_log, sc, 2, f"{name}: rt_render_cost")
        comb = 0 if "first" in name else sc.n - 1
        aov = assert_aov(pkg, orc, tr, ot, sc, "rt_render_aov", 2, name)
        assert (aov["object"] == comb).any(), "the comb is seen"
        assert cost[..., 4].max() >= 32, "a camera ray takes 32 inner steps down the comb at the least"
    finally:
        tr.close(), ot.close()


# ---------------------------------------------------------------- e. side passes
SIDE_SCENES = ["crowd1300", "stairs-near_first", "stairs-near_last"]


@pytest.mark.parametrize("name", SIDE_SCENES)
def test_cost_view_with_a_tail(pkg, api, orc_log, name):  # noqa: F811
    sc = mm.scene(pkg, api, name)
    tr, ot = _side_contexts(pkg, api, orc_log, sc)
    try:
        t0 = time.perf_counter()
        assert_cost_view(pkg, tr, ot, orc_log, sc, 1, f"{name}: rt_render_cost")
        print(f"{name}: rt_render_cost of {sc.w * sc.h} pixels, {time.perf_counter() - t0:.1f} s with the oracle's logs")
    finally:
        tr.close(), ot.close()


@pytest.mark.parametrize("name", SIDE_SCENES)
def test_aov_passes_with_a_tail(pkg, api, orc, name):
    sc = mm.scene(pkg, api, name)
    tr, ot = _side_contexts(pkg, api, orc, sc)
    try:
        for which in ("rt_render_aov", "rt_render_aov_centre"):
            aov = assert_aov(pkg, orc, tr, ot, sc, which, 3, name)
            assert (aov["object"] >= mm.FILTER_CAP).any(), f"{name}: {which}: a model of the unfiltered tail is seen"
            assert ((aov["object"] >= 63) & (aov["object"] < mm.FILTER_CAP)).any() and ((aov["object"] >= 0) & (aov["object"] < 63)).any()
    finally:
        tr.close(), ot.close()


def witness_rays(pkg, orc, sc):
    """one ray per pixel centre, and for a staircase rays from a second origin aimed at a point of each WITNESS plate's own ring"""
    o, d = mm.pixel_centre_rays(sc)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    if sc.order is None:
        return o, d, 0
    first = mm.first_hit_models(pkg, orc, sc)
    origin = np.array([0.4, -0.3, 0.0], dtype=np.float64)
    extra_o, extra_d = [], []
    for w in mm.WITNESS:
        for y, x in np.argwhere(first == w)[:3]:
            z = mm.plate_depth(sc.order, w, sc.n) - mm.THICK / 2
            tx, ty = mm.pixel_tangent(float(x), float(y))
            v = np.array([tx * z, ty * z, z]) - origin
            extra_o.append(origin), extra_d.append(v / np.linalg.norm(v))
    return np.concatenate([o, np.array(extra_o, dtype=F)]), np.concatenate([d, np.array(extra_d, dtype=F)]), len(extra_o)


@pytest.mark.parametrize("name", SIDE_SCENES)
def test_ray_queries_with_a_tail(pkg, api, orc, name):
    """rt_query_closest and rt_debug_intersect against oracle_ray_collision; rt_query_occluded at tmax = +inf (any hit), at the ray's own
    hit distance d (the comparison is strict: 0), one ulp above it (1 where there is a hit) and d / 2 (0: nothing lies before the
    closest hit).  An any-hit walk may stop early; it must not stop before the tail, where the only hit below tmax may be."""
    abi = pkg.abi
    sc = mm.scene(pkg, api, name)
    tr, ot = _side_contexts(pkg, api, orc, sc)
    try:
        o, d, n_aimed = witness_rays(pkg, orc, sc)
        hits10 = tq.oracle_hits(orc, ot, o, d)
        hit = hits10[:, 0] != 0
        got = tr.query_closest(abi.make_rays(o, d))
        tq.assert_same_records(got, tq.records_from_oracle(pkg, None, hits10, got["object"], got["triangle"]), name)
        assert np.array_equal(got["object"] >= 0, hit) and not got["reserved"].any()
        if sc.order is not None:
            plates = mm.plate_of_depth(sc.order, hits10[:, 8].astype(np.float64), sc.n)
            assert np.array_equal(got["object"][hit], plates[hit]), f"{name}: rt_query_closest names another plate than the hit's depth"
            assert set(mm.WITNESS) <= set(got["object"][len(o) - n_aimed:].tolist()), "the aimed rays reach every witness plate"
        assert (got["object"] >= mm.FILTER_CAP).any() and ((got["object"] >= 63) & (got["object"] < mm.FILTER_CAP)).any()
        dbg = tr.debug_intersect(o, d)
        ok = dbg.view(np.uint32) == hits10.view(np.uint32)
        ok[~hit, 3:] = True   # (a miss: didHit, isBackface and dst are the contract)
        assert ok.all(), f"{name}: rt_debug_intersect: {int((~ok.all(axis=1)).sum())} rays differ from oracle_ray_collision"
        dst = hits10[:, 2]
        with np.errstate(all="ignore"):
            cases = (("+inf", np.full(len(o), np.inf, dtype=F)), ("d", dst), ("one ulp above d", np.nextafter(dst, F(np.inf))), ("d / 2", (dst / F(2)).astype(F)))
            for tname, tmax in cases:
                occ = tr.query_occluded(abi.make_rays(o, d, tmax))
                expect = (hit & (dst < tmax)).astype(np.uint32)
                assert np.array_equal(occ, expect), f"{name}: rt_query_occluded at tmax = {tname}: {int((occ != expect).sum())} rays differ"
                if tname in ("+inf", "one ulp above d"):
                    assert np.array_equal(occ != 0, hit)
                else:
                    assert not occ.any()
        print(f"{name}: {int(hit.sum())} of {len(hit)} rays hit, {int((got['object'] >= mm.FILTER_CAP).sum())} of them a model of the tail")
    finally:
        tr.close(), ot.close()


@pytest.mark.parametrize("name", SIDE_SCENES)
def test_radiance_with_a_tail(pkg, api, orc, name):
    """rt_radiance_trace of (camera ray 0 of frame 2, the generator state behind its two draws), one ray per pixel at one ray per pixel
    in the parameters, in order and reversed: oracle_trace_pixel of that frame"""
    abi = pkg.abi
    sc = mm.scene(pkg, api, name)
    tr, ot = _side_contexts(pkg, api, orc, sc)
    try:
        p = sc.params(2, numRaysPerPixel=1)
        tr.set_params(p), ot.set_params(p)
        o, d, state = rr.camera_rays(orc, p, sc.w, sc.h, frame=2)
        rays = abi.make_path_rays(o.reshape(-1, 3), d.reshape(-1, 3), state.ravel())
        want = rr.oracle_pixels(orc, ot, sc.w, sc.h, 2).reshape(-1, 3)
        assert np.isfinite(want).all() and want.any()
        for what, order in (("in order", slice(None)), ("reversed", slice(None, None, -1))):
            got = tr.radiance_trace(rays[order])
            bad = np.argwhere((rr.bits(got["rgb"]) != rr.bits(want[order])).any(axis=1)).ravel()
            assert not len(bad), f"{name}, rt_radiance_trace {what}: {len(bad)} of {len(rays)} rays differ from oracle_trace_pixel"
    finally:
        tr.close(), ot.close()


@pytest.mark.parametrize("name", SIDE_SCENES)
def test_nee_with_emitters_on_either_side_of_the_boundaries(pkg, api, orc, name):
    """the emissive material on models 62, 63, 1086, 1087 and n - 1: rt_debug_light_table against the numpy table of
    tests/nee_reference.py, rt_nee_light_count, and rt_nee_trace on every other pixel's camera ray against the restated estimator"""
    abi = pkg.abi
    sc = mm.scene(pkg, api, name)
    models = mm.with_emitters(sc)
    tr = api.create_tracer(0)
    try:
        sc.upload(tr, models)
        want = nr.light_table(abi, models, sc.triangles, sc.spheres)
        got = api.light_table_arrays(models, sc.triangles, sc.spheres)
        assert got["entries"].tobytes() == want["entries"].tobytes() and got["cdf"].tobytes() == want["cdf"].tobytes(), name
        counts = (want["n_sphere_entries"], want["n_triangle_entries"])
        assert counts[0] == 0 and (got["n_sphere_entries"], got["n_triangle_entries"]) == counts and tr.nee_light_count() == counts, name
        assert all(want["in_table"][i] for i in mm.EMITTERS), "every planted emitter is in the table"
        p = sc.params(2, numRaysPerPixel=1)
        tr.set_params(p)
        o, d, state = rr.camera_rays(orc, p, sc.w, sc.h, frame=2)
        rays = abi.make_path_rays(o.reshape(-1, 3), d.reshape(-1, 3), state.ravel())[::2]
        est = nr.Estimator(pkg, orc, tr, models, sc.triangles, sc.spheres, p)
        expect = est.trace(rays)
        out = tr.radiance_trace_nee(rays)
        ok = (rr.bits(out["rgb"]) == rr.bits(expect["rgb"])).all(axis=1) & (out["rng"] == expect["rng"])
        print(f"{name}: lights {counts}, {est.samples} samples, {est.shadow_rays} shadow rays, {est.unshadowed} unshadowed")
        assert np.isfinite(expect["rgb"]).all() and expect["rgb"].any() and est.shadow_rays > 0
        assert ok.all(), f"{name}: rt_nee_trace: {int((~ok).sum())} of {len(ok)} rays differ from the restated estimator"
    finally:
        tr.close()


MIS_SCENES = SIDE_SCENES + ["crowd96", "crowd1087"]   # crowd96: the step from 1 to 2 extension words; crowd1087: the cap, 32 words
MIS_BOUNCES = (1, 2, 5)                               # (5: the catalogue's own)
MIS_STRIDE = {}                                       # every other pixel's camera ray, as the NEE test's; a coarser stride per scene if need be


def mis_emitters(sc):
    """EMITTERS where the scene has them all, otherwise those of 62, 63, 1086 and n - 1 that exist"""
    return mm.EMITTERS if sc.n > max(mm.EMITTERS) else tuple(sorted({i for i in (62, 63, 1086) if i < sc.n} | {sc.n - 1}))


def gap_rays(sc, k=16):
    """A staircase's plates face the camera: a camera path's lobe ray leaves a plate's front towards the camera and meets no emitter's
    front.  So k rays from inside the 2 mm gap between plates 1086 and 1087 — both planted emitters, both WITNESS plates, neighbours in
    depth in either order — at the front of the farther one, 2 % off grazing, around the plates' common centre (the ray of W_PIXEL): the
    vertex there samples, and its lobe ray crosses the gap to the BACK of the nearer plate, an emitter at or above index 1,086 (the
    rounded cube is closed, its back an outward face).  From the plate geometry of tests/many_models.py alone.
    -> (origins, directions, the nearer plate, the farther plate)"""
    near, far = sorted((1086, 1087), key=lambda i: mm.plate_depth(sc.order, i, sc.n))
    z_back, z_front = mm.plate_depth(sc.order, near, sc.n) + mm.THICK / 2, mm.plate_depth(sc.order, far, sc.n) - mm.THICK / 2
    assert 0.0015 < z_front - z_back < 0.0025
    tx, ty = mm.pixel_tangent(*mm.W_PIXEL)
    o, d = [], []
    for j in range(k):
        target = np.array([tx * z_front + 0.01 * (j % 4 - 1.5), ty * z_front + 0.01 * (j // 4 - 1.5), z_front])
        origin = target + np.array([0.04, 0.03, -(z_front - z_back) / 2])
        v = target - origin
        o.append(origin), d.append(v / np.linalg.norm(v))
    return np.array(o, dtype=F), np.array(d, dtype=F), near, far


@pytest.mark.parametrize("bounce", MIS_BOUNCES)
@pytest.mark.parametrize("name", MIS_SCENES)
def test_mis_with_emitters_on_either_side_of_the_boundaries(pkg, api, orc, name, bounce, monkeypatch, capfd):
    """The emissive material on models 62, 63, 1086, 1087 and n - 1 (those the scene has): rt_debug_light_table and rt_debug_light_map
    against the numpy table and map, and rt_mis_trace on every other pixel's camera ray (on a staircase also gap_rays) against
    tests/mis_reference.py bit for bit, at maxBounceCount 1, 2 and 5.  In the > 64-model instantiation the kernel takes "does this vertex
    sample" from the LDS row behind the extension words (1 at 65 ... 95 models, 2 at 96, 32 from 1,087 on), which every walk's
    begin_intersect clears up to — a row too low and the count is 0 at every vertex, so the last vertex samples: the logs say that no
    vertex at maxBounceCount did.  The reverse lookup takes the hit object: an emission weighted on an object of the extension words
    and, on the staircases, on a planted emitter of the last word or the unfiltered tail."""
    abi = pkg.abi
    t0 = time.perf_counter()
    sc = mm.scene(pkg, api, name)
    planted = mis_emitters(sc)
    models = mm.with_emitters(sc, planted)
    objects, words, table = mr.map_arrays(abi, models, sc.triangles, sc.spheres)
    got_table, got_map = api.light_table_arrays(models, sc.triangles, sc.spheres), api.light_map_arrays(models, sc.triangles, sc.spheres)
    assert got_table["entries"].tobytes() == table["entries"].tobytes() and got_table["cdf"].tobytes() == table["cdf"].tobytes(), name
    assert got_map["objects"].tobytes() == objects.tobytes() and got_map["triangles"].tobytes() == words.tobytes() and got_map["n_entries"] == len(table["entries"]), name
    assert all(table["in_table"][i] and objects[i] != mr.NO_ENTRY for i in planted), "every planted emitter is in the table and in the map"
    monkeypatch.setenv("RT_DEBUG_LAUNCH", "1")
    tr = api.create_tracer(0)
    try:
        sc.upload(tr, models)
        # which instantiation: the side passes report no launch shape, and take theirs by the rule the frame launch takes its own by
        # (rt_plan::many_models of the context's chunk count; tests/test_launch_plan.py holds the rule) — so a frame's report says it
        capfd.readouterr()
        tr.render_frame()
        tr.synchronize()
        variants = {r[0] for r in launches(capfd)}
        monkeypatch.delenv("RT_DEBUG_LAUNCH")
        assert variants and variants <= set(MANY_VARIANTS), f"{name}: the context launches variants {variants}"
        p = sc.params(2, numRaysPerPixel=1, maxBounceCount=bounce)
        tr.set_params(p)
        o, d, state = rr.camera_rays(orc, p, sc.w, sc.h, frame=2)
        rays = abi.make_path_rays(o.reshape(-1, 3), d.reshape(-1, 3), state.ravel())[::MIS_STRIDE.get(name, 2)]
        n_gap, near = 0, None
        if sc.order is not None:
            go, gd, near, _ = gap_rays(sc)
            n_gap = len(go)
            rays = np.concatenate([rays, abi.make_path_rays(go, gd, 4000 + 977 * np.arange(n_gap))])
        est = mr.Estimator(pkg, orc, tr, models, sc.triangles, sc.spheres, p)
        expect = est.trace(rays)
        t_ref = time.perf_counter() - t0
        out, plain = tr.radiance_trace_mis(rays), tr.radiance_trace(rays)
    finally:
        tr.close()
    ok = (rr.bits(out["rgb"]) == rr.bits(expect["rgb"])).all(axis=1) & (out["rng"] == expect["rng"])
    assert len(est.emission_hits) == len(est.emission_log)
    mr.rules_allowed(est, f"{name} bounce={bounce}")
    weighted_on = sorted({obj for (obj, _), e in zip(est.emission_hits, est.emission_log) if e[3] == mr.WEIGHTED})
    rules = {r: sum(1 for e in est.emission_log if e[3] == r) for r in sorted({e[3] for e in est.emission_log})}
    sampled, skipped = sorted({v for (_, v, *_r) in est.sample_log}), sorted({v for (_, v) in est.skipped_log})
    reached = [i for i in weighted_on if i in planted and i >= 1086]
    print(f"{name} bounce={bounce}: {len(rays)} rays ({n_gap} into the gap), lights ({table['n_sphere_entries']}, {table['n_triangle_entries']}), {est.samples} samples, "
          f"{est.shadow_rays} shadow rays, {est.unshadowed} unshadowed; sampled at vertices {sampled}, skipped at {skipped} ({len(est.skipped_log)}); emissions behind a sample {rules}; "
          f"weighted on {len(weighted_on)} objects, {sum(1 for i in weighted_on if i >= 64)} of them >= 64, {sum(1 for i in weighted_on if i >= mm.FILTER_CAP)} in the tail, "
          f"planted emitters >= 1086 among them {reached}; reference {t_ref:.1f} s, all {time.perf_counter() - t0:.1f} s")
    assert all(v < bounce for (_, v, *_r) in est.sample_log) and all(v == bounce for (_, v) in est.skipped_log), (sampled, skipped)
    if bounce == 2:
        assert {0, 1} <= set(sampled), sampled
    if bounce <= 2:   # (at 5, crowd96's few paths are all over before their sixth vertex)
        assert est.skipped_log, "no path reached its last vertex: the decision was never taken"
    assert est.shadow_rays > 0 and len(est.sample_log) > 0
    assert np.isfinite(expect["rgb"]).all() and expect["rgb"].any()
    assert ok.all(), f"{name}: rt_mis_trace at maxBounceCount {bounce}: {int((~ok).sum())} of {len(ok)} rays differ from the restated estimator; first is ray {int(np.argmin(ok))}"
    assert out.tobytes() != plain.tobytes(), "the records are rt_radiance_trace's: nothing was sampled"
    if name in SIDE_SCENES:
        assert any(i >= 64 for i in weighted_on), f"{name}: no weighted emission on an object at or above index 64"
    if near is not None:   # the gap rays: a planted emitter of the last extension word / the first of the tail, hit from a sampled vertex
        assert near in weighted_on, f"{name}: no weighted emission on plate {near}, the nearer of 1086 and 1087"


# ---------------------------------------------------------------- f. one context through changes
def _records_of(pkg, models, index, transform):
    models[index]["localToWorld"] = pkg.manager.matrix_to_abi(transform.localToWorldMatrix)
    models[index]["worldToLocal"] = pkg.manager.matrix_to_abi(transform.worldToLocalMatrix)


def _update_steps(pkg, sc):
    """(name, model records) per rt_update_models step on stairs-near_first"""
    base = sc.models.copy()
    front = base.copy()       # a plate of the unfiltered tail in front of everything, larger than the nearest witness
    _records_of(pkg, front, 1200, mm.plate_transform(pkg, 3.5, (7.0, 5.0)))
    gone = front.copy()       # the last filtered plate (a witness: the nearest surface of a ring) far out of view
    _records_of(pkg, gone, 1086, mm.plate_transform(pkg, mm.plate_depth(sc.order, 1086, sc.n), mm.plate_half_size(sc.order, 1086, sc.n), (4000.0, 16.0)))
    singular = gone.copy()    # a witness plate flattened: the filter cannot reject it any more
    singular[63]["localToWorld"], singular[63]["worldToLocal"] = hz.matrix_pair(hz._from_abi(base[63]["localToWorld"]), "singular")
    return [("plate 1200 in front", front), ("plate 1086 out of view", gone), ("plate 63 singular", singular), ("plate 63 back", gone.copy()),
            ("the same bytes again", gone.copy())]


def _through_changes(pkg, lib, tr, stats=False):
    """the update steps on the staircase, then uploads of 1,300, 1,087, 64 and 1,300 models, a single frame and a fused launch of two after
    each -> [(step, [(acc, frame), (acc, frame)], segments so far)]"""
    sc = mm.scene(pkg, lib, "stairs-near_first")
    tr.enable_stats(stats) if stats else None
    sc.upload(tr)
    tr.reset_counters()
    out, frame = [], 1
    for step, models in [("start", sc.models)] + _update_steps(pkg, sc):
        tr.update_models(models)
        out.append((step, mm.render_steps(sc, tr, frame), tr.counters()))
        frame += 3
    for name in ("crowd1300", "crowd1087", "crowd64", "crowd1300"):
        sc = mm.scene(pkg, lib, name)
        sc.upload(tr)
        out.append((f"upload of {name}", mm.render_steps(sc, tr, frame), tr.counters()))
        frame += 3
    return out


def test_one_context_through_updates_and_uploads(pkg, api, orc, monkeypatch, capfd):
    """rt_update_models rebuilds the filter boxes and the chunks (a tail plate becomes the nearest surface, a filtered one leaves the view,
    one becomes unfilterable and regular again, one update changes nothing), then the same context goes from 1,300 models to 1,087 (no
    tail), to 64 (not the > 64-model kernel) and back: the wave region, the extension rows and the bounce row move under a live context."""
    ot = orc.create_tracer(8)
    try:
        want = _through_changes(pkg, orc, ot)
    finally:
        ot.close()
    images = [w[1][1][0] for w in want]
    assert not same(images[0], images[1]) and not same(images[1], images[2]), "the moved plates change the image"
    monkeypatch.setenv("RT_DEBUG_LAUNCH", "1")
    for stats in (False, True):
        capfd.readouterr()
        tr = api.create_tracer(0)
        try:
            got = _through_changes(pkg, api, tr, stats)
            viol = tr.phase_profile()["filter_violations"][0] if stats else 0
        finally:
            tr.close()
        variants = [r[0] for r in launches(capfd)]
        for (step, g, c), (_, w, oc) in zip(got, want):
            what = f"{step} ({'STATS' if stats else 'shipped'})"
            for part, (ga, gf), (wa, wf) in zip(("single frame", "fused launch"), g, w):
                assert same(ga, wa), f"{what}, {part}: AccumulatedRender differs from the oracle's in {int((ga != wa).any(axis=-1).sum())} pixels"
                assert same(gf, wf), f"{what}, {part}: FrameRender differs from the oracle's in {int((gf != wf).any(axis=-1).sum())} pixels"
            assert (c["segments"], c["pixelFrames"]) == (oc["segments"], oc["pixelFrames"]), (what, c, oc)
            if stats:
                assert [c[k] for k in KEYS] == [oc[k] for k in KEYS], (what, c, oc)
        assert viol == 0
        # a > 64-model instantiation first, and (64 models) a plain BVH one in between; a shape the context has launched before is
        # not reported again
        many, plain = {4 + int(stats), 10 + int(stats)}, {int(stats), 6 + int(stats)}
        assert variants and variants[0] in many and set(variants) - many and set(variants) - many <= plain, variants


# ---------------------------------------------------------------- g. the FLAT kernel with 1,300 models
def test_flat_kernel_with_1300_models(pkg, api, orc, monkeypatch, capfd):
    sc, reports = render_both(pkg, api, orc, "flat1300", monkeypatch, capfd)
    for stats in (False, True):
        assert reports[stats] and all(r[0] in (2 + int(stats), 8 + int(stats)) for r in reports[stats]), reports
