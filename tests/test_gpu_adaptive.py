"""The calls of include/rt_adaptive.h on the GPU.  Every comparison is == on the bit patterns, against the NumPy restatement of the
header's prose in tests/adaptive_reference.py and against the CPU oracle's per-frame images.

  1. rt_adaptive_select_buffers on the hazard images: tile errors, list and counts; inputs unchanged; entries past the count unwritten;
  2. rt_adaptive_render_frames == the oracle's frames added inside the listed tiles only, for BVH, FLAT (pooled), depth-of-field and
     many-model scenes, as one call or three, fused or not; the normal path afterwards is undisturbed;
  3. the counters count the listed pixels' work;  4. the closed loop select / render / variance_update against its simulation;
  5. a partitioned context;  6. state errors, the empty list, a caller's stream and bound render targets;
  7. rounds: rt_ad_list_kernel walks the tile errors 1,024 at a time and carries the count of active tiles from round to round — the
     selection at 1,024 / 1,025 / 1,089 / 4,225 tiles, lists written down by the test around the round boundaries, and a context of
     33 x 33 tiles;
  8. queue: with RT_GRID=5 a list has more items than the launch has waves, so tiles come from the adaptive queue counter through
     tileOrder = the list (asserted from the launches RT_VERBOSE reports), and the counter is handed from launch to launch, also
     between lists of different lengths with normal frames in between;
  9. groups: RT_FRAME_GROUP=2 / 4 over a list on a FLAT scene (groups of 2 + 1, and of 3), pooled and not;
  10. cap: RT_FUSE_CAP=2 splits a call of 3 frames into a fused launch of 2 and a single-frame launch on the same list."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import adaptive_reference as aref
import variance_reference as vref
from gpu_support import DevBuf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SEED = 1


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert not len(bad), f"{what}: {len(bad)} values differ; first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def dev_array(buf, dtype, count):
    out = np.zeros(count, dtype=dtype)
    import ctypes as C
    assert buf.hip.hipMemcpy(C.c_void_p(out.ctypes.data), buf.p, C.c_size_t(out.nbytes), C.c_int(2)) == 0
    return out


# ---------------------------------------------------------------- 1. select on buffers
# (256, 256): 1,024 tiles, one full round and no second; (8193, 1): 1,025 tiles, the second round is one tile of 1 x 1 pixel;
# (257, 263): 33 x 33 tiles, ragged last column and row; (520, 515): 65 x 65 = 4,225 tiles, five rounds, the last one partial
@pytest.mark.parametrize("w,h", [(1, 1), (9, 17), (64, 36), (333, 77), (256, 256), (8193, 1), (257, 263), (520, 515)])
def test_select_buffers_equals_the_numpy_restatement(api, orc, w, h):
    tr = api.create_tracer(0)  # no scene, no rt_resize
    tx, ty = aref.tiles_xy(w, h)
    try:
        for ps in aref.PARAM_SETS:
            s, m, _ = aref.hazard_images(w, h, seed=w + h, **ps)
            _, te, tiles, active, pixels = aref.select(orc, s, m, **ps)
            d_s, d_m = DevBuf.of(s), DevBuf.of(m)
            d_te, d_tiles, d_counts = DevBuf(tx * ty * 4, fill=0xee), DevBuf(tx * ty * 4, fill=0xa5), DevBuf(16, fill=0xff)
            try:
                tr.adaptive_select_buffers(w, h, d_s.ptr, d_m.ptr, d_te.ptr, d_tiles.ptr, d_counts.ptr, api.adaptive_params(**ps))
                tr.synchronize()
                what = f"{w} x {h}, {ps}"
                assert dev_array(d_counts, np.uint32, 4).tolist() == [active, pixels, 0, 0], what
                same_bits(dev_array(d_te, F, tx * ty), te, what + ": tile errors")
                got = dev_array(d_tiles, np.uint32, tx * ty)
                assert got[:active].tolist() == tiles.tolist(), what + ": the list"
                assert (got[active:] == 0xa5a5a5a5).all(), what + ": entries past the count were written"
                assert d_s.image(h, w).tobytes() == s.tobytes() and d_m.image(h, w).tobytes() == m.tobytes(), "an input was written"
            finally:
                for d in (d_s, d_m, d_te, d_tiles, d_counts):
                    d.free()
    finally:
        tr.close()


# ---------------------------------------------------------------- 7. more than one round of rt_ad_list_kernel
ROUNDS_W, ROUNDS_H, ROUNDS_TILES = 520, 515, 4225  # 65 x 65 tiles: rounds of 1,024 start at tiles 0, 1024, 2048, 3072, 4096
ROUNDS_PARAMS = dict(threshold=0.1, darkFloor=0.01, minFrames=4, maxFrames=0)
ROUND_PATTERNS = [("none", []), ("tile_0", [0]), ("tile_1023", [1023]), ("tile_1024", [1024]), ("tiles_1023_1024", [1023, 1024]),
                  ("last_tile", [4224]), ("every_tile", list(range(4225))), ("every_64th", list(range(0, 4225, 64))),
                  ("tiles_960_to_1087", list(range(960, 1088))),
                  ("rounds_1_and_3", list(range(1024, 2048)) + list(range(3072, 4096)))]


@pytest.mark.parametrize("name,planted", ROUND_PATTERNS, ids=[p[0] for p in ROUND_PATTERNS])
def test_list_kernel_across_rounds(api, orc, name, planted):
    """The expected list is the planted one, written down above: the restatement has to agree with it too."""
    w, h = ROUNDS_W, ROUNDS_H
    tx, ty = aref.tiles_xy(w, h)
    assert tx * ty == ROUNDS_TILES and planted == sorted(set(planted)) and all(0 <= t < tx * ty for t in planted)
    s, m = aref.planted_images(w, h, planted)
    pixels = int(aref.tile_pixels(w, h).reshape(-1)[np.asarray(planted, dtype=np.int64)].sum())
    _, te, tiles, active, ref_pixels = aref.select(orc, s, m, **ROUNDS_PARAMS)
    assert tiles.tolist() == planted and (active, ref_pixels) == (len(planted), pixels), "the restatement disagrees with the planted list"
    on = np.zeros(tx * ty, dtype=bool)
    on[np.asarray(planted, dtype=np.int64)] = True
    same_bits(te, np.where(on, F(np.inf), F(0)), "the restatement's tile errors")
    tr = api.create_tracer(0)
    d_s, d_m = DevBuf.of(s), DevBuf.of(m)
    d_te, d_tiles, d_counts = DevBuf(tx * ty * 4, fill=0xee), DevBuf(tx * ty * 4, fill=0xa5), DevBuf(16, fill=0xff)
    try:
        tr.adaptive_select_buffers(w, h, d_s.ptr, d_m.ptr, d_te.ptr, d_tiles.ptr, d_counts.ptr, api.adaptive_params(**ROUNDS_PARAMS))
        tr.synchronize()
        got = dev_array(d_tiles, np.uint32, tx * ty)
        counts = dev_array(d_counts, np.uint32, 4).tolist()
        print(f"{name}: counts {counts}, want {[len(planted), pixels, 0, 0]}")
        assert got[:len(planted)].tolist() == planted, "the list"
        assert counts == [len(planted), pixels, 0, 0]
        assert (got[len(planted):] == 0xa5a5a5a5).all(), "entries past the count were written"
        same_bits(dev_array(d_te, F, tx * ty), te, "tile errors")
    finally:
        for d in (d_s, d_m, d_te, d_tiles, d_counts):
            d.free()
        tr.close()


def test_context_select_over_more_than_one_round(pkg, api, orc):
    """rt_adaptive_select on a rendered image of 33 x 33 = 1,089 tiles: the list kernel's second round, behind the context's own buffers."""
    spec, w, h = BVH, 264, 259
    tx, ty = aref.tiles_xy(w, h)
    assert (tx, ty) == (33, 33)
    tr, mgr = start(pkg, api, spec, w, h)
    try:
        for _ in range(2):
            mgr.RenderFrames(1)
            tr.variance_update()
        acc, m = tr.read_accumulated(), tr.read_moments()
        te = aref.tile_error(aref.pixel_error(orc, acc, m, 0.01, 0, 0))
        ps = dict(threshold=float(np.median(te[np.isfinite(te)])), darkFloor=0.01, minFrames=0, maxFrames=0)
        want = aref.select(orc, acc, m, **ps)
        res = tr.adaptive_select(api.adaptive_params(**ps))
        tiles = tr.adaptive_tiles()
        print(f"threshold {ps['threshold']}: {len(tiles)} tiles, want {want[3]}; {int((want[2] >= 1024).sum())} of them in the second round")
        assert tiles.tolist() == want[2].tolist()
        assert res == {"tiles_total": 1089, "tiles_active": want[3], "pixels_active": want[4]}
        same_bits(tr.adaptive_tile_error().reshape(-1), want[1], "tile errors")
        assert 0 < res["tiles_active"] < 1089
        assert (tiles < 1024).any() and (tiles >= 1024).any(), "the list lies on one side of the round boundary"
        assert tr.read_accumulated().tobytes() == acc.tobytes() and tr.read_moments().tobytes() == m.tobytes()
    finally:
        tr.close()


# ---------------------------------------------------------------- the oracle's frames, once per scene
_FRAMES = {}


def oracle_frames(pkg, orc, spec, w, h, n):
    """FrameRender of frames 1 ... n of the whole image, (h, w, 4) float32 each (alpha 1); computed once and kept."""
    key = (repr(spec), w, h)
    have = _FRAMES.setdefault(key, [])
    if len(have) < n:
        tr = orc.create_tracer(8)
        try:
            cfg, kw = spec
            mgr = pkg.scenes.get(cfg, **kw).make_manager(tr, orc, w, h)
            mgr.OnEnable(renderSeed=SEED)
            out = []
            for _ in range(n):
                mgr.RenderFrame()
                out.append(tr.read_frame().copy())
        finally:
            tr.close()
        _FRAMES[key] = have = out
    for f in have:
        f.setflags(write=False)
    return have[:n]


def start(pkg, api, spec, w, h, stats=False, partition=None):
    tr = api.create_tracer(0)
    if stats:
        tr.enable_stats(True)
    if partition:
        tr.set_partition(*partition)
    cfg, kw = spec
    mgr = pkg.scenes.get(cfg, **kw).make_manager(tr, api, w, h)
    mgr.OnEnable(renderSeed=SEED)
    return tr, mgr


def expected_after(frames, tiles, w, rows, rows_of=None):
    """2 full frames, then frames 3 ... 5 inside the listed tiles: (AccumulatedRender, FrameRender, mask)."""
    fr = [f if rows_of is None else f[rows_of] for f in frames]
    mask = aref.tile_mask(tiles, w, rows)
    acc = aref.add_frames(np.zeros((rows, w, 4), dtype=F), fr[:2])
    acc = aref.add_frames(acc, fr[2:5], mask)
    return acc, np.where(mask[..., None], fr[4], fr[1]).astype(F), mask


BVH, FLAT, POOLED, UNPOOLED = (3, {}), (2, {}), {"RT_POOL_MIN_ITEMS": "0"}, {"RT_POOL": "0"}
# RT_GRID=5: a grid of 5 waves, rounded up to whole workgroups — fewer waves than a list has items, so that items come from the queue.
# A case with RT_VERBOSE asserts that, and how the calls were split into launches, from the launches the library reports.
SMALL_GRID = {"RT_GRID": "5", "RT_VERBOSE": "1"}
SCENES = [("bvh", BVH, 37, 23, {}), ("flat_pooled", FLAT, 96, 54, POOLED),
          ("depth_of_field", (4, {"subdivisions": 3}), 80, 45, {}), ("many_models", (5, {"subdivisions": 2, "n_meshes": 5}), 80, 45, {}),
          ("bvh_small_grid", BVH, 96, 54, SMALL_GRID), ("flat_pooled_small_grid", FLAT, 96, 54, {**POOLED, **SMALL_GRID}),
          # three fused frames in groups of 2: items (tile, frames 0-1) and (tile, frame 2); 4 is clamped to 3, no power of two
          ("flat_pooled_frame_group_2", FLAT, 96, 54, {**POOLED, "RT_FRAME_GROUP": "2"}),
          ("flat_pooled_frame_group_4", FLAT, 96, 54, {**POOLED, "RT_FRAME_GROUP": "4"}),
          ("flat_unpooled_frame_group_2_small_grid", FLAT, 96, 54, {**UNPOOLED, "RT_FRAME_GROUP": "2", **SMALL_GRID}),
          ("flat_unpooled_frame_group_4", FLAT, 96, 54, {**UNPOOLED, "RT_FRAME_GROUP": "4"}),
          # a call of 3 frames = a fused launch of 2 and a single-frame launch, on the same list and queue counter
          ("bvh_fuse_cap_2", BVH, 96, 54, {"RT_FUSE_CAP": "2", "RT_VERBOSE": "1"}),
          ("flat_pooled_fuse_cap_2", FLAT, 96, 54, {**POOLED, "RT_FUSE_CAP": "2", "RT_VERBOSE": "1"})]
_LAUNCH = re.compile(r"adaptive launch variant=\d+ tiles=(\d+) of (\d+) frames=(\d+) grid=(\d+) x (\d+) waves")


def adaptive_launches(capfd):
    """The adaptive launches an RT_VERBOSE context reported since the last call: [(tiles, frames, workgroups, waves per workgroup)]."""
    return [(int(t), int(f), int(g), int(v)) for t, _, f, g, v in _LAUNCH.findall(capfd.readouterr().err)]


def assert_items_exceed_the_waves(launches, n_tiles, what):
    """Every launch has more tiles — and so more (tile, frame group) items, a launch has at least one group — than waves: the waves
    take the first items by index and every other one through the queue and the list."""
    assert launches, what + ": no adaptive launch was reported"
    for tiles, frames, groups, waves in launches:
        assert tiles == n_tiles and tiles > groups * waves, f"{what}: {tiles} tiles, frames={frames}, grid={groups} x {waves} waves"


def launch_frames(calls, fuse, cap):
    """The frames of each launch that rt_adaptive_render_frames(n) for n in calls makes."""
    out = []
    for n in calls:
        while n > 0:
            k = min(n, cap) if fuse else 1
            out.append(k)
            n -= k
    return out


# ---------------------------------------------------------------- 8. the adaptive queue counter between the normal launches' counters
def test_adaptive_queue_survives_interleaving(pkg, api, orc, monkeypatch, capfd):
    """Full frames 1 2, frame 3 on list A, full frame 4, frames 5 6 on list B (the complement of A, of another length), full frame 7:
    with a grid of 5 waves every launch takes items from its queue, the adaptive ones from a counter that the normal ones do not move.
    (In front of the cases below, so that the oracle renders this scene once, with the seven frames this test needs.)"""
    spec, w, h = BVH, 96, 54
    frames = oracle_frames(pkg, orc, spec, w, h, 7)
    tx, ty = aref.tiles_xy(w, h)
    list_a = aref.checkerboard(w, h)
    list_b = np.setdiff1d(np.arange(tx * ty, dtype=np.uint32), list_a).astype(np.uint32)
    assert len(list_a) == 51 and len(list_b) == 33  # 12 x 7 tiles
    mask_a, mask_b = aref.tile_mask(list_a, w, h), aref.tile_mask(list_b, w, h)
    assert (mask_a ^ mask_b).all()
    zero = np.zeros((h, w, 4), dtype=F)
    after_4 = aref.add_frames(aref.add_frames(aref.add_frames(zero, frames[0:2]), frames[2:3], mask_a), frames[3:4])
    after_6 = aref.add_frames(after_4, frames[4:6], mask_b)
    want_acc = aref.add_frames(after_6, frames[6:7])
    for k, v in SMALL_GRID.items():
        monkeypatch.setenv(k, v)
    tr, mgr = start(pkg, api, spec, w, h)
    try:
        mgr.RenderFrames(2)
        before = tr.counters()["pixelFrames"]
        capfd.readouterr()
        tr.adaptive_set_tiles(list_a)
        tr.adaptive_render_frames(1)
        launches_a = adaptive_launches(capfd)
        tr.render_frames(1)
        tr.adaptive_set_tiles(list_b)
        assert tr.adaptive_tiles().tolist() == list_b.tolist()
        capfd.readouterr()
        tr.adaptive_render_frames(2)
        launches_b = adaptive_launches(capfd)
        assert tr.frame() == 7
        same_bits(tr.read_accumulated(), after_6, "AccumulatedRender after list B")
        same_bits(tr.read_frame(), np.where(mask_b[..., None], frames[5], frames[3]).astype(F), "FrameRender after list B")
        tr.render_frames(1)
        assert tr.frame() == 8
        got_acc, got_frame = tr.read_accumulated(), tr.read_frame()
        same_bits(got_acc, want_acc, "AccumulatedRender")
        same_bits(got_frame, frames[6], "FrameRender")
        assert (got_acc[..., 3][mask_a] == 5).all() and (got_acc[..., 3][mask_b] == 6).all()
        assert tr.counters()["pixelFrames"] - before == int(mask_a.sum()) + 2 * int(mask_b.sum()) + 2 * w * h
        assert [l[1] for l in launches_a] == [1] and [l[1] for l in launches_b] == [2]
        assert_items_exceed_the_waves(launches_a, len(list_a), "list A")
        assert_items_exceed_the_waves(launches_b, len(list_b), "list B")
    finally:
        tr.close()


# ---------------------------------------------------------------- 2. render equals the oracle, tile by tile
@pytest.mark.parametrize("name,spec,w,h,env", SCENES, ids=[s[0] for s in SCENES])
def test_adaptive_frames_equal_the_oracle_inside_the_listed_tiles(pkg, api, orc, name, spec, w, h, env, monkeypatch, capfd):
    frames = oracle_frames(pkg, orc, spec, w, h, 6)
    tiles = aref.checkerboard(w, h)
    tx, ty = aref.tiles_xy(w, h)
    assert 0 < len(tiles) < tx * ty and tx * ty - 1 in tiles.tolist() and (w % 8 or h % 8)
    want_acc, want_frame, mask = expected_after(frames, tiles, w, h)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for fuse in (True, False):
        if not fuse:
            monkeypatch.setenv("RT_FUSE_FRAMES", "0")
        for calls in ((3,), (1, 1, 1)):
            what = f"{name}: fused {fuse}, calls {calls}"
            tr, mgr = start(pkg, api, spec, w, h)
            try:
                mgr.RenderFrames(2)
                tr.adaptive_set_tiles(tiles)
                assert tr.adaptive_tiles().tolist() == tiles.tolist()
                capfd.readouterr()
                for n in calls:
                    tr.adaptive_render_frames(n)
                assert tr.frame() == 6, what
                if "RT_VERBOSE" in env:
                    launches = adaptive_launches(capfd)
                    # not pinned, the cap is 16 or more: it splits none of these calls
                    assert [l[1] for l in launches] == launch_frames(calls, fuse, int(env.get("RT_FUSE_CAP", max(calls)))), what
                    if "RT_GRID" in env:
                        assert_items_exceed_the_waves(launches, len(tiles), what)
                same_bits(tr.read_accumulated(), want_acc, what + ": AccumulatedRender")
                same_bits(tr.read_frame(), want_frame, what + ": FrameRender")
                tr.render_frames(1)  # the normal path, undisturbed
                assert tr.frame() == 7
                same_bits(tr.read_accumulated(), aref.add_frames(want_acc, frames[5:6]), what + ": AccumulatedRender after a full frame")
                same_bits(tr.read_frame(), frames[5], what + ": FrameRender after a full frame")
            finally:
                tr.close()
    assert (want_acc[..., 3][mask] == 5).all() and (want_acc[..., 3][~mask] == 2).all()


# ---------------------------------------------------------------- 3. counters
def test_counters_count_the_listed_pixels_alone(pkg, api):
    spec, w, h = (3, {}), 37, 23
    tiles = aref.checkerboard(w, h)
    mask = aref.tile_mask(tiles, w, h)
    tr, mgr = start(pkg, api, spec, w, h, stats=True)
    try:
        mgr.RenderFrames(2)
        before = tr.counters()
        tr.adaptive_set_tiles(tiles)
        tr.adaptive_render_frames(1)
        after = tr.counters()
        cost = tr.render_cost(3)
        assert after["pixelFrames"] - before["pixelFrames"] == int(mask.sum())
        assert after["segments"] - before["segments"] == int(cost[..., 0][mask].astype(np.int64).sum())
        assert 0 < int(cost[..., 0][mask].sum()) < int(cost[..., 0].sum())
    finally:
        tr.close()


# ---------------------------------------------------------------- 4. the closed loop
LOOP = dict(threshold=0.7, darkFloor=0.01, minFrames=8, maxFrames=24)


def simulate_loop(pkg, orc, spec, w, h, ps):
    frames = oracle_frames(pkg, orc, spec, w, h, ps["maxFrames"] + 4)
    acc = snap = m = np.zeros((h, w, 4), dtype=F)
    k = 0
    for _ in range(2):
        acc = aref.add_frames(acc, frames[k:k + 4])
        k += 4
        snap, m = vref.update(orc, acc, snap, m)
    lists = []
    while True:
        tiles = aref.select(orc, acc, m, **ps)[2]
        lists.append(tiles.tolist())
        if not len(tiles) or len(lists) > 16:
            break
        acc = aref.add_frames(acc, frames[k:k + 4], aref.tile_mask(tiles, w, h))
        k += 4
        snap, m = vref.update(orc, acc, snap, m)
    return lists, acc, m


def test_closed_loop_equals_its_simulation(pkg, api, orc):
    spec, w, h = (3, {}), 64, 36
    lists, want_acc, want_m = simulate_loop(pkg, orc, spec, w, h, LOOP)
    tx, ty = aref.tiles_xy(w, h)
    # conditions on the scene and the threshold, met by the simulation: the loop ends in time, and some tile drops out before the cap
    assert lists[-1] == [] and len(lists) <= LOOP["maxFrames"] // 4
    assert want_acc[..., 3].max() <= LOOP["maxFrames"] + 3
    capped_at = (LOOP["maxFrames"] - 8) // 4  # the selection that finds every pixel at the cap
    assert any(0 < len(l) < tx * ty for l in lists[:capped_at]) or len(lists[0]) < tx * ty, "no tile dropped out before the cap"
    assert (want_acc[..., 3] < LOOP["maxFrames"]).any()
    tr, mgr = start(pkg, api, spec, w, h)
    try:
        p = api.adaptive_params(**LOOP)
        for _ in range(2):
            mgr.RenderFrames(4)
            tr.variance_update()
        got = []
        while True:
            res = tr.adaptive_select(p)
            tiles = tr.adaptive_tiles()
            assert res["tiles_total"] == tx * ty and res["tiles_active"] == len(tiles)
            assert res["pixels_active"] == int(aref.tile_mask(tiles, w, h).sum()) if len(tiles) else res["pixels_active"] == 0
            got.append(tiles.tolist())
            assert got[-1] == lists[len(got) - 1], f"selection {len(got)}"
            if not len(tiles):
                break
            tr.adaptive_render_frames(4)
            tr.variance_update()
        assert got == lists
        same_bits(tr.read_accumulated(), want_acc, "the final sum")
        same_bits(tr.read_moments(), want_m, "the final moments")
        te = tr.adaptive_tile_error()
        assert te.shape == (ty, tx) and (te <= F(LOOP["threshold"])).all()
    finally:
        tr.close()


# ---------------------------------------------------------------- 5. a partitioned context
def test_partitioned_context_selects_and_renders_its_own_tiles(pkg, api, orc):
    spec, w, h = (3, {}), 64, 36
    frames = oracle_frames(pkg, orc, spec, w, h, 6)
    tr, mgr = start(pkg, api, spec, w, h, partition=(8, 1, 2))
    try:
        rows_of = tr.local_to_global_rows()
        rows = len(rows_of)
        assert rows == 16 and rows_of.tolist() == list(range(8, 16)) + list(range(24, 32))
        for _ in range(2):
            mgr.RenderFrames(1)
            tr.variance_update()
        acc, m = tr.read_accumulated(), tr.read_moments()
        same_bits(acc, aref.add_frames(np.zeros((rows, w, 4), dtype=F), [f[rows_of] for f in frames[:2]]), "the part's two frames")
        te = aref.tile_error(aref.pixel_error(orc, acc, m, 0.01, 0, 0))
        ps = dict(threshold=float(np.median(te[np.isfinite(te)])), darkFloor=0.01, minFrames=0, maxFrames=0)
        want = aref.select(orc, acc, m, **ps)
        res = tr.adaptive_select(api.adaptive_params(**ps))
        tiles = tr.adaptive_tiles()
        assert tiles.tolist() == want[2].tolist() and 0 < len(tiles) < 16
        assert res == {"tiles_total": 16, "tiles_active": want[3], "pixels_active": want[4]}
        same_bits(tr.adaptive_tile_error().reshape(-1), want[1], "the part's tile errors")
        tr.adaptive_render_frames(3)
        want_acc, want_frame, _ = expected_after(frames, tiles, w, rows, rows_of)
        same_bits(tr.read_accumulated(), want_acc, "the part's AccumulatedRender")
        same_bits(tr.read_frame(), want_frame, "the part's FrameRender")
    finally:
        tr.close()


# ---------------------------------------------------------------- 6. state
def test_state_errors_and_the_empty_list(pkg, api):
    abi = pkg.abi
    spec, w, h = (3, {}), 37, 23
    tr, mgr = start(pkg, api, spec, w, h)
    try:
        def status(fn, *a):
            with pytest.raises(abi.RtError) as e:
                fn(*a)
            return e.value.status
        mgr.RenderFrames(2)
        assert status(tr.adaptive_render_frames, 1) == abi.RT_ERR_STATE            # no list yet
        assert status(tr.adaptive_tiles) == abi.RT_ERR_STATE
        assert status(tr.adaptive_tile_error) == abi.RT_ERR_STATE                  # no select yet
        assert status(tr.adaptive_set_tiles, [3, 1]) == abi.RT_ERR_INVALID_ARG
        assert status(tr.adaptive_set_tiles, [15]) == abi.RT_ERR_INVALID_ARG       # 5 x 3 tiles
        assert status(tr.adaptive_select, api.adaptive_params(threshold=-1.0)) == abi.RT_ERR_INVALID_ARG
        assert status(tr.adaptive_select, api.adaptive_params(struct_size=24)) == abi.RT_ERR_ABI_MISMATCH
        tr.adaptive_set_tiles([0, 14])
        assert status(tr.adaptive_render_frames, -1) == abi.RT_ERR_INVALID_ARG
        # an empty list: the targets keep their bits, the frames still count
        acc, fr = tr.read_accumulated(), tr.read_frame()
        tr.adaptive_set_tiles([])
        assert tr.adaptive_tiles().tolist() == []
        tr.adaptive_render_frames(3)
        assert tr.frame() == 6
        assert tr.read_accumulated().tobytes() == acc.tobytes() and tr.read_frame().tobytes() == fr.tobytes()
        # accumulate == 0
        p = mgr.params()
        p.frame = tr.frame()
        p.accumulate = 0
        tr.set_params(p)
        tr.adaptive_set_tiles([0])
        assert status(tr.adaptive_render_frames, 1) == abi.RT_ERR_STATE
        p.accumulate = 1
        tr.set_params(p)
        tr.adaptive_render_frames(1)
        # rt_resize drops the list and the tile errors
        tr.adaptive_select(api.adaptive_params())
        assert tr.adaptive_tile_error().shape == (3, 5)
        tr.resize(w, h)
        assert status(tr.adaptive_render_frames, 1) == abi.RT_ERR_STATE
        assert status(tr.adaptive_tile_error) == abi.RT_ERR_STATE
    finally:
        tr.close()


_TORCH_CHILD = r"""
import os
import sys
import numpy as np
import torch
torch.cuda.set_device(0)
root, blob = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
import __graft_entry__ as graft
pkg = graft.load_package()
api = pkg.load_library()
z = np.load(blob)
w, h = int(z["w"]), int(z["h"])
tr = api.create_tracer(0)
mgr = pkg.scenes.get(3).make_manager(tr, api, w, h)
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    accum = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
s.synchronize()
mgr.OnEnable(renderSeed=1)
tr.set_stream(s.cuda_stream)
tr.bind_render_targets(frame.data_ptr(), accum.data_ptr())  # (after the manager's rt_resize, which unbinds)
mgr.RenderFrames(2)
tr.adaptive_set_tiles(z["tiles"])
tr.adaptive_render_frames(3)
with torch.cuda.stream(s):
    a, f = accum.clone(), frame.clone()  # in the order of the caller's stream, behind the adaptive frames
s.synchronize()
assert tr.frame() == 6
assert a.cpu().numpy().tobytes() == z["acc"].tobytes(), "AccumulatedRender (bound, on a torch stream)"
assert f.cpu().numpy().tobytes() == z["frame"].tobytes(), "FrameRender (bound, on a torch stream)"
tr.set_stream(None)
tr.close()
print("ADAPTIVE_TORCH_OK")
"""


def test_callers_stream_and_bound_render_targets_give_the_same_bits(pkg, api, orc, tmp_path):
    """In a child process that imports torch first, so that the library shares torch's HIP runtime."""
    spec, w, h = (3, {}), 37, 23
    frames = oracle_frames(pkg, orc, spec, w, h, 6)
    tiles = aref.checkerboard(w, h)
    want_acc, want_frame, _ = expected_after(frames, tiles, w, h)
    blob = str(tmp_path / "expected.npz")
    np.savez(blob, w=w, h=h, tiles=tiles, acc=want_acc, frame=want_frame)
    p = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT, blob], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ADAPTIVE_TORCH_OK" in p.stdout, "rc=%d\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
