"""The calls of include/rt_adaptive.h on the GPU.  Every comparison is == on the bit patterns, against the NumPy restatement of the
header's prose in tests/adaptive_reference.py and against the CPU oracle's per-frame images.

  1. rt_adaptive_select_buffers on the hazard images: tile errors, list and counts; inputs unchanged; entries past the count unwritten;
  2. rt_adaptive_render_frames == the oracle's frames added inside the listed tiles only, for BVH, FLAT (pooled), depth-of-field and
     many-model scenes, as one call or three, fused or not; the normal path afterwards is undisturbed;
  3. the counters count the listed pixels' work;  4. the closed loop select / render / variance_update against its simulation;
  5. a partitioned context;  6. state errors, the empty list, a caller's stream and bound render targets."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_reference as aref
import variance_reference as vref
from test_gpu_denoise import DevBuf

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
@pytest.mark.parametrize("w,h", [(1, 1), (9, 17), (64, 36), (333, 77)])
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


SCENES = [("bvh", (3, {}), 37, 23, {}), ("flat_pooled", (2, {}), 96, 54, {"RT_POOL_MIN_ITEMS": "0"}),
          ("depth_of_field", (4, {"subdivisions": 3}), 80, 45, {}), ("many_models", (5, {"subdivisions": 2, "n_meshes": 5}), 80, 45, {})]


# ---------------------------------------------------------------- 2. render equals the oracle, tile by tile
@pytest.mark.parametrize("name,spec,w,h,env", SCENES, ids=[s[0] for s in SCENES])
def test_adaptive_frames_equal_the_oracle_inside_the_listed_tiles(pkg, api, orc, name, spec, w, h, env, monkeypatch):
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
                for n in calls:
                    tr.adaptive_render_frames(n)
                assert tr.frame() == 6, what
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
