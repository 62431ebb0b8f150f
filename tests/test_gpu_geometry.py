"""Image geometries the rest of the suite does not reach, HIP kernels against the oracle and the reference text, bit for bit.

A. Whole images narrower or shorter than one 8 x 8 tile, down to 1 x 1.  At W == 1 or H == 1 the uv of RCC:15 is 0 / 0 = NaN
   for every pixel (the kernel's `x * rcp(W - 1)`), so every primary ray has a NaN focus point and direction: the device box
   test, the packed two-sphere pre-test and the float -> uint pixel coordinate all see NaN in whole wavefronts.
B. Strip partitions with any `strip_rows` (rt_set_partition accepts every positive multiple of 8), ragged last strips,
   strips taller than the image and parts that own no rows: reads, display, checkpoint write and counters per part.
C. A context whose partition owns no rows: every call succeeds and does nothing, and the context can be moved onto rows.
D. rt_create_multi with more contexts than the image has strips.
E. One context through a series of geometries: what rt_resize / rt_set_partition must resize or invalidate (tile costs and
   order, staging slabs, pixel records, display scratch, occupancy cache) is exercised at every step.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import render
from gpu_support import KEYS, bits_equal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

ref_lib = graft._ref_lib()
SEED = 5
FLAT, BVH, MANY = (2, {}), (3, {}), (5, {"subdivisions": 3, "n_meshes": 12})


def _ref_or_none(pkg, variant, name):
    """The reference text, or None where it did not travel (only the ref-text leg is left out); a stale one fails."""
    lib = ref_lib.load(pkg, variant)
    if lib is None:
        return None
    why = ref_lib.stale_reason([name])
    if why:
        pytest.fail("stale reference library: " + why)
    return lib


@pytest.fixture(scope="module")
def refs(pkg):
    return {"": _ref_or_none(pkg, "", "libref.so"), "spheres": _ref_or_none(pkg, "spheres", "libref_spheres.so")}


def assert_image(got, want, what):
    """Bit for bit.  Where the expected image holds NaN, the NaN positions are compared and the other values bit for bit
    (a NaN's sign and payload are not part of the contract)."""
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    nan = np.isnan(want)
    if nan.any():
        assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ (the expected image has {int(nan.sum())} NaN values)"
        assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), \
            f"{what}: non-NaN values differ (NaN positions, {int(nan.sum())} values, are equal)"
        return
    bad = np.any(got.view(np.uint32) != want.view(np.uint32), axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at (row, col) {tuple(int(i) for i in np.argwhere(bad)[0])}"


def drive(pkg, lib, tr, cfg, kw, w, h, fused, builder=None):
    """Two single-frame renders, then one rt_render_frames(fused); (acc, frame) after each part, and the counters."""
    sc = pkg.scenes.get(cfg, **kw)
    mgr = sc.make_manager(tr, builder or lib, w, h)
    mgr.OnEnable(renderSeed=SEED)
    mgr.RenderFrame()
    mgr.RenderFrame()
    single = (tr.read_accumulated().copy(), tr.read_frame().copy())
    mgr.RenderFrames(fused)
    out = (single, (tr.read_accumulated().copy(), tr.read_frame().copy()), tr.counters(), tr.frame())
    tr.close()
    return out


_oracle_cache = {}


def oracle_whole(pkg, orc, cfg, kw, w, h, fused):
    key = (cfg, tuple(sorted(kw.items())), w, h, fused)
    if key not in _oracle_cache:
        _oracle_cache[key] = drive(pkg, orc, orc.create_tracer(8), cfg, kw, w, h, fused)
    return _oracle_cache[key]


def check_whole(pkg, api, orc, refs, cfg, kw, w, h, fused=3, with_ref=True):
    """Shipped and STATS kernel instantiations against the oracle (images after both parts of `drive`, exact counters) and,
    where it travelled, against the reference text (images, segments, triangle tests, inner steps)."""
    name = f"config {cfg} {w}x{h}"
    want = oracle_whole(pkg, orc, cfg, kw, w, h, fused)
    (ws, wf, wc, wn) = want
    got = [drive(pkg, api, api.create_tracer(0), cfg, kw, w, h, fused)]
    st = api.create_tracer(0)
    st.enable_stats(True)
    got.append(drive(pkg, api, st, cfg, kw, w, h, fused))
    for which, (gs, gf, gc, gn) in zip(("shipped", "stats"), got):
        for part, g, o in (("two single frames", gs, ws), (f"then {fused} fused frames", gf, wf)):
            assert_image(g[0], o[0], f"{name} {which}, {part}: AccumulatedRender != oracle")
            assert_image(g[1], o[1], f"{name} {which}, {part}: FrameRender != oracle")
        assert gn == wn
        assert (gc["segments"], gc["pixelFrames"]) == (wc["segments"], wc["pixelFrames"]), (name, which, gc, wc)
    assert [got[1][2][k] for k in KEYS] == [wc[k] for k in KEYS], (name, got[1][2], wc)
    assert wc["pixelFrames"] == w * h * (2 + fused)
    lib = refs["spheres" if pkg.scenes.get(cfg, **kw).spheres else ""] if with_ref else None
    if lib is not None:
        rs, rf, rc, _ = drive(pkg, lib, lib.create_tracer(8), cfg, kw, w, h, fused, builder=orc)  # (BVH.cs is not shader text)
        for which, (gs, gf, gc, gn) in zip(("shipped", "stats"), got):
            for part, g, o in (("two single frames", gs, rs), (f"then {fused} fused frames", gf, rf)):
                assert_image(g[0], o[0], f"{name} {which}, {part}: AccumulatedRender != reference text")
                assert_image(g[1], o[1], f"{name} {which}, {part}: FrameRender != reference text")
        assert got[0][2]["segments"] == got[1][2]["segments"] == rc["segments"]
        assert got[1][2]["triTests"] == rc["triTests"] and got[1][2]["innerSteps"] == rc["innerSteps"], (name, got[1][2], rc)
    return want


# ------------------------------------------------------------------------------------------------ A. degenerate shapes
SHAPES = [(1, 1), (1, 13), (13, 1), (2, 2), (3, 300), (300, 3), (7, 9), (8, 8), (9, 7), (17, 1), (127, 61)]
SCENES = [("flat", FLAT), ("bvh", BVH), ("many", MANY)]


@pytest.mark.parametrize("scene", SCENES, ids=[s[0] for s in SCENES])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_degenerate_and_sub_tile_images(pkg, api, orc, refs, scene, shape):
    (cfg, kw), (w, h) = scene[1], shape
    want = check_whole(pkg, api, orc, refs, cfg, kw, w, h)
    if w == 1 or h == 1:  # every primary ray is NaN (uv = 0 / 0): they all end in the sky / the dark, never in NaN
        assert np.all(np.isfinite(want[1][0]))


@pytest.mark.parametrize("shape", [(1, 13), (13, 1)], ids=["1x13", "13x1"])
def test_depth_of_field_on_a_nan_focus_point(pkg, api, orc, refs, shape):
    """config 4 (DefocusStrength 100): the literal defocus jitter of RC:565-568 around a NaN focus point"""
    check_whole(pkg, api, orc, refs, 4, {"subdivisions": 3}, *shape)


TINY = [(1, 1), (1, 13), (13, 1), (2, 2), (7, 9)]
ENVS = [{"RT_POOL_MIN_ITEMS": "0"}, {"RT_TWO_STREAMS": "0"}, {"RT_TWO_STREAMS": "1"},
        {"RT_POOL_MIN_ITEMS": "0", "RT_TWO_STREAMS": "0"}]


@pytest.mark.parametrize("env", ENVS, ids=lambda e: ",".join(f"{k[3:]}={v}" for k, v in e.items()))
def test_tiny_flat_images_pooled_and_on_one_or_two_streams(pkg, api, orc, refs, env, monkeypatch):
    """RT_POOL_MIN_ITEMS=0: a chain pool (a workgroup of waves handing pixel chains to each other) with fewer pixels than one
    wave; RT_TWO_STREAMS: the fused launch on the side stream or on the main one."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for w, h in TINY:
        check_whole(pkg, api, orc, refs, *FLAT, w, h, with_ref=False)


def test_one_pixel_for_more_frames_than_one_fused_launch_holds(pkg, api, orc):
    """rt_render_frames(150) at 1 x 1 goes out as several fused launches (at most RT_FUSE_MAX = 64 frames each)."""
    frames = 150
    probe = api.create_tracer(0)
    cap = probe.fused_frames_cap()
    probe.close()
    assert 0 < cap <= 64 < frames
    out = []
    for lib, tr in ((api, api.create_tracer(0)), (orc, orc.create_tracer(1))):
        mgr = pkg.scenes.get(*FLAT[:1], **FLAT[1]).make_manager(tr, lib, 1, 1)
        mgr.OnEnable(renderSeed=SEED)
        mgr.RenderFrames(frames)
        out.append((tr.read_accumulated(), tr.read_frame(), tr.counters(), tr.frame()))
        tr.close()
    (a, f, c, n), (b, fb, cb, nb) = out
    assert_image(a, b, "1x1, 150 frames: AccumulatedRender")
    assert_image(f, fb, "1x1, 150 frames: FrameRender")
    assert n == nb == frames + 1 and a[0, 0, 3] == frames
    assert (c["segments"], c["pixelFrames"]) == (cb["segments"], cb["pixelFrames"]) and c["pixelFrames"] == frames


# ------------------------------------------------------------------------------------------------ B. strip partitions
# (W, H, strip_rows, part_count)
PARTITIONS = [
    (61, 57, 16, 2),     # 4 strips, the last one ragged (9 rows)
    (61, 57, 24, 3),     # 3 strips, ragged last (9 rows), one per part
    (9, 130, 24, 5),     # 6 strips, ragged last (10 rows): part 0 owns two
    (9, 130, 136, 2),    # strip_rows > H: part 1 owns no rows
    (61, 23, 8, 7),      # 3 strips, ragged last: parts 3..6 own no rows
    (1, 57, 16, 3),      # one column
    (61, 1, 8, 2),       # one row: part 1 owns nothing
    (9, 7, 64, 3),       # strip_rows > H, parts 1 and 2 empty
    (61, 130, 64, 2),    # 3 strips: 64 / 64 / 2 rows, part 0 owns the ragged one
    (9, 57, 8, 5),       # 8 strips, ragged last (1 row)
    (1, 23, 24, 1),      # one strip taller than the image, one part
    (61, 130, 16, 7),    # 9 strips over 7 parts
]
PARTITION_SCENES = [("flat", FLAT, {}), ("flat_pooled", FLAT, {"RT_POOL_MIN_ITEMS": "0"}), ("bvh", BVH, {})]


def oracle_continued(pkg, orc, cfg, kw, w, h):
    """The oracle's whole image after 2 frames (acc, frame, display, srgb8) and after 2 more, and its counters."""
    key = ("continued", cfg, tuple(sorted(kw.items())), w, h)
    if key not in _oracle_cache:
        tr = orc.create_tracer(8)
        mgr = pkg.scenes.get(cfg, **kw).make_manager(tr, orc, w, h)
        mgr.OnEnable(renderSeed=SEED)
        mgr.RenderFrames(2)
        first = (tr.read_accumulated().copy(), tr.read_frame().copy(), tr.display(2).copy(), tr.display_srgb8(2, flip_y=False).copy())
        mgr.RenderFrames(2)
        _oracle_cache[key] = (first, (tr.read_accumulated().copy(), tr.read_frame().copy()), tr.counters())
        tr.close()
    return _oracle_cache[key]


@pytest.mark.parametrize("scene", PARTITION_SCENES, ids=[s[0] for s in PARTITION_SCENES])
def test_strip_partitions_of_any_height(pkg, api, orc, scene, monkeypatch):
    _, (cfg, kw), env = scene
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for (w, h, strip, parts) in PARTITIONS:
        (acc2, fr2, disp2, srgb2), (acc4, fr4), wc = oracle_continued(pkg, orc, cfg, kw, w, h)
        seg = pf = 0
        owned = []
        for p in range(parts):
            name = f"config {cfg} {w}x{h} strip_rows {strip}, part {p} of {parts}"
            rows = pkg.dist.global_rows_of(p, parts, h, strip)
            owned.extend(rows.tolist())
            tr = api.create_tracer(0)
            tr.set_partition(strip, p, parts)
            mgr = pkg.scenes.get(cfg, **kw).make_manager(tr, api, w, h)
            mgr.OnEnable(renderSeed=SEED)
            mgr.RenderFrames(2)
            assert tr.local_rows() == len(rows), name
            assert np.array_equal(tr.local_to_global_rows(), rows), name
            assert_image(tr.read_accumulated(), acc2[rows], f"{name}: AccumulatedRender")
            assert_image(tr.read_frame(), fr2[rows], f"{name}: FrameRender")
            assert_image(tr.display(2), disp2[rows], f"{name}: display")
            s8 = tr.display_srgb8(2, flip_y=False)
            assert np.array_equal(s8, srgb2[rows]), f"{name}: display_srgb8(flip_y=False)"
            # flip_y flips the LOCAL rows (row 0 = bottom of this part's packed tile), not the global image
            assert np.array_equal(tr.display_srgb8(2, flip_y=True), s8[::-1]), f"{name}: display_srgb8(flip_y=True)"
            # a checkpoint written back lands in this part's rows: zeros first (seen by the read), then the oracle's rows
            tr.write_accumulated(np.zeros((len(rows), w, 4), np.float32))
            assert not np.any(tr.read_accumulated()), name
            tr.write_accumulated(acc2[rows])
            mgr.RenderFrames(2)
            assert_image(tr.read_accumulated(), acc4[rows], f"{name}: AccumulatedRender after write_accumulated + 2 frames")
            assert_image(tr.read_frame(), fr4[rows], f"{name}: FrameRender after write_accumulated + 2 frames")
            c = tr.counters()
            assert c["pixelFrames"] == 4 * w * len(rows), (name, c)
            seg += c["segments"]
            pf += c["pixelFrames"]
            tr.close()
        assert sorted(owned) == list(range(h))
        assert (seg, pf) == (wc["segments"], wc["pixelFrames"]), (cfg, w, h, strip, parts)


def test_partition_cases_cover_the_edges(pkg):
    """the list above keeps what it is there for: ragged last strips, strips taller than the image, parts with no rows"""
    ragged = [c for c in PARTITIONS if c[1] % c[2]]
    tall = [c for c in PARTITIONS if c[2] > c[1]]
    empty = [c for c in PARTITIONS if any(len(pkg.dist.global_rows_of(p, c[3], c[1], c[2])) == 0 for p in range(c[3]))]
    assert len(ragged) >= 3 and len(tall) >= 2 and len(empty) >= 2
    assert {c[2] for c in PARTITIONS} == {8, 16, 24, 64, 136}


# ------------------------------------------------------------------------------------------------ C. parts with no rows
def test_a_part_with_no_rows_does_nothing_and_can_move_onto_rows(pkg, api, orc):
    """Every call returns RT_OK (the wrapper raises otherwise).  A kernel launched with a zero grid would leave
    hipErrorInvalidConfiguration behind, which each launching call checks and reports; pixelFrames and segments stay 0."""
    w, h = 24, 20                  # 3 strips of 8: part 3 of 4 owns none
    tr = api.create_tracer(0)
    tr.set_partition(8, 3, 4)
    mgr = pkg.scenes.get(*BVH[:1]).make_manager(tr, api, w, h)
    mgr.OnEnable(renderSeed=SEED)  # resize, upload, params, reset_accumulation: all RT_OK (a failure raises)
    assert tr.local_rows() == 0 and len(tr.local_to_global_rows()) == 0
    mgr.RenderFrame()
    mgr.RenderFrame()              # (the second may be held back: the flush below launches it)
    tr.flush()
    mgr.RenderFrames(5)            # a fused request
    mgr.RenderFrames(0)
    tr.synchronize()
    assert tr.read_accumulated().shape == (0, w, 4) and tr.read_frame().shape == (0, w, 4)
    assert tr.display(7).shape == (0, w, 4) and tr.display(7, use_accumulated=False).shape == (0, w, 4)
    assert tr.display_srgb8(7).shape == (0, w, 4) and tr.display_srgb8(7, flip_y=False).shape == (0, w, 4)
    tr.write_accumulated(np.zeros((0, w, 4), np.float32))
    c = tr.counters()
    assert c["pixelFrames"] == 0 and c["segments"] == 0, c
    assert tr.frame() == mgr.numAccumulatedFrames == 1 + 2 + 5   # the frame counter advances like every other part's
    mgr.ResetAccumulatedRender()   # rt_reset_accumulation
    tr.reset_counters()
    tr.timer_begin()
    mgr.RenderFrames(2)
    tr.timer_end()
    tr.synchronize()
    assert tr.frame() == 1 + 2
    # onto rows: the whole image, then part 0 of 2
    for strip, part, parts in ((8, 0, 1), (8, 0, 2)):
        tr.set_partition(strip, part, parts)
        mgr.ResetAccumulatedRender()
        mgr.RenderFrames(2)
        (acc2, fr2, _, _), _, _ = oracle_continued(pkg, orc, BVH[0], BVH[1], w, h)
        rows = pkg.dist.global_rows_of(part, parts, h, strip)
        assert_image(tr.read_accumulated(), acc2[rows], f"part {part} of {parts} after owning no rows")
        assert_image(tr.read_frame(), fr2[rows], f"part {part} of {parts} after owning no rows: FrameRender")
    tr.close()


def test_a_part_with_no_rows_through_the_post_render_passes(pkg, api):
    """The same zero-pixel context through the passes behind the render: the host variants return empty arrays, the device variants
    take a null pointer with 0 bytes and still refuse a misaligned one, and the calls that need the whole image say so."""
    abi = pkg.abi
    w, h = 24, 20                  # 3 strips of 8: part 3 of 4 owns none
    tr = api.create_tracer(0)
    hip = C.CDLL("libamdhip64.so")
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(64)) == 0
    try:
        tr.set_partition(8, 3, 4)
        mgr = pkg.scenes.get(*BVH[:1]).make_manager(tr, api, w, h)
        mgr.OnEnable(renderSeed=SEED)
        mgr.RenderFrames(2)
        assert tr.local_rows() == 0
        cost, aov, resolved = tr.render_cost(1), tr.render_aov(1), tr.resolve()
        assert cost.shape == (0, w, 8) and cost.dtype == np.uint32
        assert aov.shape == (0, w) and aov.dtype == abi.AOV_DTYPE
        assert resolved.shape == (0, w, 4) and resolved.dtype == np.float32
        assert api.render_aov_to_device(tr.h, 1, None, 0) == abi.RT_OK
        assert api.resolve_to_device(tr.h, None, 0) == abi.RT_OK
        assert api.render_aov_to_device(tr.h, 1, d.value + 4, 0) == abi.RT_ERR_INVALID_ARG
        assert api.resolve_to_device(tr.h, d.value + 4, 0) == abi.RT_ERR_INVALID_ARG
        # a part of an image cannot be filtered or reprojected
        dp, rp = api.denoise_params(), api.reproject_params()
        assert api.denoise(tr.h, C.byref(dp), 1, 1, None, 0) == abi.RT_ERR_STATE
        assert "part 3 of 4" in api.last_error(tr.h).decode()
        assert api.denoise_to_device(tr.h, C.byref(dp), 1, 1, None, 0) == abi.RT_ERR_STATE
        assert api.reproject_accumulated(tr.h, C.byref(rp), d.value, 1, None) == abi.RT_ERR_STATE
        assert "part 3 of 4" in api.last_error(tr.h).decode()
        tr.synchronize()
        c = tr.counters()
        assert c["pixelFrames"] == 0 and c["segments"] == 0, c
    finally:
        tr.close()
        assert hip.hipFree(d) == 0


# ------------------------------------------------------------------------------------------------ D. more contexts than strips
def test_multi_context_with_more_contexts_than_strips(pkg, api):
    """6 contexts on a 40 x 20 image (3 strips: 8 / 8 / 4 rows): contexts 3, 4 and 5 own no rows.  Host gathers, device gathers
    for a root that owns rows and for one that owns none, and the counters equal the single-context render."""
    w, h, frames = 40, 20, 3
    single = api.create_tracer(0)
    a, _ = render(pkg, api, single, 3, w, h, frames, seed=SEED)
    fa = single.read_frame()
    ca = single.counters()
    single.close()
    hip = C.CDLL("libamdhip64.so")
    multi = api.create_multi_tracer([0] * 6)
    try:
        b, _ = render(pkg, api, multi, 3, w, h, frames, seed=SEED)
        assert [multi.context(i).local_rows() for i in range(6)] == [8, 8, 4, 0, 0, 0]
        assert bits_equal(a, b) and bits_equal(fa, multi.read_frame())
        cb = multi.counters()
        assert (ca["segments"], ca["pixelFrames"]) == (cb["segments"], cb["pixelFrames"]) and cb["pixelFrames"] == w * h * frames
        nbytes = w * h * 16
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(nbytes)) == 0
        try:
            for root in (1, 4):
                for gather, want in ((multi.gather_accumulated_to_device, a), (multi.gather_frame_to_device, fa)):
                    assert hip.hipMemset(d, 0xff, C.c_size_t(nbytes)) == 0 and hip.hipDeviceSynchronize() == 0
                    gather(root, d, nbytes)
                    host = np.zeros((h, w, 4), dtype=np.float32)
                    assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), d, C.c_size_t(nbytes), C.c_int(2)) == 0   # device to host
                    assert bits_equal(host, want), (root, gather.__name__)
        finally:
            hip.hipFree(d)
    finally:
        multi.close()


# ------------------------------------------------------------------------------------------------ E. a series of geometries
def test_one_context_through_a_series_of_geometries(pkg, api, orc):
    """One context, one uploaded scene: resize up and down, the same tile count in another shape, partition changes with and
    without a resize, strip_rows 8 -> 24 -> 8, bound targets and back; a fused launch right after every change and a display
    between steps (the display scratch is reused at another size).  Every step equals a fresh oracle render of its geometry."""
    hip = C.CDLL("libamdhip64.so")
    cfg, kw = FLAT
    w0, h0 = 24, 16
    tr = api.create_tracer(0)
    mgr = pkg.scenes.get(cfg, **kw).make_manager(tr, api, w0, h0)
    mgr.OnEnable(renderSeed=SEED)
    # (w, h, strip_rows, part, parts, bind); None keeps the size (no rt_resize)
    steps = [
        (24, 16, 8, 0, 1, False),
        (72, 40, 8, 0, 1, False),    # grow
        (9, 7, 8, 0, 1, False),      # shrink below one tile
        (64, 8, 8, 0, 1, False),     # 8 tiles in a row ...
        (8, 64, 8, 0, 1, False),     # ... and in a column
        (None, None, 8, 1, 2, False),   # partition change without rt_resize
        (None, None, 24, 1, 2, False),  # strip_rows 8 -> 24 ...
        (None, None, 24, 0, 2, True),   # ... bound targets ...
        (None, None, 8, 0, 1, True),    # ... strip_rows back to 8, bound again
        (40, 20, 8, 0, 1, True),
        (40, 20, 8, 0, 1, False),    # own targets again
        (1, 1, 8, 0, 1, False),
        (33, 17, 16, 1, 2, False),
    ]
    bufs = []
    w, h = w0, h0
    partition = (8, 0, 1)
    try:
        for i, (sw, sh, strip, part, parts, bind) in enumerate(steps):
            name = f"step {i}: {steps[i]}"
            if (strip, part, parts) != partition:
                partition = (strip, part, parts)
                tr.set_partition(*partition)     # (re-sizes the targets itself and drops a binding)
            if sw is not None and (sw, sh) != (w, h):
                w, h = sw, sh
                mgr.screenSize = (w, h)
                tr.resize(w, h)                  # (drops a binding too: the new one is made below)
            rows = pkg.dist.global_rows_of(part, parts, h, strip)
            if bind:
                nbytes = max(len(rows) * w * 16, 16)
                f, a = C.c_void_p(), C.c_void_p()
                assert hip.hipMalloc(C.byref(f), C.c_size_t(nbytes)) == 0 and hip.hipMalloc(C.byref(a), C.c_size_t(nbytes)) == 0
                bufs += [f, a]
                tr.bind_render_targets(f.value, a.value)
            elif i and steps[i - 1][5]:
                tr.bind_render_targets(None, None)
            mgr.ResetAccumulatedRender()
            mgr.RenderFrames(3)          # a fused launch directly after the change
            mgr.RenderFrame()
            assert tr.local_rows() == len(rows) and np.array_equal(tr.local_to_global_rows(), rows), name
            want = oracle_geometry(pkg, orc, cfg, kw, (w0, h0), (w, h))
            assert_image(tr.read_accumulated(), want[0][rows], f"{name}: AccumulatedRender")
            assert_image(tr.read_frame(), want[1][rows], f"{name}: FrameRender")
            assert_image(tr.display(4), want[2][rows], f"{name}: display")
            assert np.array_equal(tr.display_srgb8(4, flip_y=False), want[3][rows]), f"{name}: display_srgb8"
            assert tr.counters()["pixelFrames"] == 4 * w * len(rows)
            tr.reset_counters()
            if bind:
                assert tr.render_targets() == (bufs[-2].value, bufs[-1].value), name
    finally:
        tr.close()
        for b in bufs:
            hip.hipFree(b)


def oracle_geometry(pkg, orc, cfg, kw, size0, size):
    """A fresh oracle render of `size` with the camera of a manager made at `size0` (the HIP context keeps its manager)."""
    key = ("geometry", cfg, tuple(sorted(kw.items())), size0, size)
    if key not in _oracle_cache:
        tr = orc.create_tracer(8)
        mgr = pkg.scenes.get(cfg, **kw).make_manager(tr, orc, *size0)
        mgr.screenSize = size
        mgr.OnEnable(renderSeed=SEED)
        mgr.RenderFrames(3)
        mgr.RenderFrame()
        _oracle_cache[key] = (tr.read_accumulated().copy(), tr.read_frame().copy(), tr.display(4).copy(), tr.display_srgb8(4, flip_y=False).copy())
        tr.close()
    return _oracle_cache[key]
