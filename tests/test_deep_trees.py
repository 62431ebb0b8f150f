"""The BVH traversal stack at its exact bound, without a GPU (tests/deep_trees.py makes the trees; tests/test_gpu_deep_trees.py renders them).

A wave's LDS holds `max_height` stack rows and then the pixel bookkeeping (rt_launch_plan.h, wave_lds_bytes); traverse() pushes at most one
entry per level.  So the height rt_upload_scene computes must be EXACTLY the number of levels — one less and a ray that pushes at every
level writes over row 0 of the pixel fields — and a tree of 33 levels must be refused, whether its depth was counted by the walk or read
from the memo of converted pairs.  Checked here:

  - combs of every height 1 ... 32, inner child on either side, alternating and tied: accepted with max_height == H, and walked by the
    oracle; height 33 and 34 refused (the two checks of SceneBuilder::convert / prepare_scene, each by its message);
  - a tree whose depth comes from the memo (deep_trees.shared): 32 accepted, 33 refused by the check behind the walk;
  - what the GPU half relies on: most camera rays of every comb it renders hold max_height entries (deep_trees.occupancy), none of the
    control's does, and the shared tree has such rays; and for rt_nee's two walks, which start on a catcher quad behind the camera: a
    quarter or more of the shadow rays towards the facing leaves and of the cosine-distributed next segments do
    (test_conditions_the_nee_gpu_half_rests_on);
  - the oracle's traversal of comb(32) against its brute-force loop over the triangles;
  - a 40-triangle mesh the builders take to leafDepthMax == 32, the reference's MaxDepth: every host builder writes the same bytes;
    the tree has rays that hold 32 entries."""
import ctypes as C
import time

import numpy as np
import pytest

import deep_trees as dt
from deep_trees import CATCHER_POINT, CATCHER_Z, CONE_SCALE, cone_camera, cone_mesh

F = np.float32
F3 = C.c_float * 3
RT_ERR_SCENE = -6
FORMS = ("A", "B", "alternate", "tied")


def make(abi, height, form):
    return dt.comb_tied(abi, height) if form == "tied" else dt.comb(abi, height, form)


def params(pkg, api, cam=None, w=dt.W, h=dt.H_IMG):
    mgr = dt.description(pkg, "params", [], cam).make_manager(None, api, w, h)
    mgr.renderSeed = 1
    return mgr.params()


def oracle_dst(orc, tr, o, d):
    out = (C.c_float * 10)()
    orc.ray_collision(tr.h, F3(*o), F3(*d), out)
    return out[0], out[2]


# ---------------------------------------------------------------- heights
@pytest.mark.parametrize("form", FORMS)
def test_comb_heights_1_to_32_are_accepted_at_exactly_their_height(pkg, api, orc, form):
    """max_height == H is the tightness the GPU half relies on: the launch gets H stack rows, and the witness rays fill them.  The share is
    taken over a 6 x 4 image here (the 24 x 16 images of the GPU half: test_conditions_the_gpu_half_rests_on)."""
    p = params(pkg, api, w=6, h=4)
    ot = orc.create_tracer(1)
    try:
        for height in range(1, 33):
            tris, nodes = make(pkg.abi, height, form)
            assert len(tris) == height + 1 and len(nodes) == 2 * height + 1
            scene = dt.one_model(pkg, tris, nodes)
            info = api.validate_scene_arrays(*scene)
            share = dt.witness_share(nodes, tris, p, 6, 4, height)
            print(f"comb({height}, {form}): max_height {info['max_height']}, {info['n_pairs']} pairs, witness share {share:.2f}")
            assert info["max_height"] == height and info["n_pairs"] == height and not info["flat"]
            assert share >= 0.5
            # the oracle takes it too: the central ray sees the nearest leaf that faces it (glass: not culled, so leaf 0 or a later one)
            ot.upload_scene(*scene, None)
            hit, dst = oracle_dst(orc, ot, (0, 0, 0), (0, 0, 1))
            assert hit and dt.Z0 - dt.TILT <= dst <= dt.Z0 + dt.DZ * height + dt.TILT
    finally:
        ot.close()


@pytest.mark.parametrize("height,message", [(33, "model 0: BVH depth 33 > 32"), (34, "model 0: BVH deeper than RT_MAX_BVH_DEPTH")])
def test_combs_of_33_and_34_levels_are_refused(pkg, api, height, message):
    """33: the walk's own check lets it pass (its deepest unconverted inner node is the walk's 33rd frame: `stack.size() > 33` is false) and
    `height > RT_MAX_BVH_DEPTH` refuses it; 34: the walk's check fires first."""
    for form in ("A", "B"):
        with pytest.raises(pkg.abi.RtError) as e:
            api.validate_scene_arrays(*dt.one_model(pkg, *dt.comb(pkg.abi, height, form)))
        assert e.value.status == RT_ERR_SCENE and message in str(e.value), str(e.value)
    # beside an accepted tree, as a later model
    good = dt.HandMesh("good", *dt.comb(pkg.abi, 32))
    bad = dt.HandMesh("bad", *dt.comb(pkg.abi, height))
    desc = dt.description(pkg, "mixed", [pkg.Model(good), pkg.Model(bad)])
    with pytest.raises(pkg.abi.RtError) as e:
        api.validate_scene_arrays(*dt.scene_arrays(pkg, api, desc))
    assert e.value.status == RT_ERR_SCENE and message.replace("model 0", "model 1") in str(e.value), str(e.value)


@pytest.mark.parametrize("h_top,h_shared", [(1, 31), (16, 16), (31, 1), (5, 27)])
def test_shared_tree_of_32_levels_is_accepted(pkg, api, orc, h_top, h_shared):
    tris, nodes = dt.shared(pkg.abi, h_top, h_shared)
    # two inner nodes with one child pair
    inner = nodes[nodes["triangleCount"] <= 0]
    assert len(inner) - len(set(inner["startIndex"].tolist())) == 1
    info = api.validate_scene_arrays(*dt.one_model(pkg, tris, nodes))
    print(f"shared({h_top}, {h_shared}): max_height {info['max_height']}, {info['n_pairs']} pairs")
    assert info["max_height"] == 32
    assert info["n_pairs"] == 32  # the shared pairs are converted once: root + (h_top - 1) chain pairs + h_shared comb pairs


@pytest.mark.parametrize("h_top,h_shared", [(17, 16), (2, 31), (32, 1), (1, 32), (33, 1)])
def test_shared_tree_of_33_or_more_levels_is_refused_by_the_check_behind_the_walk(pkg, api, h_top, h_shared):
    """The walk itself never stands deeper than 33 frames here (the chain has h_top <= 33 unconverted inner nodes below the root, the comb
    was converted at depth 1 ... h_shared <= 32): only `height > RT_MAX_BVH_DEPTH`, fed from pairDepth[known], can refuse these."""
    tris, nodes = dt.shared(pkg.abi, h_top, h_shared)
    with pytest.raises(pkg.abi.RtError) as e:
        api.validate_scene_arrays(*dt.one_model(pkg, tris, nodes))
    assert e.value.status == RT_ERR_SCENE and f"model 0: BVH depth {h_top + h_shared} > 32" in str(e.value), str(e.value)


def test_reference_text_takes_30_levels_and_its_driver_refuses_more(pkg, api, orc):
    """The reference's own `int stack[32]` (RC:239) stands at H + 1 entries below the deepest inner node of a comb.  Its driver
    (oracle/ref_driver.h) counts the nodes on the longest path, the root included, and lets at most 31 reach the text: the compiled text
    (oracle/_ref/libref.so) renders comb(30) like the oracle, and 31 and 32 levels are refused at upload — nothing here runs the text on
    a tree that could overrun it."""
    import __graft_entry__ as graft
    ref = graft.load_ref()
    if ref is None:
        pytest.skip("oracle/_ref/libref.so is not here (no reference checkout to build it from)")
    out = []
    for lib in (ref, orc):
        tr = lib.create_tracer(2)
        mesh = dt.HandMesh("comb30", *dt.comb(pkg.abi, 30, "alternate"))
        mgr = dt.description(pkg, "comb30", dt.tree_models(pkg, mesh)).make_manager(tr, orc)
        mgr.OnEnable(renderSeed=2)
        mgr.RenderFrames(2)
        c = tr.counters()
        out.append((tr.read_accumulated(), [c[k] for k in ("segments", "innerSteps", "triTests")]))
        if lib is ref:
            for tree in (dt.comb(pkg.abi, 31), dt.comb(pkg.abi, 32), dt.shared(pkg.abi, 16, 16)):
                with pytest.raises(pkg.abi.RtError) as e:
                    tr.upload_scene(*dt.one_model(pkg, *tree), None)
                assert e.value.status == RT_ERR_SCENE and "int stack[32]" in str(e.value), str(e.value)
        tr.close()
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32)) and out[0][1] == out[1][1] and out[0][0][..., :3].any()


# ---------------------------------------------------------------- what the GPU half rests on
GPU_COMBS = [(h, form) for h in (1, 2, 30, 31, 32) for form in ("A", "B", "alternate")] + [(32, "tied")]


@pytest.mark.parametrize("height,form", GPU_COMBS)
def test_conditions_the_gpu_half_rests_on(pkg, api, height, form):
    """At least half of the 24 x 16 pixel-centre camera rays of every comb the GPU half renders hold max_height entries, culled or not"""
    tris, nodes = make(pkg.abi, height, form)
    p = params(pkg, api)
    for cull in (False, True):
        t0 = time.perf_counter()
        share = dt.witness_share(nodes, tris, p, dt.W, dt.H_IMG, height, cull)
        print(f"comb({height}, {form}) cull={cull}: witness share {share:.3f} ({time.perf_counter() - t0:.1f} s)")
        assert share >= 0.5


NEE_COMBS = [(1, "alternate"), (31, "alternate"), (32, "alternate"), (32, "tied")]


@pytest.mark.parametrize("height,form", NEE_COMBS)
def test_conditions_the_nee_gpu_half_rests_on(pkg, api, height, form):
    """rt_nee's two walks start at a vertex on the catcher, 0.001 in front of it: a shadow ray towards a point of a comb triangle that
    faces it, and a cosine-distributed next segment.  The GPU half looks among 64 generator states for one whose first vertex has both
    on the stack's last row, and asserts that it finds one.  That rests on such rays being common, which is asserted here for the
    opaque (culled) comb: at least a quarter of 300 cosine-distributed directions, and at least a quarter of 300 rays towards
    uniformly drawn points of the even (facing) leaves, hold `height` entries.  A quarter each, with about half of the states giving
    the first vertex a shadow ray at all, leaves 64 / 2 / 4 / 4 = 2 expected witnesses; the thresholds are what that search needs,
    not what the combs give (the shares are printed: the cone of directions through every leaf box is wider than the view)."""
    tris, nodes = make(pkg.abi, height, form)
    assert api.validate_scene_arrays(*dt.one_model(pkg, tris, nodes, "emitter"))["max_height"] == height
    x = np.array([CATCHER_POINT[0], CATCHER_POINT[1], CATCHER_Z + 0.001], dtype=F)
    assert x[2] < 0, "behind the camera"
    rng = np.random.default_rng(height * 7 + len(form))
    n = 300
    # the shader's diffuse direction: normalize(normal + a uniform direction), the normal +z
    v = rng.normal(size=(n, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) + [0, 0, 1]
    cosine = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    # towards points of the leaves that face -z (even j): uniform barycentric coordinates, folded like the header's
    leaf = 2 * rng.integers(0, height // 2 + 1, n)
    u = rng.uniform(size=(n, 2))
    u = np.where((u.sum(axis=1) > 1)[:, None], 1 - u, u)
    a, b, c = (tris[k][leaf].astype(np.float64) for k in ("posA", "posB", "posC"))
    to_leaf = a + (b - a) * u[:, :1] + (c - a) * u[:, 1:] - x
    to_leaf = (to_leaf / np.linalg.norm(to_leaf, axis=1, keepdims=True)).astype(F)
    t0 = time.perf_counter()
    for what, dirs in (("cosine-distributed segments", cosine), ("shadow rays towards the facing leaves", to_leaf)):
        occ = np.array([dt.occupancy(nodes, x, d, tris, cull=True)[0] for d in dirs])
        print(f"comb({height}, {form}) from the catcher: {int((occ == height).sum())} of {n} {what} hold {height} entries ({time.perf_counter() - t0:.1f} s)")
        assert occ.max() <= height
        assert (occ == height).mean() >= 0.25, what


def test_control_and_shared_tree(pkg, api):
    tris, nodes = dt.comb_behind(pkg.abi, 32)
    assert api.validate_scene_arrays(*dt.one_model(pkg, tris, nodes))["max_height"] == 32
    p = params(pkg, api, dt.camera(pkg, behind=True))
    for cull in (False, True):
        occ = dt.occupancies(nodes, tris, p, dt.W, dt.H_IMG, cull)
        origin, dirs = dt.pixel_centre_rays(p, dt.W, dt.H_IMG)
        hits = sum(bool(np.isfinite(dt.occupancy(nodes, origin, d, tris, cull)[1])) for d in dirs.reshape(-1, 3)[::7])
        print(f"comb_behind(32) cull={cull}: largest occupancy {occ.max()}, witness share {float((occ == 32).mean())}, {hits} of 55 sampled rays hit")
        assert occ.max() == 1 and dt.witness_share(nodes, tris, p, dt.W, dt.H_IMG, 32, cull) == 0
        assert hits >= 20, "the control must hit its leaves (the pushed inner child is culled AFTER a hit)"
    tris, nodes = dt.shared(pkg.abi, 16, 16)
    occ = dt.occupancies(nodes, tris, params(pkg, api), dt.W, dt.H_IMG, False)
    print(f"shared(16, 16): {int((occ == 32).sum())} of {occ.size} pixels hold 32 entries")
    assert (occ == 32).any() and occ.max() == 32


# ---------------------------------------------------------------- the oracle's walk of comb(32)
def test_oracle_traversal_of_comb_32_equals_bruteforce(pkg, orc):
    """2,000 rays — aimed at the comb from in front, from behind, from between its leaves, and axis-parallel (invDir = inf) — as
    tests/test_bvh.py::test_bvh_traversal_equals_bruteforce does for the builder's trees"""
    rng = np.random.default_rng(32)
    z_end = dt.Z0 + 32 * dt.DZ
    for form, material in (("alternate", "glass"), ("tied", "diffuse")):
        tris, nodes = make(pkg.abi, 32, form)
        ot = orc.create_tracer(1)
        try:
            ot.upload_scene(*dt.one_model(pkg, tris, nodes, material), None)
            n = 500
            target = np.stack([rng.uniform(-4, 4, 4 * n), rng.uniform(-3, 3, 4 * n), rng.uniform(dt.Z0, z_end, 4 * n)], axis=1)
            o = np.concatenate([rng.uniform(-1, 1, (n, 3)),                                                   # in front
                                rng.uniform(-1, 1, (n, 3)) + [0, 0, z_end + 3],                                # behind
                                np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(dt.Z0, z_end, n)], axis=1),  # inside
                                np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(0, z_end + 3, n)], axis=1)])
            d = target - o
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            d[3 * n:] = np.eye(3)[rng.choice([0, 1, 2, 2, 2], n)] * rng.choice([-1, 1], (n, 1))
            o[3 * n:][d[3 * n:, 2] > 0, 2] = -1.0
            o[3 * n:][d[3 * n:, 2] < 0, 2] = z_end + 1
            o, d = o.astype(F), d.astype(F)
            hits = 0
            a, b = (C.c_float * 10)(), (C.c_float * 2)()
            for i in range(len(o)):
                orc.ray_collision(ot.h, F3(*o[i]), F3(*d[i]), a)
                orc.ray_collision_bruteforce(ot.h, F3(*o[i]), F3(*d[i]), b)
                assert a[0] == b[0], (form, i)
                if a[0]:
                    hits += 1
                    assert a[2] == b[1], (form, i, a[2], b[1])
            print(f"comb(32, {form}), {material}: {hits} of {len(o)} rays hit")
            assert hits > len(o) // 4
        finally:
            ot.close()


# ---------------------------------------------------------------- a depth-32 tree from the builder
def test_builders_agree_on_a_mesh_they_take_to_depth_32(pkg, api, orc):
    import __graft_entry__ as graft
    v, nrm, idx = cone_mesh()
    assert np.isfinite(v).all() and len(idx) // 3 <= 64
    nodes, tris, stats = api.build_bvh_arrays(v, nrm, idx, pkg.abi.BVH_QUALITY_HIGH)
    print(f"cone of {len(idx) // 3} triangles: {stats}")
    assert stats["leafDepthMax"] == 32 and stats["leafDepthMin"] == 1 and stats["leafMaxTriCount"] == 8 and stats["totalNodeCount"] == 65
    stats.pop("timeMs")
    others = [("oracle", orc.build_bvh_arrays(v, nrm, idx, 1)), ("1 thread", api.build_bvh_arrays_mt(v, nrm, idx, 1, 1)),
              ("5 threads", api.build_bvh_arrays_mt(v, nrm, idx, 1, 5))]
    ref = graft._ref_lib().load_bvh(pkg)
    if ref is not None:
        others.append(("reference text", ref.build_bvh_arrays(v, nrm, idx, 1)))
    print("compared with: " + ", ".join(name for name, _ in others))
    for name, (n2, t2, s2) in others:
        s2.pop("timeMs")
        assert n2.tobytes() == nodes.tobytes() and t2.tobytes() == tris.tobytes() and s2 == stats, name
    # the scene made of it is accepted at height 32, and rays from the apex outwards hold 32 entries
    info = api.validate_scene_arrays(*dt.one_model(pkg, tris, nodes))
    assert info["max_height"] == 32
    p = params(pkg, api, cone_camera(pkg, "apex"))
    origin, dirs = dt.pixel_centre_rays(p, dt.W, dt.H_IMG)
    s = F(1 / CONE_SCALE)  # into the model's space, as RC:351-352 do (a scale by a power of two: exact)
    occ = np.array([dt.occupancy(nodes, origin * s, d * s, tris, False)[0] for d in dirs.reshape(-1, 3)])
    print(f"cone from the apex: {int((occ == 32).sum())} of {occ.size} pixels hold 32 entries")
    assert occ.max() == 32 and (occ == 32).mean() >= 0.5


