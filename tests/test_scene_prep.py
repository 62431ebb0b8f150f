"""The host half of rt_upload_scene (ray-tracing_amd/csrc/rt_scene_prep.h) on its own, without a device and without the library.

tests/scene_prep_driver.cpp is built against the header with the host compiler, twice: plainly (-O2 -Wall -Wextra -Werror) and with the
address and undefined-behaviour sanitizers (a report ends the program with a non-zero exit, which fails the test).  The sanitized
program is a stand-alone executable with the sanitizer runtimes linked into it; nothing sanitized is loaded into python.  Every test
here runs the sanitized build; the plain build only has to compile warning-free and give the same answer to one request.

What is checked: validation of corrupted scenes (same verdicts as the library, on the worker-thread path and on the sequential walk),
the conservative root filter boxes, the packed filter pair records, the chunk partition, the sphere records."""
import os
import subprocess
import time

import numpy as np
import pytest

import host_driver
from scene_corruptions import corrupted_scenes, scene_arrays
from scene_prep_support import FILTER, ask, write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray-tracing_amd", "csrc")

CHUNK_MODELS = 16
CHUNK = np.dtype([("bMin", "<f4", 3), ("bMax", "<f4", 3), ("always", "<u4"), ("count", "<u4"), ("innerRoots", "<u4"), ("pad", "<u4", 3),
                  ("members", "<u4", CHUNK_MODELS)])


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_prep")
    plain = host_driver.build(d, "scene_prep", ["-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror"], after=["-pthread"])
    # the runtimes are linked INTO the program: it needs nothing preloaded and does not care what else the loader brings
    san = host_driver.build(d, "scene_prep", ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"],
                            exe="driver_san", after=["-pthread"])
    return {"plain": plain, "san": san, "dir": d}


def patches(which, base, cur):
    """`patch` requests that turn the driver's copy of `base` into `cur`"""
    b, c = base.view(np.uint8).reshape(-1), cur.view(np.uint8).reshape(-1)
    return [f"patch {which} {int(i)} {int(c[i]):02x}" for i in np.flatnonzero(b != c)]


def f32(u):
    return np.array([u], dtype="<u4").view("<f4")[0]


# ---------------------------------------------------------------- 5.1 validation under the sanitizer
@pytest.fixture(scope="module")
def base_scene(pkg, api, drivers):
    data, sph = scene_arrays(pkg, api, 4)  # 81,920-triangle mesh + room: 166,010 nodes, what the worker-thread path needs
    assert len(data["nodes"]) >= 1 << 16 and len({int(m["nodeOffset"]) for m in data["meshInfo"]}) >= 2
    path = str(drivers["dir"] / "config4.scene")
    write_scene(path, data["meshInfo"], data["triangles"], data["nodes"], sph)
    return data, sph, path


def _scene_requests(data, models, tris, nodes):
    req = ["reset"] + patches("m", data["meshInfo"], models) + patches("n", data["nodes"], nodes)
    return req + ["validate" + ("" if len(tris) == len(data["triangles"]) else f" ntris={len(tris)}")]


def _verdicts(exe, path, requests, sequential):
    got = ask(exe, [f"load {path}"] + requests, env={"RT_SEQUENTIAL_PREPARE": "1"} if sequential else None)
    return [g for g in got if isinstance(g, dict) and "rc" in g]


def test_validation_fuzz_under_the_sanitizer(pkg, api, drivers, base_scene, monkeypatch):
    """The 150 corrupted scenes of test_abi's fuzz (same generator, same seed, same base scene) through the sanitized driver, on the
    worker-thread path and on the sequential walk: no sanitizer report, the two paths agree, and both say what libraytrace_hip.so says
    about the same arrays — status and, where the scene is accepted, the pair count (sequential walk), tree height, flat, filter count."""
    data, sph, path = base_scene
    requests, lib = [], []
    monkeypatch.setenv("RT_SEQUENTIAL_PREPARE", "1")
    t_lib = 0.0
    for it, kind, models, tris, nodes in corrupted_scenes(data, seed=1, iterations=150):
        requests += _scene_requests(data, models, tris, nodes)
        t0 = time.perf_counter()
        try:
            i = api.validate_scene_arrays(models, tris, nodes, sph)
            lib.append((0, i["n_pairs"], i["max_height"], i["flat"], i["n_filtered"]))
        except pkg.abi.RtError as e:
            lib.append((e.status,))
        t_lib += time.perf_counter() - t0
    t0 = time.perf_counter()
    par = _verdicts(drivers["san"], path, requests, False)
    seq = _verdicts(drivers["san"], path, requests, True)
    print(f"sanitized driver: 2 x 150 scenes in {time.perf_counter() - t0:.1f} s; library, sequential walk: 150 scenes in {t_lib:.1f} s")
    assert len(par) == len(seq) == len(lib) == 150
    seen = {"ok": 0, "err": 0}
    for it, (p, s, l) in enumerate(zip(par, seq, lib)):
        def outcome(v, pairs):
            return (v["rc"],) if v["rc"] else (0,) + ((v["n_pairs"],) if pairs else ()) + (v["max_height"], v["flat"], v["n_filtered"])
        assert outcome(p, False) == outcome(s, False), (it, it % 6, p, s)
        assert outcome(s, True) == l, (it, it % 6, s, l)
        seen["ok" if s["rc"] == 0 else "err"] += 1
    assert seen["ok"] > 10 and seen["err"] > 10, seen


@pytest.mark.parametrize("sequential", [False, True])
def test_hand_made_refusals_under_the_sanitizer(pkg, drivers, base_scene, sequential):
    """What test_validate_scene_refuses_what_upload_scene_refuses hands to the library: the same scenes, the same message substrings"""
    RT_ERR_SCENE = pkg.abi.RT_ERR_SCENE
    data, sph, path = base_scene
    info, tris, nodes = data["meshInfo"], data["triangles"], data["nodes"]
    cases = []
    big = max(range(len(info)), key=lambda i: 0 if i + 1 == len(info) else int(info[i + 1]["nodeOffset"]) - int(info[i]["nodeOffset"]))
    bad = info.copy()
    bad[-1]["nodeOffset"] = info[big]["nodeOffset"]
    bad[-1]["triOffset"] = len(tris) - 1
    cases.append((bad, tris, nodes, "out of bounds"))
    root = int(info[big]["nodeOffset"])
    first = root + int(nodes[root]["startIndex"])
    assert nodes[root]["triangleCount"] <= 0 and nodes[first]["triangleCount"] <= 0
    cyc = nodes.copy()
    cyc[first]["startIndex"] = nodes[root]["startIndex"]
    cases.append((info, tris, cyc, "cycle"))
    oob = nodes.copy()
    oob[first]["startIndex"] = len(nodes)
    cases.append((info, tris, oob, "child index out of bounds"))
    empty = nodes.copy()
    empty[root]["triangleCount"] = 0
    cases.append((info, tris, empty, "empty mesh"))
    cases.append((info, tris[: len(tris) // 2], nodes, "out of"))
    off = info.copy()
    off[0]["nodeOffset"] = len(nodes)
    cases.append((off, tris, nodes, "out of range"))
    requests = []
    for models, t, n, _ in cases:
        requests += _scene_requests(data, models, t, n)
    grafted = False
    if not sequential:  # a mesh that reaches into another mesh's nodes: accepted, or refused for the triangle range or the two offsets
        other = next(i for i in range(len(info)) if int(info[i]["nodeOffset"]) != root)
        o_root = int(info[other]["nodeOffset"])
        if nodes[o_root]["triangleCount"] <= 0:
            graft = nodes.copy()
            graft[o_root]["startIndex"] = first - o_root
            requests += _scene_requests(data, info, tris, graft)
            grafted = True
    got = _verdicts(drivers["san"], path, requests, sequential)
    assert len(got) == len(cases) + grafted
    for (_, _, _, what), g in zip(cases, got):
        assert g["rc"] == RT_ERR_SCENE and what in g["msg"], (what, g)
    if grafted:
        g = got[-1]
        assert (g["rc"] == 0 and g["n_pairs"] > 0) or (g["rc"] == RT_ERR_SCENE and ("out of bounds" in g["msg"] or "two different nodeOffsets" in g["msg"])), g


def test_depth_bound_under_the_sanitizer(pkg, api, drivers):
    """tests/deep_trees.py's hand-made trees through the sanitized driver: heights 1, 31 and 32 accepted at exactly their height, 33 and 34
    refused — by the check behind the walk and by the walk's own — and so the trees whose depth comes from the memo of converted pairs;
    every verdict and message the library's (tests/test_deep_trees.py asserts those)."""
    import deep_trees as dt
    a = pkg.abi
    trees = [("comb1", dt.comb(a, 1)), ("comb31", dt.comb(a, 31, "B")), ("comb32", dt.comb(a, 32, "alternate")), ("tied32", dt.comb_tied(a, 32)),
             ("comb33", dt.comb(a, 33)), ("comb34", dt.comb(a, 34)), ("shared32", dt.shared(a, 16, 16)), ("shared33", dt.shared(a, 17, 16)),
             ("shared33b", dt.shared(a, 1, 32))]
    requests, lib = [], []
    for name, (tris, nodes) in trees:
        scene = dt.one_model(pkg, tris, nodes)
        path = str(drivers["dir"] / f"{name}.scene")
        write_scene(path, *scene, np.zeros(0, dtype=a.sphere_dtype))
        requests += [f"load {path}", "validate"]
        try:
            lib.append((0, api.validate_scene_arrays(*scene)["max_height"]))
        except a.RtError as e:
            lib.append((e.status, str(e)))
    got = [g for g in ask(drivers["san"], requests) if isinstance(g, dict) and "rc" in g]
    assert len(got) == len(trees)
    want = [(0, 1), (0, 31), (0, 32), (0, 32), "model 0: BVH depth 33 > 32", "model 0: BVH deeper than RT_MAX_BVH_DEPTH", (0, 32),
            "model 0: BVH depth 33 > 32", "model 0: BVH depth 33 > 32"]
    for (name, _), g, l, w in zip(trees, got, lib, want):
        if isinstance(w, tuple):
            assert (g["rc"], g["max_height"]) == w == l, (name, g, l)
        else:
            assert g["rc"] == a.RT_ERR_SCENE == l[0] and g["msg"] == w and w in l[1], (name, g, l)


# ---------------------------------------------------------------- 5.2 root filter boxes
def _node(bmin, bmax, start, count):
    n = np.zeros((), dtype=[("boundsMin", "<f4", 3), ("boundsMax", "<f4", 3), ("startIndex", "<i4"), ("triangleCount", "<i4")])
    n["boundsMin"], n["boundsMax"], n["startIndex"], n["triangleCount"] = bmin, bmax, start, count
    return n


def _filter_scene(pkg):
    """Meshes A (inner root, two leaves), B (leaf root, 3 triangles), C / D (A with a NaN / an inf child bound), E (leaf root, one vertex inf);
    32 well-conditioned models over A and B, then the degenerate ones.  Returns the arrays and, per model, what is expected of it."""
    a = pkg.abi
    rng = np.random.default_rng(7)
    tris = np.zeros(8, dtype=a.triangle_dtype)
    for f in ("posA", "posB", "posC"):
        tris[f] = rng.uniform(-1, 1, (8, 3)).astype(np.float32)
    tris[7]["posB"][0] = np.inf
    lo_l, hi_l, lo_r, hi_r = [-1, -0.5, -0.25], [0.2, 0.7, 0.9], [0.1, -0.3, -2], [1.5, 0.4, 0.3]
    nodes = np.zeros(11, dtype=a.node_dtype)
    for base, (l0, r1) in ((0, (lo_l, hi_r)), (4, ([-1, np.nan, -0.25], hi_r)), (7, (lo_l, [1.5, np.inf, 0.3]))):
        nodes[base] = _node([-1, -0.5, -2], [1.5, 0.7, 0.9], 1, -1)  # (a root with count 0 is an empty mesh)
        nodes[base + 1] = _node(l0, hi_l, 0, 2)
        nodes[base + 2] = _node(lo_r, r1, 2, 2)
    nodes[3] = _node([9, 9, 9], [-9, -9, -9], 0, 3)   # B: a leaf root's own bounds are never read
    nodes[10] = _node([-1, -1, -1], [1, 1, 1], 0, 1)  # E
    mesh = {"A": (0, 0), "B": (3, 4), "C": (4, 0), "D": (7, 0), "E": (10, 7)}

    def rotation():
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

    def local_to_world(k):
        """scales from 1e-3 to 1e3 over the models, non-uniform within a model by up to 30 x: invert_affine refuses a matrix whose determinant
        is below 1e-9 of its largest entry cubed, i.e. an anisotropy product near 1e9 — those are not `well-conditioned` (see `thin` below)"""
        m = np.eye(4)
        s = 10.0 ** rng.uniform(-3, 3) if k > 1 else (1e-3, 1e3)[k]
        scale = np.clip(s * 30.0 ** rng.uniform(-0.5, 0.5, 3), 1e-3, 1e3)
        if k == 5:
            scale[0] = -scale[0]  # mirrored
        m[:3, :3] = rotation() @ np.diag(scale)
        m[:3, 3] = rng.uniform(-1e4, 1e4, 3)
        return m

    specs = []  # (mesh, localToWorld or None, worldToLocal override or None, degenerate?)
    for k in range(31):
        specs.append(("AB"[k % 2], local_to_world(k), None, False))
    far = np.eye(4)
    far[0, 3] = 2e4  # no rotation, no scale: its world corners are exact, and the farthest of all — the scene extent is known exactly
    specs.append(("A", far, None, False))
    sing = np.linalg.inv(local_to_world(40))
    sing[2, :3] = 2.0 * sing[1, :3]  # rank 2
    specs.append(("A", None, sing, True))
    proj = np.linalg.inv(local_to_world(41))
    proj[3] = [0, 0, 1e-3, 1]       # last row is not (0, 0, 0, 1)
    specs.append(("A", None, proj, True))
    thin = np.eye(4)
    thin[:3, :3] = rotation() @ np.diag([1e-3, 1e3, 1e3])  # det / max^3 ~ 1e-12: refused by the conditioning rule
    specs.append(("A", thin, None, True))
    for m in "CDE":
        specs.append((m, local_to_world(42), None, True))
    models = np.zeros(len(specs), dtype=a.model_dtype)
    for i, (m, l2w, w2l, _) in enumerate(specs):
        if w2l is None:
            w2l = np.linalg.inv(l2w)
        models[i]["nodeOffset"], models[i]["triOffset"] = mesh[m]
        models[i]["worldToLocal"] = w2l.T.reshape(16).astype(np.float32)
        models[i]["localToWorld"] = (np.eye(4) if l2w is None else l2w).T.reshape(16).astype(np.float32)
    return models, tris, nodes, specs


def _hull(model, boxes):
    """float64: the corners of the local boxes through inverse(worldToLocal); (min, max, the model's own range in world units)"""
    w2l = model["worldToLocal"].astype(np.float64).reshape(4, 4).T
    inv = np.linalg.inv(w2l)
    pts = []
    for lo, hi in boxes:
        for c in range(8):
            p = [(hi if c >> d & 1 else lo)[d] for d in range(3)]
            pts.append(inv[:3, :3] @ np.array(p, dtype=np.float64) + inv[:3, 3])
    pts = np.array(pts)
    rng_local = max(float(np.max(np.abs(np.array(b, dtype=np.float64)))) for b in boxes)
    return pts.min(0), pts.max(0), rng_local * float(np.max(np.sum(np.abs(inv[:3, :3]), axis=1)))


def test_root_filter_boxes(pkg, drivers):
    """Every model that can be filtered gets a world box that holds the float64 hull of its root children (leaf root: of its triangles) and is
    not looser than twice the documented inflation — 1e-4 of the scene extent + 1e-5 of the model's own range in world units; the factor two
    covers the double-to-float rounding and the nextafterf step.  Every degenerate model is never filtered."""
    a = pkg.abi
    models, tris, nodes, specs = _filter_scene(pkg)
    sph = np.zeros(1, dtype=a.sphere_dtype)
    sph[0]["centre"], sph[0]["radius"] = [5, -3, 2], 1.0
    moved = sph.copy()
    moved[0]["centre"], moved[0]["radius"] = [3e4, 0, 0], 2.0
    path = str(drivers["dir"] / "filters.scene")
    write_scene(path, models, tris, nodes, sph)
    got = ask(drivers["san"], [f"load {path}", "validate", "dump filters"] + patches("s", sph, moved) + ["validate", "dump filters"])
    runs = [(got[1], got[2]), (got[-2], got[-1])]
    n = len(models)
    boxes_of = {"A": [(nodes[1]["boundsMin"], nodes[1]["boundsMax"]), (nodes[2]["boundsMin"], nodes[2]["boundsMax"])]}
    tb = np.concatenate([tris[4:7][f] for f in ("posA", "posB", "posC")])
    boxes_of["B"] = [(tb.min(0), tb.max(0))]
    # model 31 (translation 2e4 along x, nothing else) reaches x = 2e4 + 1.5 exactly; the others stay within 1e4 + 1e3 * 2 * sqrt(3) * 30^0.5
    extents = [2e4 + 1.5, 3e4 + 2.0]
    filters = []
    for (info, raw), extent in zip(runs, extents):
        assert info["rc"] == 0 and info["flat"] == 0 and info["n_filtered"] == n, info
        assert len(raw) == (n + 2 * ((n + 1) // 2)) * FILTER.itemsize
        f = np.frombuffer(raw, dtype=FILTER)[:n]
        filters.append(f)
        assert f32(info["max_origin"]) == np.float32(8.0 * extent)
        for i, (m, _, _, degenerate) in enumerate(specs):
            leaf = m in "BE"
            assert f[i]["always"] == (1 if degenerate else 0), (i, m, f[i])
            assert f[i]["innerRoot"] == ((3 << 8 if m == "B" else 0) if leaf else 1), (i, m, f[i])  # E: no usable box, count 0 = never filtered
            if degenerate:
                continue
            lo, hi, own = _hull(models[i], boxes_of[m])
            margin = 1e-4 * extent + 1e-5 * own
            bmin, bmax = f[i]["bMin"].astype(np.float64), f[i]["bMax"].astype(np.float64)
            assert np.all(bmin <= lo) and np.all(bmax >= hi), (i, m, bmin, lo, bmax, hi)
            assert np.all(bmin >= lo - 2 * margin) and np.all(bmax <= hi + 2 * margin), (i, m, lo - bmin, bmax - hi, margin)
    # the spheres moved: nothing but the extent term changes, 1e-4 of the difference on every side (to a few fp32 steps of the coordinate)
    before, after = filters
    assert np.array_equal(before["always"], after["always"]) and np.array_equal(before["innerRoot"], after["innerRoot"])
    grow = 1e-4 * (extents[1] - extents[0])
    for i in np.flatnonzero(before["always"] == 0):
        for side, sign in (("bMin", -1.0), ("bMax", 1.0)):
            b, c = before[i][side].astype(np.float64), after[i][side].astype(np.float64)
            steps = 4 * np.spacing(np.maximum(np.abs(after[i][side]), np.float32(1e-30))).astype(np.float64)
            assert np.all(np.abs((c - b) * sign - grow) <= steps), (i, side, b, c, grow)


def test_oversized_and_unusable_leaf_roots_are_never_filtered(pkg, drivers):
    """A leaf root of 2^23 triangles (its count would not fit beside the flag bits of innerRoot): never filtered, count 0.  The triangles are
    the driver's zero pages; the layout is the dense one (nothing to reorder)."""
    a = pkg.abi
    models = np.zeros(1, dtype=a.model_dtype)
    models[0]["worldToLocal"] = models[0]["localToWorld"] = np.eye(4, dtype=np.float32).reshape(16)
    nodes = np.zeros(1, dtype=a.node_dtype)
    nodes[0] = _node([0, 0, 0], [0, 0, 0], 0, 1 << 23)
    path = str(drivers["dir"] / "bigleaf.scene")
    write_scene(path, models, np.zeros(0, dtype=a.triangle_dtype), nodes, np.zeros(0, dtype=a.sphere_dtype))
    info, raw = ask(drivers["san"], [f"load {path}", f"validate zerotris={1 << 23} layout=dense", "dump filters"])[1:]
    assert info["rc"] == 0 and info["flat"] == 1, info
    f = np.frombuffer(raw, dtype=FILTER)[0]
    assert f["always"] == 1 and f["innerRoot"] == 0
    nodes[0]["triangleCount"] = (1 << 23) - 1  # one fewer: an ordinary leaf root
    write_scene(path, models, np.zeros(0, dtype=a.triangle_dtype), nodes, np.zeros(0, dtype=a.sphere_dtype))
    info, raw = ask(drivers["san"], [f"load {path}", f"validate zerotris={(1 << 23) - 1} layout=dense", "dump filters"])[1:]
    f = np.frombuffer(raw, dtype=FILTER)[0]
    assert info["rc"] == 0 and f["always"] == 0 and f["innerRoot"] == ((1 << 23) - 1) << 8


# ---------------------------------------------------------------- 5.3 filter pair records
def _random_filters(rng, n, always_every=0):
    f = np.zeros(n, dtype=FILTER)
    c = rng.uniform(-100, 100, (n, 3))
    h = rng.uniform(0.1, 10, (n, 3))
    f["bMin"], f["bMax"] = (c - h).astype(np.float32), (c + h).astype(np.float32)
    f["innerRoot"] = np.where(rng.integers(0, 2, n) == 1, 1, rng.integers(1, 100, n) << 8)
    if always_every:
        f["always"][rng.permutation(n)[: max(1, n // always_every)]] = 1
    return f


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_filter_pair_records(drivers, n):
    """n records as given, then ceil(n / 2) pair records of sixteen dwords: minx0 minx1 miny0 miny1 minz0 minz1 maxx0 ... maxz1 always0 always1 - -"""
    f = _random_filters(np.random.default_rng(n), n, always_every=3)
    for exe in (drivers["san"], drivers["plain"]):
        (raw,) = ask(exe, [f"filterpairs {n} {f.tobytes().hex()}"])
        pairs = (n + 1) // 2
        assert len(raw) == (n + 2 * pairs) * FILTER.itemsize
        assert raw[: n * FILTER.itemsize] == f.tobytes()
        q = np.frombuffer(raw[n * FILTER.itemsize:], dtype="<u4").reshape(pairs, 16)
        for p in range(pairs):
            for h in range(2):
                m = 2 * p + h
                if m < n:
                    want_min, want_max, always = f[m]["bMin"].view("<u4"), f[m]["bMax"].view("<u4"), f[m]["always"]
                else:  # the missing partner of an odd count
                    want_min = want_max = np.zeros(3, dtype="<u4")
                    always = 1
                assert np.array_equal(q[p, 0:6][h::2], want_min) and np.array_equal(q[p, 6:12][h::2], want_max) and q[p, 12 + h] == always
            assert q[p, 14] == 0 and q[p, 15] == 0


# ---------------------------------------------------------------- 5.4 chunks
@pytest.mark.parametrize("n", [64, 65, 200, 1086, 1087, 1088, 1300])
def test_chunks(drivers, n):
    f = _random_filters(np.random.default_rng(100 + n), n, always_every=10)
    req = [f"chunks {n} {f.tobytes().hex()}", f"filtering {n}"]
    info, raw, plan, info2, raw2, _ = ask(drivers["san"], req + req)
    assert (info, raw) == (info2, raw2)  # the same input, the same bytes
    assert (info["n_filtered"], info["ext_words"]) == (plan["n_filtered"], plan["ext_words"])
    if n > 1087:  # the cap: 63 + 32 extension words of 32 models; the models behind it are in no chunk
        assert info["n_filtered"] == 1087 and info["ext_words"] == 32
    if n <= 64:
        assert info["n_chunks"] == 0 and raw == b"" and plan == {"n_filtered": n, "ext_words": 0}
        return
    assert len(raw) == info["n_chunks"] * CHUNK.itemsize
    chunks = np.frombuffer(raw, dtype=CHUNK)
    seen = []
    for c in chunks:
        k = int(c["count"])
        assert 1 <= k <= CHUNK_MODELS
        mem = c["members"][:k].astype(np.int64)
        assert np.all(np.diff(mem) > 0) and mem[0] >= 0 and mem[-1] < info["n_filtered"]
        assert np.all(c["members"][k:] == 0) and np.all(c["pad"] == 0)
        alw = f["always"][mem] != 0
        assert c["always"] in (0, 1) and alw.all() == bool(c["always"]) and alw.any() == bool(c["always"])  # never mixed
        assert c["innerRoots"] == int(np.sum(f["innerRoot"][mem] & 1))
        if not c["always"]:
            assert np.array_equal(c["bMin"], f["bMin"][mem].min(0)) and np.array_equal(c["bMax"], f["bMax"][mem].max(0))
        seen += mem.tolist()
    assert sorted(seen) == list(range(info["n_filtered"]))  # every filtered model in exactly one chunk


# ---------------------------------------------------------------- 5.5 sphere records
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_sphere_records(pkg, drivers, n):
    a = pkg.abi
    s = np.zeros(n, dtype=a.sphere_dtype)
    for i, (c, r) in enumerate([([1e4, -2.5, 0.125], 1e-3), ([0.3, 0.2, -0.7], 0.0), ([-12.0, 7.0, 3.5], 2.25)][:n]):
        s[i]["centre"], s[i]["radius"] = c, r
    bound, raw = ask(drivers["san"], [f"spheres {n}" + (f" {s.tobytes().hex()}" if n else "")])
    pairs = (n + 1) // 2
    out = np.frombuffer(raw, dtype="<f4")
    assert len(out) == 4 * n + 8 * pairs
    c = s["centre"].astype(np.float64).reshape(n, 3)
    r2 = (s["radius"] * s["radius"]).astype(np.float32)  # one fp32 multiply
    assert np.array_equal(out[: 4 * n].reshape(n, 4), np.concatenate([s["centre"].reshape(n, 3), r2.reshape(n, 1)], axis=1))
    cc = c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]
    K = (cc - r2.astype(np.float64)).astype(np.float32)
    q = out[4 * n:].reshape(pairs, 8)
    for p in range(pairs):
        for h in range(2):
            i = min(2 * p + h, n - 1)  # the odd last sphere is paired with itself
            assert np.array_equal(q[p, 0:6][h::2], s[i]["centre"]) and q[p, 6 + h] == K[i]
    worst = float(np.max(cc + s["radius"].astype(np.float64) ** 2)) if n else 0.0
    assert worst <= float(f32(bound["bound"])) <= 1.00001 * worst


# ---------------------------------------------------------------- 5.6 plain C++ stays plain
@pytest.mark.parametrize("header", ["rt_layout.h", "rt_scene_prep.h"])
def test_header_is_plain_cxx(tmp_path, header):
    src = tmp_path / "only.cpp"
    src.write_text(f'#include "{header}"\n')
    subprocess.check_call([host_driver.compiler(), "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src)])


def test_host_side_sources_name_no_device_api():
    for path in (os.path.join(CSRC, "rt_scene_prep.h"), os.path.join(CSRC, "rt_records.h"), os.path.join(CSRC, "rt_layout.h"),
                 os.path.join(ROOT, "tests", "scene_prep_driver.cpp")):
        text = open(path).read()
        includes = [line for line in text.splitlines() if line.lstrip().startswith("#include")]
        assert not any("hip" in line for line in includes), path
        assert "RtContext" not in text and "__device__" not in text, path
