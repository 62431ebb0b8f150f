"""Hand-made BVH node arrays that put a ray on the LAST row of the traversal stack, and a NumPy walk that says which rays do.

The traversal stack of the BVH kernels is sized per scene: rt_upload_scene gives a wave `max_height` rows (the height of the deepest
tree in levels of node pairs, a leaf counting 0), and the pixel bookkeeping starts on the row behind them.  A balanced tree never fills
it; the trees here do, for most camera rays:

  comb(H)         a caterpillar of height H: every inner node has one leaf child and one inner child, the last has two leaves.  H + 1
                  leaves of one large triangle each, one behind the other along +z across the camera's whole view, slightly tilted so
                  that no leaf box is flat.  The leaf of a pair lies BEHIND everything below its inner sibling, so a camera ray from
                  the origin finds the inner child nearer and the leaf farther at every level, hits both boxes while nothing is hit
                  yet, and pushes the leaf: H entries, the last on row H - 1.
  comb_tied(H)    the same with the leaf's box drawn forward to where its inner sibling's box starts: dstA == dstB at every level and
                  the `<=` of `isNearestA = dstA <= dstB` alone decides (the inner child is A).
  comb_behind(H)  comb(H) for the camera on the far side (camera(behind=True)): the leaf is nearer, the inner child is pushed and
                  popped again at once — never more than one entry.  The control.
  shared(T, S)    one tree in which two inner nodes point at the same child pair: a comb of height S that rt_upload_scene converts
                  first under a shallow parent (the root's child A) and meets again below a chain of T further levels (child B), where
                  its height comes from the memo of converted pairs and not from the walk.  Height T + S.

All return (triangles, nodes) of ONE mesh in the caller's format (include/rt_abi.h: RtTriangle, RtBVHNode; children adjacent, the root
carries triangleCount -1 and the other inner nodes 0, as the builder writes them); scene_arrays() and description() make scenes of them.

occupancy() is written from the prose above traverse() in ray-tracing_amd/csrc/rt_kernels.h ("Model loop and per-model BVH traversal
... each lane walks its own (model, node) sequence", "push far, then near; the next pop is the near child, so it stays in `cur`") and
from RC:219-287 — not from the kernel's code: a float32 walk, near child first, the far child pushed only if `dstFar < dst`, that
returns the largest number of entries the stack held.  Test infrastructure: nothing here is imported by the product."""
import re

import numpy as np

F = np.float32
Z0, DZ, TILT = 4.0, 0.25, 0.05     # leaf j (0 = nearest) stands at z = Z0 + j * DZ, its vertices at z - TILT, z, z + TILT
FOV, W, H_IMG = 60.0, 24, 16       # the camera the combs are drawn for: at the origin, looking along +z


def _leaf_triangle(abi, j):
    """Leaf j's triangle.  Its BOX covers more than the view at its distance (half extents 0.9 z x 0.6 z or more; the view's are
    0.866 z x 0.577 z), the triangle itself a part of it that differs from leaf to leaf (which edge it stands on, where its apex is, how
    large it is): which leaf a pixel sees depends on every leaf being tested, in order.  Even leaves face the camera, odd ones away."""
    z = Z0 + DZ * j
    s = 1.15 + 0.045 * ((7 * j) % 11)
    a, b = s * 0.9 * z, s * 0.6 * z
    u = -0.8 + 1.6 * ((5 * j + 2) % 9) / 8.0
    edge = j % 4
    if edge == 0:
        p = [(-a, -b), (a, -b), (u * a, b)]
    elif edge == 1:
        p = [(a, -b), (a, b), (-a, u * b)]
    elif edge == 2:
        p = [(a, b), (-a, b), (u * a, -b)]
    else:
        p = [(-a, b), (-a, -b), (a, u * b)]
    v = np.array([(p[0][0], p[0][1], z - TILT), (p[1][0], p[1][1], z), (p[2][0], p[2][1], z + TILT)], dtype=np.float64)
    n = np.cross(v[1] - v[0], v[2] - v[0])
    # RC:196-209: a triangle faces the ray where -dot(dir, cross(AB, AC)) > 0 — for a ray along +z, where the cross product points to -z
    if (n[2] < 0) != (j % 2 == 0):
        v = v[[0, 2, 1]]
        n = -n
    t = np.zeros(1, dtype=abi.triangle_dtype)
    t["posA"], t["posB"], t["posC"] = v[0], v[1], v[2]
    t["normA"] = t["normB"] = t["normC"] = n / np.linalg.norm(n)
    return t


def _box(tris):
    pts = np.concatenate([tris["posA"], tris["posB"], tris["posC"]]).reshape(-1, 3)
    return pts.min(axis=0), pts.max(axis=0)


def _caterpillar(abi, n_leaves, first_node, inner_side, tris):
    """Nodes of a caterpillar over tris[0 .. n_leaves): the pairs' nodes in walk order, WITHOUT its root.  Returns (nodes, root's box,
    root's startIndex) with the first pair at index `first_node`.  inner_side(d) says whether the inner child of the pair at depth d is
    "A" or "B"; the last pair holds leaf 0 (in the inner child's place) and leaf 1."""
    height = n_leaves - 1
    nodes = np.zeros(2 * height, dtype=abi.node_dtype)
    for d in range(height):
        far = height - d                       # the leaf of this pair: behind leaves 0 .. far - 1
        ia = 2 * d + (0 if inner_side(d) == "A" else 1)
        ib = 2 * d + 1 - (ia - 2 * d)
        lo, hi = _box(tris[far:far + 1])
        nodes[ib] = (lo, hi, far, 1)
        lo, hi = _box(tris[:far])
        nodes[ia] = (lo, hi, first_node + 2 * (d + 1), 0) if d < height - 1 else (lo, hi, 0, 1)
    lo, hi = _box(tris[:n_leaves])
    return nodes, (lo, hi), first_node


def _side(inner_is):
    assert inner_is in ("A", "B", "alternate"), inner_is
    return (lambda d: "AB"[d % 2]) if inner_is == "alternate" else (lambda d: inner_is)


def comb(abi, height, inner_is="A"):
    """(triangles, nodes) of a caterpillar of `height` levels: height + 1 leaves, 2 * height + 1 nodes."""
    assert height >= 1
    tris = np.concatenate([_leaf_triangle(abi, j) for j in range(height + 1)])
    body, (lo, hi), first = _caterpillar(abi, height + 1, 1, _side(inner_is), tris)
    root = np.zeros(1, dtype=abi.node_dtype)
    root[0] = (lo, hi, first, -1)
    return tris, np.concatenate([root, body])


def comb_tied(abi, height):
    """comb(height, "A") with every pair's leaf box starting where its sibling's box starts (a larger box: it still holds the leaf's
    triangle and still lies inside the parent's): for a ray from the origin both are entered through z = boundsMin.z, so the two box
    distances are the same float."""
    tris, nodes = comb(abi, height, "A")
    for d in range(height):
        nodes["boundsMin"][2 + 2 * d][2] = nodes["boundsMin"][1 + 2 * d][2]
        assert nodes["triangleCount"][2 + 2 * d] == 1
    return tris, nodes


def comb_behind(abi, height):
    """comb(height, "alternate"); render it with camera(behind=True)."""
    return comb(abi, height, "alternate")


def shared(abi, h_top, h_shared):
    """One tree of height h_top + h_shared in which two inner nodes have the SAME child pair.

        node 0        root:  children (1, 2)
        node 1   P    inner, child A of the root:  children = pair S, the first pair of a comb of height h_shared over leaves
                      0 .. h_shared.  Converted first, at depth 1.
        node 2   c_1  inner, child B of the root: a chain c_1 .. c_{h_top}; c_i's children are (c_{i+1}, leaf h_shared + h_top - i),
                      and c_{h_top}'s children are pair S again.  When the post-order walk of rt_upload_scene gets there the pair is
                      known: its height is read from the memo.

    The chain's leaves stand behind the shared comb, each behind everything below its sibling, so that a camera ray pushes at every
    level of the chain as in comb().  P's own box starts 0.02 behind the comb it points at (boxes are the caller's: nothing makes them
    tight, and every implementation tests the same numbers), so that c_1, whose box starts with the comb, is the nearer child of the
    root and P is pushed: 1 + (h_top - 1) + h_shared entries."""
    assert h_top >= 1 and h_shared >= 1
    n_leaves = h_shared + h_top
    tris = np.concatenate([_leaf_triangle(abi, j) for j in range(n_leaves)])
    first_chain = 3                               # pairs of c_1 .. c_{h_top - 1}: 2 nodes each
    first_comb = first_chain + 2 * (h_top - 1)    # pair S
    body, (lo, hi), _ = _caterpillar(abi, h_shared + 1, first_comb, _side("alternate"), tris)
    head = np.zeros(first_comb, dtype=abi.node_dtype)
    all_lo, all_hi = _box(tris)
    head[0] = (all_lo, all_hi, 1, -1)
    p_lo = lo.copy()
    p_lo[2] += 0.02
    head[1] = (p_lo, hi, first_comb, 0)
    for i in range(1, h_top + 1):                 # c_i: node 2 for i = 1, else child A of c_{i-1}'s pair
        idx = 2 if i == 1 else first_chain + 2 * (i - 2)
        leaves_below = n_leaves - (i - 1)         # c_i covers leaves 0 .. leaves_below - 1
        c_lo, c_hi = _box(tris[:leaves_below])
        if i == h_top:
            head[idx] = (c_lo, c_hi, first_comb, 0)
        else:
            head[idx] = (c_lo, c_hi, first_chain + 2 * (i - 1), 0)
            far = leaves_below - 1
            l_lo, l_hi = _box(tris[far:far + 1])
            head[first_chain + 2 * (i - 1) + 1] = (l_lo, l_hi, far, 1)
    return tris, np.concatenate([head, body])


# ---------------------------------------------------------------- scenes
class HandMesh:
    """Stands where a Mesh stands in a Model: arrays instead of vertices for a builder."""

    def __init__(self, name, triangles, nodes):
        self.name, self.tris, self.nodes = name, triangles, nodes
        self.triangle_count = len(triangles)


def manager_class(pkg):
    class Manager(pkg.RayComputeManager):
        """CreateAllMeshData (RCM:206-236) with hand-made meshes taken as they are and the others built by the library in use"""

        def CreateAllMeshData(self, models):
            abi = pkg.abi
            tris, nodes, where = [], [], {}
            n_tris = n_nodes = 0
            info = np.zeros(len(models), dtype=abi.model_dtype)
            for i, model in enumerate(models):
                mesh = model.Mesh
                if id(mesh) not in where:
                    where[id(mesh)] = (n_nodes, n_tris)
                    if isinstance(mesh, HandMesh):
                        nd, tr = mesh.nodes, mesh.tris
                    else:
                        nd, tr, _ = self.api.build_bvh_arrays(mesh.vertices, mesh.normals, mesh.triangles, self.bvhQuality)
                    tris.append(tr), nodes.append(nd)
                    n_tris, n_nodes = n_tris + len(tr), n_nodes + len(nd)
                info[i]["nodeOffset"], info[i]["triOffset"] = where[id(mesh)]
                info[i]["worldToLocal"] = pkg.manager.matrix_to_abi(model.transform.worldToLocalMatrix)
                info[i]["localToWorld"] = pkg.manager.matrix_to_abi(model.transform.localToWorldMatrix)
                info[i]["material"] = model.material.pack()
            return {"meshInfo": info, "triangles": np.concatenate(tris), "nodes": np.concatenate(nodes)}
    return Manager


def camera(pkg, behind=False, depth=32):
    """At the origin looking along +z; behind: beyond the last leaf of a comb of `depth` levels, looking back, with a field of view
    narrow enough that the nearest (smallest) leaves still fill it."""
    if behind:
        return pkg.Camera(pkg.Transform((0, 0, Z0 + DZ * depth + 4.0), (0, 180, 0)), fieldOfView=20.0)
    return pkg.Camera(pkg.Transform((0, 0, 0), (0, 0, 0)), fieldOfView=FOV)


SETTINGS = dict(maxBounceCount=6, numRaysPerPixel=1, defocusStrength=0.0, divergeStrength=0.0, useSky=True, accumulate=True, bvhQuality=1)


def materials(pkg):
    M = pkg.RayTracingMaterial
    return {"glass": M(flag=2, diffuseCol=(0.9, 0.95, 1, 1), specularCol=(1, 1, 1, 1), absorption=(0.3, 0.1, 0.05, 1), absorptionMultiplier=0.4, ior=1.3,
                       smoothness=0.9, specularProbability=0.1),
            "diffuse": M(diffuseCol=(0.8, 0.4, 0.2, 1), smoothness=0.3, specularProbability=0.2),
            "emitter": M(diffuseCol=(0.2, 0.2, 0.2, 1), emissionCol=(1, 0.8, 0.5, 1), emissionStrength=2.0)}


def description(pkg, name, models, cam=None, w=W, h=H_IMG, frames=2, **settings):
    """A SceneDescription whose managers take hand-made meshes (manager_class)"""
    base = pkg.scenes.SceneDescription

    class Description(base):
        def make_manager(self, tracer, api, width=None, height=None, manager_cls=None):
            return base.make_manager(self, tracer, api, width, height, manager_cls or manager_class(pkg))
    return Description(name, w, h, frames, dict(SETTINGS, **settings), cam or camera(pkg), models, [])


def tree_models(pkg, mesh, first="glass"):
    """Three instances of one hand-made mesh: the tree as it is (model 0: the witness rays are its), a diffuse copy pushed 0.11 back and
    half a width to the right, an emitting copy pushed 0.17 back, down and to the left.  first = "glass": model 0 is not culled and
    refracted rays go on through the comb from inside it; "diffuse": it is culled (RC:355) and every other leaf is invisible from the front."""
    mats, T = materials(pkg), pkg.Transform
    return [pkg.Model(mesh, mats[first], T()), pkg.Model(mesh, mats["diffuse" if first == "glass" else "glass"], T((2.0, 0.3, 0.11))),
            pkg.Model(mesh, mats["emitter"], T((-1.5, -1.2, 0.17)))]


def scene_arrays(pkg, api, desc):
    """(meshInfo, triangles, nodes) of a description, as rt_upload_scene takes them"""
    mgr = desc.make_manager(None, api)
    d = mgr.CreateAllMeshData(mgr.models)
    return d["meshInfo"], d["triangles"], d["nodes"]


def one_model(pkg, triangles, nodes, material="glass"):
    """(meshInfo, triangles, nodes) of a single untransformed model of the mesh"""
    info = np.zeros(1, dtype=pkg.abi.model_dtype)
    eye = np.eye(4, dtype=F).reshape(16)
    info[0]["worldToLocal"], info[0]["localToWorld"] = eye, eye
    info[0]["material"] = materials(pkg)[material].pack()
    return info, triangles, nodes


# ---------------------------------------------------------------- the walk
def _box_dst(o, inv, lo, hi):
    """RC:219-231 in float32"""
    with np.errstate(all="ignore"):
        t_lo, t_hi = (lo - o) * inv, (hi - o) * inv
        near, far = np.minimum(t_lo, t_hi).max(), np.maximum(t_lo, t_hi).min()
    return (near if near > 0 else F(0)) if (far >= near and far > 0) else F(np.inf)


def _tri_dst(o, d, t, cull):
    """RC:186-216 in float32: the hit distance, or +inf"""
    with np.errstate(all="ignore"):
        a, ab, ac = t["posA"], t["posB"] - t["posA"], t["posC"] - t["posA"]
        n = np.cross(ab, ac).astype(F)
        ao = o - a
        dao = np.cross(ao, d).astype(F)
        det = -F(np.dot(d, n))
        inv = F(1) / det
        dst, u, v = F(np.dot(ao, n)) * inv, F(np.dot(ac, dao)) * inv, -F(np.dot(ab, dao)) * inv
        keep = det >= F(1e-8) if cull else abs(det) >= F(1e-8)
        return dst if keep and dst > 0 and u >= 0 and v >= 0 and F(1) - u - v >= 0 else F(np.inf)


def occupancy(nodes, origin, direction, triangles=None, cull=True, node_offset=0, tri_offset=0):
    """The largest number of entries the traversal stack of ONE ray holds while it walks the tree at `node_offset`, and the hit distance.

    The walk (float32): the current node is held apart from the stack.  At an inner node both children's boxes are tested; if the nearer
    one (A where the distances are equal) is nearer than the hit so far, the walk goes on INTO it, after pushing the farther one if that is
    nearer than the hit so far too; otherwise, and after a leaf, the next node is popped (none left: the tree is done).  The root is never
    pushed.  Without `triangles` no leaf is hit and the distance stays +inf (an upper bound of the occupancy)."""
    o, d = np.asarray(origin, dtype=F), np.asarray(direction, dtype=F)
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(F)
    stack, most, dst = [], 0, F(np.inf)
    cur = node_offset
    while cur is not None:
        n = nodes[cur]
        if n["triangleCount"] > 0:
            if triangles is not None:
                for i in range(int(n["triangleCount"])):
                    t = _tri_dst(o, d, triangles[tri_offset + int(n["startIndex"]) + i], cull)
                    if t < dst:
                        dst = t
            cur = stack.pop() if stack else None
            continue
        ia = node_offset + int(n["startIndex"])
        da = _box_dst(o, inv, nodes["boundsMin"][ia], nodes["boundsMax"][ia])
        db = _box_dst(o, inv, nodes["boundsMin"][ia + 1], nodes["boundsMax"][ia + 1])
        near, far, d_near, d_far = (ia, ia + 1, da, db) if da <= db else (ia + 1, ia, db, da)
        if d_near < dst:
            if d_far < dst:
                stack.append(far)
                most = max(most, len(stack))
            cur = near
        else:
            cur = stack.pop() if stack else None
    return most, dst


def pixel_centre_rays(p, w, h):
    """Origin and (h, w, 3) directions of the camera rays through the pixel centres as RCC:15 + RC:554-576 form them with no defocus
    and no divergence, in float32: uv = id / (size - 1), the focus point through camLocalToWorld, normalised."""
    m, vp = np.array(list(p.camLocalToWorld), dtype=F), np.array(list(p.viewParams), dtype=F)
    u = (np.arange(w, dtype=F) / F(w - 1))[None, :] - F(0.5)
    v = (np.arange(h, dtype=F) / F(h - 1))[:, None] - F(0.5)
    x, y, z = np.broadcast_to(u * vp[0], (h, w)), np.broadcast_to(v * vp[1], (h, w)), np.full((h, w), vp[2], dtype=F)
    focus = np.stack([m[r] * x + m[4 + r] * y + m[8 + r] * z + m[12 + r] for r in range(3)], axis=-1).astype(F)
    origin = m[12:15].copy()
    d = focus - origin
    return origin, (d / np.sqrt((d * d).sum(axis=-1, keepdims=True))).astype(F)


def occupancies(nodes, triangles, p, w, h, cull):
    """(h, w) occupancy of model 0's tree (untransformed, at node 0) for every pixel-centre camera ray"""
    origin, dirs = pixel_centre_rays(p, w, h)
    return np.array([[occupancy(nodes, origin, dirs[y, x], triangles, cull)[0] for x in range(w)] for y in range(h)])


def witness_share(nodes, triangles, p, w, h, max_height, cull=False):
    """The share of the image's pixel-centre camera rays whose occupancy equals max_height: that write the stack's last row"""
    occ = occupancies(nodes, triangles, p, w, h, cull)
    assert occ.max() <= max_height, (int(occ.max()), max_height)
    return float((occ == max_height).mean())


LAUNCH = re.compile(r"kernel variant (\d+): (\d+) stack entries, (\d+) B of LDS per workgroup of (\d+) threads \((\d+) B of it the top-of-tree cache: (\d+) records\)")


def launches(capfd):
    """(variant, stack entries, LDS bytes, threads, cache records) of every launch shape reported since the last call"""
    return [tuple(int(g) for g in (m.group(1), m.group(2), m.group(3), m.group(4), m.group(6))) for m in LAUNCH.finditer(capfd.readouterr().err)]


CATCHER_Z = -0.05              # tests/test_gpu_deep_trees.py::nee_scene: a small diffuse quad behind deep_trees.camera that faces the comb
CATCHER_POINT = (0.1, -0.05)   # where that file's witness ray (from z = 1 along -z) meets it


def cone_mesh(n=40, ratio=8.0, size=0.3, scale=2.0 ** 34):
    """A self-similar cone: triangle k is centred at x = scale * ratio^-k on the x axis, its size in proportion.  Whatever the evenly
    spaced split tests of a node are, they separate its outermost triangle from all the others (the next centre lies at 1/8 of the
    extent, the first test at 1/6 or 1/4), so the builder peels one triangle per level until the reference's MaxDepth = 32 stops it:
    leaves at depth 1 ... 32, the deepest with the n - 32 innermost triangles.  The coordinates span 2^34 ... 2^-83: the surface-area
    cost (squares of them) of the smallest nodes stays a normal float32 — it would underflow to 0, and end the splitting at depth 25, if
    the cone began at 1."""
    v, idx = [], []
    for k in range(n):
        c = scale * ratio ** -k
        s = size * c
        v += [(c - s, -s, -0.5 * s), (c + s, -s, 0.5 * s), (c, s, 0.0)]
        idx += [3 * k, 3 * k + 1, 3 * k + 2]
    v = np.array(v, dtype=F)
    v64 = v.astype(np.float64)  # (in float32 the cross products of the smallest triangles underflow)
    nrm = np.cross(v64[1::3] - v64[0::3], v64[2::3] - v64[0::3])
    nrm = np.repeat(nrm / np.linalg.norm(nrm, axis=1, keepdims=True), 3, axis=0).astype(F)
    return v, nrm, np.array(idx, dtype=np.int32)


CONE_SCALE = 2.0 ** -32   # model scale of the cone in a scene: its largest triangle then stands at x = 4


def cone_camera(pkg, where):
    """apex: at the cone's tip looking along its axis, every box in front of it one inside the other; outside: from the side"""
    if where == "apex":
        return pkg.Camera(pkg.Transform((0, 0, 0), (0, 90, 0)), fieldOfView=8.0)
    return pkg.Camera(pkg.Transform((2.0, 0.3, -7.0), (0, 0, 0)), fieldOfView=50.0)
