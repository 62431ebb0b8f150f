"""What tests/test_motion.py and tests/test_gpu_motion.py compare the calls of include/rt_motion.h against: NumPy fp32 restatements of that
header's prose (written from the prose, not from the code) — the centre ray, the reprojection with a motion table, rt_motion_from_scene —
and the synthetic tables both use.

Every array operation below is one IEEE binary32 operation per element (NumPy does not contract); steps 2 ... 5 are
tests/reproject_reference.py's, whose divide is the oracle's."""
import numpy as np

import aov_support as ga
import reproject_reference as ref

F = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=F)


# ---------------------------------------------------------------- B. the reprojection with a table
def moved_records(cur_aov, motion):
    """Step 1' of include/rt_motion.h: the current records with (pm, nm) in the place of (pos, normal) for every pixel whose object has an
    entry of `motion` ((n, 12) float32, or None / empty: no entry for anyone); the other pixels keep their bits.  A pixel with an entry
    whose own pos or normal is not finite (step 1 gives it no history) gets a NaN position, which gives it none either."""
    out = cur_aov.copy()
    m = np.zeros((0, 12), dtype=F) if motion is None else np.ascontiguousarray(motion, dtype=F).reshape(-1, 12)
    k = cur_aov["object"]
    has = (k >= 0) & (k < len(m))
    if not has.any():
        return out
    e = m[np.where(has, k, 0)]  # (H, W, 12)
    pos, nrm = cur_aov["pos"].astype(F), cur_aov["normal"].astype(F)
    with np.errstate(all="ignore"):
        pm = np.stack([((e[..., 4 * r] * pos[..., 0] + e[..., 4 * r + 1] * pos[..., 1]) + e[..., 4 * r + 2] * pos[..., 2]) + e[..., 4 * r + 3] for r in range(3)], axis=-1)
        nm = np.stack([(e[..., 4 * r] * nrm[..., 0] + e[..., 4 * r + 1] * nrm[..., 1]) + e[..., 4 * r + 2] * nrm[..., 2] for r in range(3)], axis=-1)
    step1 = ref.finite_all(pos) & ref.finite_all(nrm)
    pm = np.where(step1[..., None], pm, F(np.nan)).astype(F)
    out["pos"] = np.where(has[..., None], pm, cur_aov["pos"])
    out["normal"] = np.where(has[..., None], nm.astype(F), cur_aov["normal"])
    return out


def reproject_moving(orc, prev_rgba, prev_aov, cur_aov, motion, prev_view_params, prev_cam, max_plane_distance, min_normal_dot, max_history, flags=0):
    """Steps 2', 4' and the unchanged ones read the record's position and normal where rt_reproject.h reads a.pos and a.normal, and nothing
    else of them: the restatement of rt_reproject.h on the records of step 1'."""
    return ref.reproject(orc, prev_rgba, prev_aov, moved_records(cur_aov, motion), prev_view_params, prev_cam, max_plane_distance, min_normal_dot, max_history, flags)


def reproject_moving_with(orc, prev_rgba, prev_aov, cur_aov, motion, p):
    return reproject_moving(orc, prev_rgba, prev_aov, cur_aov, motion, list(p.prevViewParams), list(p.prevCamLocalToWorld), p.maxPlaneDistance, p.minNormalDot,
                            p.maxHistory, p.flags)


# ---------------------------------------------------------------- rt_motion_from_scene
def motion_from_scene(prev_spheres, cur_spheres, prev_models, cur_models):
    """(n_spheres + n_models, 12) float32: spheres first (identity rotation, prev.centre - cur.centre), then the top three rows of
    prev.localToWorld x cur.worldToLocal (column-major inputs, ((a0*b0 + a1*b1) + a2*b2) + a3*b3)."""
    ns, nm = len(prev_spheres), len(prev_models)
    out = np.zeros((ns + nm, 12), dtype=F)
    for i in range(ns):
        out[i] = IDENTITY
        out[i, 3::4] = prev_spheres[i]["centre"].astype(F) - cur_spheres[i]["centre"].astype(F)
    for j in range(nm):
        A, B = prev_models[j]["localToWorld"].astype(F), cur_models[j]["worldToLocal"].astype(F)
        for r in range(3):
            for c in range(4):
                out[ns + j, 4 * r + c] = ((A[r] * B[4 * c] + A[4 + r] * B[4 * c + 1]) + A[8 + r] * B[4 * c + 2]) + A[12 + r] * B[4 * c + 3]
    return out


# ---------------------------------------------------------------- A. the centre ray
def centre_rays(orc, p, w, h, rows=None):
    """Origin and direction of the pixel-centre ray for every pixel of the global rows `rows` (default: all) of a w x h image, (len(rows), w,
    3) float32 each: uv and focusPoint as tests/aov_support.py::camera_rays restates them, the origin the camera's, no draw."""
    ieee = b"RT_MATH_IEEE" in orc.version()
    rows = np.arange(h) if rows is None else np.asarray(rows)
    with np.errstate(all="ignore"):
        uvx = ga.oracle_eval(orc, 6, np.arange(w, dtype=np.uint32).astype(F), F(w) - F(1))
        uvy = ga.oracle_eval(orc, 6, rows.astype(np.uint32).astype(F), F(h) - F(1))
        U, V = np.broadcast_to(uvx[None, :], (len(rows), w)), np.broadcast_to(uvy[:, None], (len(rows), w))
        m = np.array(list(p.camLocalToWorld), dtype=F)
        vp = np.array(list(p.viewParams), dtype=F)

        def mul_point(x, y, z):  # mul(M, float4(v, 1)).xyz, summed left to right
            return [m[r] * x + m[4 + r] * y + m[8 + r] * z + m[12 + r] * F(1) for r in range(3)]
        focus = mul_point((U - F(0.5)) * vp[0], (V - F(0.5)) * vp[1], np.full(U.shape, F(1) * vp[2], dtype=F))
        zero = np.zeros(U.shape, dtype=F)
        origin = mul_point(zero, zero, zero)
        d = [focus[k] - origin[k] for k in range(3)]
        dot = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        if ieee:
            n = ga.oracle_eval(orc, 4, dot)
            direction = [ga.oracle_eval(orc, 6, d[k], n) for k in range(3)]
        else:
            r = ga.oracle_eval(orc, 8, dot)  # rt_normalize = v * rt_rsqrt(dot(v, v))
            direction = [d[k] * r for k in range(3)]
    return np.stack(origin, axis=-1).astype(F), np.stack(direction, axis=-1).astype(F)


# ---------------------------------------------------------------- synthetic tables
def rotation_z(angle, about=(0.0, 0.0)):
    """Rows of the rotation by `angle` about the axis parallel to z through (about, *): it keeps the wall z = 4 of reproject_reference.view
    in itself, so that moved points stay on the plane their taps lie on."""
    c, s = np.cos(angle), np.sin(angle)
    ax, ay = about
    return np.array([c, -s, 0, ax - c * ax + s * ay, s, c, 0, ay - s * ax - c * ay, 0, 0, 1, 0], dtype=F)


def translation(t):
    m = IDENTITY.copy()
    m[3::4] = t
    return m


def nonfinite(k):
    m = IDENTITY.copy()
    m[[3, 5, 10, 0][k % 4]] = [np.nan, np.inf, -np.inf, np.nan][k % 4]
    return m


def table(n, kind="mixed"):
    """n entries.  "identity": all identity.  "mixed": entry k is, by k % 4, a translation along the wall, a rotation in the wall, an entry
    with a NaN or an infinity, the identity — each a little different from entry to entry."""
    out = np.zeros((n, 12), dtype=F)
    for k in range(n):
        if kind == "identity":
            out[k] = IDENTITY
        elif k % 4 == 0:
            out[k] = translation((0.04 + 0.001 * k, -0.03, 0.01))
        elif k % 4 == 1:
            out[k] = rotation_z(0.03 + 0.0005 * k, about=(0.2, -0.1))
        elif k % 4 == 2:
            out[k] = nonfinite(k // 4)
        else:
            out[k] = IDENTITY
    return out


def spread_objects(prev, cur, factor, offset=0):
    """The records with object k >= 0 renamed to k * factor + offset in both views (the synthetic views have objects 0, 1, 2): so that a
    long table is indexed far from its start, or that every object lies beyond a short one."""
    out = []
    for rec in (prev, cur):
        rec = rec.copy()
        hit = rec["object"] >= 0
        rec["object"][hit] = rec["object"][hit] * factor + offset
        out.append(rec)
    return out


# ---------------------------------------------------------------- the step of a moving model (tests/test_gpu_motion.py, tools/reproject_cpu_check.py)
MODEL_STEP = dict(along=(0.3, 0.225, 0.3), turn=6.0)


def step_model(pkg, transform, s=1.0):
    """`transform` one step on: s * 0.3 units along each of the model's two horizontal edges (a model that stands upright, turned about the
    vertical axis by euler[1]) and s * 0.225 up — more than the default maxPlaneDistance off every face of a box, less than a third of the
    extent of the blocks of config 3 — and s * 6 degrees about the vertical axis through its own position.  Chosen on the CPU
    (tools/reproject_cpu_check.py --records centre --model-step 1 at 96 x 54): with the table 100 of the 104 pixels on the opaque block carry
    history, without it none; at two thirds of this step a pixel on a rounded edge still passes the static call's plane test."""
    a = np.radians(transform.euler[1])
    ax, ay, az = (s * v for v in MODEL_STEP["along"])
    offset = np.array([np.cos(a) * ax + np.sin(a) * az, ay, -np.sin(a) * ax + np.cos(a) * az])
    euler = (transform.euler[0], transform.euler[1] + s * MODEL_STEP["turn"], transform.euler[2])
    return pkg.Transform(tuple(np.array(transform.position) + offset), euler, transform.scale)


def movable_model(su, records, opaque=True):
    """The object number of the small model (config 3: the blocks have a scale < 3) that most pixels of `records` see — by default among the
    opaque ones: the small model most pixels see is the glass block, and a glass first hit carries nothing unless flag bit 0 asks for it
    (rule 1).  opaque=False is the rule of tests/test_gpu_reproject.py::test_a_model_moved_between_the_views_carries_nothing."""
    ids, counts = np.unique(records["object"][records["object"] >= su.n_spheres], return_counts=True)
    small = [(int(c), int(i)) for i, c in zip(ids, counts)
             if max(su.mgr.models[int(i) - su.n_spheres].transform.scale) < 3.0 and not (opaque and int(su.materials["flag"][int(i)]) == 2)]
    assert small, "no movable model in view"
    return max(small)[1]
