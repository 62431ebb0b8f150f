"""What tests/test_reproject.py and tests/test_gpu_reproject.py compare rt_reproject and rt_resolve against: a NumPy fp32 restatement of
the prose of include/rt_reproject.h (written from the prose, not from the code), and the synthetic inputs both use.

Every array operation below is one IEEE binary32 operation per element (NumPy does not contract); the divide is the oracle's
(oracle_math_eval op 6: rt_div of include/rt_math.h, which tests/test_gpu_math.py pins the device against)."""
import numpy as np

from denoise_reference import dot3, oracle_eval

F = np.float32


def finite_all(c):
    return np.isfinite(c).all(axis=-1)


def div(orc, x, y):
    return oracle_eval(orc, 6, x, np.broadcast_to(np.asarray(y, dtype=F), np.shape(x)))


def reproject(orc, prev_rgba, prev_aov, cur_aov, prev_view_params, prev_cam, max_plane_distance, min_normal_dot, max_history, flags=0, taps=None):
    """prev_rgba: (H, W, 4) float32 sums; prev_aov, cur_aov: (H, W) records of abi.AOV_DTYPE -> (H, W, 4) float32.
    `taps`: a dict that receives x0, y0 (the lower left tap, valid where `located`) and `located` (rules 1 ... 3 passed)."""
    P = np.ascontiguousarray(prev_rgba, dtype=F)
    h, w = P.shape[:2]
    out = np.zeros((h, w, 4), dtype=F)
    if w == 1 or h == 1:
        return out
    m = np.array(list(prev_cam), dtype=F)
    R, U, Fw, O = m[0:3], m[4:7], m[8:11], m[12:15]
    pw, ph, fd = (F(x) for x in prev_view_params)
    max_plane_distance, min_normal_dot, max_history = F(max_plane_distance), F(min_normal_dot), F(max_history)
    a, b = cur_aov, prev_aov
    with np.errstate(all="ignore"):
        obj = a["object"]
        n_a, pos_a = a["normal"].astype(F), a["pos"].astype(F)
        # 1
        ok = obj >= 0
        if not flags & 1:
            ok &= (a["hit"] & 3) != 2
        ok &= finite_all(pos_a) & finite_all(n_a)
        # 2
        d = pos_a - O
        lx, ly, lz = dot3(R, d), dot3(U, d), dot3(Fw, d)
        ok &= lz > 0
        # 3
        u = div(orc, lx * fd, lz * pw) + F(0.5)
        v = div(orc, ly * fd, lz * ph) + F(0.5)
        fx, fy = u * F(w - 1), v * F(h - 1)
        ok &= np.isfinite(fx) & np.isfinite(fy) & (fx > F(-1)) & (fx < F(w)) & (fy > F(-1)) & (fy < F(h))
        # 4
        xf, yf = np.floor(fx), np.floor(fy)
        tx, ty = fx - xf, fy - yf
        x0, y0 = np.where(ok, xf, 0).astype(np.int64), np.where(ok, yf, 0).astype(np.int64)
        if taps is not None:
            taps.update(x0=x0, y0=y0, located=ok.copy())
        sum_w = np.zeros((h, w), dtype=F)
        sum_n = np.zeros((h, w), dtype=F)
        sum_c = np.zeros((h, w, 3), dtype=F)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qxc, qyc = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                wgt = (tx if i else F(1) - tx) * (ty if j else F(1) - ty)
                Pq, bq = P[qyc, qxc], b[qyc, qxc]
                use = ok & inside & (bq["object"] == obj)
                use &= dot3(n_a, bq["normal"].astype(F)) >= min_normal_dot
                use &= np.abs(dot3(n_a, bq["pos"].astype(F) - pos_a)) <= max_plane_distance
                use &= finite_all(Pq) & (Pq[..., 3] > 0)
                mean_q = div(orc, Pq[..., :3], Pq[..., 3:4])
                sum_w = np.where(use, sum_w + wgt, sum_w)
                sum_c = np.where(use[..., None], sum_c + wgt[..., None] * mean_q, sum_c)
                sum_n = np.where(use, sum_n + wgt * Pq[..., 3], sum_n)
        # 5
        has = ok & (sum_w > 0)
        x = div(orc, sum_n, sum_w)
        n = np.where(x < max_history, x, max_history).astype(F)
        mean = div(orc, sum_c, sum_w[..., None])
        out[..., :3] = np.where(has[..., None], mean * n[..., None], F(0))
        out[..., 3] = np.where(has, n, F(0))
    return out


def reproject_with(orc, prev_rgba, prev_aov, cur_aov, p, taps=None):
    """The same with an abi.RtReprojectParams."""
    return reproject(orc, prev_rgba, prev_aov, cur_aov, list(p.prevViewParams), list(p.prevCamLocalToWorld), p.maxPlaneDistance, p.minNormalDot,
                     p.maxHistory, p.flags, taps)


def resolve(orc, rgba_sum):
    s = np.ascontiguousarray(rgba_sum, dtype=F)
    with np.errstate(all="ignore"):
        pos = s[..., 3] > 0
        out = np.where(pos[..., None], div(orc, s[..., :3], s[..., 3:4]), F(0)).astype(F)
    return np.concatenate([out, s[..., 3:4]], axis=-1)


# ---------------------------------------------------------------- synthetic views of one synthetic world
def camera(position=(0, 0, 0), yaw=0.0, roll=0.0):
    """Column-major camLocalToWorld of a camera with orthonormal axes: yaw about world y, then roll about its own forward axis."""
    cy, sy, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll)
    right0, up0, fwd = np.array([cy, 0, -sy]), np.array([0.0, 1, 0]), np.array([sy, 0, cy])
    right, up = cr * right0 + sr * up0, -sr * right0 + cr * up0
    m = np.zeros(16, dtype=F)
    m[0:3], m[4:7], m[8:11], m[12:15], m[15] = right, up, fwd, position, 1
    return m


VIEW_PARAMS = (F(2.0), F(1.25), F(1.0))
CAMERAS = {  # name -> (previous camera, current camera)
    "identity": (camera(), camera()),
    "translation": (camera((0.3, -0.1, 0.2)), camera()),
    "rotation": (camera((0.1, 0, 0), yaw=0.12, roll=-0.2), camera()),
    "behind": (camera((0, 0, 9.0)), camera()),  # the previous camera looks away from everything the current one sees
}


def view(pkg, w, h, cam, seed):
    """The records a camera `cam` (VIEW_PARAMS) has of a synthetic world: the wall z = 4, cut into stripes of three objects by world x
    (object 2 is glass), with holes (misses) that belong to the world, not to the view; normals and positions carry noise that depends
    on the view, so taps differ a little from their centres; a few records hold NaN positions."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    u = xs / max(w - 1, 1) - 0.5
    v = ys / max(h - 1, 1) - 0.5
    m = cam.astype(np.float64)
    direction = (u * VIEW_PARAMS[0])[..., None] * m[0:3] + (v * VIEW_PARAMS[1])[..., None] * m[4:7] + float(VIEW_PARAMS[2]) * m[8:11]
    t = (4.0 - m[14]) / direction[..., 2]
    pos = m[12:15] + direction * t[..., None]
    obj = np.floor(pos[..., 0] * 1.5).astype(np.int64) % 3
    miss = (t <= 0) | (np.sin(pos[..., 0] * 5.0) * np.sin(pos[..., 1] * 7.0) > 0.8)
    aov = np.zeros((h, w), dtype=pkg.abi.AOV_DTYPE)
    normal = np.array([0, 0, -1.0]) + rng.normal(0, 0.12, (h, w, 3))
    aov["normal"] = normal.astype(F)
    aov["pos"] = (pos + np.array([0, 0, 1.0]) * rng.normal(0, 0.04, (h, w, 1))).astype(F)
    aov["albedo"] = rng.uniform(0.2, 1.0, (h, w, 3)).astype(F)
    aov["object"] = obj
    aov["hit"] = np.where(obj == 2, 2, 1)
    aov["dst"] = np.abs(t).astype(F)
    aov["triangle"] = -1
    bad = (rng.random((h, w)) < 0.02) & ~miss
    aov["pos"][bad, rng.integers(0, 3, int(bad.sum()))] = np.nan
    for f in ("normal", "pos"):
        aov[f][miss] = 0
    aov["object"][miss] = -1
    aov["hit"][miss] = 0
    aov["dst"][miss] = np.inf
    return aov


def sums(w, h, seed):
    """A previous accumulated image: colour sums of pixels with 1 ... 40 frames, and pixels with alpha 0, negative alpha, NaN and inf."""
    rng = np.random.default_rng(seed)
    count = rng.integers(1, 41, (h, w)).astype(F)
    rgba = np.concatenate([rng.gamma(0.5, 2.0, (h, w, 3)).astype(F) * count[..., None], count[..., None]], axis=-1).astype(F)
    r = rng.random((h, w))
    rgba[r < 0.04, 3] = 0
    rgba[(r >= 0.04) & (r < 0.07), 3] = -3
    bad = (r >= 0.07) & (r < 0.10)
    vals = np.array([np.nan, np.inf, -np.inf], dtype=F)
    rgba[bad, rng.integers(0, 4, int(bad.sum()))] = vals[rng.integers(0, 3, int(bad.sum()))]
    return np.ascontiguousarray(rgba, dtype=F)


def synthetic(pkg, w, h, case, seed=1):
    """(previous sums, previous records, current records, previous camLocalToWorld) of CAMERAS[case]."""
    prev_cam, cur_cam = CAMERAS[case]
    return sums(w, h, seed), view(pkg, w, h, prev_cam, seed + 100), view(pkg, w, h, cur_cam, seed + 200), prev_cam


def edge_case(pkg):
    """A 17 x 9 image (W - 1 and H - 1 are powers of two) seen by an identity camera with pw = ph = fd = 1 in both views, one object on
    the wall z = 1: pixel (x, 0) of the current view is GIVEN the position whose fx is exactly FX[x], at fy = 2.  Returns the inputs and
    FX.  History exists exactly for -1 < fx < 17."""
    w, h = 17, 9
    fx = [-1.0, -0.5, 0.0, 0.25, 15.5, 16.0, 16.5, 17.0, -1.0000001, 8.0]
    rec = np.zeros((h, w), dtype=pkg.abi.AOV_DTYPE)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rec["normal"] = F([0, 0, -1])
    rec["pos"] = np.stack([xs / 16 - 0.5, ys / 8 - 0.5, np.ones((h, w))], axis=-1).astype(F)
    rec["object"] = 0
    rec["hit"] = 1
    rec["dst"] = 1
    rec["triangle"] = -1
    cur = rec.copy()
    for x, f in enumerate(fx):
        cur["pos"][0, x] = (F(f) / F(16) - F(0.5), F(2 / 8 - 0.5), 1)
    rng = np.random.default_rng(4)
    count = (2 ** rng.integers(0, 4, (h, w))).astype(F)  # powers of two: (P / count) * count == P
    rgba = np.concatenate([rng.integers(0, 64, (h, w, 3)).astype(F), count[..., None]], axis=-1).astype(F)
    return rgba, rec, cur, camera(), (F(1), F(1), F(1)), fx
