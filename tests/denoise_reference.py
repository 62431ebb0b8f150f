"""What tests/test_denoise.py and tests/test_gpu_denoise.py compare rt_denoise against: a NumPy fp32 restatement of the filter, written
from the prose of include/rt_denoise.h (not from the code), and the synthetic inputs both use.

Every array operation below is one IEEE binary32 operation per element (NumPy does not contract); exp and divide are the oracle's
(oracle_math_eval ops 1 and 6: rt_exp and rt_div of include/rt_math.h, which tests/test_gpu_math.py pins device against)."""
import numpy as np

F = np.float32
H5 = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))


def oracle_eval(orc, op, x, y=None):
    x = np.ascontiguousarray(x, dtype=F)
    y = np.ascontiguousarray(np.zeros_like(x) if y is None else np.broadcast_to(np.asarray(y, dtype=F), x.shape), dtype=F)
    out = np.zeros_like(x)
    if x.size:
        orc.math_eval(op, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size)
    return out


def dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]  # summed left to right


def finite3(c):
    return np.isfinite(c).all(axis=-1)


def denoise(orc, rgba, aov, iterations, sigma_colour, sigma_normal, sigma_plane, demodulate, scale):
    """rgba: (H, W, 4) float32, aov: (H, W) records of abi.AOV_DTYPE -> (H, W, 4) float32."""
    rgba = np.ascontiguousarray(rgba, dtype=F)
    h, w = rgba.shape[:2]
    with np.errstate(all="ignore"):
        c = rgba[..., :3] * F(scale)
        alpha = rgba[..., 3:4]
        if iterations == 0:
            return np.concatenate([c, alpha], axis=-1)
        obj = aov["object"]
        n, pos, alb = aov["normal"].astype(F), aov["pos"].astype(F), aov["albedo"].astype(F)
        mask = np.zeros((h, w, 3), dtype=bool)
        if demodulate:
            ok = (obj >= 0) & ((aov["hit"] & 3) == 1) & finite3(c)
            mask = ok[..., None] & (alb > F(1 / 256))
            c = np.where(mask, oracle_eval(orc, 6, c, alb), c)
        a_n = F(1) / (F(sigma_normal) * F(sigma_normal))
        a_p = F(1) / (F(sigma_plane) * F(sigma_plane))
        a_c = F(1) / (F(sigma_colour) * F(sigma_colour))
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        for i in range(iterations):
            s = 1 << i
            a_ci = a_c * F(4 ** i)
            filtered = (obj >= 0) & finite3(c)
            sum_w = np.zeros((h, w), dtype=F)
            sum_c = np.zeros((h, w, 3), dtype=F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    yy, xx = ys + dy * s, xs + dx * s
                    inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
                    yq, xq = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
                    cq = c[yq, xq]
                    use = inside & (obj[yq, xq] == obj) & finite3(cq)
                    dn = n - n[yq, xq]
                    d = pos[yq, xq] - pos
                    t = dot3(n, d)
                    dc = c - cq
                    e = (dot3(dn, dn) * a_n + (t * t) * a_p) + dot3(dc, dc) * a_ci
                    wgt = (H5[dy + 2] * H5[dx + 2]) * oracle_eval(orc, 1, -np.where(use, e, F(0)))
                    sum_w = np.where(use, sum_w + wgt, sum_w)
                    sum_c = np.where(use[..., None], sum_c + wgt[..., None] * cq, sum_c)
            new = oracle_eval(orc, 6, sum_c, np.broadcast_to(sum_w[..., None], sum_c.shape))
            c = np.where(filtered[..., None], new, c).astype(F)
        c = np.where(mask, c * alb, c).astype(F)
        return np.concatenate([c, alpha], axis=-1)


def synthetic(pkg, w, h, seed=1):
    """A random w x h image with synthetic records: three objects in irregular regions (object 2 is glass), misses, NaN and +-inf
    colours, an albedo channel below 1/256 (object 1's blue), noisy normals and positions on per-object planes."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    obj = ((xs * 3) // max(w, 3) + (ys * 2) // max(h, 2) + (rng.random((h, w)) < 0.05)) % 3
    miss = rng.random((h, w)) < 0.1
    if w * h > 8:
        miss[h // 2, w // 2] = True
    aov = np.zeros((h, w), dtype=pkg.abi.AOV_DTYPE)
    base_n = np.array([(0, 1, 0), (0.6, 0.8, 0), (0, 0.6, -0.8)], dtype=F)
    base_alb = np.array([(0.75, 0.5, 0.25), (0.5, 0.9, 0.002), (1.0, 1.0, 1.0)], dtype=F)
    aov["normal"] = base_n[obj] + rng.normal(0, 0.05, (h, w, 3)).astype(F)
    aov["pos"] = np.stack([xs * 0.05, ys * 0.05, obj * 1.5 + rng.normal(0, 0.02, (h, w))], axis=-1).astype(F)
    aov["albedo"] = base_alb[obj] * rng.uniform(0.8, 1.0, (h, w, 3)).astype(F)
    aov["object"] = obj
    aov["hit"] = np.where(obj == 2, 2, 1) | np.where(rng.random((h, w)) < 0.2, 0x100, 0)
    aov["dst"] = rng.uniform(1, 9, (h, w)).astype(F)
    aov["triangle"] = -1
    aov["emission"] = 0
    for f in ("normal", "pos"):
        aov[f][miss] = 0
    aov["object"][miss] = -1
    aov["hit"][miss] = 0
    aov["dst"][miss] = np.inf
    rgba = (aov["albedo"] * rng.gamma(0.5, 2.0, (h, w, 3))).astype(F)
    rgba = np.concatenate([rgba, rng.uniform(0, 1, (h, w, 1)).astype(F)], axis=-1)
    bad = rng.random((h, w)) < 0.03
    if w * h > 8:
        bad[0, w - 1] = True
    vals = np.array([np.nan, np.inf, -np.inf], dtype=F)
    rgba[bad, rng.integers(0, 3, int(bad.sum()))] = vals[rng.integers(0, 3, int(bad.sum()))]
    return np.ascontiguousarray(rgba, dtype=F), aov
