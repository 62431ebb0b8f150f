"""What tests/test_variance.py and tests/test_gpu_variance.py compare the calls of include/rt_variance.h against: a NumPy fp32
restatement of the moments' update and of the variance-guided filter, written from the prose of that header (not from the code), and
the synthetic inputs both use.

Every array operation below is one IEEE binary32 operation per element (NumPy does not contract); exp, sqrt and divide are the oracle's
(oracle_math_eval ops 1, 4 and 6: rt_exp, rt_sqrt and rt_div of include/rt_math.h, which tests/test_gpu_math.py pins the device against)."""
import numpy as np

from denoise_reference import F, H5, dot3, finite3, oracle_eval, synthetic

HG = (F(1 / 4), F(1 / 2), F(1 / 4))
EPS = F(2.0 ** -13)


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def div(orc, a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=F), np.asarray(b, dtype=F))
    return oracle_eval(orc, 6, a, b)


def update(orc, now, snap, moments, rebase=False):
    """One call of rt_moments_update_buffers: (H, W, 4) float32 each -> (snapshot, moments) afterwards."""
    now, snap, m = (np.ascontiguousarray(a, dtype=F) for a in (now, snap, moments))
    if rebase:
        return now.copy(), m.copy()
    with np.errstate(all="ignore"):
        dn = now[..., 3] - snap[..., 3]
        ok = (dn > 0) & np.isfinite(now).all(axis=-1) & np.isfinite(snap).all(axis=-1)
        b = div(orc, now[..., :3] - snap[..., :3], dn[..., None])
        lm = lum(b)
        q = lm * lm
        ok &= np.isfinite(q)
        new = np.stack([m[..., 0] + lm, m[..., 1] + q, np.zeros_like(q), m[..., 3] + F(1)], axis=-1)
        return now.copy(), np.where(ok[..., None], new, m).astype(F)


def variance(orc, moments, raw, c, mask, unknown):
    """Prepare, steps 1 ... 4."""
    with np.errstate(all="ignore"):
        mx, my, nb = moments[..., 0], moments[..., 1], moments[..., 3]
        known = (nb >= 2) & np.isfinite(mx) & np.isfinite(my) & np.isfinite(nb)
        mu = div(orc, mx, nb)
        d = my - mu * mx
        d = np.where(d > 0, d, F(0))  # rt_max(d, +0): a NaN and -0 give +0
        var = np.where(known, div(orc, d, nb * (nb - F(1))), F(unknown))
        l_in = lum(raw)
        k = div(orc, lum(c), l_in)
        var = np.where(mask.any(axis=-1) & np.isfinite(l_in) & (l_in > 0), var * (k * k), var)
        return np.where(np.isfinite(var), var, F(unknown)).astype(F)


def denoise(orc, rgba, moments, aov, iterations, sigma_luminance, sigma_normal, sigma_plane, demodulate, scale, unknown):
    """rgba, moments: (H, W, 4) float32, aov: (H, W) records of abi.AOV_DTYPE -> (H, W, 4) float32."""
    rgba = np.ascontiguousarray(rgba, dtype=F)
    moments = np.ascontiguousarray(moments, dtype=F)
    h, w = rgba.shape[:2]
    with np.errstate(all="ignore"):
        raw = rgba[..., :3] * F(scale)
        alpha = rgba[..., 3:4]
        if iterations == 0:
            return np.concatenate([raw, alpha], axis=-1)
        obj = aov["object"]
        n, pos, alb = aov["normal"].astype(F), aov["pos"].astype(F), aov["albedo"].astype(F)
        c = raw
        mask = np.zeros((h, w, 3), dtype=bool)
        if demodulate:
            ok = (obj >= 0) & ((aov["hit"] & 3) == 1) & finite3(raw)
            mask = ok[..., None] & (alb > F(1 / 256))
            c = np.where(mask, oracle_eval(orc, 6, raw, alb), raw)
        var = variance(orc, moments, raw, c, mask, unknown)
        a_n = F(1) / (F(sigma_normal) * F(sigma_normal))
        a_p = F(1) / (F(sigma_plane) * F(sigma_plane))
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        for i in range(iterations):
            s = 1 << i
            filtered = (obj >= 0) & finite3(c)
            lc = lum(c)

            def tap(dy, dx):
                yy, xx = ys + dy * s, xs + dx * s
                inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
                yq, xq = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
                return yq, xq, inside & (obj[yq, xq] == obj) & finite3(c[yq, xq])
            sum_k = np.zeros((h, w), dtype=F)
            sum_g = np.zeros((h, w), dtype=F)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    yq, xq, use = tap(dy, dx)
                    k = HG[dy + 1] * HG[dx + 1]
                    sum_k = np.where(use, sum_k + k, sum_k)
                    sum_g = np.where(use, sum_g + k * var[yq, xq], sum_g)
            g = div(orc, sum_g, sum_k)
            inv_l = div(orc, F(1), F(sigma_luminance) * oracle_eval(orc, 4, g) + EPS)
            sum_w = np.zeros((h, w), dtype=F)
            sum_c = np.zeros((h, w, 3), dtype=F)
            sum_v = np.zeros((h, w), dtype=F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    yq, xq, use = tap(dy, dx)
                    cq = c[yq, xq]
                    dn = n - n[yq, xq]
                    d = pos[yq, xq] - pos
                    t = dot3(n, d)
                    e = (dot3(dn, dn) * a_n + (t * t) * a_p) + np.abs(lc - lc[yq, xq]) * inv_l
                    wgt = (H5[dy + 2] * H5[dx + 2]) * oracle_eval(orc, 1, -np.where(use, e, F(0)))
                    sum_w = np.where(use, sum_w + wgt, sum_w)
                    sum_c = np.where(use[..., None], sum_c + wgt[..., None] * cq, sum_c)
                    sum_v = np.where(use, sum_v + (wgt * wgt) * var[yq, xq], sum_v)
            new_c = div(orc, sum_c, sum_w[..., None])
            new_v = div(orc, sum_v, sum_w * sum_w)
            c = np.where(filtered[..., None], new_c, c).astype(F)
            var = np.where(filtered, new_v, var).astype(F)
        c = np.where(mask, c * alb, c).astype(F)
        return np.concatenate([c, alpha], axis=-1)


def synthetic_moments(rgba, seed=1):
    """A moments image for `rgba` (the mean image of denoise_reference.synthetic): batch counts of 0, 1, 1.5, 2 and 7, per-pixel sums
    whose variance is plausible, and the cases the header names: zero variance, a pixel whose sum of L^2 - mu * sum of L cancels below
    zero, NaN, infinite and negative entries."""
    h, w = rgba.shape[:2]
    rng = np.random.default_rng(seed + 77)
    nb = rng.choice(np.array([0, 1, 1.5, 2, 7], dtype=F), size=(h, w), p=[0.08, 0.08, 0.08, 0.26, 0.5])
    with np.errstate(all="ignore"):
        mean = np.nan_to_num(lum(rgba), nan=0.5, posinf=2.0, neginf=0.25).astype(F)
    sd = (mean * rng.uniform(0.0, 1.5, (h, w))).astype(F)
    m = np.zeros((h, w, 4), dtype=F)
    m[..., 0] = mean * nb
    m[..., 1] = (mean * mean + sd * sd) * nb
    m[..., 3] = nb
    pick = rng.random((h, w))
    zero = pick < 0.05
    m[zero, 1] = (m[zero, 0] * m[zero, 0]) / np.maximum(nb[zero], F(1))  # sum of L^2 = nb mu^2 exactly or within an ulp
    below = (pick >= 0.05) & (pick < 0.1)
    m[below, 1] = m[below, 1] * F(0.5)  # smaller than nb mu^2 can ever be: cancels below zero
    bad = (pick >= 0.1) & (pick < 0.16)
    vals = np.array([np.nan, np.inf, -np.inf, -3.0], dtype=F)
    k = int(bad.sum())
    m[bad, rng.choice(np.array([0, 1, 3]), size=k)] = vals[rng.integers(0, 4, k)]
    if w * h > 8:
        m[0, 0] = (F(4), F(10), F(0), F(2))   # var 1 before the units
        m[h - 1, w - 1] = (F(6), F(6), F(0), F(7))  # mu * sum of L = 36/7 < 6; fine: positive
        m[h - 1, 0] = (F(6), F(5), F(0), F(7))  # cancels below zero
        m[0, w - 1] = (F(np.nan), F(1), F(0), F(7))
    return np.ascontiguousarray(m, dtype=F)


def synthetic_sums(w, h, seed=1):
    """(now, snapshot, moments) for the update: frame counts that grew by 0, 1 and 17, that shrank, and non-finite entries in either."""
    rng = np.random.default_rng(seed + 5)
    snap_n = rng.integers(0, 40, (h, w)).astype(F)
    dn = rng.choice(np.array([0, 1, 1, 17, 17, -3], dtype=F), size=(h, w))
    snap = np.concatenate([(rng.gamma(0.5, 2.0, (h, w, 3)) * snap_n[..., None]).astype(F), snap_n[..., None]], axis=-1)
    now = snap.copy()
    now[..., :3] += (rng.gamma(0.5, 2.0, (h, w, 3)) * np.maximum(dn, 0)[..., None]).astype(F)
    now[..., 3] += dn
    vals = np.array([np.nan, np.inf, -np.inf, 3e38], dtype=F)
    for img in (now, snap):
        bad = rng.random((h, w)) < 0.04
        k = int(bad.sum())
        img[bad, rng.integers(0, 4, k)] = vals[rng.integers(0, 4, k)]
    moments = np.zeros((h, w, 4), dtype=F)
    nb = rng.integers(0, 9, (h, w)).astype(F)
    moments[..., 0] = rng.uniform(0, 2, (h, w)).astype(F) * nb
    moments[..., 1] = rng.uniform(0, 4, (h, w)).astype(F) * nb
    moments[..., 3] = nb
    return tuple(np.ascontiguousarray(a, dtype=F) for a in (now, snap, moments))


__all__ = ["F", "lum", "update", "variance", "denoise", "synthetic", "synthetic_moments", "synthetic_sums"]
