"""What tests/test_adaptive.py and tests/test_gpu_adaptive.py compare the calls of include/rt_adaptive.h against: a NumPy fp32
restatement of the pixel error, the tile error, the ordered tile list and its counts, written from the prose of that header (not from
the code); the frame-ordered additions of a tile list; and the synthetic inputs with the hazards the header names.

Every array operation below is one IEEE binary32 operation per element (NumPy does not contract); sqrt and divide are the oracle's
(oracle_math_eval ops 4 and 6: rt_sqrt and rt_div of include/rt_math.h, which tests/test_gpu_math.py pins the device against)."""
import numpy as np

from denoise_reference import F, oracle_eval
from variance_reference import div

TILE = 8
INF = F(np.inf)
# the two parameter sets the selection tests run: an everyday one, and the edges (a strict comparison at 0, no frame limits, and a
# dark floor so small that a large variance overflows the error)
PARAM_SETS = (dict(threshold=0.1, darkFloor=0.01, minFrames=4, maxFrames=64), dict(threshold=0.0, darkFloor=1e-30, minFrames=0, maxFrames=0))


def tiles_xy(w, rows):
    return (w + TILE - 1) // TILE, (rows + TILE - 1) // TILE


def pixel_error(orc, s, m, dark_floor, min_frames, max_frames):
    """Rules 1 ... 5 of "The error of a pixel": s, m (H, W, 4) float32 -> (H, W) float32, +inf or finite and >= 0."""
    s, m = np.ascontiguousarray(s, dtype=F), np.ascontiguousarray(m, dtype=F)
    with np.errstate(all="ignore"):
        mx, my, nb = m[..., 0], m[..., 1], m[..., 3]
        mu = div(orc, mx, nb)
        d = my - mu * mx
        d = np.where(d > 0, d, F(0))  # rt_max(d, +0): a NaN and -0 give +0
        var = div(orc, d, nb * (nb - F(1)))
        err = div(orc, oracle_eval(orc, 4, var), np.abs(mu) + F(dark_floor))
        err = np.where(np.isnan(err), INF, err)                                              # rule 5
        err = np.where((nb >= 2) & np.isfinite(mx) & np.isfinite(my) & np.isfinite(nb), err, INF)  # rule 4
        err = np.where(s[..., 3] < F(min_frames), INF, err)                                  # rule 3
        if max_frames > 0:
            err = np.where(s[..., 3] >= F(max_frames), F(0), err)                            # rule 2
        err = np.where(np.isfinite(s).all(axis=-1), err, F(0))                               # rule 1
    return err.astype(F)


def tile_pixels(w, rows):
    """(tilesY, tilesX) uint32: the pixels of each tile that lie inside the image."""
    tx, ty = tiles_xy(w, rows)
    cols = np.minimum(TILE, w - TILE * np.arange(tx))
    rws = np.minimum(TILE, rows - TILE * np.arange(ty))
    return (rws[:, None] * cols[None, :]).astype(np.uint32)


def tile_error(err):
    """(H, W) pixel errors -> (tilesY * tilesX,) float32: the maximum over each tile's pixels inside the image."""
    rows, w = err.shape
    tx, ty = tiles_xy(w, rows)
    pad = np.zeros((ty * TILE, tx * TILE), dtype=F)  # +0 is the least value an error takes
    pad[:rows, :w] = err
    return pad.reshape(ty, TILE, tx, TILE).max(axis=(1, 3)).reshape(-1).astype(F)


def select(orc, s, m, threshold, darkFloor, minFrames, maxFrames):
    """One rt_adaptive_select_buffers: -> (pixel errors, tile errors, list uint32, tiles_active, pixels_active)."""
    err = pixel_error(orc, s, m, darkFloor, minFrames, maxFrames)
    te = tile_error(err)
    tiles = np.flatnonzero(te > F(threshold)).astype(np.uint32)  # strict; increasing t
    rows, w = err.shape
    pixels = int(tile_pixels(w, rows).reshape(-1)[tiles].sum())
    return err, te, tiles, len(tiles), pixels


def tile_mask(tiles, w, rows):
    """(rows, W) bool: the pixels of the listed tiles."""
    tx, ty = tiles_xy(w, rows)
    on = np.zeros(tx * ty, dtype=bool)
    on[np.asarray(tiles, dtype=np.int64)] = True
    return np.repeat(np.repeat(on.reshape(ty, tx), TILE, axis=0), TILE, axis=1)[:rows, :w]


def add_frames(acc, frames, mask=None):
    """AccumulatedRender after `frames` ((rows, W, 4) FrameRender images, alpha 1) were added in order, as float32 additions — inside
    `mask` ((rows, W) bool) only, when given."""
    acc = np.array(acc, dtype=F, copy=True)
    for fr in frames:
        new = acc + np.asarray(fr, dtype=F)  # alpha += 1: FrameRender's alpha is 1
        acc = new if mask is None else np.where(mask[..., None], new, acc)
    return acc.astype(F)


def checkerboard(w, rows):
    """Tiles with (tx + ty) even, plus the whole last tile column and the whole last tile row: includes the ragged ones."""
    tx, ty = tiles_xy(w, rows)
    gy, gx = np.meshgrid(np.arange(ty), np.arange(tx), indexing="ij")
    on = ((gx + gy) % 2 == 0) | (gx == tx - 1) | (gy == ty - 1)
    return np.flatnonzero(on.reshape(-1)).astype(np.uint32)


# ---------------------------------------------------------------- synthetic inputs
def hazards(min_frames, max_frames):
    """(name, S or None, M or None) per planted pixel: None leaves the base value."""
    nan, inf = F(np.nan), F(np.inf)
    good_s = (F(3), F(2), F(1), F(16))
    out = []
    for k in range(4):
        for name, v in (("nan", nan), ("inf", inf)):
            s = list(good_s)
            s[k] = v
            out.append((f"S[{k}]={name}", tuple(s), None))
    for name, a in (("below minFrames", np.nextafter(F(min_frames), F(-1e30))), ("at minFrames", F(min_frames)),
                    ("below maxFrames", np.nextafter(F(max_frames), F(-1e30))), ("at maxFrames", F(max_frames))):
        out.append((f"S.a {name}", (F(3), F(2), F(1), F(a)), (F(8), F(20), F(0), F(4))))
    for nb in (0, 1, 1.5, 2, np.nan):
        out.append((f"M.w={nb}", good_s, (F(4), F(10), F(0), F(nb))))
    out.append(("cancels below zero", good_s, (F(6), F(5), F(0), F(7))))
    out.append(("mu = 0", good_s, (F(0), F(3), F(0), F(3))))
    out.append(("mu < 0", good_s, (F(-2), F(3), F(0), F(1.75) + F(0.5))))
    out.append(("err overflows", good_s, (F(0), F(3e38), F(0), F(2))))
    out.append(("non-finite M.x", good_s, (inf, F(3), F(0), F(4))))
    out.append(("non-finite M.y", good_s, (F(1), nan, F(0), F(4))))
    return out


def hazard_images(w, h, seed, minFrames=4, maxFrames=64, **_):
    """(S, M, planted): random sums and moments whose tiles are partly quiet and partly noisy, with every hazard of hazards() planted
    in one tile that lies wholly inside the image and one that the image's edge clips (where the shape has such tiles), and one tile
    whose pixels all have an error of exactly +0.  planted: {name: [(y, x), ...]}."""
    rng = np.random.default_rng(seed + 31)
    tx, ty = tiles_xy(w, h)
    frames = rng.integers(max(minFrames, 1) + 1, max(maxFrames, minFrames + 40) - 1, (h, w)).astype(F)
    if maxFrames > 0:
        frames = np.minimum(frames, F(maxFrames - 1))
    mean = rng.uniform(0.05, 2.0, (h, w)).astype(F)
    s = np.concatenate([(rng.uniform(0.2, 1.5, (h, w, 3)).astype(F) * mean[..., None]) * frames[..., None], frames[..., None]], axis=-1).astype(F)
    nb = rng.choice(np.array([2, 3, 4, 7], dtype=F), size=(h, w))
    noisy = np.repeat(np.repeat(rng.random((ty, tx)) < 0.5, TILE, axis=0), TILE, axis=1)[:h, :w]
    rel = (rng.uniform(0.0, 1.0, (h, w)) * np.where(noisy, 0.6, 0.08)).astype(F)  # sd of a batch mean / mean
    m = np.zeros((h, w, 4), dtype=F)
    m[..., 0] = mean * nb
    m[..., 1] = (mean * mean) * (F(1) + rel * rel) * nb
    m[..., 3] = nb
    inner = [(j, i) for j in range(ty) for i in range(tx) if TILE * (i + 1) <= w and TILE * (j + 1) <= h]
    whole = set(inner)
    ragged = [(j, i) for j in range(ty) for i in range(tx) if (j, i) not in whole]
    every = inner + ragged
    # the all-zero tile: sum of L^2 = nb mu^2 exactly (small integers), counts inside the limits
    zj, zi = (inner or every)[0]
    zs = (slice(TILE * zj, min(TILE * zj + TILE, h)), slice(TILE * zi, min(TILE * zi + TILE, w)))
    s[zs] = (F(3), F(2), F(1), F(max(minFrames, 1) + 1))
    m[zs] = (F(4), F(8), F(0), F(2))
    planted = {"zero tile": [(TILE * zj, TILE * zi)]}
    for k, (name, sv, mv) in enumerate(hazards(minFrames, maxFrames)):
        for group in (inner, ragged):
            pool = [t for t in (group or every) if t != (zj, zi)] or every
            j, i = pool[(k * 5 + 1) % len(pool)]
            y = min(TILE * j + int(rng.integers(0, TILE)), h - 1)
            x = min(TILE * i + int(rng.integers(0, TILE)), w - 1)
            if sv is not None:
                s[y, x] = sv
            if mv is not None:
                m[y, x] = mv
            planted.setdefault(name, []).append((y, x))
    return np.ascontiguousarray(s, dtype=F), np.ascontiguousarray(m, dtype=F), planted


def planted_images(w, h, active):
    """(S, M) in which every pixel has an error of exactly +0 under minFrames = 4, maxFrames = 0 (16 frames, and the zero variance of
    hazard_images' all-zero tile), except one pixel in each tile of `active`: its S.a = 1 is below minFrames, which rule 3 turns
    into +inf.  The pixel's place inside its tile moves with the tile's index and is clamped to the image."""
    tx, _ = tiles_xy(w, h)
    s = np.empty((h, w, 4), dtype=F)
    m = np.empty((h, w, 4), dtype=F)
    s[...] = (F(3), F(2), F(1), F(16))
    m[...] = (F(4), F(8), F(0), F(2))
    t = np.asarray(active, dtype=np.int64).reshape(-1)
    y = np.minimum(TILE * (t // tx) + (t // TILE) % TILE, h - 1)
    x = np.minimum(TILE * (t % tx) + t % TILE, w - 1)
    s[y, x, 3] = F(1)
    return s, m


__all__ = ["F", "TILE", "PARAM_SETS", "tiles_xy", "pixel_error", "tile_pixels", "tile_error", "select", "tile_mask", "add_frames", "checkerboard",
           "hazards", "hazard_images", "planted_images"]
