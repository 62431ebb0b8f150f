"""The step after the hot path: what the reference shows on screen, image files, and
checkpoint / resume of a progressive render.

`RayTraceDisplay` mirrors Assets/Scripts/Tracer/RayTraceDisplay.cs: it picks the texture
and the `Frame` divisor exactly as `OnRenderImage` does (RTD:9-23) and runs the Display
pass (Display.shader:42-47, `tex / Frame`) on the device through `rt_display`.  Note the
reference's off-by-one: `numAccumulatedFrames` has already been incremented when the blit
runs, so N accumulated frames are shown divided by N+1.  `average()` is the unbiased
`sum / alpha` for people who want the estimator rather than the reference's picture.
"""
import json
import os
import struct
import zlib

import numpy as np


class RayTraceDisplay:
    def __init__(self, raytracer):
        self.raytracer = raytracer  # a RayComputeManager

    def frame_divisor(self):
        m = self.raytracer
        return m.numAccumulatedFrames if m.accumulate else 1  # RTD:14

    def OnRenderImage(self):
        """HDR float image the reference would blit (rows bottom-up, RGBA)."""
        m = self.raytracer
        return m.tracer.display(self.frame_divisor(), use_accumulated=bool(m.accumulate))  # RTD:16-17

    def srgb8(self, flip_y=True):
        """The same after the back buffer's linear->sRGB conversion, RGBA8, top row first."""
        m = self.raytracer
        return m.tracer.display_srgb8(self.frame_divisor(), use_accumulated=bool(m.accumulate), flip_y=flip_y)

    def average(self):
        """sum / alpha: the plain Monte-Carlo mean (alpha holds the true frame count, RCC:22)."""
        acc = self.raytracer.tracer.read_accumulated()
        return acc[..., :3] / np.maximum(acc[..., 3:4], 1.0)

    def save_png(self, path):
        write_png(path, self.srgb8(flip_y=True))

    def save_pfm(self, path):
        write_pfm(path, self.OnRenderImage()[..., :3])


def write_png(path, rgba8):
    """Minimal PNG writer (RGBA8, rows top-down) — no imaging library needed on the GPU box."""
    h, w, _ = rgba8.shape
    raw = b"".join(b"\x00" + rgba8[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def write_pfm(path, rgb):
    """Portable float map, rows bottom-up like the render targets (negative scale = little endian)."""
    h, w, _ = rgb.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(rgb, dtype="<f4").tobytes())


# ---------------------------------------------------------------- traversal-cost heatmap
def cost_heatmap_srgb8(cost, field, scale, flip_y=True):
    """RGBA8 heatmap of one column of a per-pixel cost image (HipTracer.render_cost / MultiTracer.render_cost: (rows, W, 8) uint32,
    rows bottom-up) — the role of the reference's declared but unused visMode / debugVisScale uniforms (RC:24-26).
    `field` is one of hip.COST_FIELDS, or "boxTests" = 2 * innerSteps (the reference's own unit, RC:271).  With t = value / scale
    in fp32, a pixel with t > 1 is pure red (255, 0, 0, 255), any other is grey g = uint8(t * 255 + 0.5).  flip_y: top row first."""
    from .hip import COST_FIELDS
    cost = np.asarray(cost)
    if cost.ndim != 3 or cost.shape[2] != len(COST_FIELDS):
        raise ValueError(f"cost image must be (rows, W, {len(COST_FIELDS)}), got {cost.shape}")
    scale = np.float32(scale)
    if not scale > 0 or not np.isfinite(scale):
        raise ValueError(f"scale must be a positive finite number, got {scale}")
    if field == "boxTests":
        value = 2 * cost[..., COST_FIELDS.index("innerSteps")].astype(np.uint64)
    elif field in COST_FIELDS:
        value = cost[..., COST_FIELDS.index(field)]
    else:
        raise ValueError(f"unknown cost field {field!r}: one of {', '.join(COST_FIELDS + ('boxTests',))}")
    t = value.astype(np.float32) / scale
    over = t > np.float32(1)
    g = (np.where(over, np.float32(0), t) * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    out = np.empty(value.shape + (4,), dtype=np.uint8)
    out[..., 0] = np.where(over, 255, g)
    out[..., 1] = np.where(over, 0, g)
    out[..., 2] = np.where(over, 0, g)
    out[..., 3] = 255
    return out[::-1].copy() if flip_y else out


# ---------------------------------------------------------------- first-hit feature buffers (AOVs)
AOV_CHANNELS = ("normal", "albedo", "emission", "depth", "object")


def aov_object_colour(obj):
    """The fixed colour of an object index (int array, >= 0) as three uint8 planes: h = (obj + 1) * 2654435761 mod 2^32
    (Knuth's multiplicative hash), r, g, b = 64 + (bits 0-7, 8-15, 16-23 of h) * 3 // 4 — never darker than 64, so that no
    object is taken for a miss."""
    h = ((np.asarray(obj).astype(np.uint64) + 1) * 2654435761) & 0xffffffff
    return [(64 + ((h >> s) & 0xff) * 3 // 4).astype(np.uint8) for s in (0, 8, 16)]


def aov_srgb8(aov, channel, flip_y=True, depth_range=None):
    """RGBA8 picture of one channel of an AOV image (HipTracer.render_aov / MultiTracer.render_aov: (rows, W) records of
    abi.AOV_DTYPE, rows bottom-up).  With q(t) = uint8(clip(t, 0, 1) * 255 + 0.5) in fp32 (NaN counts as 0):
      normal    q(n * 0.5 + 0.5) per component (a miss, n = 0, is mid grey)
      albedo    q(albedo)        (a miss shows the sky colour, or black without a sky)
      emission  q(emission)
      depth     grey q((dst - lo) / (hi - lo)), lo / hi = depth_range or the least / greatest finite dst among the hits;
                hi == lo (a constant-depth image) draws every hit as 0; misses are black
      object    aov_object_colour(object); misses are black
    Alpha is 255.  flip_y: top row first (what write_png expects)."""
    aov = np.asarray(aov)
    if aov.ndim != 2 or aov.dtype.names is None or any(f not in aov.dtype.names for f in ("dst", "normal", "albedo", "emission", "object", "hit")):
        raise ValueError("aov image must be a (rows, W) array of abi.AOV_DTYPE records")
    if channel not in AOV_CHANNELS:
        raise ValueError(f"unknown AOV channel {channel!r}: one of {', '.join(AOV_CHANNELS)}")

    def q(t):
        t = np.where(np.isnan(t), np.float32(0), t).astype(np.float32)
        return (np.clip(t, np.float32(0), np.float32(1)) * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    out = np.zeros(aov.shape + (4,), dtype=np.uint8)
    out[..., 3] = 255
    hit = (aov["hit"] & 3) != 0
    if channel == "normal":
        out[..., :3] = q(aov["normal"] * np.float32(0.5) + np.float32(0.5))
    elif channel in ("albedo", "emission"):
        out[..., :3] = q(aov[channel])
    elif channel == "depth":
        dst = aov["dst"].astype(np.float32)
        finite = hit & np.isfinite(dst)
        if depth_range is not None:
            lo, hi = np.float32(depth_range[0]), np.float32(depth_range[1])
        elif finite.any():
            lo, hi = dst[finite].min(), dst[finite].max()
        else:
            lo = hi = np.float32(0)
        span = hi - lo
        with np.errstate(invalid="ignore", over="ignore"):
            t = (np.where(finite, dst, lo) - lo) / span if span > 0 else np.zeros(dst.shape, dtype=np.float32)
        g = np.where(finite, q(t), 0).astype(np.uint8)
        out[..., 0] = out[..., 1] = out[..., 2] = g
    else:
        obj = aov["object"]
        r, g, b = aov_object_colour(np.where(obj >= 0, obj, 0))
        for k, plane in enumerate((r, g, b)):
            out[..., k] = np.where(obj >= 0, plane, 0)
    return out[::-1].copy() if flip_y else out


# ---------------------------------------------------------------- a host image as a picture (the denoised image of HipTracer.denoise)
def linear_srgb8(rgb, flip_y=True):
    """RGBA8 picture of a linear (rows, W, 3 or 4) float image, rows bottom-up: the Display pass's transfer on the host — per channel
    c = clip(c, 0, 1) (NaN counts as 0), then 12.92 c below 0.0031308 and 1.055 c^(1/2.4) - 0.055 above, then uint8(255 t + 0.5).
    Alpha is 255.  flip_y: top row first (what write_png expects).  fp32 with numpy's pow: a picture, not part of the bit contract."""
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] not in (3, 4):
        raise ValueError("image must be (rows, W, 3) or (rows, W, 4)")
    c = rgb[..., :3].astype(np.float32)
    c = np.clip(np.where(np.isnan(c), np.float32(0), c), np.float32(0), np.float32(1))
    t = np.where(c <= np.float32(0.0031308), np.float32(12.92) * c, np.float32(1.055) * np.power(c, np.float32(1 / 2.4)) - np.float32(0.055))
    out = np.full(rgb.shape[:2] + (4,), 255, dtype=np.uint8)
    out[..., :3] = (t.astype(np.float32) * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    return out[::-1].copy() if flip_y else out


# ---------------------------------------------------------------- checkpoint / resume
def save_checkpoint(path, manager):
    """Everything a progressive render needs to continue bit-identically: the accumulation sum,
    the frame counter and the seed (the scene itself is the caller's)."""
    tr = manager.tracer
    acc = tr.read_accumulated()
    meta = dict(width=int(tr.width), height=int(tr.height), numAccumulatedFrames=int(manager.numAccumulatedFrames),
                renderSeed=int(manager.renderSeed), numRaysPerPixel=int(manager.numRaysPerPixel),
                maxBounceCount=int(manager.maxBounceCount))
    np.savez_compressed(path, accumulated=acc, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))


def load_checkpoint(path, manager):
    """Restore into a manager that has the same scene and size: after this, RenderFrame continues
    the sequence Frame = saved counter, saved counter + 1, ..."""
    if not path.endswith(".npz") and not os.path.exists(path):
        path = path + ".npz"
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    tr = manager.tracer
    manager.renderSeed = meta["renderSeed"]
    manager.hasBVH = getattr(manager, "hasBVH", False)
    manager.numAccumulatedFrames = 1
    manager.InitFrame()  # sizes, scene upload, params
    if (tr.width, tr.height) != (meta["width"], meta["height"]):
        raise ValueError("checkpoint resolution %dx%d != %dx%d" % (meta["width"], meta["height"], tr.width, tr.height))
    tr.write_accumulated(z["accumulated"])
    manager.numAccumulatedFrames = meta["numAccumulatedFrames"]
    manager.SetShaderParams()
    return meta
