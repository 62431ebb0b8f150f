"""rt_denoise_buffers / rt_denoise / rt_denoise_to_device (include/rt_denoise.h) on the GPU.  Every comparison of images is == on the
bit patterns (uint32 views), every pixel, every channel, against the NumPy restatement of the header's prose in
tests/denoise_reference.py (its exp and divide are the oracle's, which tests/test_gpu_math.py pins the device against).

  6. rt_denoise_buffers on synthetic inputs: sizes with partial tiles and narrower than a halo, 0 / 1 / 3 / 5 iterations, with and
     without demodulation;
  7. rt_denoise end to end == the NumPy filter of rt_read_accumulated and rt_render_aov; the device variant into a torch tensor (child
     process) gives the same bits; the same under every RT_LAYOUT tests/test_gpu_aov.py iterates;
  8. exact properties: nothing crosses an object edge, misses and non-finite centres come out as scaled input, alpha is copied, 0
     iterations is the scaled copy;
  9. no visible state change;  10. every row of the header's error list, the partitioned context and the internal AOV pass's watchdog
     report (RT_TRAV_LIMIT, the hook tests/test_gpu_watchdog.py uses);
  11. it denoises: against the mean of 1,024 frames, the filtered mean of 4 frames has a smaller squared error than the unfiltered."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from flush_table import held_at

import aov_support as ga
import denoise_reference as ref
from gpu_support import DevBuf, assert_same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def filter_on_device(api, tr, rgba, aov, **fields):
    """rt_denoise_buffers on uploaded copies; returns the output image and the input image as it is afterwards."""
    h, w = rgba.shape[:2]
    d_in, d_aov, d_out = DevBuf.of(rgba), DevBuf.of(aov), DevBuf(rgba.nbytes, fill=0xff)
    try:
        tr.denoise_buffers(w, h, d_in.ptr, d_aov.ptr, d_out.ptr, api.denoise_params(**fields))
        tr.synchronize()
        return d_out.image(h, w), d_in.image(h, w)
    finally:
        for d in (d_in, d_aov, d_out):
            d.free()


def reference(orc, rgba, aov, p):
    return ref.denoise(orc, rgba, aov, p.iterations, p.sigmaColour, p.sigmaNormal, p.sigmaPlane, p.demodulate, p.scale)


# ---------------------------------------------------------------- 6. the filter alone, bits
@pytest.mark.parametrize("w,h", [(1, 1), (1, 37), (37, 1), (64, 36), (333, 77)])
def test_denoise_buffers_equals_the_numpy_restatement(pkg, api, orc, w, h):
    rgba, aov = ref.synthetic(pkg, w, h, seed=w + h)
    tr = api.create_tracer(0)  # no scene, no rt_resize
    try:
        for iterations in (0, 1, 3, 5):
            for demodulate in (0, 1):
                fields = dict(iterations=iterations, demodulate=demodulate, sigmaColour=0.75, sigmaNormal=0.3, sigmaPlane=0.2, scale=0.25)
                got, src = filter_on_device(api, tr, rgba, aov, **fields)
                assert src.tobytes() == rgba.tobytes(), "the source image was written"
                assert_same_bits(got, reference(orc, rgba, aov, api.denoise_params(**fields)), f"{w} x {h}, {iterations} iterations, demodulate {demodulate}")
    finally:
        tr.close()


# ---------------------------------------------------------------- 7. end to end
E2E = [((3, {}), 80, 45), ("emitters", 64, 36)]


def end_to_end(pkg, api, spec, w, h, aov_frame=2):
    tr = api.create_tracer(0)
    try:
        su = ga.Setup(pkg, api, tr, spec, w, h)
        su.mgr.RenderFrames(4)
        p = api.denoise_params(scale=0.25)
        got = tr.denoise(p, aov_frame=aov_frame)
        got_frame = tr.denoise(p, use_accumulated=False, aov_frame=aov_frame)
        return got, got_frame, tr.read_accumulated(), tr.read_frame(), tr.render_aov(aov_frame), p
    finally:
        tr.close()


@pytest.mark.parametrize("spec,w,h", E2E, ids=["config3", "emitters"])
def test_denoise_end_to_end_equals_numpy_on_the_contexts_own_buffers(pkg, api, orc, spec, w, h, monkeypatch):
    got, got_frame, acc, frame, aov, p = end_to_end(pkg, api, spec, w, h)
    assert got.shape == (h, w, 4) and (aov["object"] >= 0).any()
    assert_same_bits(got, reference(orc, acc, aov, p), f"{spec}: rt_denoise of the accumulated image")
    assert_same_bits(got_frame, reference(orc, frame, aov, p), f"{spec}: rt_denoise of the frame image")
    for layout in ("dense", "pre,arena,cache"):
        monkeypatch.setenv("RT_LAYOUT", layout)
        other = end_to_end(pkg, api, spec, w, h)[0]
        monkeypatch.delenv("RT_LAYOUT")
        assert_same_bits(other, got, f"{spec}: RT_LAYOUT={layout}")


_TORCH_CHILD = r"""
import os
import sys
import numpy as np
import torch
torch.cuda.set_device(0)
root = sys.argv[1]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import __graft_entry__ as graft
import aov_support as ga
pkg = graft.load_package()
api = pkg.load_library()
for layout in (None, "dense", "pre,arena,cache"):
    if layout:
        os.environ["RT_LAYOUT"] = layout
    for spec, w, h in (((3, {}), 80, 45), ("emitters", 64, 36)):
        tr = api.create_tracer(0)
        su = ga.Setup(pkg, api, tr, spec, w, h)
        su.mgr.RenderFrames(4)
        p = api.denoise_params(scale=0.25)
        host = tr.denoise(p, aov_frame=2)
        su.mgr.RenderFrames(3)  # frames in flight in front of the filter
        t = torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda:0")
        tr.denoise_to_device(t.data_ptr(), t.numel() * 4, p, aov_frame=2)
        tr.synchronize()
        host7 = tr.denoise(p, aov_frame=2)  # the same seven frames through the host variant
        assert t.cpu().numpy().tobytes() == host7.tobytes(), "tensor != host variant (%s, %s)" % (spec, layout)
        # rt_denoise_buffers on tensors: AOV records once per pose, then the filter per displayed frame
        acc = torch.from_numpy(tr.read_accumulated()).cuda()
        rec = torch.zeros((h, w, 16), dtype=torch.int32, device="cuda:0")
        out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        tr.render_aov_to_device(2, rec.data_ptr(), rec.numel() * 4)
        tr.denoise_buffers(w, h, acc.data_ptr(), rec.data_ptr(), out.data_ptr(), p)
        tr.synchronize()
        assert out.cpu().numpy().tobytes() == host7.tobytes(), "rt_denoise_buffers on tensors != rt_denoise (%s, %s)" % (spec, layout)
        # on the caller's stream (rt_set_stream): work enqueued on that stream behind the filter sees its pixels
        s = torch.cuda.Stream()
        tr.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            t2 = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
            s.synchronize()
            tr.denoise_to_device(t2.data_ptr(), t2.numel() * 4, p, aov_frame=2)
            first = t2.clone()
        s.synchronize()
        assert first.cpu().numpy().tobytes() == host7.tobytes(), "stream order (%s, %s)" % (spec, layout)
        tr.set_stream(None)
        tr.synchronize()
        if layout is None:
            np.save(os.path.join(sys.argv[2], "host_%dx%d.npy" % (w, h)), host)
        tr.close()
print("DENOISE_TORCH_OK")
"""


def test_device_variant_into_a_torch_tensor(pkg, api, tmp_path):
    """rt_denoise_to_device(tensor.data_ptr(), ...) == rt_denoise, rt_denoise_buffers on tensors == rt_denoise, and both in the order of a
    torch stream given to rt_set_stream, under every RT_LAYOUT.  In a child process that imports torch first, so that the library
    shares torch's HIP runtime; what the child's rt_denoise returned is compared with this process's."""
    p = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "DENOISE_TORCH_OK" in p.stdout, "rc=%d\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    for spec, w, h in E2E:
        assert_same_bits(np.load(tmp_path / f"host_{w}x{h}.npy"), end_to_end(pkg, api, spec, w, h)[0], f"{spec}: the child's rt_denoise")


# ---------------------------------------------------------------- 8. exact properties
def test_exact_properties_on_synthetic_buffers(pkg, api):
    w, h = 96, 40
    rgba, aov = ref.synthetic(pkg, w, h, seed=9)
    tr = api.create_tracer(0)
    try:
        hit = aov["object"] >= 0
        a = aov["object"] == 0
        two = rgba.copy()
        two[..., :3] = np.where(a[..., None], F([1, 0, 0]), F([0, 1, 0]))
        for demodulate in (0, 1):
            got, _ = filter_on_device(api, tr, two, aov, iterations=5, demodulate=demodulate, sigmaColour=100.0, sigmaNormal=100.0, sigmaPlane=100.0)
            assert a.any() and (hit & ~a).any()
            assert (got[..., 1][a] == 0).all(), "green crossed into object 0"
            assert (got[..., 0][hit & ~a] == 0).all(), "red crossed out of object 0"
            assert (got[..., 0][a] > 0).all()
        scale = F(0.375)
        scaled = rgba[..., :3] * scale
        unfiltered = ~hit | ~np.isfinite(rgba[..., :3]).all(axis=-1)
        assert (~hit).any() and (hit & unfiltered).any()
        for iterations in (1, 4):
            got, _ = filter_on_device(api, tr, rgba, aov, iterations=iterations, scale=float(scale))
            assert np.array_equal(got[..., :3].view(np.uint32)[unfiltered], scaled.view(np.uint32)[unfiltered])
            assert np.array_equal(got[..., 3].view(np.uint32), rgba[..., 3].view(np.uint32)), "alpha"
            assert (got[..., :3].view(np.uint32)[~unfiltered] != scaled.view(np.uint32)[~unfiltered]).any()
        for demodulate in (0, 1):
            got, _ = filter_on_device(api, tr, rgba, aov, iterations=0, demodulate=demodulate, scale=float(scale))
            assert np.array_equal(got[..., :3].view(np.uint32), scaled.view(np.uint32)) and np.array_equal(got[..., 3].view(np.uint32), rgba[..., 3].view(np.uint32))
    finally:
        tr.close()


# ---------------------------------------------------------------- 9. no visible state change
def test_denoise_calls_leave_no_trace(pkg, api, forced=False):
    cfg, w, h, seed = (3, {}), 96, 54, 5
    snaps = []
    for with_call in (True, False):
        tr = api.create_tracer(0)
        tr.enable_stats(True)
        su = ga.Setup(pkg, api, tr, cfg, w, h, seed=seed)
        mgr = su.mgr
        t, t2 = DevBuf(h * w * 16), DevBuf(h * w * 16)
        rec = DevBuf(h * w * 64)

        def probe(tag):
            if with_call:
                if tag.startswith("after held"):    # (rt_get_counters below launches held frames too: this filter comes first)
                    held_at(tr, "test_gpu_denoise: rt_denoise after held-back frames", forced)
                    met = tr.denoise(api.denoise_params(scale=1.0 / max(tr.frame() - 1, 1)), aov_frame=tr.frame())
                before = (tr.frame(), tr.counters())
                p = api.denoise_params(scale=1.0 / max(tr.frame() - 1, 1))
                a = tr.denoise(p, aov_frame=tr.frame())
                if tag.startswith("after held"):
                    assert met.tobytes() == a.tobytes(), tag
                tr.denoise_to_device(t.ptr, t.nbytes, p, aov_frame=tr.frame())
                tr.render_aov_to_device(tr.frame(), rec.ptr, rec.nbytes)
                tr.denoise_buffers(w, h, t.ptr, rec.ptr, t2.ptr, p)
                tr.denoise(p, use_accumulated=False, aov_frame=1)
                tr.synchronize()
                assert t.image(h, w).tobytes() == a.tobytes(), tag
                after = (tr.frame(), tr.counters())
                before[1].pop("gpuMs"), after[1].pop("gpuMs")
                assert before == after, tag
        mgr.RenderFrame()                       # frame 1
        probe("after rt_render_frame")
        mgr.RenderFrames(17)                    # frames 2-18: a fused launch, still running when the filter comes
        probe("after rt_render_frames(17)")
        for _ in range(3):                      # frames 19-21: rt_render_frame may hold them back (pending)
            mgr.RenderFrame()
        probe("after held-back frames")
        acc_mid, frame_mid = tr.read_accumulated(), tr.read_frame()
        mgr.RenderFrames(3)                     # the next RenderFrames(3) after the calls
        c = tr.counters()
        c.pop("gpuMs")
        snaps.append((acc_mid, frame_mid, tr.read_accumulated(), tr.read_frame(), tr.frame(), c))  # (the reads succeed: the watchdog word is clear)
        tr.close()
        for d in (t, t2, rec):
            d.free()
    a, b = snaps
    for k in range(4):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a[4] == b[4] == 25 and a[5] == b[5]


def test_denoise_calls_leave_no_trace_with_frames_held_back_for_certain(pkg, api, monkeypatch):
    """The same with RT_HOLD_BACK=1: frames 19-21 ARE held back when the filter comes (asserted right before it)."""
    monkeypatch.setenv("RT_HOLD_BACK", "1")
    test_denoise_calls_leave_no_trace(pkg, api, forced=True)


# ---------------------------------------------------------------- 10. errors
def test_errors(pkg, api):
    abi = pkg.abi
    w, h = 64, 36
    img = np.zeros((h, w, 4), dtype=F)
    d_in, d_out, d_aov = DevBuf(img.nbytes), DevBuf(img.nbytes), DevBuf(h * w * 64)
    ok = api.denoise_params()
    tr = api.create_tracer(0)

    def buffers(p=ok, ww=w, hh=h, a=None, b=None, c=None):
        return api.denoise_buffers(tr.h, C.byref(p) if p is not None else None, ww, hh, d_in.ptr if a is None else a, d_aov.ptr if b is None else b,
                                   d_out.ptr if c is None else c)

    def context_calls(p=ok, frame=1, nbytes=img.nbytes, host=img.ctypes.data, dev=None):
        pp = C.byref(p) if p is not None else None
        return (api.denoise(tr.h, pp, 1, frame, host, nbytes), api.denoise_to_device(tr.h, pp, 1, frame, d_out.ptr if dev is None else dev, nbytes))
    try:
        # the context calls need an image, a scene and parameters; rt_denoise_buffers needs none of them
        assert context_calls() == (abi.RT_ERR_STATE,) * 2  # before rt_resize
        assert buffers() == abi.RT_OK
        tr.resize(w, h)
        assert context_calls() == (abi.RT_ERR_STATE,) * 2  # before rt_upload_scene
        mgr = ga.scene_of(pkg, (3, {})).make_manager(tr, api, w, h)
        mgr.InitTexturesAndBuffers()
        mgr.InitBVH()
        assert context_calls() == (abi.RT_ERR_STATE,) * 2  # before rt_set_params
        tr.close()
        tr = api.create_tracer(0)
        ga.Setup(pkg, api, tr, (3, {}), w, h)
        bad = []
        for fields in (dict(iterations=-1), dict(iterations=9), dict(sigmaColour=0.0), dict(sigmaNormal=-1.0), dict(sigmaPlane=float("nan")),
                       dict(sigmaColour=float("inf")), dict(sigmaNormal=1e-23), dict(sigmaColour=5e-18, iterations=8), dict(scale=float("inf")), dict(scale=float("nan")), dict(reserved=1)):
            bad.append(api.denoise_params(**fields))
        for p in bad:
            assert buffers(p) == abi.RT_ERR_INVALID_ARG, bytes(p)
            assert context_calls(p) == (abi.RT_ERR_INVALID_ARG,) * 2, bytes(p)
        assert buffers(None) == abi.RT_ERR_INVALID_ARG and context_calls(None) == (abi.RT_ERR_INVALID_ARG,) * 2
        for size in (0, 28, 36):
            p = api.denoise_params(struct_size=size)
            assert buffers(p) == abi.RT_ERR_ABI_MISMATCH and context_calls(p) == (abi.RT_ERR_ABI_MISMATCH,) * 2
        # sizes and pointers
        assert buffers(ww=0) == abi.RT_ERR_INVALID_ARG and buffers(hh=0) == abi.RT_ERR_INVALID_ARG and buffers(ww=-4) == abi.RT_ERR_INVALID_ARG
        for which in "abc":
            assert buffers(**{which: 0}) == abi.RT_ERR_INVALID_ARG  # null
            assert buffers(**{which: d_in.ptr + 4}) == abi.RT_ERR_INVALID_ARG  # misaligned
            assert buffers(**{which: img.ctypes.data}) == abi.RT_ERR_INVALID_ARG  # host memory
        assert buffers(a=d_in.ptr + 16) == abi.RT_ERR_INVALID_ARG  # runs past the allocation
        assert buffers(c=d_in.ptr) == abi.RT_ERR_INVALID_ARG  # out == in
        assert buffers(hh=h // 2, c=d_in.ptr + (h // 4) * w * 16) == abi.RT_ERR_INVALID_ARG  # out overlaps in
        assert buffers(hh=h // 2, c=d_in.ptr + (h // 2) * w * 16) == abi.RT_OK  # adjacent halves of one allocation do not
        assert context_calls(frame=0) == (abi.RT_ERR_INVALID_ARG,) * 2 and context_calls(frame=-2) == (abi.RT_ERR_INVALID_ARG,) * 2
        assert context_calls(nbytes=img.nbytes - 16) == (abi.RT_ERR_INVALID_ARG,) * 2 and context_calls(nbytes=img.nbytes + 16) == (abi.RT_ERR_INVALID_ARG,) * 2
        assert api.denoise(tr.h, C.byref(ok), 1, 1, None, img.nbytes) == abi.RT_ERR_INVALID_ARG
        assert api.denoise_to_device(tr.h, C.byref(ok), 1, 1, None, img.nbytes) == abi.RT_ERR_INVALID_ARG
        assert api.denoise_to_device(tr.h, C.byref(ok), 1, 1, img.ctypes.data, img.nbytes) == abi.RT_ERR_INVALID_ARG  # host memory
        assert api.denoise_to_device(tr.h, C.byref(ok), 1, 1, d_out.ptr + 4, img.nbytes) == abi.RT_ERR_INVALID_ARG
        assert api.denoise_to_device(tr.h, C.byref(ok), 1, 1, d_out.ptr + 16, img.nbytes) == abi.RT_ERR_INVALID_ARG  # runs past the allocation
        frame_ptr, accum_ptr = tr.render_targets()
        assert api.denoise_to_device(tr.h, C.byref(ok), 1, 1, accum_ptr, img.nbytes) == abi.RT_ERR_INVALID_ARG  # the source image itself
        assert context_calls() == (abi.RT_OK,) * 2 and buffers() == abi.RT_OK
        tr.synchronize()
        tr.close()
        # a context that owns part of the image
        tr = api.create_tracer(0)
        tr.set_partition(8, 0, 2)
        ga.Setup(pkg, api, tr, (3, {}), w, h)
        rows = tr.local_rows()
        assert 0 < rows < h
        assert api.denoise(tr.h, C.byref(ok), 1, 1, img.ctypes.data, rows * w * 16) == abi.RT_ERR_STATE
        assert api.denoise_to_device(tr.h, C.byref(ok), 1, 1, d_out.ptr, rows * w * 16) == abi.RT_ERR_STATE
        assert buffers() == abi.RT_ERR_STATE
        assert b"part" in api.last_error(tr.h)
        tr.set_partition(8, 0, 1)  # the whole image again
        assert context_calls() == (abi.RT_OK,) * 2
        tr.synchronize()
    finally:
        tr.close()
        for d in (d_in, d_out, d_aov):
            d.free()


def test_watchdog_of_the_internal_aov_pass_is_reported_like_the_aov_calls(pkg, api, monkeypatch):
    """RT_TRAV_LIMIT=4 (read at rt_upload_scene; the step limit is a software counter, nothing can hang): the internal pass's walks are
    cut short.  rt_denoise says so when it returns, rt_denoise_to_device at the next rt_synchronize, once; the context is untouched."""
    tr = api.create_tracer(0)
    t = DevBuf(36 * 64 * 16)
    try:
        monkeypatch.setenv("RT_TRAV_LIMIT", "4")
        ga.Setup(pkg, api, tr, (3, {}), 64, 36)
        monkeypatch.delenv("RT_TRAV_LIMIT")
        with pytest.raises(pkg.abi.RtError) as e:
            tr.denoise()
        assert e.value.status == pkg.abi.RT_ERR_HIP and "watchdog" in str(e.value), str(e.value)
        tr.denoise_to_device(t.ptr, t.nbytes)  # enqueued: RT_OK
        with pytest.raises(pkg.abi.RtError) as e:
            tr.synchronize()
        assert e.value.status == pkg.abi.RT_ERR_HIP and "watchdog" in str(e.value), str(e.value)
        tr.synchronize()  # reported once
        c = tr.counters()  # RT_OK: the context's watchdog word was not set
        assert c["segments"] == 0
        assert not tr.read_accumulated().any()
        assert tr.frame() == 1
    finally:
        tr.close()
        t.free()


def test_a_set_watchdog_word_stays_as_it_is(pkg, api, monkeypatch):
    """The context's watchdog word, read explicitly: every read of a context whose word is set fails with a message that holds the
    word's value ("fired N times").  After frames rendered under RT_TRAV_LIMIT=4 (as tests/test_gpu_watchdog.py sets it), the three
    filter calls leave that message — the word — exactly as it was; that a clear word stays clear is test_denoise_calls_leave_no_trace."""
    w, h = 64, 36
    tr = api.create_tracer(0)
    t, t2, rec = DevBuf(h * w * 16), DevBuf(h * w * 16), DevBuf(h * w * 64)
    try:
        monkeypatch.setenv("RT_TRAV_LIMIT", "4")
        su = ga.Setup(pkg, api, tr, (3, {}), w, h)
        monkeypatch.delenv("RT_TRAV_LIMIT")
        su.mgr.RenderFrames(2)

        def word():
            with pytest.raises(pkg.abi.RtError) as e:
                tr.read_accumulated()
            assert "fired" in str(e.value) and "rt_reset_accumulation" in str(e.value), str(e.value)
            return str(e.value)
        before = word()
        with pytest.raises(pkg.abi.RtError):
            tr.denoise()  # (its own AOV pass is cut short too)
        tr.denoise_to_device(t.ptr, t.nbytes)
        with pytest.raises(pkg.abi.RtError):
            tr.synchronize()
        tr.denoise_buffers(w, h, t.ptr, rec.ptr, t2.ptr)
        tr.synchronize()
        assert word() == before
        assert tr.frame() == 3
    finally:
        tr.close()
        for d in (t, t2, rec):
            d.free()


# ---------------------------------------------------------------- 11. it denoises
def test_it_denoises(pkg, api):
    """Config 3 at 320 x 180 (sky, diffuse-dominated).  G: the accumulated mean of 1,024 frames; N: the mean of frames 1 ... 4;
    D = denoise(N) with the default parameters.  Over the pixels that are not misses, mse(D, G) < mse(N, G).
    Measured on an MI355X with the defaults (5 iterations, sigma 4 / 0.25 / 0.1, demodulation on), the only set tried:
    mse(N, G) = 0.16251, mse(D, G) = 0.036233, ratio 0.223 over 57,600 hit pixels (profiles/r07_denoise.txt)."""
    w, h = 320, 180

    def run(frames, denoise):
        tr = api.create_tracer(0)
        try:
            su = ga.Setup(pkg, api, tr, (3, {}), w, h)
            su.mgr.RenderFrames(frames)
            mean = tr.read_accumulated()[..., :3].astype(np.float64) / frames
            if not denoise:
                return mean
            return mean, tr.denoise(api.denoise_params(scale=1.0 / frames), aov_frame=1)[..., :3].astype(np.float64), tr.render_aov(1)
        finally:
            tr.close()
    truth = run(1024, False)
    noisy, filtered, aov = run(4, True)
    hit = aov["object"] >= 0
    assert hit.mean() > 0.2
    mse_n = float(((noisy - truth)[hit] ** 2).mean())
    mse_d = float(((filtered - truth)[hit] ** 2).mean())
    print(f"rt_denoise defaults: mse(noisy, truth) = {mse_n:.6g}, mse(denoised, truth) = {mse_d:.6g}, ratio = {mse_d / mse_n:.4f} over {int(hit.sum())} hit pixels")
    assert np.isfinite(mse_d) and mse_d < mse_n
