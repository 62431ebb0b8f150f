"""What a caller is told after a kernel watchdog fired.

Both watchdogs (rt_kernels.h: traverse's step limit, pool_exchange's spin limit) add to word 7 of counter slot 0, and the
images rendered since are wrong by design: walks were cut short, or chains dropped.  Every path that hands pixels to a
caller must then fail — rt_read_*, rt_display*, the multi-context gathers, rt_gather_rccl, rt_get_counters — and
rt_reset_counters must not hide it.  Only rt_reset_accumulation, rt_write_accumulated and rt_resize clear it, and what is
rendered after them is exact again.

The watchdog is tripped only through RT_TRAV_LIMIT=4, which rt_upload_scene reads: walks end sooner, nothing can hang.  The
limit is set around the upload alone, so a context stays tripped until its scene is uploaded again.  Every image that should
be valid is compared bit for bit with the CPU oracle driven through the same calls."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import render

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG, W, H, SEED = 3, 64, 36, 2
NBYTES = W * H * 16

# every single-context path that hands pixels to the host (tr, manager) -> image
READS = {
    "read_frame": lambda tr, m: tr.read_frame(),
    "read_accumulated": lambda tr, m: tr.read_accumulated(),
    "display_accumulated": lambda tr, m: tr.display(m.numAccumulatedFrames, use_accumulated=True),
    "display_frame": lambda tr, m: tr.display(1, use_accumulated=False),
    "srgb8_flip": lambda tr, m: tr.display_srgb8(m.numAccumulatedFrames, use_accumulated=True, flip_y=True),
    "srgb8_no_flip": lambda tr, m: tr.display_srgb8(m.numAccumulatedFrames, use_accumulated=True, flip_y=False),
    "srgb8_frame": lambda tr, m: tr.display_srgb8(1, use_accumulated=False, flip_y=True),
}


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def expect_watchdog(pkg, fn, *args, **kw):
    with pytest.raises(pkg.abi.RtError) as e:
        fn(*args, **kw)
    assert "watchdog" in str(e.value), str(e.value)
    return str(e.value)


def every_read_fails(pkg, tr, mgr):
    for name, read in READS.items():
        expect_watchdog(pkg, read, tr, mgr)
    expect_watchdog(pkg, tr.counters)


def every_read(tr, mgr):
    return {name: read(tr, mgr) for name, read in READS.items()}


def assert_reads_equal(got, want):
    for name in READS:
        assert same(got[name], want[name]), name


def tripped(pkg, api, monkeypatch, tracer, frames=2, bind=None):
    """OnEnable with the traversal limit forced to 4 (read at the upload), then `frames` frames: the watchdog fires.  bind =
    (frame, accum) device pointers to render into instead of the library's own targets."""
    monkeypatch.setenv("RT_TRAV_LIMIT", "4")
    mgr = pkg.scenes.get(CFG).make_manager(tracer, api, W, H)
    mgr.OnEnable(renderSeed=SEED)
    monkeypatch.delenv("RT_TRAV_LIMIT")
    if bind:
        tracer.bind_render_targets(*bind)
        tracer.reset_accumulation()
    mgr.RenderFrames(frames)
    return mgr


def clean(pkg, api, tracer, frames=2, bind=None):
    mgr = pkg.scenes.get(CFG).make_manager(tracer, api, W, H)
    mgr.OnEnable(renderSeed=SEED)
    if bind:
        tracer.bind_render_targets(*bind)
        tracer.reset_accumulation()
    mgr.RenderFrames(frames)
    return mgr


def upload_clean(mgr):
    """Upload the scene again without RT_TRAV_LIMIT: the context's own limit is back."""
    mgr.hasBVH = False
    mgr.InitFrame()


def on_oracle(pkg, orc, drive=None, frames=2):
    """The oracle through the manager: OnEnable, `frames` frames, then drive(tracer, manager); every read path's image."""
    tr = orc.create_tracer(8)
    mgr = pkg.scenes.get(CFG).make_manager(tr, orc, W, H)
    mgr.OnEnable(renderSeed=SEED)
    mgr.RenderFrames(frames)
    if drive:
        drive(tr, mgr)
    out = every_read(tr, mgr)
    tr.close()
    return out


class DeviceBuffers:
    """hipMalloc'd buffers through the HIP runtime the library already loaded (see test_gather_into_device_memory_*)."""

    def __init__(self, n, nbytes=NBYTES, device=0):
        self.hip = C.CDLL("libamdhip64.so")
        self.nbytes = nbytes
        self.ptrs = []
        assert self.hip.hipSetDevice(C.c_int(device)) == 0
        for _ in range(n):
            d = C.c_void_p()
            assert self.hip.hipMalloc(C.byref(d), C.c_size_t(nbytes)) == 0
            self.ptrs.append(d.value)

    def host(self, i):
        out = np.empty((H, W, 4), dtype=np.float32)
        assert self.hip.hipDeviceSynchronize() == 0
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(self.ptrs[i]), C.c_size_t(self.nbytes), C.c_int(2)) == 0
        return out

    def fill(self, i, byte):
        assert self.hip.hipMemset(C.c_void_p(self.ptrs[i]), C.c_int(byte), C.c_size_t(self.nbytes)) == 0
        assert self.hip.hipDeviceSynchronize() == 0

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(C.c_void_p(p))
        self.ptrs = []


# ---------------------------------------------------------------------------------------------------- one context
@pytest.mark.parametrize("targets", ["owned", "bound"])
def test_every_read_path_fails_after_a_watchdog_fired(pkg, api, monkeypatch, targets):
    """read_frame, read_accumulated, display (accumulated / frame), display_srgb8 (both flips, frame) and counters all raise —
    on the library's own targets and on caller-owned targets bound with rt_bind_render_targets (whose direct readers have
    rt_get_counters to ask)."""
    bufs = DeviceBuffers(2) if targets == "bound" else None
    try:
        tr = api.create_tracer(0)
        mgr = tripped(pkg, api, monkeypatch, tr, bind=bufs.ptrs if bufs else None)
        every_read_fails(pkg, tr, mgr)
        every_read_fails(pkg, tr, mgr)          # asking does not clear it
        tr.close()
    finally:
        if bufs:
            bufs.free()


@pytest.mark.parametrize("targets", ["owned", "bound"])
def test_a_clean_render_reads_the_oracle_bits_through_every_path(pkg, api, orc, targets):
    """No false alarm: without a fire, every read path returns OK and the oracle's bits; bound targets hold the same bits."""
    bufs = DeviceBuffers(2) if targets == "bound" else None
    try:
        tr = api.create_tracer(0)
        mgr = clean(pkg, api, tr, bind=bufs.ptrs if bufs else None)
        got = every_read(tr, mgr)
        assert tr.counters()["segments"] > 0
        if bufs:
            assert same(bufs.host(0), got["read_frame"]) and same(bufs.host(1), got["read_accumulated"])
        tr.close()
    finally:
        if bufs:
            bufs.free()
    assert np.all(got["read_accumulated"][..., 3] == 2)
    assert_reads_equal(got, on_oracle(pkg, orc))


def test_reset_counters_does_not_clear_the_watchdog(pkg, api, monkeypatch):
    """fire, rt_reset_counters, a clean upload, 2 more frames: the accumulated image still holds the truncated frames, so
    counters() and read_accumulated() still raise (bench.py resets the counters between its regions)."""
    tr = api.create_tracer(0)
    mgr = tripped(pkg, api, monkeypatch, tr)
    tr.reset_counters()
    upload_clean(mgr)
    mgr.RenderFrames(2)
    expect_watchdog(pkg, tr.counters)
    expect_watchdog(pkg, tr.read_accumulated)
    expect_watchdog(pkg, tr.display_srgb8, mgr.numAccumulatedFrames)
    tr.close()


def test_reset_accumulation_clears_the_watchdog_and_what_follows_is_exact(pkg, api, orc, monkeypatch):
    tr = api.create_tracer(0)
    mgr = tripped(pkg, api, monkeypatch, tr)
    upload_clean(mgr)
    mgr.ResetAccumulatedRender()
    mgr.RenderFrames(3)
    got = every_read(tr, mgr)
    assert tr.counters()["segments"] > 0
    tr.close()
    want = on_oracle(pkg, orc, lambda t, m: (m.ResetAccumulatedRender(), m.RenderFrames(3)))
    assert_reads_equal(got, want)


def test_write_accumulated_clears_the_watchdog_and_resumes_exactly(pkg, api, orc, monkeypatch, tmp_path):
    """A checkpoint of a clean 2-frame run written into a tripped context, 3 more frames: == the straight 5-frame run."""
    t1 = api.create_tracer(0)
    _, m1 = render(pkg, api, t1, CFG, W, H, 2, seed=SEED)
    ck = str(tmp_path / "ck.npz")
    pkg.display.save_checkpoint(ck, m1)
    t1.close()
    tr = api.create_tracer(0)
    mgr = tripped(pkg, api, monkeypatch, tr)
    mgr.hasBVH = False                          # load_checkpoint's InitFrame uploads the scene clean
    pkg.display.load_checkpoint(ck, mgr)
    mgr.RenderFrames(3)
    got = every_read(tr, mgr)
    assert tr.counters()["segments"] > 0
    tr.close()
    assert_reads_equal(got, on_oracle(pkg, orc, frames=5))


def test_resize_clears_the_watchdog(pkg, api, orc, monkeypatch):
    """rt_resize gives the context new, zeroed targets: reads succeed at once, and frames rendered after a clean upload
    equal the oracle's run of the same calls."""
    tr = api.create_tracer(0)
    mgr = tripped(pkg, api, monkeypatch, tr)
    tr.resize(W, H)
    assert not np.any(tr.read_accumulated())
    assert tr.counters()["segments"] > 0
    upload_clean(mgr)
    mgr.RenderFrames(2)
    got = every_read(tr, mgr)
    tr.close()
    assert_reads_equal(got, on_oracle(pkg, orc, lambda t, m: (t.resize(W, H), m.RenderFrames(2))))


def test_the_watchdog_belongs_to_the_context_that_tripped_it(pkg, api, orc, monkeypatch):
    """A tripped and a clean context on one device, driven in turn: the clean one reads the oracle's bits, the tripped one fails."""
    bad = api.create_tracer(0)
    mb = tripped(pkg, api, monkeypatch, bad, frames=1)
    good = api.create_tracer(0)
    mg = clean(pkg, api, good, frames=1)
    mb.RenderFrames(1)
    assert same(good.read_frame(), on_oracle(pkg, orc, frames=1)["read_frame"])
    every_read_fails(pkg, bad, mb)
    mg.RenderFrames(1)
    mb.RenderFrames(1)
    got = every_read(good, mg)
    assert good.counters()["segments"] > 0
    every_read_fails(pkg, bad, mb)
    bad.close()
    good.close()
    assert_reads_equal(got, on_oracle(pkg, orc, frames=2))


# ---------------------------------------------------------------------------------------------------- several contexts
def _multi_fails(pkg, multi, bufs):
    expect_watchdog(pkg, multi.read_accumulated)
    expect_watchdog(pkg, multi.read_frame)
    for root in (0, 1):
        expect_watchdog(pkg, multi.gather_accumulated_to_device, root, bufs.ptrs[0], NBYTES)
        expect_watchdog(pkg, multi.gather_frame_to_device, root, bufs.ptrs[0], NBYTES)
    expect_watchdog(pkg, multi.counters)


@pytest.mark.parametrize("which", ["both", "second"])
def test_multi_context_gathers_fail_after_a_watchdog_fired(pkg, api, orc, monkeypatch, which):
    """rt_create_multi([0, 0]): with both contexts tripped, or only context 1 (its scene uploaded again under the forced limit),
    rt_gather_accumulated / _frame, both _to_device gathers and rt_multi_get_counters fail.  A clean multi-context made after
    that gathers the oracle's bits on the host and into device memory."""
    bufs = DeviceBuffers(1)
    try:
        if which == "both":
            monkeypatch.setenv("RT_TRAV_LIMIT", "4")
        multi = api.create_multi_tracer([0, 0])
        mgr = pkg.scenes.get(CFG).make_manager(multi, api, W, H)
        mgr.OnEnable(renderSeed=SEED)
        if which == "second":
            monkeypatch.setenv("RT_TRAV_LIMIT", "4")
            data = mgr.CreateAllMeshData(mgr.models)
            multi.context(1).upload_scene(data["meshInfo"], data["triangles"], data["nodes"], mgr._pack_spheres())
        monkeypatch.delenv("RT_TRAV_LIMIT")
        mgr.RenderFrames(2)
        _multi_fails(pkg, multi, bufs)
        if which == "second":
            c0 = multi.context(0)
            assert c0.counters()["segments"] > 0          # context 0 itself is clean
            expect_watchdog(pkg, multi.context(1).counters)
        multi.close()

        multi = api.create_multi_tracer([0, 0])
        mgr = clean(pkg, api, multi)
        got = {"read_accumulated": multi.read_accumulated(), "read_frame": multi.read_frame()}
        assert multi.counters()["segments"] > 0
        want = on_oracle(pkg, orc)
        for name in got:
            assert same(got[name], want[name]), name
        for root in (0, 1):
            for gather, name in ((multi.gather_accumulated_to_device, "read_accumulated"), (multi.gather_frame_to_device, "read_frame")):
                bufs.fill(0, 0xff)
                gather(root, bufs.ptrs[0], NBYTES)
                assert same(bufs.host(0), want[name]), (root, name)
        multi.close()
    finally:
        bufs.free()


# ---------------------------------------------------------------------------------------------------- RCCL
# The RCCL cases run in a child process: loading librccl here, before test_zz_dist_gpu.py imports torch (which brings its own
# RCCL), would leave two RCCL builds in the test process.  The child renders, gathers with one host thread per rank, and
# reports each rank's outcome and the root's images; the parent checks them against the oracle.
_RCCL_CHILD = r"""
import ctypes as C, json, os, sys, threading
import numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as g
pkg = g.load_package()
api = pkg.load_library()
devices = [int(v) for v in sys.argv[2].split(",")]
tripped = [int(v) for v in sys.argv[3].split(",")]
CFG, W, H, SEED = (int(v) for v in sys.argv[5].split(","))
NBYTES = W * H * 16
n = len(devices)
hip = C.CDLL("libamdhip64.so")
rccl = C.CDLL("librccl.so.1")
comms = (C.c_void_p * n)()
assert rccl.ncclCommInitAll(comms, n, (C.c_int * n)(*devices)) == 0
assert hip.hipSetDevice(C.c_int(devices[0])) == 0
d = C.c_void_p()
assert hip.hipMalloc(C.byref(d), C.c_size_t(NBYTES)) == 0
trs = []
for r in range(n):
    tr = api.create_tracer(devices[r])
    tr.set_partition(8, r, n)
    if tripped[r]:
        os.environ["RT_TRAV_LIMIT"] = "4"
    mgr = pkg.scenes.get(CFG).make_manager(tr, api, W, H)
    mgr.OnEnable(renderSeed=SEED)
    os.environ.pop("RT_TRAV_LIMIT", None)
    mgr.RenderFrames(2)
    trs.append(tr)
result, images = {}, {}
for name, acc in (("read_accumulated", True), ("read_frame", False)):
    assert hip.hipSetDevice(C.c_int(devices[0])) == 0
    assert hip.hipMemset(d, C.c_int(0xff), C.c_size_t(NBYTES)) == 0 and hip.hipDeviceSynchronize() == 0
    got = ["no return"] * n
    def gather(r):
        try:
            trs[r].gather_rccl(comms[r], 0, d.value if r == 0 else None, NBYTES if r == 0 else 0, accumulated=acc)
            got[r] = "ok"
        except pkg.abi.RtError as e:
            got[r] = str(e)
    threads = [threading.Thread(target=gather, args=(r,)) for r in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    result[name] = got
    host = np.empty((H, W, 4), dtype=np.float32)
    assert hip.hipSetDevice(C.c_int(devices[0])) == 0 and hip.hipDeviceSynchronize() == 0
    assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), d, C.c_size_t(NBYTES), C.c_int(2)) == 0
    images[name] = host
for tr in trs:
    tr.close()
for i in range(n):
    rccl.ncclCommDestroy(C.c_void_p(comms[i]))
hip.hipFree(d)
np.savez(sys.argv[4], **images)
print("RESULT " + json.dumps(result))
"""


def _gpu_count():
    n = C.c_int(0)
    return n.value if C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(n)) == 0 else 0


def _rccl_gather(tmp_path, devices, tripped):
    """Per rank, the outcome of rt_gather_rccl (root 0) for both images ("ok" or the error), and the root's two images."""
    out = str(tmp_path / ("rccl_%s_%s.npz" % ("".join(map(str, devices)), "".join(map(str, tripped)))))
    p = subprocess.run([sys.executable, "-c", _RCCL_CHILD, ROOT, ",".join(map(str, devices)), ",".join(map(str, tripped)), out,
                        "%d,%d,%d,%d" % (CFG, W, H, SEED)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, "rc=%d\n%s\n%s" % (p.returncode, p.stdout[-4000:], p.stderr[-4000:])
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    z = np.load(out)
    return json.loads(line[len("RESULT "):]), {k: z[k] for k in z.files}


def test_rccl_gather_fails_after_a_watchdog_fired_on_a_one_rank_communicator(pkg, api, orc, tmp_path):
    """rt_gather_rccl over a one-rank communicator (as test_gather_over_a_caller_owned_rccl_communicator): a tripped context's
    gather fails, for either image; a clean context's gather is the oracle's image."""
    result, _ = _rccl_gather(tmp_path, [0], [1])
    for name in ("read_accumulated", "read_frame"):
        assert "watchdog" in result[name][0], result
    result, images = _rccl_gather(tmp_path, [0], [0])
    want = on_oracle(pkg, orc)
    for name in ("read_accumulated", "read_frame"):
        assert result[name] == ["ok"], result
        assert same(images[name], want[name]), name


def test_rccl_gather_root_fails_when_another_rank_tripped(pkg, api, orc, tmp_path):
    """Two ranks (devices 0 and 1), only rank 1 tripped: rank 1 still sends its tile and fails on its own word; the root learns
    of it through the exchange and fails too.  Both clean: the root gathers the oracle's image.  Needs two GPUs — RCCL refuses
    two ranks on one device — so on a one-GPU machine this case is skipped and only the one-rank test above runs."""
    if _gpu_count() < 2:
        pytest.skip("one GPU: the two-rank rt_gather_rccl case needs a second device")
    result, _ = _rccl_gather(tmp_path, [0, 1], [0, 1])
    for name in ("read_accumulated", "read_frame"):
        root, other = result[name]
        assert "watchdog" in root and "rank 1" in root, result
        assert "watchdog" in other, result
    result, images = _rccl_gather(tmp_path, [0, 1], [0, 0])
    want = on_oracle(pkg, orc)
    for name in ("read_accumulated", "read_frame"):
        assert result[name] == ["ok", "ok"], result
        assert same(images[name], want[name]), name
