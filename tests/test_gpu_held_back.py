"""Every entry point that takes a context, called with three frames held back (tests/flush_table.py is the list).

rt_render_frame holds a frame back while the GPU is busy and launches the held frames later, fused, with the state the context has THEN;
whether it holds one back is a race between the caller and a kernel of a few dozen microseconds.  RT_HOLD_BACK=1 (a test hook read by
rt_create) makes the context answer "busy" every time, and rt_debug_pending_frames shows how many frames are held, so each case here IS
the held-back path and says so with an assertion:

    create, upload, parameters, resize; two frames and a synchronise; three rt_render_frame calls -> pending == 3, rt_get_frame == 6;
    the call under test, once, with valid arguments that change something observable where the call can;
    pending == 0 (flushes), 3 (leaves) or 4 (holds); two more rt_render_frame calls; rt_read_accumulated -> pending == 0.

Compared bit for bit, no tolerance: the accumulated image, the last frame, segments, pixelFrames and rt_get_frame at the end with the CPU
oracle driven through the same logical sequence frame by frame (the oracle holds nothing back), and what the call itself hands back — and
the final state again — with the same sequence on an eager twin context (RT_COALESCE=0, the mode the other suites pin to their
references).  A flush that is missing, or that comes after the state change, renders the held frames with the new state, loses them from
a snapshot, or sends them to the wrong target: each shows as a different bit.

64 x 40 pixels, two scenes: config 2 (FLAT: no trees, within the caps, so the table of origin constants and the per-tile candidate
tables are on) and config 3 (BVH) with one sphere added; two rays per pixel, four bounces.  Multi rows run on two contexts on device 0."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import flush_table as ft
from held_back_support import Case, Side, run_modes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = (2, 3)


# ---------------------------------------------------------------- the scenes, and one side of a comparison
class OracleSide(Side):
    def __init__(self, pkg, orc, cfg):
        super().__init__(pkg, orc, cfg)
        self.fresh()

    def fresh(self):
        if getattr(self, "tr", None) is not None:
            self.tr.close()
        self.tr = self.lib.create_tracer(8)
        self.setup()

    def frame(self):
        return self.tr.frame()

    def close(self):
        self.tr.close()


_ORACLE = {}


def drive_oracle(pkg, orc, cfg, step):
    """the same logical sequence, frame by frame, on the oracle; one run per (scene, step), shared by the rows that make that step"""
    key = (cfg, step)
    if key not in _ORACLE:
        o = OracleSide(pkg, orc, cfg)
        o.frames(2, one_by_one=False)
        o.frames(3)
        ret = step(o) if step else None
        o.frames(2)
        c = ft.counters_of(o)
        _ORACLE[key] = {"ret": ret or {}, "accumulated": o.tr.read_accumulated().copy(), "frame": o.tr.read_frame().copy(),
                        "counters": {"segments": c["segments"], "pixelFrames": c["pixelFrames"]}, "get_frame": o.tr.frame()}
        o.close()
    return _ORACLE[key]


def differs(a, b):
    """'' when a and b are the same bits, else where they differ"""
    if isinstance(a, dict) or isinstance(b, dict):
        if not (isinstance(a, dict) and isinstance(b, dict)) or sorted(a) != sorted(b):
            return f"keys {a!r} / {b!r}"
        return next((f"[{k!r}] {d}" for k in a for d in [differs(a[k], b[k])] if d), "")
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.shape != b.shape or a.dtype != b.dtype:
            return f"shape / type {a.shape} {a.dtype} / {b.shape} {b.dtype}"
        if a.tobytes() == b.tobytes():
            return ""
        ab, bb = np.frombuffer(a.tobytes(), np.uint8), np.frombuffer(b.tobytes(), np.uint8)
        return f"{int((ab != bb).sum())} of {ab.size} bytes differ, the first at byte {int(np.argmax(ab != bb))}"
    return "" if a == b else f"{a!r} != {b!r}"


def compare(row, held, eager, want):
    # the call's own results and the state at the end: the eager twin's
    for k in ("ret", "accumulated", "frame", "counters", "get_frame"):
        d = differs(held[k], eager[k])
        assert not d, f"{row.id}: {k} differs from the eager twin's: {d}"
    # ... and the oracle's, where the oracle has the call
    common = {k: v for k, v in held["ret"].items() if k in want["ret"]}
    d = differs(common, {k: _rows(want["ret"][k], held, k) for k in common})
    assert not d, f"{row.id}: what the call returned differs from the oracle's: {d}"
    if row.oracle_final:
        for k in ("accumulated", "frame"):
            d = differs(held[k], _rows(want[k], held))
            assert not d, f"{row.id}: {k} at the end differs from the oracle's: {d}"
        assert held["get_frame"] == want["get_frame"]
        if row.oracle_counters:
            assert {k: held["counters"][k] for k in want["counters"]} == want["counters"]


def _rows(image, held, key=None):
    """the oracle renders the whole image; a context with a partition holds its rows only"""
    if held["rows"] is None or key is not None or not isinstance(image, np.ndarray):
        return image
    return image[held["rows"]]


# ---------------------------------------------------------------- one test per row and scene
@pytest.fixture(scope="module", autouse=True)
def wall_time_report():
    """what the cases of this file took, slowest first (pytest -s shows it)"""
    yield
    if ELAPSED:
        print(f"\n[held back] {len(ELAPSED)} cases, {sum(ELAPSED.values()):.1f} s in all; slowest: " +
              ", ".join(f"{k} {v:.2f} s" for k, v in sorted(ELAPSED.items(), key=lambda kv: -kv[1])[:8]))


IN_PROCESS = [r for r in ft.ROWS if not r.child]
CHILD = [r for r in ft.ROWS if r.child]
ELAPSED = {}


@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: f"config{c}")
@pytest.mark.parametrize("row", IN_PROCESS, ids=lambda r: r.id)
def test_call_with_three_frames_held_back(pkg, api, orc, monkeypatch, row, cfg):
    t0 = time.perf_counter()
    out = run_modes(pkg, api, cfg, row, monkeypatch)
    compare(row, out["held"], out["eager"], drive_oracle(pkg, orc, cfg, row.oracle))
    ELAPSED[f"{row.id}-config{cfg}"] = time.perf_counter() - t0


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import held_back_support as t
t.child_main(sys.argv[2], int(sys.argv[3]), sys.argv[4])
"""


@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: f"config{c}")
@pytest.mark.parametrize("row", CHILD, ids=lambda r: r.id)
def test_call_with_three_frames_held_back_in_a_child_process(pkg, api, orc, tmp_path, row, cfg):
    t0 = time.perf_counter()
    path = str(tmp_path / "out.npz")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, row.id, str(cfg), path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "rc=%d\n%s\n%s" % (p.returncode, p.stdout[-4000:], p.stderr[-4000:])
    scalars = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    z = np.load(path)
    out = {}
    for mode in ("held", "eager"):
        out[mode] = dict(scalars[mode], rows=None, accumulated=z[f"{mode}.accumulated"], frame=z[f"{mode}.frame"],
                         ret={k[len(mode) + 5:]: z[k] for k in z.files if k.startswith(f"{mode}.ret.")})
    compare(row, out["held"], out["eager"], drive_oracle(pkg, orc, cfg, row.oracle))
    ELAPSED[f"{row.id}-config{cfg}"] = time.perf_counter() - t0


def test_every_row_has_a_test_id_per_scene():
    assert len({r.id for r in ft.ROWS}) == len(ft.ROWS) == len(IN_PROCESS) + len(CHILD)


# ---------------------------------------------------------------- the cap, and the hook itself
def oracle_image(pkg, orc, cfg, n):
    o = OracleSide(pkg, orc, cfg)
    o.frames(n)
    out = o.tr.read_accumulated().copy(), o.tr.read_frame().copy()
    o.close()
    return out


@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: f"config{c}")
def test_a_pinned_cap_launches_every_fifth_frame(pkg, api, orc, monkeypatch, cfg):
    """RT_FUSE_CAP=5: the fifth held frame launches all five"""
    c = Case(pkg, api, cfg, "held", False, monkeypatch, {"RT_FUSE_CAP": "5"})
    try:
        seen = []
        for _ in range(12):
            c.frames(1)
            seen.append(c.pending())
        assert seen == [1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2] and c.frame() == 13
        acc, frame = oracle_image(pkg, orc, cfg, 12)
        assert not differs(c.tr.read_accumulated(), acc) and not differs(c.tr.read_frame(), frame) and c.pending() == 0
    finally:
        c.close()


def test_the_default_cap_launches_the_sixteenth_frame(pkg, api, orc, monkeypatch):
    c = Case(pkg, api, 3, "held", False, monkeypatch)
    try:
        assert c.tr.fused_frames_cap() == 16
        seen = []
        for _ in range(17):
            c.frames(1)
            seen.append(c.pending())
        assert seen == list(range(1, 16)) + [0, 1]
        acc, frame = oracle_image(pkg, orc, 3, 17)
        assert not differs(c.tr.read_accumulated(), acc) and not differs(c.tr.read_frame(), frame)
    finally:
        c.close()


def test_without_the_hook_an_idle_context_holds_nothing_back(pkg, api, monkeypatch):
    """so the hook is the only thing that forces the hold in the cases above"""
    c = Case(pkg, api, 3, "plain", False, monkeypatch)
    try:
        for _ in range(3):
            c.tr.synchronize()
            c.frames(1)
            assert c.pending() == 0
        assert c.frame() == 4
    finally:
        c.close()


def test_the_hook_holds_nothing_back_that_is_not_eligible(pkg, api, monkeypatch):
    """RT_HOLD_BACK changes the answer to "is the GPU idle" and nothing else: with RT_COALESCE=0 every frame still launches at once"""
    c = Case(pkg, api, 2, "held", False, monkeypatch, {"RT_COALESCE": "0"})
    try:
        for _ in range(3):
            c.frames(1)
            assert c.pending() == 0
    finally:
        c.close()


def test_multi_accessor_reports_the_largest_count(pkg, api, monkeypatch):
    """context 1 alone renders two frames more: the multi accessor follows it, and the forwarded calls empty both"""
    c = Case(pkg, api, 3, "held", True, monkeypatch)
    try:
        c.frames(3)
        one = c.tr.context(1)
        one.render_frame()
        one.render_frame()
        assert [c.tr.context(i).pending_frames() for i in range(2)] == [3, 5] and c.pending() == 5
        c.tr.synchronize()
        assert [c.tr.context(i).pending_frames() for i in range(2)] == [0, 0] and c.pending() == 0
    finally:
        c.close()


def test_null_handles(api):
    assert api.debug_pending_frames(None) == -1 and api.debug_multi_pending_frames(None) == -1
