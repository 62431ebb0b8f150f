"""Seeded scenes within the caps of the FLAT trace kernel's three tables — the per-launch origin constants (rt_primary.h), the per-tile
sphere masks and the per-tile triangle masks (rt_tile_cand.h) — on the GPU, and one context walked through the calls whose arguments are
part of the TileCandKey.

tests/capfuzz_scenes.py makes the scenes; tests/test_tile_fuzz.py runs the same scenes through the host drivers and asserts what the
family reaches (cleared bits, empty triangle masks, every count and split).  What exists only on the device is what these tests are
for: the fill kernel's masks as the trace kernel reads them, the union of the lanes' triangle masks in begin_intersect, the tk / pr
bookkeeping of traverse_flat when whole models are skipped, the `tile` word of a chain that changed lanes in the pool, and the host's
bytewise key compare that decides when a stream's table is refilled.

Nothing here is a tolerance: images and counters are compared exactly with ONE render of the CPU oracle per case, the audit of the
filters (filter_violations) with 0 and the three rt_debug_* calls with what the caps say — a table that silently stayed off would pass
everything else.  The one inequality is strict and between two runs of the same code: fewer `tri` wave executions with the masks."""
import numpy as np
import pytest

import capfuzz_scenes as cs
from capfuzz_scenes import WALK_SEEDS, _walk
from gpu_support import KEYS, bits, environment

pytestmark = pytest.mark.gpu
ENV = ("RT_TILE_TRI", "RT_TILE_CAND", "RT_PRIMARY", "RT_POOL", "RT_POOL_MIN_ITEMS")   # the variables tests/test_gpu_tile_tri.py clears
POOLED, SINGLE = {"RT_POOL_MIN_ITEMS": "0"}, {"RT_POOL": "0"}   # pooled workgroups also at these small sizes / single waves


def _idle(tr):
    """an idle GPU starts a single frame at once, as two parts, one per stream, instead of holding it back"""
    getattr(tr, "synchronize", lambda: None)()


def _render(lib, tr, sc, render_seed):
    mgr = sc.make_manager(tr, lib)
    mgr.OnEnable(renderSeed=render_seed)
    mgr.RenderFrame()
    mgr.RenderFrames(2)
    return tr.read_accumulated(), tr.counters()


def _check_scene(pkg, api, orc, make, part, table):
    """make() -> (scene, render seed), a fresh one per render (the manager writes into its scene's camera)"""
    c = orc.create_tracer(8)
    want, wantCounters = _render(orc, c, *make())
    c.close()
    assert wantCounters["segments"] > 0
    first = None
    for name, env in (("pooled", POOLED), ("single waves", SINGLE)):
        with environment(env, ENV):
            for stats in (False, True):
                g = api.create_tracer(0)
                if part:
                    g.set_partition(*part)
                g.enable_stats(stats)
                got, counters = _render(api, g, *make())
                prof = g.phase_profile() if stats else None
                debug = (g.primary_table(), g.tile_cand(), g.tile_tri())
                g.close()
                what = f"{name}, stats={stats}"
                print(f"{what}: segments {counters['segments']} (oracle {wantCounters['segments']}) debug {debug}" + (f" filter_violations {prof['filter_violations'][0]} tri {prof['tri'][0]}" if stats else ""))
                if part:
                    rows = pkg.dist.global_rows_of(part[1], part[2], want.shape[0], part[0])
                    assert np.array_equal(bits(got), bits(want[rows])), f"{what}: image differs from the oracle's rows"
                    first = first or counters   # (a part's share of the counters, which the oracle does not have: the four ways must agree)
                    for k in ("segments", "pixelFrames"):
                        assert counters[k] == first[k], (what, k)
                    assert counters["pixelFrames"] == 3 * len(rows) * want.shape[1], what
                else:
                    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), f"{what}: image differs from the oracle's"
                    assert counters["segments"] == wantCounters["segments"] and counters["pixelFrames"] == wantCounters["pixelFrames"], what
                    if stats:
                        assert [counters[k] for k in KEYS] == [wantCounters[k] for k in KEYS], what
                if stats:
                    assert prof["filter_violations"][0] == 0, what
                assert debug == ((1, 1, 1) if table else (0, 0, 0)), f"{what}: rt_debug_primary_table / _tile_cand / _tile_tri = {debug}"


@pytest.mark.parametrize("seed", cs.SEEDS)
def test_in_cap_scene_bit_exact(pkg, api, orc, seed):
    _check_scene(pkg, api, orc, lambda: cs.scene(pkg, seed), cs.partition_of(seed), table=True)


@pytest.mark.parametrize("seed", range(10))
def test_over_a_cap_scene_bit_exact(pkg, api, orc, seed):
    """33 spheres, 5 models, 17 triangles, a defocus of 1e-30, a root that is not a leaf (twice each): all three tables stay off"""
    _check_scene(pkg, api, orc, lambda: cs.scene_over_a_cap(pkg, seed), cs.partition_of(seed), table=False)


def test_masks_cut_work_over_the_family(pkg, api):
    """masks that clear nothing on the device would pass every comparison above: over six scenes whose host run showed a tile with an
    empty triangle mask, the STATS phase profile must count fewer `tri` wave executions with the masks than with RT_TILE_TRI=0"""
    total = {}
    for switch in ("1", "0"):
        total[switch] = 0
        with environment({"RT_TILE_TRI": switch, **POOLED}, ENV):
            for seed in cs.EMPTY_TRI_MASK_SEEDS:
                g = api.create_tracer(0)
                if cs.partition_of(seed):
                    g.set_partition(*cs.partition_of(seed))
                g.enable_stats(True)
                _render(api, g, *cs.scene(pkg, seed))
                n = g.phase_profile()["tri"][0]
                assert g.tile_tri() == int(switch) and g.tile_cand() == 1
                g.close()
                print(f"RT_TILE_TRI={switch} seed {seed}: {n} tri wave executions")
                total[switch] += n
    assert total["1"] < total["0"], total


# ---- one context through the calls whose arguments are part of the TileCandKey ----------------------------------------------------------

class _Walker:
    """one manager on one tracer; step() applies a step of the walk and renders: on an idle device one RenderFrame (two parts, one per
    stream), then RenderFrames(k) (a fused launch on the other stream)"""

    def __init__(self, pkg, lib, tr, seed):
        self.pkg, self.lib, self.tr = pkg, lib, tr
        sc, render_seed = cs.scene(pkg, seed)
        self.mgr = sc.make_manager(tr, lib)
        self.mgr.OnEnable(renderSeed=render_seed)
        self.in_cap = True
        self.defocus_off_at = None
        self.n = 0

    def tables(self):
        """what rt_debug_tile_cand and rt_debug_tile_tri must say after a launch in this state"""
        return 1 if self.in_cap and self.mgr.defocusStrength == 0.0 else 0

    def _geometry(self, sc, in_cap):
        self.mgr.models, self.mgr.spheres, self.mgr.bvhQuality = list(sc.models), list(sc.spheres), sc.settings["bvhQuality"]
        self.mgr.hasBVH = False   # InitFrame -> InitBVH -> upload_scene
        self.in_cap = in_cap

    def step(self, s):
        pkg, mgr, u = self.pkg, self.mgr, s["u"]
        T = pkg.manager.Transform
        self.n += 1
        if self.defocus_off_at == self.n:
            mgr.defocusStrength = 0.0
        kind = s["kind"]
        if kind == "sphere" and not mgr.spheres:
            kind = "camera"
        if kind == "model" and not mgr.models:
            kind = "camera"
        if kind == "sphere":   # move and resize one, through rt_update_spheres
            i = int(u[0] * len(mgr.spheres))
            old = mgr.spheres[i]
            mgr.spheres[i] = pkg.manager.Sphere(tuple(c + 2 * (v - 0.5) for c, v in zip(old.centre, u[1:4])), 0.05 + 2.0 * u[4], old.material)
            self.tr.update_spheres(mgr._pack_spheres())
        elif kind == "model":   # InitFrame -> rt_update_models; every second time to a mirrored transform
            m = mgr.models[int(u[0] * len(mgr.models))]
            t = m.transform
            scale = tuple(0.3 + 2.2 * v for v in u[7:10])
            if u[10] < 0.5:
                scale = (-scale[0], scale[1], scale[2]) if u[11] < 0.5 else tuple(-v for v in scale)
            m.transform = T(tuple(c + 3 * (v - 0.5) for c, v in zip(t.position, u[1:4])), tuple(360 * v for v in u[4:7]), scale)
        elif kind == "camera":   # move and turn
            t = mgr.camera.transform
            mgr.camera.transform = T(tuple(c + 2 * (v - 0.5) for c, v in zip(t.position, u[0:3])), (40 * u[3] - 20, 60 * u[4] - 30, 50 * u[5] - 25 if u[6] < 0.4 else 0.0))
        elif kind == "fov":
            mgr.camera.fieldOfView = [f for f in cs.FOVS if f != mgr.camera.fieldOfView][int(u[0] * 4)]
        elif kind == "diverge":
            mgr.divergeStrength = [v for v in cs.DIVERGE if v != mgr.divergeStrength][int(u[0] * 3)]
        elif kind == "defocus":
            mgr.defocusStrength, mgr.focusDistance = 20.0 + 100.0 * u[0], 1.0 + 6.0 * u[1]
            self.defocus_off_at = self.n + 2
        elif kind in ("resize_same_tiles", "resize"):
            w, h = mgr.screenSize
            if kind == "resize_same_tiles":   # other W and H, the same tiles per row and per column
                w2 = (w + 7) // 8 * 8 if w % 8 else w - 1 - int(u[0] * 6)
                h2 = (h + 7) // 8 * 8 if h % 8 else h - 1 - int(u[1] * 6)
                assert ((w2 + 7) // 8, (h2 + 7) // 8) == ((w + 7) // 8, (h + 7) // 8) and (w2, h2) != (w, h)
            else:
                w2, h2 = 9 + int(u[0] * 72), 9 + int(u[1] * 42)
            mgr.screenSize = (w2, h2)
            mgr.camera.aspect = w2 / h2
            self.tr.resize(w2, h2)
            mgr.ResetAccumulatedRender()   # (a resize drops the targets: both sides start over)
        elif kind in ("upload_in_cap", "upload_in_cap_again"):
            self._geometry(cs.scene(pkg, s["other"])[0], True)
        elif kind == "upload_over_a_cap":   # 33 spheres, 5 models or 17 triangles
            self._geometry(cs.scene_over_a_cap(pkg, 5 * WALK_SEEDS.index(s["other"]) + s["over"])[0], False)
        elif kind == "reset":
            mgr.ResetAccumulatedRender()
        else:
            raise AssertionError(kind)
        _idle(self.tr)
        mgr.RenderFrame()
        _idle(self.tr)
        mgr.RenderFrames(s["k"])
        return kind


_oracle_walks = {}


def _oracle_walk(pkg, orc, seed):
    """(image, segments, what the tables must say) after every step: computed once, shared by the shipped and the STATS run, never written"""
    if seed not in _oracle_walks:
        tr = orc.create_tracer(8)
        w = _Walker(pkg, orc, tr, seed)
        out = []
        for s in _walk(pkg, seed):
            w.step(s)
            out.append((tr.read_accumulated().copy(), tr.counters()["segments"], w.tables()))
        tr.close()
        _oracle_walks[seed] = out
    return _oracle_walks[seed]


@pytest.mark.parametrize("stats", [False, True], ids=["shipped", "stats"])
@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_one_context_through_key_changing_calls(pkg, api, orc, seed, stats):
    """a stale table shows as a wrong pixel: after every step the accumulated image and `segments` equal the oracle's, which took the
    same steps, and the two debug calls say what the step's state says (off over a cap and under defocus, on again afterwards)"""
    want = _oracle_walk(pkg, orc, seed)
    with environment(POOLED, ENV):
        g = api.create_tracer(0)
        g.enable_stats(stats)
        w = _Walker(pkg, api, g, seed)
        try:
            for i, s in enumerate(_walk(pkg, seed)):
                kind = w.step(s)
                got, segments = g.read_accumulated(), g.counters()["segments"]
                debug = (g.tile_cand(), g.tile_tri())
                what = f"step {i} ({kind}, then 1 + {s['k']} frames at {w.mgr.screenSize})"
                print(f"{what}: segments {segments} (oracle {want[i][1]}) debug {debug} (expected {want[i][2]})")
                assert got.shape == want[i][0].shape and np.array_equal(bits(got), bits(want[i][0])), f"{what}: image differs from the oracle's"
                assert segments == want[i][1], what
                assert w.tables() == want[i][2] and debug == (want[i][2], want[i][2]), f"{what}: rt_debug_tile_cand / _tile_tri = {debug}"
                if stats:
                    assert g.phase_profile()["filter_violations"][0] == 0, what
        finally:
            g.close()
