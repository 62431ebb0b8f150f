"""The arithmetic that sizes a launch (ray-tracing_amd/csrc/rt_launch_plan.h), checked without a GPU.

tests/launch_plan_driver.cpp is built against the header with the host compiler and answers requests on stdin, one line each.  The checks:
the tile counter's conservation against a simulation of the kernel's consumption rule, frame groups, pooling at 256 CUs as DESIGN.md
("Which workgroup shape a launch gets") states it, the variant slots and LDS bytes, the staging slabs and the frames per fused launch,
and the suspension tuner's rule."""
import math
import random
import subprocess

import pytest

from launch_plan_support import one, plan  # noqa: F401  (plan: the fixture that builds tests/launch_plan_driver.cpp)

CUS = 256
MIB = 1 << 20
SLAB_BUDGET = 1536 * MIB  # RT_FUSE_SLAB_BYTES


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tile_queue_is_conserved_across_launches(plan, seed):
    """Seeded random launches on one context's two tile counters: tiles 1 ... 40,000, 1 or 2 parts, 1 ... 64 frames, 1 / 12 / 16 waves per
    group, 1 ... 2,048 resident groups, RT_GRID off / below / above the items, RT_FRAME_GROUP.  For each launch the simulated kernel takes
    every position in [0, items) exactly once and leaves the counter where the plan starts the next launch; the parts' tiles are disjoint
    and cover the image."""
    out = subprocess.run([plan.exe], input=f"queue seed={seed} n=150\n", capture_output=True, text=True, timeout=600, check=True).stdout
    assert out.startswith("clean "), out


def test_queue_bookkeeping_of_one_launch(plan):
    """The counter contract in figures: 1,000 tiles on 100 resident single waves — positions 0 ... 99 by wave index, 900 fetched, 100
    overshoots; a half kernel (two parts) fetches every position."""
    p = one(plan, "part", tiles=1000, frames=1, spp=1, resident=100, wpg=1, part=0, parts=1, next=5000)
    assert (p["items"], p["grid"], p["byindex"], p["qstart"]) == (1000, 100, 100, 0)
    assert p["base"] == 5000 - 100 and p["next"] == 5000 + 900 + 100
    h = one(plan, "part", tiles=1001, frames=1, spp=1, resident=100, wpg=1, part=1, parts=2, next=7)
    assert (h["tiles"], h["qstart"], h["base"], h["next"]) == (500, 1, 7, 7 + 500 + 100)


def test_frame_groups(plan):
    rng = random.Random(5)
    reqs = []
    for _ in range(4000):
        kw = dict(tiles=rng.choice([1, 64, 1024, 8100, 32400]), frames=rng.choice([1, 2, 3, 5, 8, 16, 17, 33, 64]), flat=rng.random() < 0.7,
                  spp=rng.choice([1, 4, 1000, 65535, 65536, 100000]), fg=rng.choice([0, 0, 0, 1, 2, 3, 8, 100]),
                  resident=rng.choice([1, 64, 512, 2048]), wpg=rng.choice([1, 12, 16]), parts=rng.choice([1, 2]))
        kw["part"] = rng.randrange(kw["parts"])
        reqs.append(("part", kw))
    for (_, kw), p in zip(reqs, plan(*reqs)):
        g, n = p["group"], kw["frames"]
        if not kw["flat"] or n == 1 or kw["spp"] >= 65536:
            assert g == 1, (kw, p)
        elif kw["fg"] > 0:
            assert g == min(kw["fg"], n), (kw, p)
        else:
            assert 1 <= g <= 4, (kw, p)
        assert p["groups"] * g >= n > (p["groups"] - 1) * g, (kw, p)
        assert p["shift"] == int(math.log2(g)), (kw, p)


def test_frame_group_needs_eight_items_per_resident_wave(plan):
    """1080p FLAT launch of 16 frames at 8,192 resident waves: groups of 4 keep 32,400 x 4 items >= 8 per wave; 256 x 256 does not"""
    big = one(plan, "part", tiles=32400, frames=16, flat=True, spp=1, resident=512, wpg=16, part=0, parts=1)
    small = one(plan, "part", tiles=1024, frames=16, flat=True, spp=1, resident=512, wpg=16, part=0, parts=1)
    assert (big["group"], big["groups"], big["shift"]) == (4, 4, 2)
    assert small["group"] == 1


def flat_shape(**kw):
    base = dict(flat=True, stack=0, pool=64, poolwaves=16, minitems=4, cus=CUS, wpg=1)
    base.update(kw)
    return ("shape", base)


def test_pooling_at_256_cus(plan):
    """a 1080p fused launch of >= 2 frames is pooled; a single 1080p frame (32,400 tiles for 8,192 waves) and a 256 x 256 image
    of 16 frames are not; RT_POOL_MIN_ITEMS=0 pools every FLAT launch, RT_POOL=0 none."""
    one_frame, two_frames, small, anything, no_pool = plan(
        flat_shape(tiles=240 * 135, frames=1), flat_shape(tiles=240 * 135, frames=2), flat_shape(tiles=32 * 32, frames=16),
        flat_shape(tiles=1, frames=1, minitems=0), flat_shape(tiles=240 * 135, frames=64, pool=0))
    assert not one_frame["pooled"] and one_frame["wpg"] == 1 and one_frame["hotunits"] == 0
    assert two_frames["pooled"] and two_frames["wpg"] == 16 and two_frames["threads"] == 16 * 64 and two_frames["poolcells"] == 64
    assert not small["pooled"]
    assert anything["pooled"]
    assert not no_pool["pooled"] and no_pool["poolcells"] == 0


def test_variant_slots_and_lds(plan):
    reqs, keys = [], []
    for flat in (False, True):
        for many in ((False,) if flat else (False, True)):
            for hot in (False, True):
                for stats in (False, True):
                    kw = dict(flat=flat, stats=stats, stack=0 if flat else 20, ext=3 if many else 0, chunks=5 if many else 0,
                              hot=1792 if hot and not flat else 0, wpg=12, pool=64, poolwaves=16, minitems=0 if hot else 10**6,
                              cus=CUS, tiles=32400, frames=16)
                    reqs.append(("shape", kw))
                    keys.append((flat, many, hot, stats))
    shapes = plan(*reqs)
    slots = [s["variant"] for s in shapes]
    assert len(set(slots)) == 12 and all(0 <= v < 16 for v in slots), slots
    for (flat, many, hot, stats), s in zip(keys, shapes):
        assert (bool(s["many"]), bool(s["hot"])) == (many, hot)
        assert s["lds"] == s["hotunits"] * 16 + s["wpg"] * s["wavedwords"] * 4
        wave = ((0 if flat else 20) + 4 + (2 + 3 if many else 0)) * 256 + (2 * 64 * 16 if flat else 0)
        assert s["wavedwords"] * 4 == wave
        assert s["wpg"] == ((16 if flat else 12) if hot else 1)
    # the rule for the > 64-model instantiation, as the passes outside launch_shape ask for it: chunks, and not FLAT
    assert [m["many"] for m in plan(*[("many", dict(chunks=c, flat=f)) for c, f in ((0, False), (5, False), (5, True), (0, True))])] == [0, 1, 0, 0]
    # the BVH top-of-tree cache of config 3 (448 records) around 12 waves of 20-entry stacks
    assert shapes[keys.index((False, False, True, False))]["lds"] == 1792 * 16 + 12 * 24 * 256


@pytest.mark.parametrize("stack", [1, 31, 32])
def test_lds_of_the_shallowest_and_the_deepest_stacks(plan, stack):
    """Stack heights 1, 31 and 32 = RT_MAX_BVH_DEPTH (tests/test_deep_trees.py: the trees that fill them): a wave's region is exactly
    [stack][64] stack rows + [RT_PIXEL_FIELDS = 4][64] pixel fields + — more than 64 models — [2 + ext][64] mask extension, and a
    workgroup's LDS the cache plus its waves' regions: the arithmetic of wave_lds_bytes, for the single-wave, hot and MANY shapes."""
    reqs, keys = [], []
    for ext in (0, 1, 3, 32):
        for hot in (0, 64, 1792):
            for stats in (False, True):
                reqs.append(("shape", dict(flat=False, stats=stats, stack=stack, ext=ext, chunks=5 if ext else 0, hot=hot, wpg=12, pool=64, poolwaves=16,
                                           minitems=10**6, cus=CUS, tiles=96, frames=2)))
                keys.append((ext, hot))
    for (ext, hot), s in zip(keys, plan(*reqs)):
        rows = stack + 4 + (2 + ext if ext else 0)
        assert s["wavedwords"] == rows * 64, (stack, ext, hot, s)
        assert s["wpg"] == (12 if hot else 1) and s["threads"] == 64 * s["wpg"], (stack, ext, hot, s)
        assert s["hotunits"] == hot and s["lds"] == hot * 16 + s["wpg"] * rows * 64 * 4, (stack, ext, hot, s)
        assert (bool(s["many"]), bool(s["hot"])) == (ext > 0, hot > 0)
    # and plan_groups sizes the cache from the same wave region ("Which workgroup shape a launch gets"): as many waves as a
    # CU's 160 KB hold, 24 at the most, in whole groups of at most `want`; a group's share less 1 KB and its waves is the cache, and
    # fewer than 16 records are not worth a group.  1, 97 and 2,000 models: 0, 2 and 32 extension words.
    seen = {}
    for models, ext in ((1, 0), (97, 2), (2000, 32)):
        for asked in (12, 8, 4):
            wave = (stack + 4 + (2 + ext if ext else 0)) * 256
            per_cu = min(24, 160 * 1024 // wave)
            want = next(w for w in range(asked, 0, -1) if per_cu % w == 0)
            records = max(0, 160 * 1024 // (per_cu // want) - 1024 - want * wave) // 64
            g = one(plan, "groups", height=stack, models=models, want=asked)
            assert g == ({"wpg": want, "records": records} if records >= 16 else {"wpg": 1, "records": 0}), (stack, models, asked, g, want, records)
            seen[models, asked] = g["wpg"]
    # what that means for the deepest trees: with up to 64 models, stacks of 31 and 32 rows leave no room for a cache, whatever group size
    # is asked for (18 or 17 waves per CU: no whole groups with room to spare) — such scenes run as single-wave workgroups; the two
    # extension rows of 65 ... 94 models make it 16 waves again: groups of 8 around 16 records under a 32-row stack
    # (tests/test_gpu_deep_trees.py reads both from the launch's own report)
    assert [seen[1, asked] for asked in (12, 8, 4)] == ([1, 1, 1] if stack >= 31 else [12, 8, 4])
    assert one(plan, "groups", height=32, models=65, want=12) == {"wpg": 8, "records": 16}


def test_group_plan_shares_the_filter_rule(plan):
    f = plan(*[("filter", dict(models=m)) for m in (1, 64, 65, 95, 96, 1087, 1088, 5000)])
    assert [(x["nf"], x["ext"]) for x in f] == [(1, 0), (64, 0), (65, 1), (95, 1), (96, 2), (1087, 32), (1087, 32), (1087, 32)]
    g = one(plan, "groups", height=20, models=1, want=12)
    assert g["wpg"] == 12 and g["records"] == (160 * 1024 // 2 - 1024 - 12 * 24 * 256) // 64
    assert one(plan, "groups", height=20, models=1, want=12, hotkb=4)["records"] == 64  # RT_HOT_KB caps the cache
    assert one(plan, "groups", height=20, models=1, want=12, hotkb=0) == {"wpg": 1, "records": 0}
    assert one(plan, "groups", height=20, models=1, want=5)["wpg"] == 4  # whole groups fill the CU's 24 wave slots
    # more models: the mask extension's words make the waves larger, the cache smaller
    assert one(plan, "groups", height=20, models=2000, want=12)["records"] < g["records"]


def test_records_hold_every_wave_of_the_grid(plan):
    assert one(plan, "records", resident=100, wpg=12, grid=0)["waves"] == 1212
    assert one(plan, "records", resident=100, wpg=1, grid=5000)["waves"] == 5001


def test_slab_frames(plan):
    sizes = [1920 * 1080, 3840 * 2160, 1920 * 1080 // 8]
    assert [s["frames"] for s in plan(*[("slab", dict(npix=n, budget=SLAB_BUDGET, frames=16)) for n in sizes])] == [48, 16, 64]
    assert one(plan, "slab", npix=3840 * 2160, budget=SLAB_BUDGET, frames=20)["frames"] == 20  # at least this launch's
    assert one(plan, "slab", npix=0, budget=SLAB_BUDGET, frames=1)["frames"] == 64


def test_fuse_cap(plan):
    big = 64 * 1920 * 1080 * 16
    assert one(plan, "fuse", ms=0.71 * 16, frames=16, npix=1920 * 1080, slab0=big, slab1=big)["cap"] == 29
    assert one(plan, "fuse", ms=0.71 * 16, frames=16, npix=1920 * 1080, slab0=0, slab1=0)["cap"] == 29
    rng = random.Random(3)
    reqs = []
    for _ in range(3000):
        npix = rng.choice([0, 1, 64 * 64, 1920 * 135, 1920 * 1080, 3840 * 2160])
        slabs = [rng.choice([0, 0, npix * 16 * rng.randint(1, 80)]) for _ in range(2)]
        reqs.append(("fuse", dict(ms=rng.choice([0.01, 0.3, 0.71, 1.3, 5.0, 40.0]) * rng.randint(1, 64), frames=rng.randint(1, 64), npix=npix,
                                  slab0=slabs[0], slab1=slabs[1])))
    for (_, kw), f in zip(reqs, plan(*reqs)):
        assert 16 <= f["cap"] <= 64, (kw, f)
        held = [s // (kw["npix"] * 16) for s in (kw["slab0"], kw["slab1"]) if s and kw["npix"]]
        if held:
            assert f["cap"] <= max(16, min(held)), (kw, f)


def test_fuse_cap_never_outgrows_the_slabs_it_sized(plan):
    """one rule in both places: slabs made by slab_frames, then any measured frame time"""
    for npix in (1920 * 1080, 3840 * 2160, 1920 * 1080 // 8, 2560 * 1440):
        frames = one(plan, "slab", npix=npix, budget=SLAB_BUDGET, frames=16)["frames"]
        slab = frames * npix * 16
        for ms in (0.05, 0.3, 0.71, 2.0):
            assert one(plan, "fuse", ms=ms * 16, frames=16, npix=npix, slab0=slab, slab1=slab)["cap"] <= frames


def test_pinned_fuse_cap(plan):
    assert [one(plan, "pin", v=v)["cap"] for v in (-3, 0, 1, 16, 40, 64, 65, 1000)] == [0, 0, 1, 16, 40, 64, 64, 64]


def test_tuner(plan):
    ok = dict(flat=False, staged=True, frames=8, stats=False, since=48)
    assert one(plan, "tuner", **ok)["samples"] == 1
    for change in (dict(flat=True), dict(staged=False), dict(frames=7), dict(stats=True), dict(since=47)):
        assert one(plan, "tuner", **{**ok, **change})["samples"] == 0, change
    n = dict(n0=3, n1=3)
    assert one(plan, "tuner", ms0=3.0, ms1=3 * 0.9899, **n)["decision"] == 4  # more than 1 % faster
    assert one(plan, "tuner", ms0=3.0, ms1=3 * 0.991, **n)["decision"] == 3
    assert one(plan, "tuner", ms0=3.0, ms1=1.0, n0=3, n1=2)["decision"] == 0  # not yet: 3 samples each
