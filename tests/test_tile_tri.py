"""The per-tile triangle candidates (tile_tri_mask of ray-tracing_amd/csrc/rt_tile_cand.h) on their own, without a device and without the kernels.

tests/tile_tri_driver.cpp is built against the header with the host compiler, twice: plainly (-O2 -Wall -Wextra -Werror) and with the
address and undefined-behaviour sanitizers, as a stand-alone executable with the runtimes linked into it (nothing sanitized is loaded into
python; a report ends the program with a non-zero exit, which fails the test).  Both are built without contraction, the arithmetic
contract of include/rt_math.h.

What the driver checks: for every tile it visits, every camera ray built with the kernel's own raygen formulas — all 64 pixels clipped at
W / H, the jitter at the centre, at 16 points of the unit circle and at 16 random interior points — goes through traverse_flat's transform
and tri_test's PRIMARY form in the kernel's operation order, and every triangle that ACCEPTS a ray must have its bit in the tile's mask:
0 misses.  Cases: seeded random cameras with 1 ... 4 models and up to 16 triangles (every fourth case 4 models with 16 triangles) — rotated,
non-uniformly scaled and mirrored models, triangles across the frustum's edges, behind the camera, degenerate ones, the camera in a
triangle's plane and on a vertex, cull on and off — at 37x23 and 96x54 over every tile, whole images and the 2-of-3 strip partition,
diverge 0 / 1.5 / 50; and config 2's camera and ground quad (horizon, diagonal and far edge cross tiles) at 96x54, 37x23, as partition
1 of 3 and at 1920x1080 (every 50th tile plus all edge tiles), also with the quad small, rotated, non-uniformly and mirror scaled, with
culling off, and with the camera under the ground.

Selectivity keeps a mask of all ones from passing: on config 2 at 1920x1080 the mean number of bits of the mask may exceed the mean number
of triangles the tile's sampled rays were really accepted by (a function of the scene alone, and a lower bound of what any correct mask
holds) by at most 0.15 — the sphere masks sit 0.015 above theirs — and that bound lies far below the 2 bits of an all-ones mask.  The
same run is the measurement the kernel path rests on: at least a quarter of the headline image's tiles must get an empty mask."""
import os
import re
import subprocess

import pytest

import host_driver
from capfuzz_scenes import triangle_scene_file as scene_file   # (the driver's text form: shared with tests/test_tile_fuzz.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_tri")
    plain = host_driver.build(d, "tile_tri", ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"])
    san = host_driver.build(d, "tile_tri", ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                         "-static-libasan", "-static-libubsan"], exe="driver_san")
    return {"plain": plain, "san": san, "dir": d}


def run(exe, *args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RT_")}
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, env=env, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, (p.returncode, out[-3000:], p.stderr.decode(errors="replace")[-3000:])
    last = out.strip().splitlines()[-1]
    assert last.startswith("ok ") and " misses=0 " in last + " ", out[-3000:]
    return {k: float(v) for k, v in re.findall(r"(\w+)=([-0-9.e+]+)", last)}


@pytest.mark.parametrize("seed", [1, 2, 20261019])
def test_no_accepted_triangle_is_missing_from_a_tile_mask(drivers, seed):
    r = run(drivers["san"], "random", seed, 48)
    assert r["cases"] == 48 and r["rays"] > 1e6


def test_plain_build_agrees(drivers):
    """-O2 without the sanitizers: the optimiser must not make the mask less conservative either"""
    run(drivers["plain"], "random", 1, 48)


@pytest.mark.parametrize("size,part", [((37, 23), (8, 0, 1)), ((96, 54), (8, 0, 1)), ((96, 54), (8, 1, 3))])
def test_config2_small(pkg, api, drivers, size, part):
    r = run(drivers["san"], "scene", scene_file(pkg, api, drivers["dir"], 2, *size, part), 1)
    assert r["triangles"] == 2


def _ground(pkg, **kw):
    def change(sc):
        t = sc.models[0].transform
        sc.models[0].transform = type(t)(position=kw.get("position", (0, 0, 0)), euler=kw.get("euler", (90, 0, 0)), scale=kw.get("scale", (40, 40, 1)))
        if kw.get("glass"):
            sc.models[0].material.flag = pkg.abi.MATERIAL_GLASS   # RC:355: no backface culling
        if "camera" in kw:
            c = sc.camera.transform
            sc.camera.transform = type(c)(position=kw["camera"][0], euler=kw["camera"][1])
    return change


VARIANTS = {
    "small_quad_all_edges_in_view": dict(scale=(6, 9, 1), position=(0.5, 0, 1.0)),
    "rotated_nonuniform": dict(scale=(30, 7, 1), euler=(84, 25, 10), position=(0.5, -0.25, 1.0)),
    "mirrored": dict(scale=(-12, 8, 1), euler=(78, -30, 5)),
    "cull_off": dict(scale=(10, 10, 1), glass=True),
    "camera_under_the_ground": dict(camera=((0, -2.0, -8.8), (-12, 0, 0))),
    "camera_under_the_ground_cull_off": dict(camera=((0, -2.0, -8.8), (-12, 0, 0)), glass=True),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_config2_ground_variants(pkg, api, drivers, name):
    run(drivers["san"], "scene", scene_file(pkg, api, drivers["dir"], 2, 96, 54, change=_ground(pkg, **VARIANTS[name]), tag="_" + name), 1)


def test_config2_full_size_and_selectivity(pkg, api, drivers):
    """every 50th tile plus all edge tiles of the headline image: 0 misses; the mask is nearly as tight as the scene allows; and the premise
    of the kernel path: at least a quarter of the tiles meet no triangle at all"""
    r = run(drivers["plain"], "scene", scene_file(pkg, api, drivers["dir"], 2, 1920, 1080), 50)
    print("config 2 at 1920x1080:", r)
    assert r["tiles"] == 240 * 135 and r["triangles"] == 2
    assert r["mean_brute"] + 0.15 < 1.0, "the bound leaves no room: an all-ones mask (2 bits) must be far above it"
    assert r["mean_mask"] <= r["mean_brute"] + 0.15
    assert r["share0"] >= 0.25


def test_config2_full_size_partition(pkg, api, drivers):
    run(drivers["plain"], "scene", scene_file(pkg, api, drivers["dir"], 2, 1920, 1080, (8, 1, 3)), 50)


def test_public_header_symbol_is_exported(pkg, api):
    """include/rt_tile_tri.h (included by include/rt_tile_cand.h) declares one call; hip.TILE_TRI_SYMBOLS mirrors it and the library exports it"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_tile_tri.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(rt_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(pkg.hip.TILE_TRI_SYMBOLS) == ["rt_debug_tile_tri"]
    assert not set(names) & (set(pkg.hip.ABI_SYMBOLS) | set(pkg.hip.TILE_CAND_SYMBOLS))
    assert '#include "rt_tile_tri.h"' in open(os.path.join(ROOT, "include", "rt_tile_cand.h")).read()
    for n in names:
        assert hasattr(api.lib, n), f"libraytrace_hip.so does not export {n}"
    assert api.lib.rt_debug_tile_tri(None) == pkg.abi.RT_ERR_INVALID_ARG
