"""include/rt_variance.h without a GPU: the header is plain C (C99 and C++17) and RtVarianceDenoiseParams is the same 40 bytes in C, in
ctypes and through a numpy view; the library exports the header's ten calls and each refuses a null context; the default parameters
are valid; the arithmetic of ray-tracing_amd/csrc/rt_variance_math.h — the functions the kernels call, here run by the host driver
tests/variance_math_driver.cpp — equals the NumPy restatement of the header's prose (tests/variance_reference.py) bit for bit, every
pixel, every channel; small-integer cases are exact; and the moments image is a layout the existing reprojection carries."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import host_driver
import reproject_reference as rp
import variance_reference as ref
from gpu_support import assert_same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
F = np.float32
OFFSETS = {"struct_size": 0, "iterations": 4, "sigmaLuminance": 8, "sigmaNormal": 12, "sigmaPlane": 16, "demodulate": 20, "scale": 24, "unknownVariance": 28,
           "reserved": 32}
FUNCTIONS = sorted(["rt_denoise_variance", "rt_denoise_variance_buffers", "rt_denoise_variance_default_params", "rt_denoise_variance_to_device",
                    "rt_moments_update_buffers", "rt_variance_carry", "rt_variance_moments_to_device", "rt_variance_read_moments", "rt_variance_reset",
                    "rt_variance_update"])
SHAPES = [(1, 1), (1, 37), (37, 1), (64, 36), (333, 77)]
PARAMS = dict(sigmaLuminance=1.5, sigmaNormal=0.3, sigmaPlane=0.2, scale=0.5, unknownVariance=0.75)


def header_functions():
    text = open(os.path.join(INCLUDE, "rt_variance.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z_0-9]+)\s*\(", text)))


# ---------------------------------------------------------------- 1. the header and the three layouts
@pytest.mark.parametrize("lang", ["c99", "c++17"])
def test_header_compiles_and_has_the_documented_layout(lang, tmp_path):
    cxx = lang.startswith("c++")
    src = tmp_path / ("vr.cpp" if cxx else "vr.c")
    checks = "\n".join(f"typedef char at_{f}[offsetof(RtVarianceDenoiseParams, {f}) == {o} ? 1 : -1];" for f, o in OFFSETS.items())
    src.write_text('#include <stddef.h>\n#include "rt_variance.h"\ntypedef char size_is_40[sizeof(RtVarianceDenoiseParams) == 40 ? 1 : -1];\n' + checks +
                   "\nint use(RtContext* c, RtVarianceDenoiseParams* p, RtReprojectParams* r, RtDenoiseParams* d, float* f, RtPixelAov* a) { return rt_denoise_variance_default_params(p)"
                   " + rt_moments_update_buffers(c, 1, 1, f, f, f, 0) + rt_denoise_variance_buffers(c, p, 1, 1, f, f, a, f) + rt_variance_update(c) + rt_variance_reset(c)"
                   " + rt_variance_carry(c, r, a, a, NULL, 0) + rt_variance_read_moments(c, f, 16) + rt_variance_moments_to_device(c, f, 16)"
                   " + rt_denoise_variance(c, p, 1, f, 16) + rt_denoise_variance_to_device(c, p, 1, f, 16) + rt_denoise_default_params(d); }\n")
    cmd = ["g++", "-x", "c++"] if cxx else ["gcc", "-x", "c"]
    subprocess.check_call(cmd + [f"-std={lang}", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])


def test_ctypes_struct_and_numpy_view_are_the_same_40_bytes(pkg):
    abi = pkg.abi
    assert C.sizeof(abi.RtVarianceDenoiseParams) == 40 and abi.VARIANCE_DENOISE_PARAMS_DTYPE.itemsize == 40
    assert tuple(n for n, _ in abi.RtVarianceDenoiseParams._fields_) == tuple(OFFSETS) == abi.VARIANCE_DENOISE_PARAMS_DTYPE.names
    for f, off in OFFSETS.items():
        assert getattr(abi.RtVarianceDenoiseParams, f).offset == off and getattr(abi.RtVarianceDenoiseParams, f).size == (8 if f == "reserved" else 4), f
        assert abi.VARIANCE_DENOISE_PARAMS_DTYPE.fields[f][1] == off, f
    p = abi.RtVarianceDenoiseParams(struct_size=40, iterations=3, sigmaLuminance=0.5, sigmaNormal=0.25, sigmaPlane=2.0, demodulate=1, scale=0.125, unknownVariance=8.0)
    p.reserved[1] = 7
    a = np.frombuffer(bytes(p), dtype=abi.VARIANCE_DENOISE_PARAMS_DTYPE)[0]
    assert a.tolist()[:8] == (40, 3, 0.5, 0.25, 2.0, 1, 0.125, 8.0) and a["reserved"].tolist() == [0, 7]
    assert struct.unpack("<Iifffiffii", bytes(p)) == (40, 3, 0.5, 0.25, 2.0, 1, 0.125, 8.0, 0, 7)


# ---------------------------------------------------------------- 2. symbols  3. null context  4. default parameters
def test_header_symbols_are_exported_and_listed(pkg, api):
    names = header_functions()
    assert names == FUNCTIONS
    assert sorted(pkg.hip.VARIANCE_SYMBOLS) == names, "hip.VARIANCE_SYMBOLS is out of sync with include/rt_variance.h"
    for other in (pkg.hip.ABI_SYMBOLS, pkg.hip.COST_SYMBOLS, pkg.hip.AOV_SYMBOLS, pkg.hip.DENOISE_SYMBOLS, pkg.hip.REPROJECT_SYMBOLS, pkg.hip.MOTION_SYMBOLS):
        assert not set(names) & set(other)
    for n in names:
        assert hasattr(api.lib, n), f"libraytrace_hip.so does not export {n}"
    exported = subprocess.run(["nm", "-D", "--defined-only", api.lib._name], capture_output=True, text=True, check=True).stdout
    mine = sorted(set(re.findall(r"\b(rt_(?:variance_|moments_|denoise_variance)[a-z_0-9]*)\b", exported)))
    assert mine == names, "the library exports a variance call the header does not declare"


def test_every_call_refuses_a_null_context(pkg, api):
    bad = pkg.abi.RT_ERR_INVALID_ARG
    p = api.variance_denoise_params()
    r = api.reproject_params()
    buf = np.zeros(64, dtype=F)
    d = buf.ctypes.data
    assert api.moments_update_buffers(None, 1, 1, d, d, d, 0) == bad
    assert b"null context" in api.last_error(None)
    assert api.denoise_variance_buffers(None, C.byref(p), 1, 1, d, d, d, d) == bad
    assert api.variance_update(None) == bad and api.variance_reset(None) == bad
    assert api.variance_carry(None, C.byref(r), d, d, None, 0) == bad
    assert api.variance_read_moments(None, d, 16) == bad and api.variance_moments_to_device(None, d, 16) == bad
    assert api.denoise_variance(None, C.byref(p), 1, d, 16) == bad and api.denoise_variance_to_device(None, C.byref(p), 1, d, 16) == bad
    assert api.denoise_variance(None, None, 1, None, 0) == bad
    assert api.denoise_variance_default_params(None) == bad


def test_default_params_are_valid(pkg, api):
    raw = (C.c_uint8 * 40)(*([0xff] * 40))
    p = pkg.abi.RtVarianceDenoiseParams.from_buffer(raw)
    assert api.denoise_variance_default_params(C.byref(p)) == pkg.abi.RT_OK
    assert p.struct_size == 40 and list(p.reserved) == [0, 0]
    assert 1 <= p.iterations <= pkg.abi.DENOISE_MAX_ITERATIONS
    for s in (p.sigmaLuminance, p.sigmaNormal, p.sigmaPlane):
        assert np.isfinite(s) and s > 0
    assert np.isfinite(p.unknownVariance) and p.unknownVariance >= 0
    assert p.demodulate == 1 and p.scale == 1.0
    q = api.variance_denoise_params(iterations=2, unknownVariance=0.25)
    assert (q.iterations, q.unknownVariance, q.sigmaLuminance) == (2, 0.25, p.sigmaLuminance)
    with pytest.raises(TypeError):
        api.variance_denoise_params(sigmaColour=1.0)


# ---------------------------------------------------------------- 5. the math header, through the host driver, against NumPy
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = host_driver.build(tmp_path_factory.mktemp("variance_math"), "variance_math", ["-std=c++17", "-O2", "-fno-fast-math", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"])

    class Driver:
        @staticmethod
        def denoise(rgba, moments, aov, iterations, sigma_l, sigma_n, sigma_p, demodulate, scale, unknown):
            h, w = rgba.shape[:2]
            blob = struct.pack("<5i5f", 0, w, h, iterations, int(demodulate), scale, sigma_l, sigma_n, sigma_p, unknown) + rgba.tobytes() + moments.tobytes() + aov.tobytes()
            out = subprocess.run([exe], input=blob, capture_output=True, timeout=600, check=True).stdout
            return np.frombuffer(out, dtype=F).reshape(h, w, 4)

        @staticmethod
        def update(now, snap, moments, rebase):
            h, w = now.shape[:2]
            blob = struct.pack("<4i", 1, w, h, int(rebase)) + now.tobytes() + snap.tobytes() + moments.tobytes()
            out = subprocess.run([exe], input=blob, capture_output=True, timeout=600, check=True).stdout
            both = np.frombuffer(out, dtype=F).reshape(2, h, w, 4)
            return both[0], both[1]
    return Driver


def reference_denoise(orc, rgba, moments, aov, iterations, demodulate, p=PARAMS):
    return ref.denoise(orc, rgba, moments, aov, iterations, p["sigmaLuminance"], p["sigmaNormal"], p["sigmaPlane"], demodulate, p["scale"], p["unknownVariance"])


def test_the_synthetic_inputs_cover_what_they_are_there_for(pkg, orc):
    rgba, aov = ref.synthetic(pkg, 64, 36, seed=100)
    m = ref.synthetic_moments(rgba, seed=100)
    assert set(np.unique(m[..., 3][np.isfinite(m[..., 3])]).tolist()) >= {0.0, 1.0, 1.5, 2.0, 7.0}
    assert np.isnan(m).any() and np.isinf(m).any() and (m[..., [0, 1, 3]] < 0).any()
    known = (m[..., 3] >= 2) & np.isfinite(m).all(axis=-1)
    with np.errstate(all="ignore"):
        d = m[..., 1] - ref.div(orc, m[..., 0], m[..., 3]) * m[..., 0]
    assert (d[known] < 0).any(), "no pixel cancels below zero"
    raw = rgba[..., :3]
    var = ref.variance(orc, m, raw, raw, np.zeros(raw.shape, dtype=bool), 0.75)
    assert np.isfinite(var).all() and (var >= 0).all()
    assert (var[known] == 0).any() and (var[known] > 0).any() and var[0, 0] == 1.0
    now, snap, mom = ref.synthetic_sums(64, 36, seed=100)
    dn = now[..., 3] - snap[..., 3]
    assert (dn == 0).any() and (dn < 0).any() and (dn == 17).any() and not np.isfinite(now).all() and not np.isfinite(snap).all()


@pytest.mark.parametrize("w,h", SHAPES)
def test_math_header_equals_the_numpy_restatement(pkg, orc, driver, w, h):
    """0, 1, 3 and 5 iterations, with and without demodulation, at shapes narrower than a halo and with spacings beyond the image."""
    rgba, aov = ref.synthetic(pkg, w, h, seed=w + h)
    moments = ref.synthetic_moments(rgba, seed=w + h)
    for iterations in (0, 1, 3, 5):
        for demodulate in (0, 1):
            got = driver.denoise(rgba, moments, aov, iterations, PARAMS["sigmaLuminance"], PARAMS["sigmaNormal"], PARAMS["sigmaPlane"], demodulate, PARAMS["scale"],
                                 PARAMS["unknownVariance"])
            want = reference_denoise(orc, rgba, moments, aov, iterations, demodulate)
            assert_same_bits(got, want, f"{w} x {h}, {iterations} iterations, demodulate {demodulate}")
            # exact properties of the definition itself
            scaled = rgba[..., :3] * F(PARAMS["scale"])
            unfiltered = (aov["object"] < 0) | ~np.isfinite(rgba[..., :3]).all(axis=-1)
            assert np.array_equal(got[..., :3].view(np.uint32)[unfiltered], scaled.view(np.uint32)[unfiltered])
            assert np.array_equal(got[..., 3].view(np.uint32), rgba[..., 3].view(np.uint32)), "alpha is the input's"
            if iterations == 0:
                assert np.array_equal(got[..., :3].view(np.uint32), scaled.view(np.uint32))
            elif w * h > 100:
                changed = (got[..., :3].view(np.uint32) != scaled.view(np.uint32)).any(axis=-1)
                assert changed[~unfiltered].mean() > 0.9  # it is a filter


@pytest.mark.parametrize("w,h", SHAPES)
def test_update_and_rebase_equal_the_numpy_restatement(orc, driver, w, h):
    now, snap, moments = ref.synthetic_sums(w, h, seed=w + h)
    for rebase in (0, 1):
        got_snap, got_m = driver.update(now, snap, moments, rebase)
        want_snap, want_m = ref.update(orc, now, snap, moments, rebase=bool(rebase))
        assert_same_bits(got_snap, want_snap, f"{w} x {h}: snapshot, rebase {rebase}")
        assert_same_bits(got_m, want_m, f"{w} x {h}: moments, rebase {rebase}")
        assert got_snap.tobytes() == now.tobytes()
        if rebase:
            assert got_m.tobytes() == moments.tobytes()


def test_the_variance_steers_the_filter(pkg, orc, driver):
    """The same image with a small and a large variance everywhere: a converged image is left nearly alone, a noisy one is smoothed."""
    rgba, aov = ref.synthetic(pkg, 48, 20, seed=3)
    hit = (aov["object"] >= 0) & np.isfinite(rgba[..., :3]).all(axis=-1)
    nb = F(16)
    with np.errstate(all="ignore"):
        mean = np.nan_to_num(ref.lum(rgba), nan=0, posinf=0, neginf=0).astype(F)

    def moments(sd):
        m = np.zeros(rgba.shape, dtype=F)
        m[..., 0], m[..., 1], m[..., 3] = mean * nb, (mean * mean + F(sd * sd)) * nb, nb
        return m
    args = (3, 1.0, 10.0, 10.0, 0, 1.0, 1.0)
    calm, noisy = driver.denoise(rgba, moments(1e-3), aov, *args), driver.denoise(rgba, moments(10.0), aov, *args)
    moved = lambda out: float(np.abs(out[..., :3][hit] - rgba[..., :3][hit]).mean())
    assert moved(calm) < 0.1 * moved(noisy), (moved(calm), moved(noisy))


# ---------------------------------------------------------------- 6. small integers, exactly
def image(*pixels):
    return np.array([list(pixels)], dtype=F)


def test_two_batches_with_luminance_1_and_3(pkg, orc, driver):
    """Grey batches, so L is the grey level (the weights of lum sum to 1 within rounding: checked): a frame of 1, then two frames of 3
    as ONE batch, give M = (4, 10, 0, 2).  The header's step 1 then gives mu = 2, d = 10 - 2 * 4 = 2 and var = d / (nb * (nb - 1)) = 2 / 2
    = 1, exactly: the unbiased sample variance of {1, 3} is 2, and the variance of the mean of two samples is half of it.  (The issue
    that asked for this feature names 0.5 for this case next to the very formula that yields 1; 0.5 is d / nb^2, the biased estimate,
    which would need no "nb >= 2" rule.  The formula is what is built, and this test holds it to its exact value.)"""
    assert ref.lum(np.array([1, 1, 1], dtype=F)) == 1 and ref.lum(np.array([3, 3, 3], dtype=F)) == 3
    zero = image((0, 0, 0, 0))
    s1 = image((1, 1, 1, 1))
    s2 = image((7, 7, 7, 3))  # + two frames of 3
    snap, m = driver.update(s1, zero, zero, 0)
    assert m.tolist() == [[[1, 1, 0, 1]]] and snap.tolist() == s1.tolist()
    snap, m = driver.update(s2, snap, m, 0)
    assert m.tolist() == [[[4, 10, 0, 2]]] and snap.tolist() == s2.tolist()
    assert ref.update(orc, s2, s1, image((1, 1, 0, 1)))[1].tolist() == [[[4, 10, 0, 2]]]
    grey = np.array([[[2, 2, 2]]], dtype=F)
    var = ref.variance(orc, m, grey, grey, np.zeros((1, 1, 3), dtype=bool), 99.0)
    assert var.tolist() == [[1.0]]
    # in demodulated units: albedo 1/2 doubles the colour, so the variance is four times as large
    assert ref.variance(orc, m, grey, grey * F(2), np.ones((1, 1, 3), dtype=bool), 99.0).tolist() == [[4.0]]
    # fewer than two batches, and 1.5 blended ones: unknown
    for nb in (0, 1, 1.5):
        assert ref.variance(orc, image((4, 10, 0, nb)), grey, grey, np.zeros((1, 1, 3), dtype=bool), 99.0).tolist() == [[99.0]]


def test_a_count_that_did_not_grow_leaves_the_moments_and_still_moves_the_snapshot(orc, driver):
    m0 = image((4, 10, 0, 2), (4, 10, 0, 2), (4, 10, 0, 2), (4, 10, 0, 2))
    snap = image((6, 6, 6, 3), (6, 6, 6, 3), (6, 6, 6, 3), (6, 6, 6, 3))
    now = image((9, 9, 9, 3), (1, 1, 1, 2), (np.inf, 8, 8, 4), (3e38, 3e38, 3e38, 4))  # dn = 0, dn < 0, a non-finite sum, a square that overflows
    for fn in (lambda: driver.update(now, snap, m0, 0), lambda: ref.update(orc, now, snap, m0)):
        got_snap, got_m = fn()
        assert got_m.tobytes() == m0.tobytes()
        assert got_snap.tobytes() == now.tobytes()


# ---------------------------------------------------------------- 7. the layout is one the reprojection carries
@pytest.mark.parametrize("case", ["translation", "rotation"])
def test_reprojection_carries_a_moments_image(pkg, orc, case):
    w, h = 40, 24
    sums, prev, cur, cam = rp.synthetic(pkg, w, h, case, seed=11)
    m = np.zeros((h, w, 4), dtype=F)
    rng = np.random.default_rng(4)
    nb = np.where(np.isfinite(sums[..., 3]) & (sums[..., 3] > 0), sums[..., 3], 0).astype(F)
    mean = rng.uniform(0.1, 2.0, (h, w)).astype(F)
    m[..., 0], m[..., 1], m[..., 3] = mean * nb, (mean * mean * F(1.5)) * nb, nb
    out = rp.reproject(orc, m, prev, cur, rp.VIEW_PARAMS, cam, 0.1, 0.9, 16.0)
    carried = out[..., 3] > 0
    assert carried.any() and (~carried).any()
    assert (out[..., 2].view(np.uint32) == 0).all(), "channel 2 is +0 everywhere"
    assert (out[..., 3] <= 16.0).all() and (out[..., 3][carried] > 0).all()
    assert np.isfinite(out).all() and (out[..., 1][carried] > 0).all()
    # the carried pixel's moments are blended MEANS times the blended count: the mean of L stays inside the range of the means
    mu = out[..., 0][carried] / out[..., 3][carried]
    assert mu.min() >= 0.1 * (1 - 1e-5) and mu.max() <= 2.0 * (1 + 1e-5)
