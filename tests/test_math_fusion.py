"""The exact-product fusions of the kernels' math sequences (ray-tracing_amd/csrc/rt_math_device.h), proven on the host.

tests/math_fusion_driver.cpp enumerates, for each fused step, every multiplier the function can produce, decides with the double-precision
product whether the binary32 product is exact, and compares std::fma with multiply-then-add bit for bit over addends the function meets.
A fusion is sound where `inexact` and `differ` are 0.  The second Cody-Waite step of rt_reduce_pio2 is the counter-example the header keeps
unfused: exact for |n| < 2^13, not for every n that |x| < 3e4 admits."""
import subprocess

import pytest

import host_driver

FUSED = ["reduce_P1", "cos_half_z", "smoothstep_2t", "exp_k_ln2hi", "log_k_ln2hi"]


def build_and_run(tmp, extra):
    exe = host_driver.build(tmp, "math_fusion", ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", *extra])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, check=True).stdout
    rows = {}
    for line in out.splitlines():
        name, *fields = line.split()
        rows[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return rows


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    return build_and_run(tmp_path_factory.mktemp("math_fusion"), ["-O2"])


@pytest.mark.parametrize("name", FUSED)
def test_fused_product_is_exact_and_fma_has_the_same_bits(rows, name):
    r = rows[name]
    assert r["multipliers"] > 0 and r["addends"] >= r["multipliers"]
    assert r["inexact"] == 0, r
    assert r["differ"] == 0, r


def test_multiplier_ranges_cover_what_the_functions_produce(rows):
    assert rows["reduce_P1"]["multipliers"] == 2 * 19100 + 1  # |x| < 3e4: |n| <= 19099
    assert rows["exp_k_ln2hi"]["multipliers"] == 129 + 151 + 1  # -103.98 < x < 88.73: k = -150 ... 128, one wider
    assert rows["log_k_ln2hi"]["multipliers"] == 129 + 150 + 1  # exponents -149 (subnormals) ... 128, one wider


def test_halving_below_the_exact_range_still_gives_the_same_result(rows):
    """z / 2 can drop a bit for z < 2^-125; 1 - z / 2 is 1 in both forms there"""
    r = rows["cos_half_z_below_2^-125"]
    assert r["inexact"] > 0 and r["differ"] == 0, r


def test_second_reduction_step_is_not_exact_for_every_argument(rows):
    """why t - n P2 stays a multiply and a subtract"""
    assert rows["reduce_P2_below_8192"]["inexact"] == 0
    assert rows["reduce_P2_above"]["inexact"] > 0


def test_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path, rows):
    san = build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert san == rows
