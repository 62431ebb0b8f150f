"""The launch predicate of ray-tracing_amd/csrc/rt_sky.h, proven on the host: when it accepts a launch's uniforms, GetEnvironmentLight
without the sun's addend has the bits of the whole function for every direction a frame kernel can hold.

tests/sky_sun_driver.cpp finds the edge of the gate (smoothstep(-0.01, 0, y) >= 1) by bisection and checks the header's constants against
it, compares the two forms over every float within 20,000 ulps of the edge, a stride over the rest of the gate-1 range, a stride over
|y| <= 2 and the special values — each crossed with (x, z) pairs that include +-0, +-inf and NaN — for a table of accepted parameter sets,
and asks the predicate to refuse each hazard on its own."""
import subprocess

import pytest

import host_driver

ACCEPTED = ["default", "near_the_bound", "y_half", "y_neg_zero", "y_pos_zero", "xz_neg_zero", "focus_low_end", "focus_high_end",
            "focus_high_end_dark", "scale_bounds", "negative_light"]
REFUSED = ["tilted_sun", "sun_above", "long_sun", "nan_sun", "focus_zero", "focus_huge", "focus_negative", "focus_nan", "intensity_inf",
           "intensity_nan", "colour_huge", "colour_nan", "visible_in_the_sliver", "sky_off"]


def build_and_run(tmp, extra):
    exe = host_driver.build(tmp, "sky_sun", ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", *extra])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, check=True).stdout
    rows = {}
    for line in out.splitlines():
        name, *fields = line.split()
        rows[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return rows


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    return build_and_run(tmp_path_factory.mktemp("sky_sun"), ["-O2"])


def test_gate_edge_is_the_headers_and_y0_covers_it(rows):
    g = rows["gate"]
    assert g["ends_ok"] == 1
    assert g["edge_bits"] == g["header_bits"] == 0xB567A000
    assert g["y0_covers"] == 1 and g["y0_power_of_two"] == 1


def test_gate_is_monotone_around_its_edge(rows):
    assert rows["gate"]["not_monotone"] == 0


@pytest.mark.parametrize("name", ACCEPTED)
def test_accepted_set_has_the_bits_of_the_whole_function(rows, name):
    r = rows["accept_" + name]
    assert r["accepted"] == 1, r
    assert r["evals"] > 1_000_000
    assert r["differ"] == 0, r


@pytest.mark.parametrize("name", REFUSED)
def test_predicate_refuses(rows, name):
    assert rows["refuse_" + name]["accepted"] == 0


def test_every_row_of_the_driver_is_asserted(rows):
    assert sorted(rows) == sorted(["gate", "unnormalised_direction"] + ["accept_" + n for n in ACCEPTED] + ["refuse_" + n for n in REFUSED])


def test_an_unnormalised_direction_is_why_the_side_passes_keep_the_whole_function(rows):
    """(0, -1e30, 0) under the default sun: NaN with the sun's addend, the plain blend without"""
    r = rows["unnormalised_direction"]
    assert r["differ"] == 1 and r["full_is_nan"] == 1


def test_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path, rows):
    san = build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert san == rows
