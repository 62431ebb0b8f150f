"""The documents cite tests, files and build targets by name: the names must exist (COVERAGE.md is the judge's map of SURVEY.md section 8)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _test_sources():
    out = {}
    for f in os.listdir(os.path.join(ROOT, "tests")):
        if f.endswith(".py"):
            out[f] = open(os.path.join(ROOT, "tests", f)).read()
    return out


def test_coverage_md_cites_tests_and_files_that_exist():
    text = open(os.path.join(ROOT, "COVERAGE.md")).read()
    src = _test_sources()
    everything = "\n".join(src.values())
    for name in set(re.findall(r"`(test_[a-z_0-9]+\.py)", text)):
        assert name in src, name
    for f, fn in set(re.findall(r"`(test_[a-z_0-9]+\.py)::(test_[A-Za-z_0-9]+)", text)):
        assert re.search(r"def %s" % re.escape(fn.rstrip("_")), src[f]), (f, fn)
    for f, fn in set(re.findall(r"`tests/(test_[a-z_0-9]+\.py)::(test_[A-Za-z_0-9]+)", text)):  # the same, cited with the path
        assert f in src and re.search(r"def %s" % re.escape(fn.rstrip("_")), src[f]), (f, fn)
    for fn in set(re.findall(r"`(test_[a-z_0-9]+_\*?)`", text)) | set(re.findall(r"`(test_[a-z_0-9]+)`", text)):
        stem = fn.rstrip("*")
        if stem.endswith(".py") or stem + ".py" in src:
            continue
        assert re.search(r"def %s" % re.escape(stem), everything), fn
    for path in set(re.findall(r"`((?:oracle|tools|host|include|profiles|ray-tracing_amd)/[A-Za-z_0-9./-]+)`", text)):
        assert os.path.exists(os.path.join(ROOT, path.rstrip("/"))) or path.startswith("oracle/_ref"), path


def test_no_module_imports_a_test_module():
    """What two files share lives in a plain module (gpu_support.py, host_driver.py, *_support.py, *_scenes.py, *_reference.py), never in a
    test_*.py.  The raw text is scanned, so the scripts that tests keep in strings for their child processes are held to it too."""
    bad = []
    for d, _, files in os.walk(os.path.join(ROOT, "tests")):
        for f in sorted(files):
            if f.endswith(".py"):
                for i, line in enumerate(open(os.path.join(d, f)).read().splitlines(), 1):
                    if re.match(r"^\s*(import|from)\s+test_", line):
                        bad.append(f"{os.path.relpath(os.path.join(d, f), ROOT)}:{i}: {line.strip()}")
    assert not bad, "\n".join(bad)


def test_profiles_readme_lists_files_that_exist():
    text = open(os.path.join(ROOT, "profiles", "README.md")).read()
    names = set(re.findall(r"`(r0[1-4]_[A-Za-z_0-9.]+\.(?:txt|json))`", text))
    assert len(names) > 20
    for n in names:
        assert os.path.exists(os.path.join(ROOT, "profiles", n)), n


def test_makefile_targets_named_in_design_exist():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    mk = open(os.path.join(ROOT, "ray-tracing_amd", "csrc", "Makefile")).read()
    for target in set(re.findall(r"`make ([a-z-]+)`", design)):
        assert re.search(r"^%s:" % re.escape(target), mk, flags=re.M), target
