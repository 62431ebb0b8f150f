"""The stand-alone host programs of the CPU tests (tests/*_driver.cpp): finding the compiler, building one, and the line protocol
several of them speak.  The flags are the caller's: what a driver is built with is part of what its test checks."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compiler():
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    return cxx


def build(directory, name, flags, exe="driver", after=()):
    """tests/<name>_driver.cpp compiled with `flags` into <directory>/<exe> (`after`: what follows the output on the command line);
    returns the executable's path"""
    exe = str(directory / exe)
    subprocess.check_call([compiler(), *flags, os.path.join(ROOT, "tests", name + "_driver.cpp"), "-o", exe, *after])
    return exe


def ask(exe, *requests):
    """requests: (command, {key: value}); one dict of the answer's fields per request"""
    text = "".join(cmd + "".join(f" {k}={int(v) if isinstance(v, bool) else v}" for k, v in kw.items()) + "\n" for cmd, kw in requests)
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600, check=True).stdout.splitlines()
    assert len(lines) == len(requests), lines[:3]
    out = []
    for line in lines:
        assert "=" in line and not line.startswith(("ERROR", "BROKEN")), line
        out.append({k: float(v) if "." in v else int(v) for k, v in (t.split("=") for t in line.split())})
    return out
