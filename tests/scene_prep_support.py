"""Talking to tests/scene_prep_driver.cpp: the scene file it reads, its request lines and its answers."""
import os
import subprocess

import numpy as np

FILTER = np.dtype([("bMin", "<f4", 3), ("bMax", "<f4", 3), ("always", "<u4"), ("innerRoot", "<u4")])


def _parse(buf):
    """The driver's answers in order: a dict per `key=value` line (msg = the rest of the line), bytes per dump"""
    out, pos = [], 0
    while pos < len(buf):
        nl = buf.index(b"\n", pos)
        line, pos = buf[pos:nl].decode(), nl + 1
        assert not line.startswith("ERROR"), line
        if line.startswith("bytes="):
            n = int(line[6:])
            out.append(buf[pos:pos + n])
            assert len(out[-1]) == n
            pos += n
            continue
        head, _, msg = line.partition(" msg=")
        d = {k: int(v) for k, v in (t.split("=") for t in head.split())}
        if " msg=" in line:
            d["msg"] = msg
        out.append(d)
    return out


def ask(exe, requests, env=None, timeout=900):
    """Runs the driver over the request lines; a sanitizer report (or any other failure) is a non-zero exit"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("RT_")}
    e.update(env or {})
    p = subprocess.run([exe], input=("\n".join(requests) + "\n").encode(), capture_output=True, env=e, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-4000:], p.stdout[-300:])
    return _parse(p.stdout)


def write_scene(path, models, tris, nodes, spheres):
    with open(path, "wb") as f:
        f.write(np.array([len(models), len(tris), len(nodes), len(spheres)], dtype="<i4").tobytes())
        for a in (models, tris, nodes, spheres):
            f.write(np.ascontiguousarray(a).tobytes())
