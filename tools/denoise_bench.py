#!/usr/bin/env python3
"""Times rt_denoise_buffers (include/rt_denoise.h) on one GPU: config 3's accumulated image and AOV records at 1920 x 1080, 5 iterations,
demodulation on.

HIP events on the stream the context renders on (a stream of this tool's, given to rt_set_stream) around back-to-back enqueued calls;
after a warm-up, each figure is the median of --regions regions (default 9, at least 7) of at least --region-ms (default 60, at least 50)
each, with the regions' minimum and maximum next to it.  The passes run inside one call, so a pass is timed as the MARGINAL cost of its
spacing: t(k iterations) - t(k - 1 iterations) is the pass with spacing 2^(k-1) (both calls end in a pass with the fused finish step, whose
extra 16-byte load per pixel cancels).  Bytes: 48 per tap fetched algorithmically (25 taps per filtered pixel), 64 per pixel compulsory
(colour in, guide in, colour out).  Prints one JSON line; --out FILE also writes the tables as text.

Every kernel on its own, spacing 1 and the prepare kernel included, comes from a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/denoise_bench.py --trace-calls 40
    python tools/denoise_bench.py --parse-trace DIR
The second command needs no GPU: it reads the dispatches of the rt_dn_* kernels in order (prepare, then one pass per spacing, per call),
drops the first 5 calls and prints per kernel the median, minimum and maximum duration.  Two builds of the library (RT_HIP_LIB) measured
this way in one session are how the plain global-load form and the LDS-tiled form of a pass are compared (profiles/r07_denoise.txt)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def parse_trace(root, iterations):
    import csv
    import glob
    rows = []
    for path in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name") or r.get("kernel_name") or ""
                if "rt_dn_" in name:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), name))
    rows.sort()
    per_call = iterations + 1
    # the filter's dispatches of the timed calls: the last whole groups of (prepare, pass 0 ... pass iterations-1)
    starts = [k for k, r in enumerate(rows) if "prepare" in r[2]]
    calls = [rows[k:k + per_call] for k in starts if len(rows[k:k + per_call]) == per_call and all("pass" in q[2] for q in rows[k + 1:k + per_call])]
    calls = calls[5:]
    if not calls:
        raise SystemExit("no complete rt_denoise_buffers call found in the trace")
    out = {"tool": "denoise_bench", "mode": "kernel trace", "calls": len(calls), "kernels": []}
    for pos in range(per_call):
        d = sorted(c[pos][1] / 1e6 for c in calls)
        kind = "prepare" if pos == 0 else ("tiled" if "tiled" in calls[0][pos][2] else "plain")
        out["kernels"].append({"kernel": "prepare" if pos == 0 else f"pass spacing {1 << (pos - 1)}", "form": kind, "median_ms": statistics.median(d), "min_ms": d[0], "max_ms": d[-1]})
    out["sum_of_medians_ms"] = sum(k["median_ms"] for k in out["kernels"])
    print(json.dumps(out))
    for k in out["kernels"]:
        print(f"{k['kernel']:>18}  {k['form']:>7}  {k['median_ms']:.4f} ms  [{k['min_ms']:.4f}, {k['max_ms']:.4f}]")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4, help="frames accumulated before the filter runs")
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--region-ms", type=float, default=60.0)
    ap.add_argument("--out", help="also write the tables to this text file")
    ap.add_argument("--trace-calls", type=int, help="no event timing: 5 warm-up calls and this many calls, for a run under rocprofv3 --kernel-trace")
    ap.add_argument("--parse-trace", metavar="DIR", help="no GPU: per-kernel durations from the *kernel_trace.csv files under DIR")
    a = ap.parse_args()
    if a.parse_trace:
        return parse_trace(a.parse_trace, a.iterations)
    if a.regions < 7 or a.region_ms < 50:
        ap.error("at least 7 regions of at least 50 ms")
    pkg = graft.load_package()
    api = pkg.load_library()
    hip = C.CDLL("libamdhip64.so")

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP call failed with {rc}")
    w, h = a.width, a.height
    tr = api.create_tracer(0)
    mgr = pkg.scenes.get(3).make_manager(tr, api, w, h)
    mgr.OnEnable(renderSeed=1)
    mgr.RenderFrames(a.frames)
    tr.synchronize()
    stream = C.c_void_p()
    ok(hip.hipStreamCreate(C.byref(stream)))
    tr.set_stream(stream)
    d_aov, d_out = C.c_void_p(), C.c_void_p()
    ok(hip.hipMalloc(C.byref(d_aov), C.c_size_t(w * h * 64)))
    ok(hip.hipMalloc(C.byref(d_out), C.c_size_t(w * h * 16)))
    tr.render_aov_to_device(1, d_aov.value, w * h * 64)
    tr.synchronize()
    _, d_acc = tr.render_targets()
    aov = tr.render_aov(1)
    filtered = int((aov["object"] >= 0).sum())
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        ok(hip.hipEventCreate(C.byref(e)))

    if a.trace_calls:
        p = api.denoise_params(iterations=a.iterations, demodulate=1, scale=1.0 / a.frames)
        for _ in range(5 + a.trace_calls):
            tr.denoise_buffers(w, h, d_acc, d_aov.value, d_out.value, p)
        tr.synchronize()
        tr.set_stream(None)
        tr.close()
        print(json.dumps({"tool": "denoise_bench", "traced_calls": a.trace_calls, "warm_up_calls": 5}))
        return

    def region(params, calls):
        ok(hip.hipEventRecord(ev[0], stream))
        for _ in range(calls):
            tr.denoise_buffers(w, h, d_acc, d_aov.value, d_out.value, params)
        ok(hip.hipEventRecord(ev[1], stream))
        ok(hip.hipEventSynchronize(ev[1]))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
        return ms.value / calls

    def measure(k):
        p = api.denoise_params(iterations=k, demodulate=1, scale=1.0 / a.frames)
        one = max(min(region(p, 3), region(p, 3)), 1e-3)  # warm-up, and the call count a region needs
        calls = max(3, int(a.region_ms / one) + 1)
        region(p, calls)
        return sorted(region(p, calls) for _ in range(a.regions)), calls
    rows = []
    for k in range(0, a.iterations + 1):
        t, calls = measure(k)
        rows.append({"iterations": k, "median_ms": statistics.median(t), "min_ms": t[0], "max_ms": t[-1], "calls_per_region": calls})
    passes = []
    for k in range(2, a.iterations + 1):  # (k = 1 also holds the prepare kernel: listed as it is)
        m = rows[k]["median_ms"] - rows[k - 1]["median_ms"]
        spread = (rows[k]["max_ms"] - rows[k]["min_ms"]) + (rows[k - 1]["max_ms"] - rows[k - 1]["min_ms"])
        tap_bytes = filtered * 25 * 48
        passes.append({"spacing": 1 << (k - 1), "marginal_ms": m, "spread_ms": spread, "algorithmic_GB": tap_bytes / 1e9, "compulsory_GB": w * h * 64 / 1e9,
                       "algorithmic_TB_per_s": tap_bytes / 1e9 / max(m, 1e-9), "compulsory_GB_per_s": w * h * 64 / 1e6 / max(m, 1e-9)})
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    full = rows[a.iterations]
    result = {"tool": "denoise_bench", "width": w, "height": h, "iterations": a.iterations, "frames": a.frames, "filtered_pixels": filtered,
              "ms_per_denoise": full["median_ms"], "ms_min": full["min_ms"], "ms_max": full["max_ms"],
              "regions": a.regions, "region_ms": a.region_ms, "by_iterations": rows, "passes": passes, "commit": commit}
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"rt_denoise_buffers, {w} x {h}, config 3 ({a.frames} frames accumulated), demodulation on; commit {commit}\n")
            f.write(f"{filtered} of {w * h} pixels filtered (hits); median of {a.regions} regions of >= {a.region_ms:g} ms, [min, max] of the regions\n\n")
            f.write("iterations   ms per call   [min, max]\n")
            for r in rows:
                f.write(f"{r['iterations']:10d}   {r['median_ms']:11.4f}   [{r['min_ms']:.4f}, {r['max_ms']:.4f}]\n")
            f.write("\n(0 iterations: the scaled copy; 1: prepare + the pass with spacing 1 and the fused finish)\n\n")
            f.write("spacing   marginal ms   spread ms   algorithmic GB (48 B x 25 taps)   TB/s   compulsory GB (64 B/pixel)   GB/s\n")
            for q in passes:
                f.write(f"{q['spacing']:7d}   {q['marginal_ms']:11.4f}   {q['spread_ms']:9.4f}   {q['algorithmic_GB']:31.3f}   {q['algorithmic_TB_per_s']:4.2f}   "
                        f"{q['compulsory_GB']:26.3f}   {q['compulsory_GB_per_s']:4.0f}\n")
    print(json.dumps(result))
    tr.set_stream(None)
    tr.close()
    hip.hipFree(d_aov)
    hip.hipFree(d_out)


if __name__ == "__main__":
    main()
