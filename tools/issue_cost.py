"""Issue-cost accounting of one trace kernel: every VALU instruction of the kernel attributed to the source function it was inlined from and to
the phase of a wave iteration it runs in, classed fast / base / packed / quarter after profiles/r03_valu_op_rates.txt, and weighted by how often
the phase runs per wave iteration (the STATS phase profile that `RT_PHASES=1 RT_PHASE_FRAMES=16 python tools/qb.py 2 16` prints).

Needs a device code object with line tables: `make -C ray-tracing_amd/csrc asm EXTRA=-gline-tables-only` leaves it in build/asm/ (the
*-gfx950.out file).  The attribution is the debug info's own inline stack per instruction (llvm-symbolizer --inlines), not a guess from the
listing's order: the innermost frame names the function, the trace_body / begin_intersect / traverse_flat frames name the call site.

usage: python tools/issue_cost.py <code object> <phase profile text> [--kernel=MANGLED] [--by=function|site] [--list=FUNCTION] [--src=TREE]
   --by=site adds the call site to every row; --list prints the instructions under FUNCTION with their stacks; --src names the tree the code
   object was built from when it is not this one (the phase boundaries are found in its text)
Static counts x executions x class cost: a model.  It knows nothing of lanes switched off inside a phase (both sides of a per-lane branch are
counted as executed) and nothing of scalar or memory time."""
import collections, os, re, subprocess, sys

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
KERNEL = "_ZN3rtk15rt_trace_kernelILb0ELb1ELb0ELb1EEEv5KArgs"
N_SPHERES = 16  # config 2: the pre-test loop of the general branch runs once per pair of spheres; its root leaf holds two triangles
COST = {"fast": 2.7, "base": 4.4, "packed": 5.0, "quarter": 8.2}  # cycles per wave64 instruction per SIMD (r03; packed: csrc/Makefile)

FAST = re.compile(r"v_(add|sub|subrev|mul|fma|fmac|mac|mad)_f32|v_mov_b32|v_(xor|and|or|not)_b32|v_(lshlrev|lshrrev|ashrrev)_b32|"
                  r"v_(add|sub|subrev)_u32|v_(add|sub|subrev)_co_u32|v_accvgpr|v_nop")
QUARTER = re.compile(r"v_(rcp|rsq|sqrt|exp|log|sin|cos)_")
SGPR_SRC = re.compile(r"\b(s\d+|s\[\d+:\d+\]|ttmp\d+|m0)\b")


def classify(mnem, ops):
    if QUARTER.match(mnem): return "quarter"
    if mnem.startswith("v_pk_"): return "packed"
    if not FAST.match(mnem): return "base"
    srcs = ops.split(",")[1:]
    if mnem.startswith("v_cmp"): srcs = ops.split(",")
    return "base" if any(SGPR_SRC.search(s) for s in srcs) else "fast"


def disassemble(obj, kernel):
    out = subprocess.run([f"{LLVM}/llvm-objdump", "-d", f"--disassemble-symbols={kernel}", obj], check=True, capture_output=True, text=True).stdout
    insts = []
    for l in out.split("\n"):
        m = re.match(r"\s+(\S+)\s*(.*?)\s*// ([0-9A-F]{12}):", l)
        if m: insts.append((int(m.group(3), 16), m.group(1), m.group(2)))
    return insts


def symbolize(obj, addrs):
    p = subprocess.run([f"{LLVM}/llvm-symbolizer", f"--obj={obj}", "--inlines", "--functions=short", "--basenames"],
                       input="".join(f"0x{a:x}\n" for a in addrs), check=True, capture_output=True, text=True).stdout
    stacks = []
    for block in p.strip("\n").split("\n\n"):
        ls = block.split("\n")
        fr = []
        for k in range(0, len(ls) - 1, 2):
            f, line = ls[k + 1].rsplit(":", 2)[0:2]
            fr.append((re.sub(r"<.*", "", ls[k]), ls[k], f, int(line)))
        stacks.append(fr)  # innermost first: (function, function with template arguments, file, line within that function)
    assert len(stacks) == len(addrs), (len(stacks), len(addrs))
    return stacks


SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")  # --src=DIR: the tree the code object was built from, when it is not this one


def anchors():
    """line numbers of the phase boundaries inside trace_body, found by their text so that they follow the source"""
    root = os.path.join(SRC, "ray-tracing_amd", "csrc")
    src = open(os.path.join(root, "rt_kernels.h")).read()
    blk = open(os.path.join(root, "rt_shade_block.inl")).read()
    def line(text, s=src):
        assert s.count(text) == 1, text
        return s[:s.index(text)].count("\n") + 1
    return {"refill": line("---- hand pixels to idle lanes"), "loop": line("phase_mark<STATS>(st, PH_LOOP)"), "raygen": line("if (!laneDone && sample < c.spp)"),
            "spheres": line("phase_mark<STATS>(st, PH_SPHERES)"), "tail": line("if constexpr (!POOL) {\n#include"), "epilogue": line("exact work counters"), "defocus": src[:src.index("rt_f2 dj = rand_circle(&rng);", src.index("void trace_body("))].count("\n") + 1,
            "fallback": fallback_ranges(),
            "table_end": line("    } else {\n        const RT_CAS float* sph = (const RT_CAS float*)a.spheres;"),
            "shade_hit": line("resolve the winner", blk), "glass": line("phase_mark<STATS>(st, PH_GLASS)", blk), "opaque": line("bool isSpecular = mat.specularProbability >= uSpec", blk)}


WRAPPERS = ("rt_pow", "rt_normalize", "rt_smoothstep_edges", "rt_div", "operator/", "rt_linear_to_srgb")
MATH = ("rt_math.h", "rt_math_device.h")  # the second: the kernels' own sequences (rtd_*), listed under the names of the functions they restate


def label(stack):
    """the math function an instruction belongs to: the outermost frame in a math header, looking through the wrappers above; else the file"""
    inner = [(f[0].replace("rtd_", "rt_"),) + f[1:] for f in stack if f[2] in MATH]
    for k in range(len(inner) - 1, -1, -1):
        if k == 0 or inner[k][0] not in WRAPPERS: return {"rt_exp_ordinary": "rt_exp"}.get(inner[k][0], inner[k][0])
    return "(" + stack[0][2] + ")"


def fallback_ranges():
    """rt_math.h keeps each function's special cases (zeros, infinities, NaNs, subnormals, huge arguments) in a per-lane copy behind the
    wave-uniform one (RT_WAVE_ALL), and the IEEE divide / sqrt sequences behind the short ones: line ranges of those copies, which a wave of
    ordinary values never issues.  Found by their text."""
    out = []
    for name, path in (("rt_math.h", os.path.join(SRC, "include", "rt_math.h")), ("rt_math_device.h", os.path.join(SRC, "ray-tracing_amd", "csrc", "rt_math_device.h"))):
        if not os.path.exists(path): continue
        src = open(path).read().split("\n")
        for k, l in enumerate(src):
            if "RT_WAVE_ALL(" in l and "#define" not in l and "*" not in l[:3]:
                e = k if l.rstrip().endswith(";") else next(j for j in range(k, len(src)) if src[j] == "    }")
                out.append((name, e + 2, next(j for j in range(e, len(src)) if src[j] == "}") + 1))
            if l.strip() in ("return __builtin_sqrtf(x);", "return 1.0f / x;"): out.append((name, k + 1, k + 1))
    return out


def phase_of(stack, A):
    """(phase, call site) of one instruction from its inline stack"""
    if any(any(f[2] == n and a <= f[3] <= b for n, a, b in A["fallback"]) for f in stack): return "fallback", ""
    fn = [f[0] for f in stack]
    by = {f[0]: f for f in reversed(stack)}  # innermost frame of each function
    site = ""
    if "begin_intersect" in by:
        f = by["begin_intersect"]
        src_line = f[3]
        in_roots = (A["roots_table"][0] <= src_line <= A["roots_table"][1]) or (A["roots_general"][0] <= src_line <= A["roots_general"][1])
        kind = "table" if src_line < A["table_end"] else ("pretest" if A["pretest"][0] <= src_line <= A["pretest"][1] else "general")
        targs = f[1][f[1].index("<") + 1:].rstrip(">").replace(" ", "").split(",")  # <STATS, FLAT, MANY, ANY, PRIMARY, ...>
        if kind != "table" and len(targs) > 4 and targs[4] == "true": return "no_tile_table", f"begin_intersect:{src_line}"  # all-camera-ray waves of a launch without the tile table
        if in_roots: return ("roots_table" if kind == "table" else "roots_general"), f"begin_intersect:{src_line}"
        return "spheres_" + kind, f"begin_intersect:{src_line}"
    if "traverse_flat" in by:
        f = by["traverse_flat"]
        kind = "table" if f[1].replace(" ", "").endswith(",true>") else "general"  # traverse_flat<STATS, ANY, PRIMARY>
        return ("tri_" if "tri_test" in by else "trav_") + kind, f"traverse_flat:{f[3]}"
    if "pool_exchange" in by: return "loop", f"pool_exchange:{by['pool_exchange'][3]}"
    if "trace_body" not in by: return "once", fn[-1]
    f = by["trace_body"]
    if f[2] == "rt_shade_block.inl":
        ln = f[3]
        site = f"shade_block:{ln}"
        if ln < A["shade_hit"]: return "sky", site
        if "rand_normal" in by: return "rand_normal", site
        if A["glass"] <= ln < A["opaque"]: return "glass", site
        return "shade_hit", site
    if f[2] == "rt_shade_phase.inl": return "loop", f"shade_phase:{f[3]}"
    ln = f[3]
    site = f"trace_body:{ln}"
    if ln >= A["epilogue"] or ln < A["refill"]: return "once", site
    if ln < A["loop"]: return "refill", site
    if ln < A["raygen"]: return "loop", site
    if A["defocus"] <= ln <= A["defocus"] + 1: return "defocus", site
    if ln < A["spheres"]: return "raygen", site
    return ("spheres" if ln < A["tail"] else "loop"), site


def read_phases(path):
    ph = {}
    for l in open(path):
        m = re.match(r"\s+(\w+)\s+wave-execs\s+(\d+)\s+lanes\s+(\d+)", l)
        if m: ph[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    return ph


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opts = dict((a.split("=", 1) + ["1"])[:2] for a in sys.argv[1:] if a.startswith("--"))
    obj, phases = args[0], read_phases(args[1])
    kernel = opts.get("--kernel", KERNEL)
    global SRC
    SRC = opts.get("--src", SRC)
    A = anchors()
    src = open(os.path.join(SRC, "ray-tracing_amd", "csrc", "rt_kernels.h")).read().split("\n")
    marks = [k + 1 for k, l in enumerate(src) if "phase_mark<STATS>(st, PH_SPHERE_ROOTS)" in l]
    ends = [k + 1 for k, l in enumerate(src) if l.strip() in ("} while (cand != 0u);", "if (ANY && d < tmax) cand = 0;")]
    A["pretest"] = (next(k + 1 for k, l in enumerate(src) if "for (int k = 0; k < n; k += 2) {" in l), next(k + 1 for k, l in enumerate(src) if "cand |= ((keep0 ? 1u : 0u) << k)" in l))
    A["roots_table"] = (marks[0] - 1, ends[0]); A["roots_general"] = (marks[1] - 1, ends[1] + 4)

    loop = phases["loop"][0]
    # executions per wave iteration.  The profile does not split `spheres` into the table branch (all-camera-ray waves) and the general one; the
    # split below is r16's reading (as many table intersections as sky executions), marked as an estimate in the output.
    table = min(phases["sky"][0], phases["spheres"][0])
    per = {"loop": 1.0, "once": 0.0, "fallback": 0.0, "defocus": 0.0, "no_tile_table": 0.0, "raygen": phases["raygen"][0] / loop, "spheres": phases["spheres"][0] / loop, "spheres_table": table / loop,
           "spheres_general": (phases["spheres"][0] - table) / loop, "roots_table": phases["sphere_roots"][0] / loop * table / phases["spheres"][0], "roots_general": phases["sphere_roots"][0] / loop * (1.0 - table / phases["spheres"][0]),
           "spheres_pretest": (phases["spheres"][0] - table) / loop * ((N_SPHERES + 1) // 2), "trav_table": table / loop, "trav_general": (phases["spheres"][0] - table) / loop,
           "tri_general": 2.0 * (phases["spheres"][0] - table) / loop, "tri_table": (phases["tri"][0] - 2.0 * (phases["spheres"][0] - table)) / loop,
           "sky": phases["sky"][0] / loop, "shade_hit": phases["shade_hit"][0] / loop, "rand_normal": 3.0 * phases["shade_hit"][0] / loop,
           "glass": phases["glass"][0] / loop, "refill": phases["refill"][0] / loop}

    insts = disassemble(obj, kernel)
    valu = [(a, m, o) for a, m, o in insts if m.startswith("v_")]
    stacks = symbolize(obj, [a for a, _, _ in valu])
    rows = collections.defaultdict(lambda: collections.Counter())
    listing = []
    for (a, m, o), st in zip(valu, stacks):
        cls = classify(m, o)
        phase, site = phase_of(st, A)
        func = label(st)
        key = (func, phase) if opts.get("--by", "function") == "function" else (func, phase, site)
        rows[key][cls] += 1
        if opts.get("--list") and opts["--list"] in [f[0] for f in st]:
            listing.append(f"  {phase:14s} {cls:7s} {m:22s} {o:46s} " + " < ".join(f"{f[0]}:{f[3]}" for f in st[:4]))

    total = sum(sum(COST[c] * n for c, n in r.items()) * per[k[1]] for k, r in rows.items())
    print(f"kernel {kernel}: {len(insts)} instructions, {len(valu)} VALU, {sum(1 for _, m, _ in insts if m.startswith('s_'))} SALU")
    print("executions per wave iteration: " + "  ".join(f"{k} {v:.3f}" for k, v in per.items() if v) + "   (the split of spheres, tri and sphere_roots into table / general: estimates, see the source)")
    print(f"class cost (cycles per wave64 instruction per SIMD): {COST}")
    print(f"{'function / file':30s} {'phase':16s} {'fast':>5s} {'base':>5s} {'pk':>4s} {'qtr':>4s} {'execs':>6s} {'cycles':>8s} {'share':>6s}")
    agg = collections.Counter()
    for k, r in sorted(rows.items(), key=lambda kr: -sum(COST[c] * n for c, n in kr[1].items()) * per[kr[0][1]]):
        cyc = sum(COST[c] * n for c, n in r.items()) * per[k[1]]
        agg[k[1]] += cyc
        print(f"{k[0][:30]:30s} {k[1]:16s} {r['fast']:5d} {r['base']:5d} {r['packed']:4d} {r['quarter']:4d} {per[k[1]]:6.3f} {cyc:8.1f} {cyc / total:6.2%}" + (f"  {k[2]}" if len(k) > 2 else ""))
    print(f"{'weighted total per wave iteration':80s} {total:8.1f}")
    print(f"modelled VALU instructions per wave iteration: {sum(sum(r.values()) * per[k[1]] for k, r in rows.items()):.0f}"
          "   (measured: SQ_INSTS_VALU of a launch / `loop` wave-execs)")
    print("by phase: " + "  ".join(f"{p} {c / total:.1%}" for p, c in agg.most_common()))
    for l in listing: print(l)


if __name__ == "__main__":
    main()
