"""tests/flush_table.py covers the C ABI: every function of include/*.h that takes a context has exactly one place in the table of the
hold-back contract, so a new entry point cannot be added without saying whether it launches the frames rt_render_frame holds back.
A function takes a context as its first parameter, or inside the call descriptor its first parameter points to, as rt_mis_trace does.
No GPU: the headers are parsed the way tests/test_abi.py parses them."""
import glob
import os
import re

import flush_table as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTEXT_TYPES = ("RtContext", "RtMulti")


def _blank_comments(text):
    """comments blanked, not removed: offsets into `text` stay valid for finding the comment above a declaration"""
    return re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)


def descriptor_types(paths):
    """the structs declared in these headers (`typedef struct [Tag] { ... } Name;`) that have an RtContext* / RtMulti* member: a call
    descriptor names the context it is for, so a function whose first parameter points to one is a call on that context"""
    out = set()
    member = re.compile(r"(?:^|[;{])\s*(?:const\s+)?(?:%s)\s*\*\s*[A-Za-z_0-9]+\s*(?=;)" % "|".join(CONTEXT_TYPES))
    for path in paths:
        code = _blank_comments(open(path).read())
        for m in re.finditer(r"\btypedef\s+struct\s*[A-Za-z_0-9]*\s*\{([^{}]*)\}\s*([A-Za-z_0-9]+)\s*;", code):
            if member.search(m.group(1)):
                out.add(m.group(2))
    return out


def declared(headers=None):
    """{function: (header, the comment right above its declaration)} for every function declared in include/*.h whose first parameter is
    an RtContext* / RtMulti* (const or not) or a pointer to a call descriptor (descriptor_types of the same headers), plus the two that
    create one"""
    out = {}
    paths = sorted(headers or glob.glob(os.path.join(ROOT, "include", "*.h")))
    takes = "|".join(sorted(set(CONTEXT_TYPES) | descriptor_types(paths)))
    for path in paths:
        text = open(path).read()
        code = _blank_comments(text)
        for m in re.finditer(r"\b(rt_[a-z_0-9]+)\s*\(([^;{()]*)\)\s*;", code):
            name, first = m.group(1), re.sub(r"\s+", " ", m.group(2).split(",")[0]).strip()
            takes_context = re.fullmatch(r"(?:const )?(%s) ?\* ?[A-Za-z_0-9]*" % takes, first) is not None
            if not takes_context and name not in ft.CREATES_ALLOWED:
                continue
            start = code.rfind("\n", 0, m.start()) + 1          # the declaration's line (its return type sits in front of the name)
            before = text[:start].rstrip()
            comment = before[before.rfind("/*"):] if before.endswith("*/") else ""
            if name in out:     # only rt_held_back.h may restate a declaration of rt_abi.h, to say in its comment which side it is on
                assert os.path.basename(path) == "rt_held_back.h" and out[name][0] == "rt_abi.h", f"{name} is declared twice ({out[name][0]}, {path})"
                out[name] = (out[name][0], out[name][1] + " " + comment)
            else:
                out[name] = (os.path.basename(path), comment)
    return out


def problems(decl, rows):
    """what is wrong with the table for these declarations, as a list of sentences"""
    bad = []
    names = [r.function for r in rows if not r.case]
    for n in sorted(set(names)):
        if names.count(n) > 1:
            bad.append(f"{n} is listed twice")
    for r in rows:
        if r.case and r.function not in names:
            bad.append(f"{r.id} is a further case of a function that has no row of its own")
    ids = [r.id for r in rows]
    for i in sorted(set(ids)):
        if ids.count(i) > 1 and f"{i} is listed twice" not in bad:
            bad.append(f"{i} is listed twice")
    for n in sorted(set(decl) - set(names)):
        bad.append(f"{n} ({decl[n][0]}) has no row")
    for n in sorted(set(names) - set(decl)):
        bad.append(f"{n} has a row but no declaration in include/*.h")
    for r in rows:
        if r.cls not in (ft.FLUSHES, ft.LEAVES, ft.HOLDS, ft.CREATES):
            bad.append(f"{r.id}: unknown class {r.cls!r}")
        if not r.how or not callable(r.call):
            bad.append(f"{r.id}: the row does not say how the GPU test calls it")
        if r.cls == ft.CREATES and r.function not in ft.CREATES_ALLOWED:
            bad.append(f"{r.id}: only {sorted(ft.CREATES_ALLOWED)} create a context")
        if r.cls == ft.HOLDS and r.function not in ft.HOLDS_ALLOWED:
            bad.append(f"{r.id}: only {sorted(ft.HOLDS_ALLOWED)} hold frames back")
        if (r.function in ft.CREATES_ALLOWED) != (r.cls == ft.CREATES) or (r.function in ft.HOLDS_ALLOWED) != (r.cls == ft.HOLDS):
            bad.append(f"{r.id}: class {r.cls} is not this function's")
        if r.cls == ft.LEAVES and r.function not in ft.LEAVES_ALLOWED:
            comment = re.sub(r"[\s*]+", " ", decl.get(r.function, ("", ""))[1])
            if ft.LEAVES_SENTENCE not in comment:
                bad.append(f"{r.id}: a call that leaves held frames alone must say in its header comment that it \"{ft.LEAVES_SENTENCE}\"")
        if r.multi != (r.function.startswith(("rt_multi_", "rt_gather_", "rt_debug_multi_")) and r.function != "rt_gather_rccl"
                       or r.function in ("rt_create_multi", "rt_destroy_multi")):
            bad.append(f"{r.id}: multi = {r.multi} does not fit the function's first parameter")
    return bad


def test_every_context_function_has_exactly_one_row():
    decl = declared()
    assert len(decl) >= 100, len(decl)     # 99 when this test was written, + rt_mis_trace: the parser still finds the headers' functions
    assert decl["rt_mis_trace"][0] == "rt_mis.h" and "rt_debug_light_map_free" not in decl
    assert problems(decl, ft.ROWS) == []


def test_the_multi_rows_are_the_functions_that_take_an_rtmulti():
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        code = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        for m in re.finditer(r"\b(rt_[a-z_0-9]+)\s*\(\s*(?:const\s+)?RtMulti\s*\*", code):
            rows = [r for r in ft.ROWS if r.function == m.group(1)]
            assert rows and all(r.multi for r in rows), m.group(1)


def test_the_hooks_header_is_mirrored_and_exported(pkg, api):
    """include/rt_held_back.h declares the two hooks (and restates rt_multi_context); hip.HELD_BACK_SYMBOLS mirrors it, the library exports them"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_held_back.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(rt_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(pkg.hip.HELD_BACK_SYMBOLS + ["rt_multi_context"])
    assert not set(pkg.hip.HELD_BACK_SYMBOLS) & set(pkg.hip.ABI_SYMBOLS)
    for n in names:
        assert hasattr(api.lib, n), f"libraytrace_hip.so does not export {n}"
    assert api.debug_pending_frames(None) == pkg.abi.RT_ERR_INVALID_ARG == api.debug_multi_pending_frames(None)


def test_a_missing_row_a_stale_row_and_a_double_row_are_found():
    decl = declared()
    rows = list(ft.ROWS)
    gone = [r for r in rows if r.function != "rt_update_spheres"]
    assert problems(decl, gone) == ["rt_update_spheres (rt_abi.h) has no row"]
    assert "rt_update_spheres is listed twice" in problems(decl, rows + [r for r in rows if r.function == "rt_update_spheres"])
    fewer = {k: v for k, v in decl.items() if k != "rt_resolve"}
    assert problems(fewer, rows) == ["rt_resolve has a row but no declaration in include/*.h"]


def test_a_new_declaration_without_a_row_is_found(tmp_path):
    """a dummy `int rt_x(RtContext*)` in a header, in each of the forms a first parameter takes"""
    for i, first in enumerate(("RtContext* ctx", "const RtContext *ctx", "RtMulti* m", "const RtMulti* m")):
        h = tmp_path / f"rt_new{i}.h"
        h.write_text("/* a new pass */\nint rt_x%d(%s, int n);\nint rt_helper%d(int n);\n" % (i, first, i))
        decl = declared([str(h)])
        assert list(decl) == [f"rt_x{i}"]
        assert f"rt_x{i} (rt_new{i}.h) has no row" in problems(decl, ft.ROWS)


def test_a_descriptor_call_without_a_row_is_found_and_a_plain_struct_is_not_taken(tmp_path):
    """`int rt_y(const RtYBatch*)` where RtYBatch has a context member is a call on that context, in each form the member takes, with a
    comment and a nested-looking member in the way; a struct of plain data (as RtLightMapDump) in the first place makes no such call"""
    for i, member in enumerate(("RtContext* ctx;", "const RtContext *ctx;", "RtMulti*  multi;", "const RtMulti * m;")):
        h = tmp_path / f"rt_desc{i}.h"
        h.write_text("typedef struct RtYBatch%d {\n    uint32_t struct_size; /* RtContext* not here */\n    %s\n    const void* rays;\n} RtYBatch%d;\n"
                     "typedef struct RtYDump%d { int32_t n; uint32_t* objects; /* RtContext* ctx; */ } RtYDump%d;\n"
                     "/* a new pass */\nint rt_y%d(const RtYBatch%d* batch);\nint rt_z%d(RtYBatch%d *b, int n);\nvoid rt_y_free%d(RtYDump%d* d);\n" % ((i, member) + (i,) * 9))
        assert descriptor_types([str(h)]) == {f"RtYBatch{i}"}
        decl = declared([str(h)])
        assert sorted(decl) == [f"rt_y{i}", f"rt_z{i}"]
        assert decl[f"rt_y{i}"] == (f"rt_desc{i}.h", "/* a new pass */")
        bad = problems(decl, ft.ROWS)
        assert f"rt_y{i} (rt_desc{i}.h) has no row" in bad and f"rt_z{i} (rt_desc{i}.h) has no row" in bad
        assert not any(f"rt_y_free{i}" in b for b in bad)


def test_a_struct_without_a_context_member_is_not_taken(tmp_path):
    """the headers' own: RtMisBatch is a descriptor, RtLightMapDump (plain data, next to it in rt_mis.h) is not; and a struct that only
    MENTIONS a context type — in a comment, or as a value of another name (RtContextInfo*) — is not one"""
    types = descriptor_types(glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert "RtMisBatch" in types and "RtLightMapDump" not in types
    decl = declared()
    assert "rt_mis_trace" in decl and "rt_debug_light_map" not in decl and "rt_debug_light_map_free" not in decl
    h = tmp_path / "rt_plain.h"
    h.write_text("typedef struct RtPlain { int n; /* RtContext* ctx; */ RtContextInfo* info; float* x; } RtPlain;\nint rt_plain(const RtPlain* p);\n")
    assert descriptor_types([str(h)]) == set() and declared([str(h)]) == {}
    assert not any("rt_plain" in b for b in problems(declared([str(h)]), ft.ROWS) if "has no row" in b)


def test_only_the_listed_functions_leave_held_frames_alone_without_saying_so():
    decl = declared()
    quiet = [r for r in ft.ROWS if r.cls == ft.LEAVES and r.function not in ft.LEAVES_ALLOWED]
    assert [r.function for r in quiet] == ["rt_multi_context"]        # a lookup; its header comment carries the sentence
    loud = ft.Row("rt_get_counters", ft.LEAVES, "read", lambda c: None)
    assert any(ft.LEAVES_SENTENCE in p for p in problems(decl, [loud if r.function == "rt_get_counters" else r for r in ft.ROWS]))
    assert sorted(r.function for r in ft.ROWS if r.cls == ft.LEAVES and r.function in ft.LEAVES_ALLOWED) == sorted(ft.LEAVES_ALLOWED)
