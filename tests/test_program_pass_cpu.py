"""CPU tests of the SDF-program pass and the program editor: what sdfv_program_grid_pass refuses (before it asks for a device),
the editor's parameters against the numpy restatement of the machine (tests/program_ref.py), what the built pass kernels look
like, and the headers as C99.  No device needed."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import program_ref as R
from kernel_objects import code_objects, disassembly, kernel_table  # noqa: F401 (code_objects is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NO_DEVICE = -1, -4


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


def test_the_pass_refuses_bad_arguments_before_it_asks_for_a_device(pkg, PM):
    lib, K = pkg.lib, pkg._capi
    prog = R.catalogue(PM)["anchor"].build()
    g = pkg.make_grid((4, 4, 4))
    odd = pkg.make_grid((4, 3, 4))
    box = (C.c_float * 6)(-1, -1, -1, 1, 1, 1)

    def refused(text, p=prog.h, grid=g, step=1, bx=None, t0=16, t1=16, dist=None, flags=0):
        rc = lib.sdfv_program_grid_pass(p, C.byref(grid) if grid is not None else None, step, bx, t0, t1, dist, flags, None)
        assert rc == INVALID and text in lib.sdfv_last_error(), (rc, lib.sdfv_last_error())

    refused(b"program is NULL", p=None)
    refused(b"", grid=None)
    refused(b"texture pointer is NULL", t0=None)
    refused(b"texture pointer is NULL", t1=None)
    refused(b"step 0 is not a power of two", step=0)
    refused(b"step 3 is not a power of two", step=3, bx=box)
    refused(b"unknown pass flags 0x20", flags=32)
    refused(b"SDFV_PASS_VIRGIN_GRID is not supported for programs", flags=K.PASS_VIRGIN_GRID)
    refused(b"SDFV_PASS_VIRGIN_GRID is not supported for programs", flags=K.PASS_VIRGIN_GRID | K.PASS_SAME_LOAD, dist=16)
    refused(b"SDFV_PASS_VOLUME_INTERLEAVED without a volume", flags=K.PASS_VOLUME_INTERLEAVED)
    refused(b"H = 3 must be even", grid=odd, dist=16, flags=K.PASS_VOLUME_INTERLEAVED)
    refused(b"8-byte aligned", dist=20, flags=K.PASS_VOLUME_INTERLEAVED)
    refused(b"16-byte aligned", t0=24)
    refused(b"16-byte aligned", t1=8)
    refused(b"dist must be 4-byte aligned", dist=18)
    big = pkg.make_grid((2048, 2048, 1025))            # 2^32 + 2^22 voxels
    refused(b"at most 2^32 voxels", grid=big)
    if lib.sdfv_device_count() == 0:
        # the accepted forms get as far as the device check, and no further
        for flags, dist in ((0, None), (K.PASS_FRESH_GRID, 16), (K.PASS_SAME_LOAD | K.PASS_EXPECT_NOOP, None),
                            (K.PASS_VOLUME_INTERLEAVED, 16)):
            assert lib.sdfv_program_grid_pass(prog.h, C.byref(g), 2, box, 16, 16, dist, flags, None) == NO_DEVICE
            assert b"no HIP device" in lib.sdfv_last_error()
        exactly = pkg.make_grid((2048, 2048, 1024))    # 2^32 voxels are taken
        assert lib.sdfv_program_grid_pass(prog.h, C.byref(exactly), 1, None, 16, 16, None, 0, None) == NO_DEVICE


# ---- the editor ----
def editable(PM):
    """A model with one parameter of each target kind (and one of two kinds at once): the builder and what each name edits."""
    b = PM.Program((-1.0, -1.0, -1.0, 1.0, 1.0, 1.0))
    b.material(0.8, 0.2, 0.1, 0.1, 0.6, 0.9)
    b.push_affine(PM.translation(0.25, 0.0, 0.0))
    affine = len(b.ops) - 1
    b.box(0.5, 0.3, 0.2).pop()
    box = len(b.ops) - 2
    b.material(0.1, 0.9, 0.3, 0.0, 1.0, 0.5).push_scale(0.5)
    push = len(b.ops) - 1
    b.torus(1.2, 0.3).pop_scale(0.5)
    pop = len(b.ops) - 1
    b.smooth_union(0.15)
    smooth = len(b.ops) - 1
    b.param("tx", [(affine, 3, PM.PARAM_NEGATED)], -0.5, 0.5, 0.01, 0.25, box=(-1.0, -0.4, -0.3, 1.0, 0.4, 0.3), description="the box along x")
    b.param("scale", [(push, 0, PM.PARAM_VALUE), (push, 1, PM.PARAM_RECIPROCAL), (pop, 0, PM.PARAM_VALUE)], 0.25, 0.75, 0.05, 0.5)
    b.param("k", [(smooth, 0, PM.PARAM_VALUE)], -1.0, 1.0, 0.01, 0.15, box=(-0.5, -0.5, -0.5, 0.5, 0.5, 0.5))
    b.param("hx", [(box, 0, PM.PARAM_VALUE)], 0.1, 0.9, 0.1, 0.5, box=(-0.9, -0.2, -0.1, 0.7, 0.6, 0.8))
    return b


def restated(ops, targets, value):
    """The instruction list after the edit, in numpy float32: v, -v, or 1 / v in one division."""
    ops = [(op, [np.float32(a) for a in operands]) for op, operands in ops]
    v = np.float32(value)
    for op, operand, kind in targets:
        ops[op][1].extend([np.float32(0)] * (operand + 1 - len(ops[op][1])))
        ops[op][1][operand] = {0: v, 1: -v, 2: np.float32(1.0) / v}[kind]
    return [(op, tuple(a)) for op, a in ops]


def host_records(V, surface, pts):
    s = surface.struct
    out = np.full((len(pts), 7), np.nan, np.float32)
    assert s.sample_batch(s.user, pts.ctypes.data_as(V.FP), len(pts), 0, out.ctypes.data_as(C.POINTER(V.Sample))) == 0
    return out


def test_editor_sets_all_three_target_kinds_and_samples_like_the_restatement(pkg, PM):
    V = importlib.import_module("sdf-viewer_amd.viewer")
    b = editable(PM)
    ed = b.build_editor()
    surface = ed.as_surface()
    assert surface.struct.changed and surface.bounding_box() == b.bb
    pts = R.points()
    by_name = {p["name"]: p for p in b.params}
    ops = restated(b.ops, [], 0.0)
    same = lambda got, want: (np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)).all()  # noqa: E731
    assert same(host_records(V, surface, pts), R.run(ops, pts))               # the initial values are the builder's operands
    for name, value in (("tx", -0.375), ("scale", 0.3), ("k", 0.07), ("hx", 0.7), ("scale", 0.7)):
        before = R.run(ops, pts)
        ed.set(name, value)
        ops = restated(ops, by_name[name]["targets"], value)
        want = R.run(ops, pts)
        assert not same(before, want), name                                   # the edit shows on these points
        assert same(host_records(V, surface, pts), want), name                # the surface follows the current snapshot
        assert same(host_records(V, ed.program.as_surface(), pts), want), name
        assert ed.get(name) == np.float32(value)
        got_ops, bb = ed.program.ops()
        assert same(got_ops["a"], np.array([list(a) + [0.0] * (12 - len(a)) for _, a in ops], np.float32)) and bb == b.bb
    assert ops[by_name["scale"]["targets"][1][0]][1][1] == np.float32(1.0) / np.float32(0.7)   # 1 / v, not a rounded 1.4285...
    ed.trim()                                                                 # the replaced snapshots go, the current one stays
    assert same(host_records(V, surface, pts), R.run(ops, pts))


def test_editor_refusals_change_nothing_and_changed_reports_the_merged_box_once(pkg, PM):
    b = editable(PM)
    ed = b.build_editor()
    assert ed.changed() is None
    ed.set("tx", 0.1)
    ed.set("hx", 0.6)
    snapshot, values = ed.program.h.value, [p["value"] for p in ed.parameters()]
    for name, value, text in (("tx", 0.75, "outside"), ("tx", float("nan"), "outside"), (17, 0.5, "unknown parameter id 17"),
                              ("k", 0.0, "must be > 0"), ("k", -0.25, "SMOOTH_UNION")):
        with pytest.raises(pkg.SdfvError, match=text):
            ed.set(name, value)
        assert ed.program.h.value == snapshot and [p["value"] for p in ed.parameters()] == values, (name, value)
    # the two accepted edits, merged (merge_bounding_boxes: min of the mins, max of the maxes), exactly once
    f = lambda *v: tuple(float(np.float32(x)) for x in v)  # noqa: E731
    assert ed.changed() == f(-1.0, -0.4, -0.3, 1.0, 0.6, 0.8)
    assert ed.changed() is None
    ed.set("scale", 0.4)                                     # no box of its own: the program's
    assert ed.changed() == b.bb and ed.changed() is None
    # parameters() round-trips what the builder declared
    got = ed.parameters()
    assert [p["name"] for p in got] == ["tx", "scale", "k", "hx"] and [p["id"] for p in got] == [0, 1, 2, 3]
    assert got[0]["description"] == "the box along x" and got[1]["description"] == ""
    for p, q in zip(got, b.params):
        assert (p["min"], p["max"], p["step"]) == f(q["lo"], q["hi"], q["step"]) and p["targets"] == q["targets"]
        assert p["box"] == (None if q["box"] is None else f(*q["box"]))
    assert [p["value"] for p in got] == list(f(0.1, 0.4, 0.15, 0.6))
    # what the constructor refuses
    for edit, text in ((dict(value=2.0), "outside its range"), (dict(targets=[]), "0 targets"), (dict(targets=[(99, 0, 0)]), "outside the program"),
                       (dict(targets=[(1, 0, 7)]), "unknown kind"), (dict(lo=1.0, hi=0.0), "is not one"),
                       (dict(box=(0.5, 0, 0, -0.5, 1, 1)), "inverted")):
        bad = editable(PM)
        bad.params[0].update(edit)
        with pytest.raises(pkg.SdfvError, match=text):
            bad.build_editor()
    bad = editable(PM)
    bad.params[2]["value"] = -0.5                            # a value the validator refuses, with its message
    with pytest.raises(pkg.SdfvError, match="SMOOTH_UNION.*must be > 0"):
        bad.build_editor()


# ---- the built kernels (tests/kernel_objects.py) ----
PASS_KERNELS = ("sdfprog_pass_box", "sdfprog_pass_scan", "sdfprog_pass_scan_nt")


def instructions(co, name):
    """[(opcode, operands' text, address, branch target address or None)] from the disassembly's own address column."""
    ins = []
    for ln in disassembly(co, name).split("\n"):
        m = re.match(r"\s+(\S+)([^/]*)//\s*([0-9A-Fa-f]{12}):[^<]*(?:<[^>+]*\+0x([0-9a-f]+)>)?", ln)
        if m:
            ins.append([m.group(1), m.group(2), int(m.group(3), 16), None if m.group(4) is None else int(m.group(4), 16)])
    base = ins[0][2]
    return [(o, args, at, None if to is None else base + to) for o, args, at, to in ins]


def largest_cycle(ins):
    """The instructions of the largest strongly connected component of the kernel's control flow graph: the interpreter loop.
    (Not "the widest backward branch": the compiler lays cold blocks out behind the kernel's end, and their way back is one.)"""
    index = {at: i for i, (_, _, at, _) in enumerate(ins)}
    succ = []
    for i, (o, _, _, to) in enumerate(ins):
        s = []
        if o != "s_endpgm" and o != "s_branch" and i + 1 < len(ins):
            s.append(i + 1)
        if to is not None and o.startswith(("s_branch", "s_cbranch")):
            s.append(index[to])
        succ.append(s)
    reach = [0] * len(ins)                      # bit j of reach[i]: j is reachable from i in one step or more
    changed = True
    while changed:
        changed = False
        for i in range(len(ins) - 1, -1, -1):
            r = reach[i]
            for j in succ[i]:
                r |= (1 << j) | reach[j]
            if r != reach[i]:
                reach[i], changed = r, True
    best = []
    seen = 0
    for i in range(len(ins)):
        if (seen >> i) & 1 or not (reach[i] >> i) & 1:
            continue
        comp = [j for j in range(len(ins)) if (reach[i] >> j) & 1 and (reach[j] >> i) & 1]
        for j in comp:
            seen |= 1 << j
        if len(comp) > len(best):
            best = comp
    return [ins[j] for j in best]


def test_pass_kernels_keep_their_state_in_registers_and_fetch_instructions_by_scalar_loads(code_objects):
    table = kernel_table(code_objects)
    for name in PASS_KERNELS:
        k = table[name]                                   # stable C names
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (name, k)
        assert k["vgpr"] <= 80, (name, k)                 # 6 waves per SIMD (512 / 80), the step the tx64 / tx128 fills are held to
        assert k["kernarg"] <= 256, (name, k)
        ins = instructions(k["co"], name)
        loop = [o for o, _, _, _ in largest_cycle(ins)]
        assert len(loop) > 200, (name, len(loop))          # it does hold the eighteen instruction bodies
        assert [o for o in loop if re.match(r"s_load_dwordx(4|8|16)$", o)], (name, "no wide scalar load in the interpreter loop")
        # no vector memory operation in it, load or store
        assert not any(o.startswith(("global_", "flat_", "buffer_", "scratch_")) for o in loop), name
        # the texels leave as two 16-byte streamed stores
        stores = [args for o, args, _, _ in ins if o == "global_store_dwordx4"]
        assert len(stores) == 2 and all("nt" in a.split() for a in stores), (name, stores)
    # the scan reads ONE value per lane before it decides (nontemporal in the _nt kernel); the box launch decides nothing: all it
    # loads is the colour table (staged before the interpreter runs) and tex1.a where there is no volume
    for name, nt in (("sdfprog_pass_scan", False), ("sdfprog_pass_scan_nt", True)):
        ins = instructions(table[name]["co"], name)
        cycle_at = min(at for _, _, at, _ in largest_cycle(ins))
        before = [(o, args) for o, args, at, _ in ins if at < cycle_at and o.startswith(("global_load", "flat_load", "buffer_load"))]
        assert len(before) == 1 and before[0][0] == "global_load_dword" and ("nt" in before[0][1].split()) == nt, (name, before)
    ins = instructions(table["sdfprog_pass_box"]["co"], "sdfprog_pass_box")
    loads = [(o, args) for o, args, _, _ in ins if o.startswith(("global_load", "flat_load", "buffer_load"))]
    assert len(loads) == 2 and all(o == "global_load_dword" for o, _ in loads), loads


def test_headers_compile_as_pedantic_c99_with_the_pass(tmp_path):
    src = tmp_path / "program_pass_headers.c"
    src.write_text('#include "sdfprogram.h"\n#include "sdfgrid.h"\n'
                   "int main(void) {\n"
                   "    sdfv_prog_op op[1] = {{SDFV_OP_SPHERE, {0, 0, 0}, {0.5f}}};\n"
                   "    float bb[6] = {-1, -1, -1, 1, 1, 1};\n"
                   "    sdfv_grid g;\n"
                   "    sdfv_program *p = 0;\n"
                   "    if (sdfv_program_create(op, 1, bb, &p) != 0) return 2;\n"
                   "    if (sdfv_grid_from_bb(bb, bb + 3, 8, &g) != 0) return 3;\n"
                   "    if (sdfv_program_grid_pass(p, &g, 3, bb, 0, 0, 0, 0, 0) != SDFV_ERR_INVALID_ARGUMENT) return 4;\n"
                   "    sdfv_program_free(p);\n"
                   "    {\n"
                   "        sdfv_program_param prm = {7, \"radius\", 0, 0.1f, 0.9f, 0.01f, 0.5f, 1, {{0, 0, SDFV_PARAM_VALUE}}, 0, {0}};\n"
                   "        sdfv_program_editor *e = 0;\n"
                   "        sdfv_surface s;\n"
                   "        float box[6];\n"
                   "        const sdfv_program_param *params = 0;\n"
                   "        size_t n = 0;\n"
                   "        if (sdfv_program_editor_create(op, 1, bb, &prm, 1, &e) != 0) return 5;\n"
                   "        if (sdfv_program_editor_changed(e, box) != 0) return 6;\n"
                   "        if (sdfv_program_editor_set(e, 7, 2.0f) != SDFV_ERR_INVALID_ARGUMENT || !sdfv_program_editor_last_error(e)[0]) return 7;\n"
                   "        if (sdfv_program_editor_set(e, 7, 0.25f) != 0 || sdfv_program_editor_changed(e, box) != 1 || box[3] != 1.0f) return 8;\n"
                   "        if (sdfv_program_editor_parameters(e, &params, &n) != 0 || n != 1 || params[0].value != 0.25f) return 9;\n"
                   "        if (sdfv_program_editor_as_surface(e, &s) != 0 || !s.changed || s.user != (void *)e) return 10;\n"
                   "        if (!sdfv_program_editor_program(e) || sdfv_program_editor_trim(e) != 0) return 11;\n"
                   "        if (sdfv_viewer_update_program(0, e, 0, &n) != SDFV_ERR_INVALID_ARGUMENT) return 12;\n"
                   "        sdfv_program_editor_free(e);\n"
                   "    }\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "program_pass_headers"
    lib_dir = os.path.join(ROOT, "sdf-viewer_amd")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", lib_dir, "-lsdfviewer_host", "-lsdfgrid", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)], timeout=120).returncode == 0
