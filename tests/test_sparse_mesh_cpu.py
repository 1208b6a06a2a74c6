"""CPU tests of sparse meshing over SDF programs (include/sdfgrid.h, "SDF programs: sparse meshing"): the entry point is
declared, exported and bound; what it refuses, in the header's order, with its messages and a zeroed *out; the numpy restatement
the GPU tests compare against (tests/sparse_mesh_ref.py) held to the dense restatement (tests/program_mesh_ref.py) on every
(program, cells) the GPU tests use with the promise; the steep plane that breaks the promise; and what the built kernels look
like.  No device needed."""
import ctypes as C
import functools
import importlib
import os
import re

import numpy as np
import pytest

import program_mesh_ref as M
import sparse_mesh_ref as S
from kernel_objects import code_objects, disassembly, kernel_table  # noqa: F401 (code_objects is a fixture)

INVALID, NO_DEVICE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


# ---- the ABI ----
def test_the_entry_point_and_both_structs_are_declared_exported_and_bound(pkg, PM):
    K = pkg._capi
    header = open(os.path.join(ROOT, "include", "sdfgrid.h")).read()
    assert re.search(r"^int sdfv_program_mesh_extract_sparse\(const sdfv_sparse_mesh_desc \*desc, void \*stream\);", header, re.M)
    assert "} sdfv_sparse_mesh_stats;" in header and "} sdfv_sparse_mesh_desc;" in header
    assert "SDF programs: sparse meshing" in header
    assert "sdfv_program_mesh_extract_sparse" in K.PROTOTYPES and getattr(C.CDLL(K.LIB_PATH), "sdfv_program_mesh_extract_sparse")
    assert C.sizeof(K.SparseMeshStats) == 128 and C.sizeof(K.SparseMeshDesc) == 64
    assert K.SparseMeshStats.bricks.offset == 104 and K.SparseMeshDesc.out.offset == 48 and K.SparseMeshDesc.lipschitz.offset == 44
    assert callable(PM.CompiledProgram.mesh_sparse)
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "sdfv_program_mesh_extract_sparse" in open(os.path.join(ROOT, doc)).read(), doc
    assert pkg.lib.sdfv_abi_version() == 5     # additive: the version stays


def test_every_refusal_in_the_header_s_order_with_its_message_and_a_zeroed_out(pkg, PM):
    lib, K = pkg.lib, pkg._capi
    prog = S.builder(PM, "single").build()
    lo, hi = pkg.f3((-1, -1, -1)), pkg.f3((1, 1, 1))
    m = K.Mesh()

    class Wide(C.Structure):                     # a caller built against a LATER header: eight bytes this library does not know
        _fields_ = [("d", K.SparseMeshDesc), ("beyond", C.c_uint8 * 8)]

    def call(size=None, extra=None, out=m, box=(lo, hi), stats_size=None, **kw):
        w, s = Wide(), K.SparseMeshStats()
        d = w.d
        d.size = C.sizeof(K.SparseMeshDesc) if size is None else size
        d.program, d.cells = prog.h, 8
        if box[0] is not None:
            d.bb_min = box[0]
        if box[1] is not None:
            d.bb_max = box[1]
        if out is not None:
            d.out = C.pointer(out)
        if stats_size is not None:
            s.size = stats_size
            d.stats = C.pointer(s)
        for k, v in kw.items():
            setattr(d, k, v)
        if extra is not None:
            w.beyond[extra] = 1
        m.vertices, m.indices, m.n_vertices, m.n_indices = 1, 1, 7, 7
        rc = lib.sdfv_program_mesh_extract_sparse(C.cast(C.byref(w), C.POINTER(K.SparseMeshDesc)), None)
        return rc, lib.sdfv_last_error().decode()

    def cleared():
        return (m.vertices, m.indices, m.n_vertices, m.n_indices) == (None, None, 0, 0)

    assert (lib.sdfv_program_mesh_extract_sparse(None, None), lib.sdfv_last_error()) == (INVALID, b"desc is NULL")
    rc, msg = call(size=56)
    assert rc == INVALID and msg == "sdfv_sparse_mesh_desc.size = 56 is smaller than the descriptor's first version (64)"
    rc, msg = call(size=72, extra=3)
    assert rc == INVALID and "byte 67 beyond them is not 0" in msg and cleared()
    assert call(size=72)[0] in (0, NO_DEVICE)                                   # a longer descriptor of zeros is accepted
    # each rule alone, then with the NEXT rule violated as well: the earlier one answers
    rules = [(dict(reserved=1), "sdfv_sparse_mesh_desc.reserved must be 0"),
             (dict(out=None), "out is NULL"),
             (dict(program=None), "program is NULL"),
             (dict(box=(lo, None)), "bounding box: bb_min and bb_max are both given or both NULL (the program's box)"),
             (dict(algorithm=4), "Unsupported algorithm 4"),
             (dict(cells=12), "cells 12 is not a power of two in [4, 4096]"),
             (dict(flags=2), "unknown flags 0x2"),
             (dict(lipschitz=0.5), "lipschitz 0.5 is neither 0 (= 1) nor a finite number >= 1"),
             (dict(stats_size=120), "sdfv_sparse_mesh_stats.size = 120 is smaller than the structure (128)")]
    for k, (bad, text) in enumerate(rules):
        assert call(**bad) == (INVALID, text), bad
        assert cleared() or "out" in bad
        if k + 1 < len(rules):
            both = dict(bad, **rules[k + 1][0])
            assert call(**both) == (INVALID, text), both
    assert call(box=(None, hi))[1] == rules[3][1]
    for algorithm in (1, 2, 3, 4, 5):
        assert call(algorithm=algorithm) == (INVALID, "Unsupported algorithm %d" % algorithm) and cleared()
    for cells in (0, 1, 2, 3, 5, 24, 1000, 4097, 8192, 2 ** 31):
        assert call(cells=cells) == (INVALID, "cells %d is not a power of two in [4, 4096]" % cells), cells
    for flags in (2, 3, 0x80000000):
        assert call(flags=flags) == (INVALID, "unknown flags 0x%x" % flags)
    for L in (NAN, INF, -INF, -1.0, 0.999, 1e-30):
        rc, msg = call(lipschitz=L)
        assert rc == INVALID and "is neither 0 (= 1) nor a finite number >= 1" in msg and cleared(), L
    assert call(stats_size=0)[0] == INVALID
    # what is valid reaches the device check
    valid = [dict(), dict(box=(None, None)), dict(cells=4), dict(cells=4096), dict(flags=1), dict(lipschitz=1.0), dict(lipschitz=3.0),
             dict(lipschitz=-0.0), dict(stats_size=128), dict(stats_size=136)]
    if lib.sdfv_device_count() == 0:
        for kw in valid:
            rc, msg = call(**kw)
            assert rc == NO_DEVICE and "no HIP device" in msg and cleared(), kw


# ---- the restatement held to the dense restatement: the condition that makes the GPU comparison meaningful ----
@functools.lru_cache(maxsize=None)
def both(name, n):
    PM = importlib.import_module("sdf-viewer_amd.program")
    b, bb, L, materials = S.case(PM, name)
    return b, S.extract(b.ops, n, bb, materials, L), M.extract(b.ops, n, bb, materials)


@pytest.mark.parametrize("name,n", S.PROMISE)
def test_with_the_promise_the_sparse_restatement_is_the_dense_one_as_a_set(pkg, PM, name, n):
    b, (sv, si, stats), (dv, di, _) = both(name, n)
    _, bb, L, _ = S.case(PM, name)
    active, outside = S.active_cells(b.ops, n, bb, L)
    print(name, n, "active cells", active, "outside the bricks", outside, stats)
    assert outside == 0                                                         # every cell with a crossing edge lies in a brick
    assert S.record_set(sv) == S.record_set(dv)
    assert S.triangle_set(sv, si) == S.triangle_set(dv, di)
    assert len(si) == len(di) and (len(si) == 0 or si.max() < len(sv))
    assert stats["evaluations"] == sum(stats["tested"]) + 125 * stats["bricks"]
    assert stats["levels"] == {4: 0, 8: 1, 16: 2, 32: 3, 64: 4}[n] and stats["tested"][0] == 8
    assert stats["bricks"] == (stats["kept"][-1] if stats["levels"] else 1)


def test_the_stated_constant_and_box_are_needed(pkg, PM):
    """deep with L = 1 misses cells (so the promise list states 1.34 for it); ties over its own box has exact zeros on the lattice."""
    b = S.builder(PM, "deep")
    assert S.active_cells(b.ops, 32, b.bb, 1.0) == (1245, 9)
    b = S.builder(PM, "ties")
    assert all((M.lattice(b.ops, n, b.bb)[1] == 0).any() for n in (8, 16, 32))
    assert sum(len(both(name, n)[1][0]) > 0 for name, n in S.PROMISE) >= 18       # most cases have a surface to compare


def test_the_tiny_sphere_s_counts(pkg):
    b, (sv, si, stats), (dv, _, _) = both("tiny", 16)
    assert stats["bricks"] == 4 and len(sv) == 0 and len(si) == 0 and len(dv) == 0
    assert S.active_cells(b.ops, 16, b.bb) == (0, 0)
    b, (sv, si, stats), _ = both("tiny", 32)
    assert S.active_cells(b.ops, 32, b.bb) == (24, 0) and len(sv) > 0


def test_four_cells_are_one_untested_brick(pkg, PM):
    b = S.builder(PM, "single")
    sv, si, stats = S.extract(b.ops, 4, b.bb)
    dv, di, _ = M.extract(b.ops, 4, b.bb)
    assert stats == dict(levels=0, tested=[], kept=[], bricks=1, evaluations=125)
    assert len(sv) > 0 and (M.bits(sv) == M.bits(dv)).all() and (si == di).all()   # one brick that owns everything: the same ORDER


def test_the_steep_plane_breaks_the_promise_at_1_and_keeps_it_at_3(pkg, PM):
    b = S.builder(PM, "steep")
    assert S.active_cells(b.ops, 16, b.bb, 1.0) == (296, 88)
    assert S.refine(b.ops, 16, b.bb, 1.0)[1] == dict(levels=2, tested=[8, 32], kept=[4, 16], bricks=16, evaluations=8 + 32 + 125 * 16)
    for n in (16, 32):
        assert S.active_cells(b.ops, n, b.bb, 3.0)[1] == 0
        dv, di, _ = M.extract(b.ops, n, b.bb)
        sv, si, _ = S.extract(b.ops, n, b.bb, L=3.0)
        assert S.record_set(sv) == S.record_set(dv) and S.triangle_set(sv, si) == S.triangle_set(dv, di)
        hv, hi, _ = S.extract(b.ops, n, b.bb, L=1.0)                             # holes, and nothing out of range
        assert len(hi) and hi.max() < len(hv)
        holes, whole = set(S.triangle_set(hv, hi)), set(S.triangle_set(dv, di))
        assert holes < whole


# ---- the built kernels (tests/kernel_objects.py) ----
INTERPRETING = ("sdfprog_sparse_refine", "sdfprog_sparse_bricks")
SDF_FREE = ("sparse_compact", "sparse_brick_edges", "sparse_brick_neighbours", "sparse_brick_cells", "sparse_brick_positions", "sparse_brick_triangles")


def test_sparse_kernels_keep_the_resource_ceilings(code_objects):
    """C names; no scratch, no spill, at most 256 bytes of kernel arguments; the two kernels that run the interpreter need no more
    VGPRs than sdfprog_mesh_lattice of the same build (they use the same bare, distance-only run), and none of them contracts a
    multiply and an add."""
    table = kernel_table(code_objects)
    assert sorted(n for n in table if "sparse_" in n) == sorted(INTERPRETING + SDF_FREE)
    ceiling = table["sdfprog_mesh_lattice"]["vgpr"]
    for name in INTERPRETING + SDF_FREE:
        k = table[name]
        print(name, {a: b for a, b in k.items() if a != "co"})
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (name, k)
        assert k["kernarg"] <= 256, (name, k)
        ops = [ln.split("//")[0].split()[0] for ln in disassembly(k["co"], name).split("\n") if ln.split("//")[0].split()]
        assert not any(o.startswith(("scratch_", "buffer_")) for o in ops), name
        assert not any(o.startswith("v_pk_fma") for o in ops), name   # nothing contracted (IEEE divide and sqrt expand to scalar fmas)
        if name in INTERPRETING:
            assert k["vgpr"] <= ceiling, (name, k["vgpr"], ceiling)
