"""Containment of the point-list entry points (tests/arena.py): every input and output carved from one arena with guard bands,
16-byte aligned or off by 4 bytes -- all four combinations of input and output alignment -- at the batch sizes around the
256-thread workgroup.  Values come from the oracle and the numpy restatements, never from the library; what is held here is
WHERE each call reads and writes: nothing beside an output, no output word left stale, no result that depends on the words
beside an input (Arena.twin over canary and NaN poison)."""
import functools
import importlib

import numpy as np
import pytest

import arena as A
import lattice_mesh_ref as LM
import mesh_ref as MR
import program_mesh_ref as M
import program_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = (1, 255, 256, 257, 513)  # one thread; one short of, exactly, one past a 256-thread workgroup; two workgroups and one thread
BB = (-1.0, -0.75, -1.0, 1.0, 1.0, 0.5)
CELLS = 9                        # a (9 + 1)^3 lattice: 1000 points >= 513 + the offset below
FIRST = 97                       # lattice_points starts in the middle of a row
ALIGNMENTS = [(i, o) for i in (0, 4) for o in (0, 4)]  # bytes off a 16-byte boundary: input, output
# Which kernel a combination reaches -- launch_staged_then_tail (csrc/kernel_common.h): when the launcher's alignment test holds,
# the first n / 256 whole workgroups go to the STAGED kernel (records through LDS, whole 3, 7 and 12 KiB tiles stored with
# 16-byte accesses: tile_store<3 / 7 / 12>) and the remaining n % 256 points to the scalar kernel; when it fails, all n go to
# the scalar kernel.  The test is "points and out both 16-byte aligned" for sample_points, normal_points, source_sample_normal
# and the program calls, "points 16-byte, out 4-byte aligned" for source_sample_scalar, "vertices 16-byte aligned" for the two
# postprocs.  So the staged kernels run for (0, 0) at n = 256 (staged alone), 257 (one tile + a tail of 1) and 513 (two tiles + a
# tail of 1); for source_sample_scalar also for (0, 4); for the postprocs whenever the vertices (the output offset) are at 0.
# n = 1 and 255 and every other combination are the scalar kernel alone: the fallback must be chosen per pointer, a 16-byte store
# through a pointer off by 4 would write 12 bytes past a tile.  lattice_points, lattice_from_samples and lattice_normals have no
# staged form.


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


@functools.lru_cache(maxsize=None)
def demo_points():
    rng = np.random.default_rng(41)
    pts = rng.uniform(-1.2, 1.2, size=(SIZES[-1], 3)).astype(F)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def program_points():
    """The first 513 of program_ref.points() at which all_ops' records and normals are numbers (the NaN payload of the others is
    open, include/sdfgrid.h; tests/test_gpu_program.py holds those)."""
    PM = importlib.import_module("sdf-viewer_amd.program")
    ops = R.catalogue(PM)["all_ops"].ops
    pts = R.points()
    ok = np.isfinite(R.run(ops, pts)).all(axis=1) & np.isfinite(M.normals(ops, pts)).all(axis=1) & \
        np.isfinite(M.normals(ops, pts, 0.01)).all(axis=1)
    pts = np.ascontiguousarray(pts[ok][:SIZES[-1]])
    assert len(pts) == SIZES[-1]
    pts.setflags(write=False)
    return pts


def vertices_over(pts, seed):
    """[n, 12] vertices at pts: every second normal below |n|^2 = 1e-4 (postproc recomputes it), the others kept; material
    fields 9.0."""
    rng = np.random.default_rng(seed)
    n = len(pts)
    v = np.zeros((n, 12), F)
    v[:, :3] = pts
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    v[:, 3:6] = (d * np.where(np.arange(n) % 2 == 0, 0.009, 0.0101)[:, None]).astype(F)
    v[:, 6:] = 9.0
    return v


def assert_postproc_contract(v, want):
    """Mesh::postproc leaves every position word alone, and the normal where |n|^2 >= 1e-4."""
    nn = v[:, 3] * v[:, 3] + v[:, 4] * v[:, 4] + v[:, 5] * v[:, 5]
    kept = nn >= F(1e-4)
    assert kept.any() and (~kept).any()
    assert (want[:, :3].view(np.uint32) == v[:, :3].view(np.uint32)).all()
    assert (want[kept, 3:6].view(np.uint32) == v[kept, 3:6].view(np.uint32)).all()
    assert (want[~kept, 3:6].view(np.uint32) != v[~kept, 3:6].view(np.uint32)).any()


@functools.lru_cache(maxsize=None)
def reference(entry):
    """(inputs {name: host array}, in-place {name: host array}, outputs {name: expected}) of `entry` at the largest size; a
    smaller batch is the first n of each.  Computed once, shared, never modified."""
    import oracle_binding as oracle
    PM = importlib.import_module("sdf-viewer_amd.program")
    prm = oracle.default_params()
    ops = R.catalogue(PM)["all_ops"].ops
    pts, ppts = demo_points(), program_points()
    unit = ((pts + F(1.2)) / F(2.4)).astype(F)
    if entry == "sample_points":
        return {"points": pts}, {}, {"out": oracle.sample_many(prm, pts)}
    if entry == "sample_points_distance_only":
        return {"points": pts}, {}, {"out": oracle.sample_many(prm, pts, True)}
    if entry == "normal_points":
        return {"points": pts}, {}, {"out": oracle.normal_many(prm, pts)}
    if entry == "source_sample_scalar":
        return {"points": unit}, {}, {"out": oracle.source_scalar_many(prm, unit, BB[:3], BB[3:])}
    if entry == "source_sample_normal":
        return {"points": unit}, {}, {"out": oracle.source_normal_many(prm, unit, BB[:3], BB[3:])}
    if entry == "mesh_postproc":
        v = vertices_over(pts * F(0.8), 3)
        want = oracle.mesh_postproc(prm, v)
        assert_postproc_contract(v, want)
        return {}, {"vertices": v}, {"vertices": want}
    if entry == "program_sample_points":
        return {"points": ppts}, {}, {"out": R.run(ops, ppts)}
    if entry == "program_normal_points":
        return {"points": ppts}, {}, {"out": M.normals(ops, ppts, 0.01)}
    if entry == "program_mesh_postproc":
        v = vertices_over(ppts, 5)
        want = M.postproc(ops, v)
        assert_postproc_contract(v, want)
        return {}, {"vertices": v}, {"vertices": want}
    if entry == "lattice_points":
        return {}, {}, {"out": MR.lattice_points(CELLS, BB)[FIRST:FIRST + SIZES[-1]]}
    if entry == "lattice_from_samples":
        s = oracle.sample_many(prm, pts)
        return {"samples": s}, {}, {"out": np.ascontiguousarray(s[:, 0])}
    if entry == "lattice_normals":
        d = LM.gyroid_lattice(CELLS, BB)
        v = vertices_over(pts, 7)   # positions inside and outside the box (the border cell's values)
        want = v.copy()
        want[:, 3:6] = MR.lattice_normals(d, BB, v[:, :3])
        assert np.isfinite(want).all()
        return {"dist": np.ascontiguousarray(d, F).reshape(-1)}, {"vertices": v}, {"vertices": want}
    raise KeyError(entry)


ENTRIES = ("sample_points", "sample_points_distance_only", "normal_points", "source_sample_scalar", "source_sample_normal",
           "mesh_postproc", "program_sample_points", "program_normal_points", "program_mesh_postproc", "lattice_points",
           "lattice_from_samples", "lattice_normals")
WHOLE_INPUTS = {"dist"}  # inputs that are not one record per point: carved whole at every n


@functools.lru_cache(maxsize=None)
def built_program():
    return R.catalogue(importlib.import_module("sdf-viewer_amd.program"))["all_ops"].build()


def launch(pkg, PM, entry, t, n, prm=None):
    """The call under test over the arena's tensors t[name]; prm: the caller's sdfv_demo_params instead of fresh defaults."""
    prm = pkg.default_params() if prm is None else prm
    if entry.startswith("program_"):
        prog = built_program()
    if entry == "sample_points":
        pkg.sample_points(prm, t["points"], out=t["out"])
    elif entry == "sample_points_distance_only":
        pkg.sample_points(prm, t["points"], distance_only=True, out=t["out"])
    elif entry == "normal_points":
        pkg.normal_points(prm, t["points"], out=t["out"])
    elif entry == "source_sample_scalar":
        pkg.source_sample_scalar(prm, t["points"], BB[:3], BB[3:], out=t["out"])
    elif entry == "source_sample_normal":
        pkg.source_sample_normal(prm, t["points"], BB[:3], BB[3:], out=t["out"])
    elif entry == "mesh_postproc":
        pkg.mesh_postproc(prm, t["vertices"])
    elif entry == "program_sample_points":
        prog.sample_points(t["points"], out=t["out"])
    elif entry == "program_normal_points":
        prog.normal_points(t["points"], 0.01, out=t["out"])
    elif entry == "program_mesh_postproc":
        prog.mesh_postproc(t["vertices"])
    elif entry == "lattice_points":
        pkg.lattice_points(BB, CELLS, first=FIRST, n=n, out=t["out"])
    elif entry == "lattice_from_samples":
        pkg.lattice_from_samples(t["samples"], out=t["out"])
    elif entry == "lattice_normals":
        pkg.lattice_normals(t["dist"], BB, CELLS, t["vertices"])
    else:
        raise KeyError(entry)


@pytest.mark.parametrize("in_off,out_off", ALIGNMENTS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_point_lists_stay_inside_their_buffers(pkg, PM, entry, in_off, out_off):
    """Samples, vertices, normals and points are 4-byte aligned by include/sdfgrid.h ("16-byte aligned arrays take 16-byte
    accesses"): the vector form must be chosen per pointer, so an aligned input with a misaligned output (and the reverse) must
    fall back or split, not misstore.  In-place vertices follow the output's alignment."""
    inputs, inplace, outputs = reference(entry)
    for n in SIZES:
        ar = A.Arena(A.arena_bytes(A.MIN_BAND, *[(a.shape, a.dtype) for a in (*inputs.values(), *inplace.values(), *outputs.values())]))
        t, expected = {}, {}
        for name, a in inputs.items():
            t[name] = ar.input(a if name in WHOLE_INPUTS else a[:n], align=16, misalign=in_off, name=name)
        for name, a in inplace.items():
            t[name] = ar.inout(a[:n], align=16, misalign=out_off, name=name)
        for name, a in outputs.items():
            if name not in inplace:
                t[name] = ar.output(a[:n].shape, a.dtype, align=16, misalign=out_off, name=name)
            expected[name] = np.ascontiguousarray(a[:n])
        for name, tensor in t.items():
            off = in_off if name in inputs else out_off
            assert tensor.data_ptr() % 32 == 16 + off, (name, "exactly 16-byte aligned, plus the offset")
        ar.twin(lambda: launch(pkg, PM, entry, t, n), expected, kinds=("canary", "nan"))
