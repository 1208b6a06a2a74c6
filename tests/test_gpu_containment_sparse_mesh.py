"""Containment of sparse meshing (tests/arena.py): sdfv_program_mesh_extract_sparse takes no device array from its caller -- the
program is a handle, the box and the descriptor are host memory -- so nothing of the caller's on the device may be read or written:
a bystander array in an arena must come back untouched and the mesh must be the restatement's (tests/sparse_mesh_ref.py) whatever
poison lies around it.  On the host the descriptor, the mesh structure and the stats sit in one buffer between guard words: the
call writes *out and *stats and nothing else, the descriptor included.

Shapes: all_ops (the non-cubic box, materials) at 32 cells and the steep plane with the default constant at 16, whose refused
cells are where a wrong neighbour lookup would read beside the scratch."""
import ctypes as C
import importlib

import numpy as np
import pytest

import arena as A
import sparse_mesh_ref as S
import test_gpu_sparse_mesh as T

pytestmark = pytest.mark.gpu
GUARD = 0x5A


@pytest.mark.parametrize("name,n,L", [("all_ops", 32, 1.0), ("steep", 16, 0.0)])
def test_the_call_touches_out_stats_and_its_scratch_only(pkg, name, n, L):
    import torch
    K = pkg._capi
    PM = importlib.import_module("sdf-viewer_amd.program")
    b, bb, _, materials = S.case(PM, name)
    prog = b.build()
    want_v, want_i, want_stats = T.restated(name, n, L or 1.0)
    assert len(want_i) > 0

    class Fenced(C.Structure):
        _fields_ = [("g0", C.c_uint8 * 64), ("desc", K.SparseMeshDesc), ("g1", C.c_uint8 * 64), ("mesh", K.Mesh), ("g2", C.c_uint8 * 64),
                    ("stats", K.SparseMeshStats), ("g3", C.c_uint8 * 64), ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("g4", C.c_uint8 * 64)]

    bystander = np.arange(4096, dtype=np.float32)
    ar = A.Arena(A.arena_bytes(A.MIN_BAND, bystander), band=A.MIN_BAND)
    ar.input(bystander, align=16, name="bystander")
    meshes = []

    def run():
        f = Fenced()
        C.memset(C.byref(f), GUARD, C.sizeof(f))
        f.lo[:], f.hi[:] = bb[:3], bb[3:]
        d = f.desc
        C.memset(C.byref(d), 0, C.sizeof(d))
        d.size, d.program, d.cells, d.flags, d.lipschitz = C.sizeof(d), prog.h, n, int(materials), L
        d.bb_min, d.bb_max = C.cast(f.lo, C.POINTER(C.c_float)), C.cast(f.hi, C.POINTER(C.c_float))
        d.out, d.stats = C.pointer(f.mesh), C.pointer(f.stats)
        f.stats.size = C.sizeof(K.SparseMeshStats)
        before = bytes(f)
        pkg.check(pkg.lib.sdfv_program_mesh_extract_sparse(C.byref(d), None))
        after = bytes(f)
        open_ = np.zeros(C.sizeof(f), bool)
        for field in (Fenced.mesh, Fenced.stats):
            open_[field.offset:field.offset + field.size] = True
        changed = np.frombuffer(before, np.uint8) != np.frombuffer(after, np.uint8)
        assert not (changed & ~open_).any(), np.flatnonzero(changed & ~open_)[:8]
        assert f.stats.size == C.sizeof(K.SparseMeshStats) and f.stats.bricks == want_stats["bricks"]
        assert list(f.stats.tested[want_stats["levels"]:]) == [0] * (12 - want_stats["levels"])
        m = K.Mesh()
        C.memmove(C.byref(m), C.byref(f.mesh), C.sizeof(m))
        v, i = pkg.mesh_tensors(m)
        torch.cuda.synchronize()
        meshes.append((v.cpu().numpy(), i.cpu().numpy().astype(np.int64)))
    ar.twin(run, {}, kinds=("nan", "hit"))
    for v, i in meshes:
        assert v.shape == want_v.shape and i.shape == want_i.shape
        np.testing.assert_array_equal(i, want_i)
        np.testing.assert_array_equal(S.M.bits(v), S.M.bits(want_v))
