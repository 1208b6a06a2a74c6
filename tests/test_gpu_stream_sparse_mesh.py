"""Sparse meshing on the caller's stream (tests/stream_gate.py).  sdfv_program_mesh_extract_sparse is documented to synchronise
`stream` (the block counts and the output size depend on the data) and is held to THAT, outside capture, as the other extractors
are (tests/test_gpu_stream_march.py): the mesh is the restatement's, the stream is idle when the call returns, and the host was
held for as long as the sleep in front of the call -- every one of its launches, copies and host reads is ordered behind the work
the caller had on the stream.  Programs and expected values are tests/test_gpu_sparse_mesh.py's."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import sparse_mesh_ref as S
import stream_gate as SG
import test_gpu_sparse_mesh as T
from stream_gate import gate  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,n", [("all_ops", 32), ("single", 4)])
def test_the_sparse_extractor_synchronises_its_stream(pkg, gate, name, n):
    K = pkg._capi
    PM = importlib.import_module("sdf-viewer_amd.program")
    b, bb, L, materials = S.case(PM, name)
    prog = b.build()
    want_v, want_i, want_stats = T.restated(name, n)
    assert len(want_i) > 0
    meshes = []

    def host():
        return {"bb_min": pkg.f3(bb[:3]), "bb_max": pkg.f3(bb[3:]), "desc": K.SparseMeshDesc(), "stats": K.SparseMeshStats()}

    def call(t, h):
        m, d, s = K.Mesh(), h["desc"], h["stats"]
        s.size, d.size = C.sizeof(s), C.sizeof(d)
        d.program, d.cells, d.flags, d.lipschitz = prog.h, n, int(materials), L
        d.bb_min, d.bb_max = C.cast(h["bb_min"], C.POINTER(C.c_float)), C.cast(h["bb_max"], C.POINTER(C.c_float))
        d.out, d.stats = C.pointer(m), C.pointer(s)
        rc = pkg.lib.sdfv_program_mesh_extract_sparse(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        meshes.append((m, s.bricks))   # (converted and freed after the gate: mesh_tensors synchronises the device)
        pkg.check(rc)
    try:
        gate.run_synchronous(pkg, SG.Case(f"program_mesh_extract_sparse-{name}-{n}", call, {}, inputs={}, host=host))
    finally:
        got = [(pkg.mesh_tensors(m), bricks) for m, bricks in meshes]
    assert len(got) == 4   # a warm-up and a gated call per poison kind
    for (v, i), bricks in got:
        v, i = v.cpu().numpy(), i.cpu().numpy().astype(np.int64)
        assert bricks == want_stats["bricks"]
        assert v.shape == want_v.shape and i.shape == want_i.shape
        np.testing.assert_array_equal(i, want_i)
        np.testing.assert_array_equal(S.M.bits(v), S.M.bits(want_v))
