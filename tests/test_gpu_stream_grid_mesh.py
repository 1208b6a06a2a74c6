"""Meshing a loaded grid on the caller's stream (tests/stream_gate.py).  sdfv_grid_vertex_materials only enqueues: it is held to
the gate's five assertions behind a sleep and captured into a graph whose second replay reads other positions.
sdfv_grid_mesh_extract is documented to synchronise `stream` (the output size is data dependent) and is held to THAT, outside
capture, as its siblings are (tests/test_gpu_stream_march.py): the mesh is the restatement's with the grid arriving late, the
stream is idle when the call returns, and the host was held for as long as the sleep in front of the call.  Grids and expected
values are tests/test_gpu_containment_grid_mesh.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

import grid_mesh_ref as G
import stream_gate as SG
import test_gpu_containment_grid_mesh as CG
from program_fill_check import interleave
from stream_gate import capture, gate  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
F = np.float32


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def materials_case(pkg, lod, n, misalign):
    t0, t1, v, want = CG.material_case(lod, n)
    _, _, v2, want2 = CG.material_case(lod, n, seed=6)

    def call(t, h):
        pkg.check(pkg.lib.sdfv_grid_vertex_materials(C.byref(h["grid"]), C.c_void_p(t["tex0"].data_ptr()), C.c_void_p(t["tex1"].data_ptr()),
                                                     lod, C.c_void_p(t["vertices"].data_ptr()), n, stream_ptr()))
    return SG.Case(f"grid_vertex_materials[{n}+{misalign}, lod {lod}]", call, {"vertices": want},
                   inputs={"tex0": (t0, 16), "tex1": (t1, 16)}, inouts={"vertices": (v, 16, misalign)},
                   host=lambda: {"grid": pkg.make_grid(CG.DIMS, CG.BB[:3], CG.BB[3:])}, second=({"vertices": v2}, {"vertices": want2}))


@pytest.mark.parametrize("n,misalign", [(257, 0), (255, 4)])
@pytest.mark.parametrize("lod", [1, 2])
def test_grid_vertex_materials_runs_on_the_callers_stream(pkg, gate, lod, n, misalign):
    gate.run(pkg, materials_case(pkg, lod, n, misalign))


@pytest.mark.parametrize("n,misalign", [(257, 0), (255, 4)])
def test_grid_vertex_materials_only_enqueues(pkg, capture, n, misalign):
    capture.run(pkg, materials_case(pkg, 1, n, misalign))


@pytest.mark.parametrize("algorithm", [0, G.DUAL], ids=["marching_cubes", "dual_contouring"])
@pytest.mark.parametrize("source", ["tex0", "volume", "interleaved"])
def test_grid_mesh_extract_synchronises_its_stream(pkg, gate, source, algorithm):
    lod = 2 if source == "tex0" else 1
    t0, t1, want_v, want_i = CG.grid_and_mesh(lod, algorithm)
    vol = np.ascontiguousarray(t0[..., 0])
    inputs = {"tex0": (t0, 16), "tex1": (t1, 16)}
    if source == "volume":
        inputs["dist"] = (vol, 4)
    elif source == "interleaved":
        inputs["dist"] = (interleave(vol), 8)
    meshes = []

    def call(t, h):
        m = pkg._capi.Mesh()
        dist = C.c_void_p(t["dist"].data_ptr()) if "dist" in t else None
        rc = pkg.lib.sdfv_grid_mesh_extract(C.byref(h["grid"]), C.c_void_p(t["tex0"].data_ptr()), C.c_void_p(t["tex1"].data_ptr()), dist,
                                            CG.INTERLEAVED if source == "interleaved" else 0, lod, algorithm, 1, C.byref(m), stream_ptr())
        meshes.append(m)   # (converted and freed after the gate: mesh_tensors synchronises the device)
        pkg.check(rc)
    try:
        gate.run_synchronous(pkg, SG.Case(f"grid_mesh_extract-{source}-{algorithm}", call, {}, inputs=inputs,
                                          host=lambda: {"grid": pkg.make_grid(CG.DIMS, CG.BB[:3], CG.BB[3:])}))
    finally:
        got = [pkg.mesh_tensors(m) for m in meshes]
    assert len(got) == 4   # a warm-up and a gated call per poison kind
    for v, i in got:
        v, i = v.cpu().numpy(), i.cpu().numpy().astype(np.int64)
        assert v.shape == want_v.shape and i.shape == want_i.shape
        np.testing.assert_array_equal(i, want_i)
        np.testing.assert_array_equal(G.bits(v), G.bits(want_v))
