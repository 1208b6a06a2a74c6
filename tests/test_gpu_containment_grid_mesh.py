"""Containment of meshing a loaded grid (tests/arena.py): sdfv_grid_mesh_extract reads the grid's arrays only -- tex0, tex1 and
the distance volume go through the arena, the mesh comes out of the library's own allocations and must be the restatement's
(tests/grid_mesh_ref.py) whatever lies around the grid, and the grid must come back untouched; sdfv_grid_vertex_materials reads
the two textures and the positions and writes the six material words of each vertex, nothing else.  The grids are synthetic
(grid_mesh_ref.synthetic_grid): this is about where the kernels touch memory, the fills have their own files.

Shapes: 9 x 8 x 5 (45 and 360 texels per row pair and slice: no multiple of a workgroup; the last lattice point's voxel is the
grid's last texel) at lod 1 and 2, from each of the three sources of the distances."""
import functools

import numpy as np
import pytest

import arena as A
import grid_mesh_ref as G
from program_fill_check import interleave

pytestmark = pytest.mark.gpu
F = np.float32
DIMS, BB = (9, 8, 5), (-1.0, -0.75, -1.0, 1.0, 1.0, 0.5)
INTERLEAVED = 8


@functools.lru_cache(maxsize=None)
def grid_and_mesh(lod, algorithm):
    t0, t1 = G.synthetic_grid(DIMS, BB, lod, seed=lod)
    v, i, _ = G.extract(t0, t1, BB, lod, algorithm)
    assert len(i) > 0
    for a in (v, i):
        a.setflags(write=False)
    return t0, t1, v, i


@pytest.mark.parametrize("algorithm", [0, G.DUAL], ids=["marching_cubes", "dual_contouring"])
@pytest.mark.parametrize("source", ["tex0", "volume", "interleaved"])
@pytest.mark.parametrize("lod", [1, 2])
def test_grid_mesh_extract_reads_the_grid_only(pkg, lod, source, algorithm):
    import torch
    t0, t1, want_v, want_i = grid_and_mesh(lod, algorithm)
    vol = np.ascontiguousarray(t0[..., 0])
    arrays = [t0, t1] + ([] if source == "tex0" else [vol])
    band = A.band_for(*arrays)
    ar = A.Arena(A.arena_bytes(band, *arrays), band=band)
    d0, d1 = ar.input(t0, align=16, name="tex0"), ar.input(t1, align=16, name="tex1")
    dist = None
    if source == "volume":
        dist = ar.input(vol, align=4, misalign=4, name="dist")
    elif source == "interleaved":
        dist = ar.input(interleave(vol), align=8, name="dist")
    grid = pkg.make_grid(DIMS, BB[:3], BB[3:])
    meshes = []

    def run():
        v, i = pkg.grid_mesh_extract(grid, d0, d1, dist=dist, volume_flags=INTERLEAVED if source == "interleaved" else 0, lod=lod,
                                     algorithm=algorithm, materials=True)
        torch.cuda.synchronize()
        meshes.append((v.cpu().numpy(), i.cpu().numpy().astype(np.int64)))
    ar.twin(run, {}, kinds=("nan", "hit"))
    for v, i in meshes:
        assert v.shape == want_v.shape and i.shape == want_i.shape
        np.testing.assert_array_equal(i, want_i)
        np.testing.assert_array_equal(G.bits(v), G.bits(want_v))


def material_case(lod, n, seed=5):
    """(tex0, tex1, vertices, expected): n positions in and around the lattice's box, every other word of a record 9.0."""
    t0, t1 = G.synthetic_grid(DIMS, BB, lod, seed=lod)
    _, box = G.lattice_of(DIMS, BB, lod)
    lo, hi = np.array(box[:3]), np.array(box[3:])
    rng = np.random.default_rng(seed)
    p = rng.uniform(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), size=(n, 3))
    p[:8] = [[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)]      # the corners: the grid's first and last voxel
    v = np.full((n, 12), 9.0, F)
    v[:, :3] = p.astype(F)
    want = v.copy()
    want[:, 6:] = G.materials(t0, t1, BB, lod, v[:, :3])
    return t0, t1, v, want


@pytest.mark.parametrize("n,misalign", [(257, 0), (255, 4)])
@pytest.mark.parametrize("lod", [1, 2])
def test_grid_vertex_materials_writes_the_material_words_only(pkg, lod, n, misalign):
    """257 vertices are a workgroup and one more, 255 leave the last lanes idle; the records 16-byte aligned and 4 bytes off."""
    t0, t1, v, want = material_case(lod, n)
    band = A.band_for(t0, t1)
    ar = A.Arena(A.arena_bytes(band, t0, t1, v), band=band)
    d0, d1 = ar.input(t0, align=16, name="tex0"), ar.input(t1, align=16, name="tex1")
    vertices = ar.inout(v, align=16, misalign=misalign, name="vertices")
    grid = pkg.make_grid(DIMS, BB[:3], BB[3:])
    ar.twin(lambda: pkg.grid_vertex_materials(grid, d0, d1, vertices, lod=lod), {"vertices": want}, kinds=("canary", "nan"))
