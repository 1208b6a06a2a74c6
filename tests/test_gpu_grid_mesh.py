"""Meshing a loaded grid on the device (include/sdfgrid.h, "Meshing a loaded grid") over grids the library's own fills wrote:
cubic grids against sdfv_lattice_mesh_extract over the numpy-unpacked lattice, grids that are no cube against the numpy
restatement (tests/grid_mesh_ref.py) from tex0 alone, the plain and the interleaved volume, partly loaded grids at lod 2 and 4,
an empty grid, sdfv_grid_vertex_materials at arbitrary points, and what the demo's mesh means against float64 geometry.
Everything is compared bit for bit."""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import demo_geometry as DG
import grid_mesh_ref as G
from program_fill_check import interleave

pytestmark = pytest.mark.gpu
F = np.float32
BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
SLAB_BOX = (-1.0, -0.5, -1.25, 1.0, 1.0, 1.0)             # tests/golden/grid_9x7x5.npz's box: three different voxel sides
ALGORITHMS = (0, G.DUAL)
INTERLEAVED = 8                                           # SDFV_PASS_VOLUME_INTERLEAVED


@pytest.fixture(scope="module")
def PM(pkg):  # noqa: N802
    return importlib.import_module("sdf-viewer_amd.program")


def spheres8(PM, bb):  # noqa: N803
    """Eight blended spheres with a material each (tools/program_mesh_bench.py's model): colours and material values vary over
    the surface."""
    s = PM.Program(bb)
    for i in range(8):
        ang = math.radians(45.0 * i)
        s.material(0.1 + 0.1 * i, 0.9 - 0.1 * i, 0.5, 0.1 * i, 0.5, 1.0)
        s.push_affine(PM.translation(0.55 * math.cos(ang), 0.55 * math.sin(ang), 0.1 * (i % 3 - 1))).sphere(0.22).pop()
        if i:
            s.smooth_union(0.1)
    return s.build()


def box_in(bb, scale):
    return tuple(v * scale for v in bb)


class Loaded:
    """A grid on the device with its volumes, and its textures on the host."""

    def __init__(self, pkg, dims, bb, fill):
        self.dims, self.bb = dims, bb
        self.grid = pkg.make_grid(dims, bb[:3], bb[3:])
        self.t0, self.t1 = pkg.alloc_textures(self.grid)
        self.dist = torch.empty((dims[2], dims[1], dims[0]), dtype=torch.float32, device="cuda")
        fill(self)
        torch.cuda.synchronize()
        self.h0, self.h1 = self.t0.cpu().numpy(), self.t1.cpu().numpy()
        assert (G.bits(self.dist.cpu().numpy()) == G.bits(self.h0[..., 0])).all()        # the volume mirrors tex0.r
        self.ilv = torch.from_numpy(interleave(self.h0[..., 0])).cuda() if dims[1] % 2 == 0 else None


@functools.lru_cache(maxsize=None)
def loaded(model, dims, bb):
    """Filled once per (model, dims, box), shared, never modified."""
    pkg = importlib.import_module("sdf-viewer_amd")
    PM = importlib.import_module("sdf-viewer_amd.program")  # noqa: N806
    if model == "demo":
        prm = pkg.default_params()
        return Loaded(pkg, dims, bb, lambda g: pkg.fill_grid(prm, g.grid, g.t0, g.t1, dist=g.dist))
    prog = spheres8(PM, bb)
    return Loaded(pkg, dims, bb, lambda g: prog.fill_grid(g.grid, g.t0, g.t1, dist=g.dist))


def host(v, i):
    return v.cpu().numpy(), i.cpu().numpy().astype(np.int64)


def assert_same_mesh(got, want, what, fields=slice(0, 12)):
    (gv, gi), (wv, wi) = got, want
    assert gv.shape == wv.shape and gi.shape == wi.shape, (what, gv.shape, wv.shape, gi.shape, wi.shape)
    assert (gi == wi).all(), (what, "indices")
    for name, cols in (("positions", slice(0, 3)), ("normals", slice(3, 6)), ("materials", slice(6, 12))):
        if cols.start >= fields.start and cols.stop <= fields.stop:
            bad = np.nonzero((G.bits(gv[:, cols]) != G.bits(wv[:, cols])).any(axis=1))[0]
            assert bad.size == 0, (what, name, bad[:5], gv[bad[:5], cols], wv[bad[:5], cols])


# ---- cubic grids: the lattice route over the unpacked lattice is the yardstick ----
@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("n", [17, 33])
@pytest.mark.parametrize("model", ["demo", "spheres8"])
def test_a_cubic_grid_meshes_as_its_unpacked_lattice_does(pkg, model, n, algorithm):
    g = loaded(model, (n, n, n), BOX)
    cells, box = G.lattice_of(g.dims, g.bb, 1)
    assert cells == (n - 1,) * 3 and box == BOX
    d = G.unpack(g.h0[..., 0], 1)
    want = host(*pkg.lattice_mesh_extract(torch.from_numpy(d).cuda(), box, n - 1, algorithm))
    assert want[0].shape[0] > 100 and want[1].shape[0] > 100
    mats = G.materials(g.h0, g.h1, g.bb, 1, want[0][:, :3])
    assert len(np.unique(mats[:, :3], axis=0)) > (1 if model == "demo" else 4)       # the colours vary over the surface
    with_mats = want[0].copy()
    with_mats[:, 6:] = mats
    keep0, keep1, keepd = g.t0.clone(), g.t1.clone(), g.dist.clone()
    for what, kw in (("tex0", {}), ("volume", dict(dist=g.dist)), ("interleaved", dict(dist=g.ilv, volume_flags=INTERLEAVED))):
        if what == "interleaved" and g.ilv is None:
            continue
        got = host(*pkg.grid_mesh_extract(g.grid, g.t0, g.t1, algorithm=algorithm, materials=True, **kw))
        assert_same_mesh(got, (with_mats, want[1]), (model, n, algorithm, what))
        bare = host(*pkg.grid_mesh_extract(g.grid, g.t0, None, algorithm=algorithm, materials=False, **kw))
        assert_same_mesh(bare, want, (model, n, algorithm, what, "no materials"))          # zero materials, tex1 not needed
    assert torch.equal(g.t0, keep0) and torch.equal(g.t1, keep1) and torch.equal(g.dist, keepd), "the grid is read, never written"


# ---- grids that are no cube: the restatement is the yardstick ----
@functools.lru_cache(maxsize=None)
def restated(model, dims, bb, lod, algorithm):
    g = loaded(model, dims, bb)
    v, i, info = G.extract(g.h0, g.h1, bb, lod, algorithm)
    v.setflags(write=False)
    i.setflags(write=False)
    return v, i, info


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("dims", [(9, 7, 5), (9, 8, 5), (33, 18, 10)])
def test_a_grid_that_is_no_cube_meshes_as_the_restatement_from_every_source(pkg, dims, algorithm):
    """tex0 alone, the plain volume and the interleaved volume give the restatement's mesh, so identical meshes.  9 x 7 x 5 has
    an odd height, which the interleaved layout refuses by its own rule (the pairs of rows): that grid goes through the two
    other sources and the refusal is held; 9 x 8 x 5 beside it takes all three."""
    g = loaded("spheres8", dims, SLAB_BOX)
    want_v, want_i, info = restated("spheres8", dims, SLAB_BOX, 1, algorithm)
    assert want_v.shape[0] > 20 and want_i.shape[0] > 20 and np.isfinite(want_v).all()
    assert len(np.unique(want_v[:, 6:9], axis=0)) > 1
    assert info["lattice"].shape == (dims[2], dims[1], dims[0])
    sources = [("tex0", {}), ("volume", dict(dist=g.dist))]
    if dims[1] % 2 == 0:
        sources.append(("interleaved", dict(dist=g.ilv, volume_flags=INTERLEAVED)))
    else:
        with pytest.raises(pkg.SdfvError, match="must be even"):
            pkg.grid_mesh_extract(g.grid, g.t0, g.t1, dist=g.dist, volume_flags=INTERLEAVED)
    for what, kw in sources:
        got = host(*pkg.grid_mesh_extract(g.grid, g.t0, g.t1, algorithm=algorithm, materials=True, **kw))
        assert_same_mesh(got, (want_v, want_i), (dims, algorithm, what))


# ---- partly loaded grids ----
@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("lod", [2, 4])
@pytest.mark.parametrize("n", [12, 17])
def test_a_partly_loaded_grid_meshes_over_its_published_voxels_only(pkg, PM, n, lod, algorithm):
    """A fresh grid and one pass at step `lod`: the published voxels hold samples, every other one AIR_DIST.  On 12^3 the step does
    not divide dim - 1: the lattice stops short of the grid's far faces and the mesh's box with it.  The mesh is the
    restatement's, and stays the same bits when every voxel off the lattice is overwritten."""
    bb = box_in(BOX, 1.0)
    dims = (n, n, n)
    prog = spheres8(PM, bb)
    grid = pkg.make_grid(dims, bb[:3], bb[3:])
    t0, t1 = pkg.alloc_textures(grid)
    dist = torch.empty((n, n, n), dtype=torch.float32, device="cuda")
    pkg.grid_init_unvisited(grid, 0, t0, t1, dist)
    prog.grid_pass(grid, lod, t0, t1, dist=dist)
    torch.cuda.synchronize()
    h0, h1 = t0.cpu().numpy(), t1.cpu().numpy()
    idx = np.arange(n)
    on = (idx[:, None, None] % lod == 0) & (idx[None, :, None] % lod == 0) & (idx[None, None, :] % lod == 0)
    assert (h0[~on] == F(pkg.AIR_DIST)).all() and (h0[on][:, 0] != F(pkg.AIR_DIST)).all()
    cells, box = G.lattice_of(dims, bb, lod)
    assert cells == ((n - 1) // lod,) * 3 and (box[3] < bb[3]) == ((n - 1) % lod != 0)
    want_v, want_i, _ = G.extract(h0, h1, bb, lod, algorithm)
    assert want_v.shape[0] > 0 and (want_i.shape[0] > 0 or cells[0] == 2)      # (two cells per axis: 12^3 at lod 4, a handful of vertices)
    first = None
    for garbage in (None, float("nan"), -1.0):
        if garbage is not None:
            mask = torch.from_numpy(~on).cuda()
            t0[mask] = garbage
            t1[mask] = garbage
            dist[mask] = garbage
        for what, kw in (("tex0", {}), ("volume", dict(dist=dist))):
            got = host(*pkg.grid_mesh_extract(grid, t0, t1, lod=lod, algorithm=algorithm, materials=True, **kw))
            assert_same_mesh(got, (want_v, want_i), (n, lod, algorithm, what, garbage))
            first = first or got
            assert (G.bits(got[0]) == G.bits(first[0])).all()


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_a_grid_entirely_at_air_dist_gives_an_empty_mesh(pkg, algorithm):
    grid = pkg.make_grid((12, 10, 7), SLAB_BOX[:3], SLAB_BOX[3:])
    t0, t1 = pkg.alloc_textures(grid)
    dist = torch.empty((7, 10, 12), dtype=torch.float32, device="cuda")
    pkg.grid_init_unvisited(grid, 0, t0, t1, dist)
    for lod in (1, 2):
        for kw in ({}, dict(dist=dist)):
            v, i = pkg.grid_mesh_extract(grid, t0, t1, lod=lod, algorithm=algorithm, materials=True, **kw)
            assert tuple(v.shape) == (0, 12) and tuple(i.shape) == (0,)


# ---- the materials alone ----
@pytest.mark.parametrize("lod,dims", [(1, (9, 7, 5)), (2, (33, 18, 10))])
def test_vertex_materials_at_arbitrary_points(pkg, lod, dims):
    """Points inside cells, on the box's corners and outside the box (the clamp), through a pointer that is only 4-byte aligned:
    the six material words equal the restatement's, the other six stay as they were.  Colours that are no table entries (a NaN,
    a negative, one above 1, one between two entries) go through the same rule."""
    g = loaded("spheres8", dims, SLAB_BOX)
    h0 = g.h0.copy()
    h0[0, 0, 0, 1:] = (np.nan, -0.25, 7.0)
    h0[-1, -1, -1, 1:] = ((G.TABLE[10].astype(np.float64) + G.TABLE[11]) / 2, G.TABLE[255], np.inf)
    t0 = torch.from_numpy(h0).cuda()
    cells, box = G.lattice_of(dims, SLAB_BOX, lod)
    lo, hi = np.array(box[:3]), np.array(box[3:])
    rng = np.random.default_rng(lod)
    m = 1300
    p = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), size=(m, 3))
    p[:600] = rng.uniform(lo, hi, size=(600, 3))
    p[600:608] = [[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)]
    v = np.full((m, 12), 9.0, F)
    v[:, :3] = p.astype(F)
    want = v.copy()
    want[:, 6:] = G.materials(h0, g.h1, SLAB_BOX, lod, v[:, :3])
    assert want[600, 6] == 0 and want[600, 7] == 0 and want[600, 8] == 1               # the NaN, the negative, above the table
    if lod == 1:
        assert want[607, 6] == F(11) / F(255) and want[607, 7] == 1 and want[607, 8] == 1
    for offset in (0, 1):
        buf = torch.zeros(m * 12 + 4, dtype=torch.float32, device="cuda")
        t = buf[offset:offset + m * 12].view(m, 12)
        t.copy_(torch.from_numpy(v))
        pkg.grid_vertex_materials(g.grid, t0, g.t1, t, lod=lod)
        got = t.cpu().numpy()
        bad = np.nonzero((G.bits(got) != G.bits(want)).any(axis=1))[0]
        assert bad.size == 0, (offset, bad[:5], got[bad[:5]], want[bad[:5]])
        assert (buf[:offset] == 0).all() and (buf[offset + m * 12:] == 0).all(), offset


# ---- meaning ----
def test_the_demo_s_marching_cubes_vertices_lie_within_half_a_cell_edge_of_the_true_surface(pkg):
    """The demo at 33^3 over [-1, 1]^3: every marching-cubes vertex has |true distance| <= half a cell edge + 1e-6, the true
    distance from tests/demo_geometry.py in float64.  The ends of a crossing edge differ in sign and the SDF is 1-Lipschitz, so
    with a = |d| at the inside end, b at the outside end and s = a + b <= h the interpolated point has |d| <= (h^2 - s^2) / (2 h)
    <= h / 2.  The cell edge, 2 / 32, is below 0.1: no clamped value takes part."""
    g = loaded("demo", (33, 33, 33), BOX)
    v, i = host(*pkg.grid_mesh_extract(g.grid, g.t0, g.t1, dist=g.dist, materials=True))
    assert v.shape[0] > 1000
    true = DG.evaluate(DG.Params(), v[:, :3].astype(np.float64), distance_only=True).d
    worst = np.abs(true).max()
    print("vertices", v.shape[0], "worst |true distance|", worst, "half a cell edge", 1.0 / 32)
    assert worst <= 1.0 / 32 + 1e-6
