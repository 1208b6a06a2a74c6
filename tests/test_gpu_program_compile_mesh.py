"""The mesh route of sdfv_program_compile (SDFV_COMPILE_MESH) against the plain handle of the same program, bytes for bytes:
dense extraction (marching cubes and dual contouring, with and without materials), sparse extraction with its statistics,
normal_points and mesh_postproc over aligned and unaligned arrays, at the smallest shapes where a kernel can go wrong; the
launch counter against the formula of include/sdfgrid.h (sdfv_compiled_info.launches); the other routes of such a handle, which
interpret; a handle compiled for another processor, which is refused before anything runs.  Each program is compiled once per
module."""
import functools
import importlib

import numpy as np
import pytest
import torch

import program_compile_cases as CC
import program_fuzz as Z
import program_ref as R
from test_gpu_program_compile import CANARY, assert_equal, builders, expected_point_launches, launches, special_points, words

pytestmark = pytest.mark.gpu
F = np.float32
DENSE_PROGRAMS = ["spheres8", "every_opcode", "tiny_k", "pow2_k", "identities", "subnormal_sizes"]
DENSE_CELLS = (1, 5, 12, 33)     # 8 lattice points: less than a wave; 34^3: no multiple of 256
SPARSE_CELLS = (8, 16, 32, 64)
DUAL = 4                         # SDFV_MESHER_DUAL_CONTOURING_PARTICLE
LIPSCHITZ = {"spheres8": 0.0, "every_opcode": 2.0, "tiny_k": 0.0, "pow2_k": 1.5, "identities": 2.0, "subnormal_sizes": 0.0}


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


def all_builders(PM):
    b = dict(builders(PM))
    b.update(CC.folding_programs(PM))
    return b


@pytest.fixture(scope="module")
def handles(PM):
    """name -> (builder, plain handle, handle compiled with MESH alone), each made on first use and kept for the module."""
    made = {}
    known = all_builders(PM)

    def get(name):
        if name not in made:
            plain = known[name].build()
            made[name] = (known[name], plain, plain.compile(PM.MESH))
        return made[name]
    return get


def assert_same_mesh(a, b, what):
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape, f"{what}: {tuple(a[0].shape)} / {tuple(b[0].shape)} vertices"
    assert_equal(a[0], b[0], f"{what} vertices")
    assert torch.equal(a[1], b[1]), f"{what} indices"


def octants(bb):
    lo, hi = np.array(bb[:3], F), np.array(bb[3:], F)
    mid = (lo + hi) * F(0.5)
    for o in range(8):
        up = [(o >> a) & 1 for a in range(3)]
        yield tuple(float((mid if u else lo)[a]) for a, u in enumerate(up)) + tuple(float((hi if u else mid)[a]) for a, u in enumerate(up))


@functools.lru_cache(maxsize=None)
def crossing_box(name, cells):
    """The box a program is meshed over at `cells`: its own if its distance takes both signs on that lattice (the numpy
    restatement), else the first of its octants, then of their octants, where it does -- so that no comparison is between two
    empty meshes."""
    PM = importlib.import_module("sdf-viewer_amd.program")
    builder = all_builders(PM)[name]
    level = [builder.bb]
    for _ in range(3):
        for box in level:
            if Z.changes_sign(builder.ops, box, n=cells + 1):
                return box
        level = [o for box in level for o in octants(box)]
    # ... else (one cell, a thin surface) the cell of a 16^3 lattice over the box whose corners are deepest on both sides
    n = 17
    bb = builder.bb
    pos = R.grid_positions((n, n, n), bb[:3], bb[3:]).reshape(n, n, n, 3)
    d = R.run(builder.ops, pos.reshape(-1, 3), True)[:, 0].reshape(n, n, n)
    corners = np.stack([d[dz:n - 1 + dz, dy:n - 1 + dy, dx:n - 1 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)])
    margin = np.minimum(corners.max(axis=0), -corners.min(axis=0))
    k, j, i = np.unravel_index(np.argmax(margin), margin.shape)
    assert margin[k, j, i] > 0, f"{name}: no box found that crosses a lattice of {cells} cells"
    box = tuple(float(v) for v in pos[k, j, i]) + tuple(float(v) for v in pos[k + 1, j + 1, i + 1])
    assert Z.changes_sign(builder.ops, box, n=cells + 1), (name, cells, box)
    return box


# ---- dense extraction ----
@pytest.mark.parametrize("name", DENSE_PROGRAMS)
def test_dense_extraction(pkg, PM, handles, name):
    builder, plain, comp = handles(name)
    for cells in DENSE_CELLS:
        bb = crossing_box(name, cells)
        for materials in (False, True):
            for algorithm in (0, DUAL):
                what = f"{name} cells={cells} materials={materials} algorithm={algorithm}"
                before = launches(comp)
                a = plain.mesh(cells, bb=bb, materials=materials, algorithm=algorithm)
                b = comp.mesh(cells, bb=bb, materials=materials, algorithm=algorithm)
                assert_same_mesh(a, b, what)
                assert a[0].shape[0] > 0, f"{what}: an empty mesh"
                if algorithm == 0:                                          # (a quad needs a crossing edge off the box's faces)
                    assert a[1].numel() > 0, f"{what}: no triangle"
                assert launches(comp) - before == 1 + (2 if algorithm == DUAL else 1), what
    assert launches(plain) == 0


def test_a_program_without_a_surface_skips_the_vertex_launch(pkg, PM, handles):
    """example_sixteen has no surface in its box at these lattices: both handles give an empty mesh, and the compiled one has
    launched the lattice kernel alone."""
    _, plain, comp = handles("example_sixteen")
    for cells in (1, 12):
        for algorithm in (0, DUAL):
            before = launches(comp)
            a = plain.mesh(cells, materials=True, algorithm=algorithm)
            b = comp.mesh(cells, materials=True, algorithm=algorithm)
            assert a[0].shape[0] == 0 and b[0].shape[0] == 0 and a[1].numel() == 0 and b[1].numel() == 0
            assert launches(comp) - before == 1
    assert launches(plain) == 0


# ---- sparse extraction ----
@pytest.mark.parametrize("name", DENSE_PROGRAMS)
def test_sparse_extraction(pkg, PM, handles, name):
    _, plain, comp = handles(name)
    L = LIPSCHITZ[name]
    for cells in SPARSE_CELLS:
        for materials in (False, True):
            what = f"{name} sparse cells={cells} materials={materials} L={L}"
            before = launches(comp)
            av, ai, astats = plain.mesh_sparse(cells, materials=materials, lipschitz=L, want_stats=True)
            bv, bi, bstats = comp.mesh_sparse(cells, materials=materials, lipschitz=L, want_stats=True)
            assert_same_mesh((av, ai), (bv, bi), what)
            assert astats == bstats, what
            if name in ("spheres8", "every_opcode"):                        # (1-Lipschitz within L: the dense mesh's set)
                assert av.shape[0] > 0 and ai.numel() > 0, f"{what}: an empty mesh"
            # the header's formula: refinement levels run + the brick lattice + the vertex phase
            levels_run = sum(1 for lv in range(astats["levels"]) if lv == 0 or astats["kept"][lv - 1] > 0)
            want = levels_run + (1 if astats["bricks"] else 0) + (1 if av.shape[0] else 0)
            assert launches(comp) - before == want, (what, astats)
    assert any(v > 1.0 for v in LIPSCHITZ.values())
    assert launches(plain) == 0


# ---- normal_points ----
@pytest.mark.parametrize("eps", [0.0, 0.01])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off_by_a_float"])
def test_normal_points(pkg, PM, handles, off, eps):
    for name in ("every_opcode", "spheres8"):
        _, plain, comp = handles(name)
        for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
            host = special_points(n)
            before = launches(comp)
            got = []
            for p in (plain, comp):
                pin = torch.zeros(n * 3 + 8, device="cuda")
                pout = torch.full((n * 3 + 8,), CANARY, device="cuda")
                assert pin.data_ptr() % 16 == 0 and pout.data_ptr() % 16 == 0
                pts = pin[off:off + n * 3].view(n, 3)
                pts.copy_(torch.from_numpy(host))
                p.normal_points(pts, eps, out=pout[off:off + n * 3].view(n, 3))
                got.append(pout)
            assert_equal(got[0], got[1], f"{name} n={n}")                 # as bits: NaN normals occur; the canaries too
            assert bool((got[1][off + n * 3:] == CANARY).all()) and bool((got[1][:off] == CANARY).all())
            assert launches(comp) - before == expected_point_launches(n, off == 0), n
        assert launches(plain) == 0


# ---- mesh_postproc ----
def postproc_vertices(n, normals):
    """[n, 12] vertices at seeded points: normals all unset (postproc computes them), all set (kept), or mixed within one wave."""
    rng = np.random.default_rng(17)
    v = np.zeros((n, 12), F)
    v[:, :3] = rng.uniform(-1.0, 1.0, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    unset = {"unset": np.ones(n, bool), "set": np.zeros(n, bool), "mixed": (np.arange(n) % 64) % 3 == 0}[normals]
    if normals == "mixed" and n > 128:
        unset[64:128] = False                                             # one whole wave skips the taps
    v[:, 3:6] = (d * np.where(unset, 0.005, 1.0)[:, None]).astype(F)
    v[:, 6:] = 9.0
    return v


@pytest.mark.parametrize("normals", ["unset", "set", "mixed"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off_by_a_float"])
def test_mesh_postproc(pkg, PM, handles, off, normals):
    for name in ("every_opcode", "spheres8"):
        _, plain, comp = handles(name)
        for n in (1, 65, 300):
            host = postproc_vertices(n, normals)
            before = launches(comp)
            got = []
            for p in (plain, comp):
                buf = torch.full((n * 12 + 8,), CANARY, device="cuda")
                assert buf.data_ptr() % 16 == 0
                v = buf[off:off + n * 12].view(n, 12)
                v.copy_(torch.from_numpy(host))
                p.mesh_postproc(v)
                got.append(buf)
            assert_equal(got[0], got[1], f"{name} n={n} {normals}")
            assert bool((got[1][off + n * 12:] == CANARY).all()) and bool((got[1][:off] == CANARY).all())
            changed = words(got[1][off:off + n * 12].view(n, 12)[:, 3:6]) != words(torch.from_numpy(host[:, 3:6]).cuda())
            assert bool(changed.any()) == (normals != "set"), (name, n, normals)
            assert launches(comp) - before == 1, n
        assert launches(plain) == 0


# ---- the fuzz share ----
@functools.lru_cache(maxsize=None)
def fuzz_share():
    short = CC.short_extreme(Z.seed())
    return [short[k] for k in Z.share([(ops, bb) for _, ops, bb in short])]


@pytest.mark.parametrize("k", range(13))
def test_fuzz_share(pkg, PM, k):
    """Short programs of the extreme corpus (legal operands from the edges) that change sign on their lattice: dense extraction
    at 12 cells, sparse at 16, 300 normals.  SDFV_SOAK_SEED re-seeds the corpus."""
    share = fuzz_share()
    assert len(share) >= 13
    for index, ops, bb in share[k:k + 1] + (share[13:] if k == 12 else []):  # (a re-seeded corpus may share out more than 13)
        one_fuzz_program(PM, index, ops, bb)


def one_fuzz_program(PM, index, ops, bb):
    what = Z.label(Z.seed(), index, ops, bb)
    plain = Z.builder(PM, ops, bb).build()
    comp = plain.compile(PM.MESH)
    for algorithm in (0, DUAL):
        assert_same_mesh(plain.mesh(12, materials=True, algorithm=algorithm), comp.mesh(12, materials=True, algorithm=algorithm),
                         f"{what} algorithm={algorithm}")
    av, ai, astats = plain.mesh_sparse(16, materials=True, lipschitz=4.0, want_stats=True)
    bv, bi, bstats = comp.mesh_sparse(16, materials=True, lipschitz=4.0, want_stats=True)
    assert_same_mesh((av, ai), (bv, bi), f"{what} sparse")
    assert astats == bstats, what
    pts = torch.from_numpy(np.ascontiguousarray(R.points()[:300])).cuda()
    assert_equal(plain.normal_points(pts, 0.0), comp.normal_points(pts, 0.0), f"{what} normals")
    assert launches(comp) > 0 and launches(plain) == 0


# ---- the other routes of a MESH-only handle interpret ----
def test_a_mesh_only_handle_interprets_fill_sampler_and_march(pkg, PM, handles):
    _, plain, comp = handles("spheres8")
    before = launches(comp)
    g = pkg.make_grid((20, 12, 10))
    pts = torch.from_numpy(special_points(300)).cuda()
    cam = pkg.camera_look_at(eye=(1.9, 2.3, 3.8), target=(0.0, 0.0, 0.0), aspect=24 / 16)
    got = []
    for p in (plain, comp):
        t0, t1 = pkg.alloc_textures(g)
        p.fill_grid(g, t0, t1)
        got.append((t0, t1, p.sample_points(pts), p.render(cam, 24, 16)))
    for a, b, what in zip(got[0], got[1], ("tex0", "tex1", "records", "rgba")):
        a, b = (x[0] if isinstance(x, (tuple, list)) else x for x in (a, b))
        assert_equal(a, b, what)
    assert launches(comp) == before and launches(plain) == 0


# ---- a handle compiled for another processor ----
def test_wrong_architecture_is_refused_before_anything_runs(pkg, PM):
    plain = builders(PM)["demo3"].build()
    comp = plain.compile(PM.MESH, arch="gfx90a")                             # (compiles without that device; never loaded here)
    here = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    assert here != "gfx90a"
    pts = torch.zeros((65, 3), device="cuda")
    out = torch.full((65, 3), CANARY, device="cuda")
    verts = torch.full((65, 12), CANARY, device="cuda")
    calls = (lambda: comp.mesh(5), lambda: comp.mesh(5, algorithm=DUAL), lambda: comp.mesh_sparse(8),
             lambda: comp.normal_points(pts, out=out), lambda: comp.mesh_postproc(verts))
    for call in calls:
        with pytest.raises(pkg.SdfvError) as e:
            call()
        assert e.value.code == -1 and "gfx90a" in str(e.value) and here in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and bool((verts == CANARY).all())
    assert launches(comp) == 0
    # the routes that interpret still work on this handle
    assert_equal(plain.sample_points(pts + 0.3), comp.sample_points(pts + 0.3), "sample_points")
