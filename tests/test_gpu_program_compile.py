"""GPU tests of sdfv_program_compile: every compiled route against the interpreted handle of the same program through the same
call.  "Equal" means every 32-bit word is equal -- the specialised kernels are the interpreter's text with the instructions as
constants, built by the same compiler under the same flags -- with the one exception include/sdfgrid.h makes for programs: where
a NaN distance arises, both sides are NaN.  A compile is part of each test: only the route the test needs."""
import ctypes as C
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

import program_geometry as G

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from program_mesh_bench import spheres8  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY = -7.0


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


def builders(PM):
    return {"demo3": PM.Program().cube(0.95).sphere(1.05).subtract(), "spheres8": spheres8(PM), "example_sixteen": PM.example_sixteen(),
            "every_opcode": G.emit(G.scene_every_opcode(), PM)}


def words(t):
    return t.contiguous().view(torch.int32)


def assert_equal(a, b, what):
    assert torch.equal(words(a), words(b)), f"{what}: {int((words(a) != words(b)).sum())} words differ"


def assert_equal_nan_rule(a, b, what):
    """Records [n, 7]: bit for bit, or both distances NaN."""
    both_nan = (torch.isnan(a[:, 0]) & torch.isnan(b[:, 0]))[:, None]
    same = (words(a) == words(b)) | both_nan
    assert bool(same.all()), f"{what}: {int((~same).sum())} words differ"


def launches(p):
    return p.compiled_info()["launches"]


# ---- fill ----
FILL_GRIDS = {"9x7x5": ((9, 7, 5), 0, 5), "70x6x3": ((70, 6, 3), 0, 3), "130x4x3": ((130, 4, 3), 0, 3), "slab": ((70, 6, 8), 2, 5)}


@pytest.mark.parametrize("grid", list(FILL_GRIDS))
@pytest.mark.parametrize("name", ["demo3", "spheres8", "example_sixteen", "every_opcode"])
def test_fill(pkg, PM, name, grid):
    K = pkg._capi
    plain = builders(PM)[name].build()
    comp = plain.compile(PM.FILL)
    dims, z0, z1 = FILL_GRIDS[grid]
    g = pkg.make_grid(dims, z_begin=z0, z_end=z1)
    shape = (z1 - z0, dims[1], dims[0])
    count = 0
    for volume in (None, "plain") + (("ilv",) if dims[1] % 2 == 0 else ()):   # (the interleaved volume pairs rows: H even)
        for nt in (0, 1):
            for quant in (0, 1):
                got = []
                for p in (plain, comp):
                    t0, t1 = (torch.full(shape + (4,), CANARY, device="cuda") for _ in range(2))
                    dist = None if volume is None else torch.full(shape, CANARY, device="cuda")
                    with pkg.options({K.OPT_FILL_NONTEMPORAL: nt, K.OPT_EXT_SRGB_QUANT: quant}):
                        p.fill_grid(g, t0, t1, dist=dist, flags=K.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0)
                    got.append((t0, t1, dist))
                count += 1
                what = f"{name} {grid} volume={volume} nt={nt} quant={quant}"
                assert_equal(got[0][0], got[1][0], what + " tex0")
                assert_equal(got[0][1], got[1][1], what + " tex1")
                if volume is not None:
                    assert_equal(got[0][2], got[1][2], what + " dist")
                assert not bool((got[1][0] == CANARY).any())
                assert launches(comp) == count and launches(plain) == 0, what


# ---- points ----
def special_points(n):
    rng = np.random.default_rng(5)
    p = rng.uniform(-1.2, 1.2, (max(n, 1), 3)).astype(np.float32)
    specials = [0.0, -0.0, 1e-42, -1e-42, 1e30, -1e30, np.inf, -np.inf, np.nan]
    for i, v in enumerate(specials):
        if i < n:
            p[i, i % 3] = v
    return p[:n]


def expected_point_launches(n, aligned):
    if n == 0:
        return 0
    whole = n // 256 if aligned else 0
    return (1 if whole else 0) + (1 if whole * 256 < n else 0)


@pytest.mark.parametrize("distance_only", [False, True])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off_by_a_float"])
def test_points(pkg, PM, off, distance_only):
    plain = builders(PM)["example_sixteen"].build()
    comp = plain.compile(PM.POINTS)
    for n in (0, 1, 63, 64, 65, 4099):
        host = special_points(n)
        before = launches(comp)
        got = []
        for p in (plain, comp):
            pin = torch.zeros(n * 3 + 8, device="cuda")
            pout = torch.full((n * 7 + 8,), CANARY, device="cuda")
            assert pin.data_ptr() % 16 == 0 and pout.data_ptr() % 16 == 0
            pts = pin[off:off + n * 3].view(n, 3)
            pts.copy_(torch.from_numpy(host))
            out = pout[off:off + n * 7].view(n, 7)
            p.sample_points(pts, distance_only=distance_only, out=out)
            got.append(pout)
        assert_equal_nan_rule(got[0][off:off + n * 7].view(n, 7), got[1][off:off + n * 7].view(n, 7), f"n={n}")
        assert bool((got[1][off + n * 7:] == CANARY).all()) and bool((got[1][:off] == CANARY).all())
        assert launches(comp) - before == expected_point_launches(n, off == 0), n
        # ... and through host buffers (evaluated on the device)
        before = launches(comp)
        a, b = plain.sample_points_host(host, distance_only), comp.sample_points_host(host, distance_only)
        assert_equal_nan_rule(torch.from_numpy(a), torch.from_numpy(b), f"host n={n}")
        assert launches(comp) - before in {expected_point_launches(n, True), expected_point_launches(n, False)}, n
        assert (launches(comp) - before > 0) == (n > 0)
    assert launches(plain) == 0


# ---- march ----
@pytest.mark.parametrize("n_cam", [2, 17])
@pytest.mark.parametrize("name", ["spheres8", "demo3"])
def test_march(pkg, PM, name, n_cam):
    width, height, y0, y1 = 70, 45, 3, 41
    plain = builders(PM)[name].build()
    comp = plain.compile(PM.MARCH)
    cams = []
    for k in range(n_cam):
        ang = 0.37 * k
        cams.append(pkg.camera_look_at(eye=(1.9 * math.cos(ang) + 2.3 * math.sin(ang), 2.3, 3.8 - 0.1 * k), aspect=width / height))
    worst = 0.0
    count = 0
    for normal_h in (0.0, 0.01):
        for kw in (dict(want_aux=True, want_depth=True), dict(rgba8=True), dict()):
            a = plain.render(cams, width, height, normal_h=normal_h, y0=y0, y1=y1, **kw)
            b = comp.render(cams, width, height, normal_h=normal_h, y0=y0, y1=y1, **kw)
            count += (n_cam + 15) // 16
            a, b = (x if isinstance(x, tuple) else (x,) for x in (a, b))
            what = f"{name} cams={n_cam} normal_h={normal_h} {kw}"
            if kw.get("rgba8"):
                assert_equal(a[0], b[0], what + " rgba8")
            else:
                delta = float((a[0] - b[0]).abs().max())
                worst = max(worst, delta)
                assert delta <= 1e-4, (what, delta)          # the bound of tests/test_gpu_program_march.py
            if kw.get("want_aux"):
                assert bool((words(a[1])[..., 0] == 1).any()), "some pixels hit"
                assert_equal(a[1], b[1], what + " aux")      # every field of the record
                assert_equal(a[2], b[2], what + " depth")
            assert launches(comp) == count and launches(plain) == 0, what
    print(f"{name} cams={n_cam}: max |d rgba| between the interpreted and the compiled march = {worst:.3e}")


# ---- routes that were not compiled ----
def test_routes_not_compiled_interpret(pkg, PM):
    K = pkg._capi
    plain = builders(PM)["spheres8"].build()
    comp = plain.compile(PM.FILL)
    g = pkg.make_grid((20, 12, 10))
    t0, t1 = pkg.alloc_textures(g)
    comp.fill_grid(g, t0, t1)
    after_fill = launches(comp)
    assert after_fill == 1
    pts = torch.from_numpy(special_points(300)[9:]).cuda()
    assert_equal_nan_rule(plain.sample_points(pts), comp.sample_points(pts), "sample_points")
    assert_equal(plain.normal_points(pts, 0.01), comp.normal_points(pts, 0.01), "normal_points")
    cam = pkg.camera_look_at(eye=(1.9, 2.3, 3.8), aspect=40 / 30)
    ra, rb = plain.render(cam, 40, 30, want_aux=True), comp.render(cam, 40, 30, want_aux=True)
    assert_equal(ra[1], rb[1], "aux")
    assert float((ra[0] - rb[0]).abs().max()) <= 1e-4
    (va, ia), (vb, ib) = plain.mesh(12, materials=True), comp.mesh(12, materials=True)
    assert_equal(va, vb, "mesh vertices")
    assert torch.equal(ia, ib) and ia.numel() > 0
    # a pass with a box: the box launch and the scan interpret
    box = (-0.2, -0.3, -0.4, 0.5, 0.6, 0.7)
    passes = []
    for p in (plain, comp):
        a0, a1 = t0.clone(), t1.clone()
        a0[5:] = pkg.AIR_DIST
        a1[5:] = pkg.AIR_DIST
        p.grid_pass(g, 1, a0, a1, changed_box=box)
        passes.append((a0, a1))
    assert_equal(passes[0][0], passes[1][0], "pass tex0")
    assert_equal(passes[0][1], passes[1][1], "pass tex1")
    assert launches(comp) == after_fill


def test_grid_pass_takes_the_specialised_fill_where_it_is_the_dense_fill(pkg, PM):
    K = pkg._capi
    plain = builders(PM)["example_sixteen"].build()
    comp = plain.compile(PM.FILL)
    g = pkg.make_grid((70, 6, 5))
    got = []
    for p in (plain, comp):
        t0, t1 = (torch.full((5, 6, 70, 4), float(pkg.AIR_DIST), device="cuda") for _ in range(2))
        p.grid_pass(g, 1, t0, t1, flags=K.PASS_FRESH_GRID)
        got.append((t0, t1))
    assert_equal(got[0][0], got[1][0], "tex0")
    assert_equal(got[0][1], got[1][1], "tex1")
    assert launches(comp) == 1 and launches(plain) == 0
    assert bool((got[1][0][..., 0] != float(pkg.AIR_DIST)).any())


# ---- the viewer ----
def test_viewer_loads_a_compiled_program(pkg, PM):
    """sdfv_program_as_surface of a compiled handle needs nothing new: whichever route the viewer takes for the surface (its
    device sampler is sdfv_program_sample_points over the handle, a whole pass is sdfv_program_grid_pass / _fill_grid_commit
    over the handle) arrives at a compiled route."""
    V = importlib.import_module("sdf-viewer_amd.viewer")
    builder = builders(PM)["example_sixteen"]
    plain = builder.build()
    comp = plain.compile(PM.FILL | PM.POINTS)
    loaded = []
    for p in (plain, comp):
        surf = p.as_surface()
        v = V.Viewer.new_voxels((16, 16, 16), builder.bb, 3)
        for _ in range(64):
            if not v.state()["remaining"]:
                break
            v.update(surf, budget_s=10.0)
        assert not v.state()["remaining"]
        torch.cuda.synchronize()
        loaded.append(v.download())
        v.close()
    assert loaded[0][0].tobytes() == loaded[1][0].tobytes() and loaded[0][1].tobytes() == loaded[1][1].tobytes()
    assert len(np.unique(loaded[1][0][..., 0])) > 16                  # a loaded model, not a constant grid
    assert launches(comp) > 0 and launches(plain) == 0


# ---- a handle compiled for another architecture ----
def test_wrong_architecture_is_refused_before_anything_runs(pkg, PM):
    plain = builders(PM)["demo3"].build()
    comp = plain.compile(PM.FILL | PM.POINTS | PM.MARCH, arch="gfx90a")     # (compiles without that device; never loaded here)
    here = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    assert here != "gfx90a"
    g = pkg.make_grid((9, 7, 5))
    t0, t1 = (torch.full((5, 7, 9, 4), CANARY, device="cuda") for _ in range(2))
    pts = torch.zeros((65, 3), device="cuda")
    out = torch.full((65, 7), CANARY, device="cuda")
    rgba = torch.full((1, 8, 8, 4), CANARY, device="cuda")
    cam = pkg.camera_look_at(aspect=1.0)
    for call in (lambda: comp.fill_grid(g, t0, t1), lambda: comp.sample_points(pts, out=out), lambda: comp.render(cam, 8, 8, out=rgba)):
        with pytest.raises(pkg.SdfvError) as e:
            call()
        assert e.value.code == -1 and "gfx90a" in str(e.value) and here in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for t in (t0, t1, out, rgba):
        assert bool((t == CANARY).all())
    assert launches(comp) == 0
    # the routes that interpret still work on this handle
    assert_equal(plain.normal_points(pts + 0.3, 0.01), comp.normal_points(pts + 0.3, 0.01), "normal_points")
