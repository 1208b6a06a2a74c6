"""GPU parity of the grid march over content the demo fill never produces (tests/march_fields.py: rays that run out of steps,
overshoots into the solid, texels that all differ, ray positions exactly on cell boundaries, a surface through the box's
faces, grids filled by SDF programs): march_compare.compare() -- every kernel variant, every aux field bit for bit, RGBA to
RGBA_TOL -- on the grids and cameras tests/test_march_fields_cpu.py holds to their purpose on the oracle alone."""
import importlib

import numpy as np
import pytest
import torch

import march_fields as MF
from march_compare import compare, load_textures

pytestmark = pytest.mark.gpu
AUX_NORMAL = slice(14, 17)  # words of sdfv_march_aux.normal


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


@pytest.fixture(scope="module")
def par(pkg):
    return importlib.import_module("sdf-viewer_amd.parallel")


def on_device(pkg, field, grid):
    dims, lo, hi = MF.GRIDS[grid]
    g = pkg.make_grid(dims, lo, hi)
    h0, h1 = MF.make(field, grid)
    t0, t1 = load_textures(pkg, g, h0, h1)
    return g, t0, t1, h0, h1


class BothNaNNormalsAreEqual:
    """The package, except that where the oracle's normal of a pixel is NaN (a zero tap sum: 0 / 0, whose sign and payload
    differ between the host's and the device's divide) AND the kernel's word is a NaN too, the aux record handed to
    compare() carries the oracle's word.  `normal` only, those pixels only; a NaN on one side alone still fails.
    It relies on how compare() calls raymarch(): ONE camera, the whole image (want_normal is [height, width, 3]: no y0 / y1),
    want_aux passed by keyword, and the aux record last in the result (rgba, depth, aux; no rgba8)."""

    def __init__(self, pkg, want_normal):
        self._pkg = pkg
        self._nan = torch.from_numpy(np.isnan(want_normal)).cuda()
        self._words = torch.from_numpy(want_normal.view(np.int32).copy()).cuda()

    def __getattr__(self, name):
        return getattr(self._pkg, name)

    def raymarch(self, *args, **kw):
        out = self._pkg.raymarch(*args, **kw)
        if kw.get("want_aux"):
            normal = out[-1][0][..., AUX_NORMAL]
            both = self._nan & torch.isnan(normal.view(torch.float32))
            normal[both] = self._words[both]
        return out


def compare_field(pkg, oracle, g, t0, t1, h0, h1, cam_kw, width, height, nan_cap=0.01, **kw):
    """compare(), with BothNaNNormalsAreEqual around the package when the oracle's image holds NaN normals: at most `nan_cap`
    of the hits (1 % for every entry of march_fields' tables, as tests/test_march_fields_cpu.py asserts too).  The oracle
    marches once more here than compare() needs, to know those pixels beforehand: a few milliseconds at these sizes."""
    assert "y0" not in kw and "y1" not in kw
    rp = pkg.default_render_params(g)
    if kw.get("rp_edit"):
        kw["rp_edit"](rp)
    cam = pkg.camera_look_at(aspect=width / height, **cam_kw)
    _, want = oracle.raymarch(oracle.copy_struct(oracle.RenderParams, rp), h0, h1, oracle.copy_struct(oracle.Camera, cam),
                              width, height)
    nan = np.isnan(want["normal"]).any(axis=-1)
    assert nan.sum() <= nan_cap * (want["status"] == 1).sum(), (int(nan.sum()), int((want["status"] == 1).sum()))
    p = BothNaNNormalsAreEqual(pkg, want["normal"]) if nan.any() else pkg
    return compare(p, oracle, g, t0, t1, h0, h1, cam_kw, width, height, **kw)


@pytest.mark.parametrize("grid", list(MF.GRIDS))
@pytest.mark.parametrize("field", list(MF.FIELDS))
def test_every_variant_equals_the_oracle(pkg, oracle, field, grid):
    env = on_device(pkg, field, grid)
    W, H = MF.image_of(field)
    for cam_kw in MF.cameras(field, grid):
        _, aux = compare_field(pkg, oracle, *env, cam_kw=cam_kw, width=W, height=H)
        assert (aux["status"] == 1).any() and (aux["status"] == -2).any()
    if field == "slow":
        assert (aux["status"] == -1).sum() >= 200  # (the axis-aligned camera, outside the box)


@pytest.mark.parametrize("name,grid", MF.PROGRAM_ENTRIES)
def test_every_variant_equals_the_oracle_over_a_program_grid(pkg, oracle, PM, name, grid):
    """The grid as CompiledProgram.fill_grid leaves it on the device (`envelope`: many materials; `deep`), read back for the
    oracle; it must be the restatement's grid (march_fields.program_textures) the CPU tests chose the cameras on.  Every
    camera: hits and rays that leave, at most 1 % NaN normals.  (`deep` over flat8x2x8 is not run: MF.PROGRAM_ENTRIES.)"""
    dims, lo, hi = MF.GRIDS[grid]
    g = pkg.make_grid(dims, lo, hi)
    t0, t1 = MF.fill_program(pkg, PM, name, g)
    torch.cuda.synchronize()
    h0, h1 = t0.cpu().numpy(), t1.cpu().numpy()
    w0, w1 = MF.program_textures(pkg, PM, name, grid)
    np.testing.assert_array_equal(h0.view(np.uint32), w0.view(np.uint32))
    np.testing.assert_array_equal(h1.view(np.uint32), w1.view(np.uint32))
    W, H = MF.IMAGE
    for cam_kw in MF.cameras(name, grid):
        _, aux = compare_field(pkg, oracle, g, t0, t1, h0, h1, cam_kw=cam_kw, width=W, height=H)
        assert (aux["status"] == 1).any() and (aux["status"] == -2).any()


@pytest.mark.parametrize("lod", MF.LODS)
def test_loading_lod_nearest_path_over_noise(pkg, oracle, lod):
    """sdfLODDistBetweenSamples > 1: the NEAREST path over texels that all differ.  NaN normals up to MF.LOD_NAN_CAP of the
    hits (why: march_fields), at least MF.LOD_FINITE_HITS hits with a finite normal over the three cameras -- both held on the
    oracle alone by tests/test_march_fields_cpu.py."""
    env = on_device(pkg, "noise", "cube32")

    def edit(rp):
        rp.lod_dist_between_samples = lod

    W, H = MF.IMAGE
    finite = 0
    for cam_kw in MF.cameras("noise", "cube32"):
        _, aux = compare_field(pkg, oracle, *env, cam_kw=cam_kw, width=W, height=H, rp_edit=edit, nan_cap=MF.LOD_NAN_CAP)
        finite += int(((aux["status"] == 1) & np.isfinite(aux["normal"]).all(axis=-1)).sum())
    assert finite >= MF.LOD_FINITE_HITS


def unorm8_of(rgba):
    """The 8-bit UNORM image of an fp32 one: rint(clamp(c, 0, 1) * 255), NaN -> 0 (sdfv_march_desc.rgba8)."""
    return torch.nan_to_num(rgba, nan=0.0).clamp(0.0, 1.0).mul(255.0).round().to(torch.uint8)


def test_rgba8_output_is_the_quantised_fp32_output_over_noise(pkg):
    """sdfv_march_desc.rgba8 equals rint(clip(fp32) * 255) on every pixel of a twelve-camera batch over noise, written beside
    the fp32 plane or instead of it, over tex0.r and over the distance volume; at least 1000 distinct colours."""
    g, t0, t1, _, _ = on_device(pkg, "noise", "cube32")
    dist = pkg.commit_distance(g, t0)
    rp = pkg.default_render_params(g)
    W, H = MF.IMAGE
    cams = [pkg.camera_look_at(aspect=W / H, **kw) for kw in MF.rgba8_cameras()]
    ref = pkg.raymarch(rp, t0, t1, cams, W, H)
    both, img8 = pkg.raymarch(rp, t0, t1, cams, W, H, rgba8="both")
    only8 = pkg.raymarch(rp, t0, t1, cams, W, H, dist=dist, rgba8="only")
    torch.cuda.synchronize()
    want = unorm8_of(ref)
    assert torch.equal(both.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(img8, want) and torch.equal(only8, want)
    colours = len(torch.unique(want.view(-1, 4), dim=0))
    print(f"{colours} distinct 8-bit colours")
    assert colours >= 1000
    rows = pkg.raymarch(rp, t0, t1, cams[3], W, H, y0=13, y1=50, rgba8="only")
    assert torch.equal(rows[0], want[3, 13:50])


def test_row_ranges_and_camera_batches_over_steep(pkg):
    """Row ranges whose ends are no multiples of the 16-row tile, and a 19-camera batch: RGBA, depth plane and aux record equal
    the single full calls' bit for bit, over tex0.r and over the distance volume."""
    g, t0, t1, _, _ = on_device(pkg, "steep", "cube32")
    dist = pkg.commit_distance(g, t0)
    rp = pkg.default_render_params(g)
    W, H = MF.IMAGE
    kws = MF.cameras("steep", "cube32")
    cams = [pkg.camera_look_at(aspect=W / H, **kws[k % 3]) for k in range(3)] + pkg.orbit_cameras(16, aspect=W / H, eye0=(1.2, 1.4, 2.0))
    assert len(cams) == 19
    for vol in (None, dist):
        singles = [pkg.raymarch(rp, t0, t1, c, W, H, want_aux=True, want_depth=True, dist=vol) for c in cams]
        batch = pkg.raymarch(rp, t0, t1, cams, W, H, want_aux=True, want_depth=True, dist=vol)
        torch.cuda.synchronize()
        for k in range(3):
            assert torch.equal(batch[k].view(torch.int32), torch.cat([s[k] for s in singles]).view(torch.int32)), k
        assert int((batch[2][..., 0] == 1).sum()) > 19 * 300
        for cam, full in zip(cams[:3], singles[:3]):
            parts = [pkg.raymarch(rp, t0, t1, cam, W, H, y0=a, y1=b, want_aux=True, want_depth=True, dist=vol)
                     for a, b in ((0, 13), (13, 30), (30, 31), (31, H))]
            for k in range(3):
                assert torch.equal(torch.cat([p[k] for p in parts], dim=1).view(torch.int32), full[k].view(torch.int32)), k


@pytest.mark.parametrize("grid", ["cube32", "box16x32x64", "odd20x34x27"])
@pytest.mark.parametrize("field", ["steep", "crossing"])
def test_sharded_march_equals_single_gpu_march_over_fields(pkg, par, field, grid):
    """parallel.ShardedMarch, z-sharded over 3 "ranks" in lockstep on the one GPU: the merged image and every aux word
    test_gpu_sharded_march.py compares equal the single-GPU march's.  Normals: the slab kernel computes them only where the
    launcher's rule allows the clamping fetch for the taps, (1e-4 + h) * N / size <= 0.45 on every axis (march_plan.cpp: derive_raymarch_args); over
    odd20x34x27 the y axis gives 0.474, so there every normal stays zero -- asserted, so that a change of the rule shows."""
    from test_gpu_sharded_march import run_lockstep
    world = 3
    dims, lo, hi = MF.GRIDS[grid]
    full, f0, f1, _, _ = on_device(pkg, field, grid)
    rp = pkg.default_render_params(full)
    W, H = MF.IMAGE
    slabs, grids = [], []
    for r in range(world):
        slab = par.alloc_slab(dims, r, world, "cuda", fill_value=float("nan"))
        a, b = slab.z_begin - slab.ghost_lo, slab.z_end + slab.ghost_hi
        slab.tex0.copy_(f0[a:b])  # owned slices and the ghosts the halo exchange would bring
        slab.tex1.copy_(f1[a:b])
        slabs.append(slab)
        grids.append(pkg.make_grid(dims, lo, hi, slab.z_begin, slab.z_end))
    h = 1.0 / np.sqrt(float(sum(n * n for n in dims)))
    taps_clamp = all((1e-4 + h) * dims[a] / (hi[a] - lo[a]) <= 0.45 for a in range(3))
    assert taps_clamp == (grid != "odd20x34x27")
    handed_total = filled_total = 0
    for cam_kw in MF.cameras(field, grid):
        cam = pkg.camera_look_at(aspect=W / H, **cam_kw)
        want_rgba, want_aux = pkg.raymarch(rp, f0, f1, cam, W, H, want_aux=True)
        got_rgba, got_aux, handed = run_lockstep(pkg, par, rp, slabs, grids, cam, W, H)
        handed_total += handed
        np.testing.assert_array_equal(got_rgba.cpu().numpy().view(np.uint32), want_rgba[0].cpu().numpy().view(np.uint32))
        ga, wa = got_aux.cpu().numpy(), want_aux[0].cpu().numpy()
        np.testing.assert_array_equal(ga[..., :14], wa[..., :14])   # status, steps, hit_pos, t, raw0, raw1
        np.testing.assert_array_equal(ga[..., 17], wa[..., 17])     # depth
        filled = (ga[..., AUX_NORMAL] != 0).any(axis=-1)             # (normals: where the taps' slices are resident)
        np.testing.assert_array_equal(ga[..., AUX_NORMAL][filled], wa[..., AUX_NORMAL][filled])
        filled_total += int(filled.sum())
        if taps_clamp:
            assert filled.any() and ((wa[..., 0] == 1) & ~filled).sum() < (wa[..., 0] == 1).sum()
        assert (wa[..., 0] == 1).any() and (wa[..., 0] == -2).any()
    assert handed_total > 0  # rays did cross slab boundaries
    print(f"{field} {grid}: {handed_total} rays handed over, {filled_total} normals filled")
    assert (filled_total > 0) == taps_clamp
