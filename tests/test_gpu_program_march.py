"""GPU tests of the direct march of SDF programs (sdfv_program_raymarch): the device against the host mirror -- the same
per-pixel source compiled by g++ -- bit for bit on every field of the march record, rgba within the grid march's tolerance,
rgba8 and depth against what the record and rgba imply, row ranges and camera batches against single full calls, and a render
enqueued behind a fill of the same program on the same stream."""
import importlib

import numpy as np
import pytest
import torch

import program_march_ref as M

pytestmark = pytest.mark.gpu
RGBA_TOL = 1e-4            # tests/test_gpu_raymarch.py's tolerance for the grid march's rgba: pow() is the one inexact step


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


def compare(prog, cams, w, h, rp, what, threads=16, **kw):
    """device render == host mirror: aux and depth bitwise, rgba to RGBA_TOL.  Returns the device outputs as numpy arrays."""
    rgba, aux, depth = prog.render(cams, w, h, rp=rp, want_aux=True, want_depth=True, **kw)
    torch.cuda.synchronize()
    h_rgba, h_aux, h_depth = prog.render_host(cams, w, h, rp=rp, want_aux=True, want_depth=True, threads=threads, **kw)
    rgba, aux, depth = rgba.cpu().numpy(), aux.cpu().numpy(), depth.cpu().numpy()
    for i in range(len(h_aux)):
        M.assert_aux_bitwise(M.aux_view(aux[i]), M.aux_view(h_aux[i]), (what, i))
    assert (depth.view(np.uint32) == h_depth.view(np.uint32)).all(), what
    assert (depth.view(np.uint32) == M.aux_view(aux)["depth"].view(np.uint32)).all(), what
    err = float(np.abs(rgba - h_rgba).max())
    assert err <= RGBA_TOL, (what, err)
    return rgba, M.aux_view(aux), depth, err


def test_device_equals_host_mirror_bitwise(pkg, PM):
    worst, hits = 0.0, 0
    try:
        for policy in (0, 1):
            pkg.set_option(pkg._capi.OPT_EXT_SRGB_QUANT, policy)
            for name, b in M.builders(PM).items():
                prog, rp = b.build(), M.render_params(pkg, name)
                for size in M.SIZES:
                    for ci, cam in enumerate(M.cameras(pkg, name, *size)):
                        _, aux, _, err = compare(prog, cam, size[0], size[1], rp, (name, size, ci, policy))
                        worst = max(worst, err)
                        hits += int((aux["status"] == 1).sum())
    finally:
        pkg.set_option(pkg._capi.OPT_EXT_SRGB_QUANT, 0)
    print(f"device == host mirror bit for bit over {hits} hits; max |d rgba| = {worst:.2e}")
    assert hits > 100000


def test_full_hd_frames_on_every_pixel(pkg, PM):
    """1920 x 1080 of example_sixteen (a frame of misses: the model's closing plane leaves its value positive in the whole box) and
    of `deep`, compared on every pixel."""
    for name in ("sixteen", "deep"):
        prog, rp = M.builders(PM)[name].build(), M.render_params(pkg, name)
        cam = M.cameras(pkg, name, 1920, 1080)[0]
        _, aux, _, err = compare(prog, cam, 1920, 1080, rp, name)
        st = aux["status"]
        print(f"{name} 1080p: hits {int((st == 1).sum())}, -2 {int((st == -2).sum())}, off the box {int((st == 0).sum())}, "
              f"sum steps {int(aux['steps'].sum())}, max |d rgba| {err:.2e}")
        assert (st == -2).sum() > 100000 and (name == "sixteen" or (st == 1).sum() > 100000)


def test_rgba8_is_what_rgba_implies(pkg, PM):
    """`envelope`: 85 materials, so the frame holds many colours (counted, so that the comparison is not one of constants)."""
    prog, rp = M.builders(PM)["envelope"].build(), M.render_params(pkg, "envelope")
    cam = M.cameras(pkg, "envelope", 160, 120)[0]
    rgba = prog.render(cam, 160, 120, rp=rp).cpu().numpy()
    r8 = prog.render(cam, 160, 120, rp=rp, rgba8=True).cpu().numpy().view(np.uint32)
    want = np.rint(np.clip(rgba, 0.0, 1.0) * np.float32(255.0)).astype(np.uint32)
    assert (r8 == (want[..., 0] | want[..., 1] << 8 | want[..., 2] << 16 | want[..., 3] << 24)).all()
    assert len(np.unique(r8)) > 16


def test_row_ranges_and_camera_batches_equal_single_full_calls(pkg, PM):
    b = M.builders(PM)["deep"]
    prog, rp = b.build(), M.render_params(pkg, "deep")
    w, h = 160, 120
    cams = list(M.cameras(pkg, "deep", w, h)) + list(M.cameras(pkg, "all_ops", w, h))
    full = [[t.cpu().numpy() for t in prog.render(c, w, h, rp=rp, want_aux=True, want_depth=True)] for c in cams]
    for y0, y1 in ((0, 120), (7, 100), (64, 65), (113, 120)):
        rgba, aux, depth = [t.cpu().numpy() for t in prog.render(cams, w, h, rp=rp, want_aux=True, want_depth=True, y0=y0, y1=y1)]
        assert rgba.shape == (4, y1 - y0, w, 4)
        for i, (fr, fa, fd) in enumerate(full):
            assert (rgba[i].view(np.uint32) == fr[0, y0:y1].view(np.uint32)).all(), (y0, y1, i)
            assert (aux[i].view(np.uint32) == fa[0, y0:y1].view(np.uint32)).all(), (y0, y1, i)
            assert (depth[i].view(np.uint32) == fd[0, y0:y1].view(np.uint32)).all(), (y0, y1, i)
    # more cameras than one launch carries in its arguments
    many = (cams * 5)[:18]
    rgba = prog.render(many, w, h, rp=rp).cpu().numpy()
    for i in range(18):
        assert (rgba[i].view(np.uint32) == full[i % 4][0][0].view(np.uint32)).all(), i


def test_a_render_behind_a_fill_on_the_same_stream_leaves_both_intact(pkg, PM):
    b = M.builders(PM)["deep"]
    prog, rp = b.build(), M.render_params(pkg, "deep")
    cam = M.cameras(pkg, "deep", 320, 240)[0]
    g = pkg.make_grid((128, 128, 128))
    t0, t1 = pkg.alloc_textures(g)
    prog.fill_grid(g, t0, t1)
    alone_rgba, alone_aux = prog.render(cam, 320, 240, rp=rp, want_aux=True)
    torch.cuda.synchronize()
    want0, want1 = t0.clone(), t1.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t0.zero_()
        t1.zero_()
        prog.fill_grid(g, t0, t1, stream=s)
        rgba, aux = prog.render(cam, 320, 240, rp=rp, want_aux=True, stream=s)
        prog.fill_grid(g, t0, t1, stream=s)
    s.synchronize()
    assert torch.equal(t0.view(torch.int32), want0.view(torch.int32)) and torch.equal(t1.view(torch.int32), want1.view(torch.int32))
    assert torch.equal(aux.view(torch.int32), alone_aux.view(torch.int32)) and torch.equal(rgba.view(torch.int32), alone_rgba.view(torch.int32))
    assert (M.aux_view(aux.cpu().numpy())["status"] == 1).sum() > 1000


def test_both_routes_cover_the_same_pixels(pkg, PM):
    """The grid march (sdfv_raymarch_ex over a 16^3 fill of `single`) and the direct march of the same program, same render
    parameters, 40 x 36 (the right and bottom tiles have lanes beyond the image): aux.status == 0 -- the pixel's ray is off
    the box -- on exactly the same pixels.  Cameras: the scene's orbit camera and one that looks past the box, which puts it
    across the image's right and bottom edges (the outside pair: each has pixels on the box and off it), and the scene's
    camera inside the box, where every ray leaves through a face: no pixel of it is off the box, in either route."""
    w, h = 40, 36
    lo, hi = M.SCENES["single"][:2]
    g = pkg.make_grid((16, 16, 16), lo, hi)
    rp = pkg.default_render_params(g)
    prog = M.builders(PM)["single"].build()
    t0, t1 = pkg.alloc_textures(g)
    prog.fill_grid(g, t0, t1)
    orbit, inside = M.cameras(pkg, "single", w, h)
    past = pkg.camera_look_at(eye=M.CLOSE, target=(-1.0, 0.9, 0.0), aspect=w / h)
    cams = [orbit, past, inside]
    _, grid_aux = pkg.raymarch(rp, t0, t1, cams, w, h, want_aux=True)
    _, prog_aux = prog.render(cams, w, h, rp=rp, want_aux=True)
    torch.cuda.synchronize()
    off_grid = M.aux_view(grid_aux.cpu().numpy())["status"] == 0
    off_prog = M.aux_view(prog_aux.cpu().numpy())["status"] == 0
    assert off_grid.shape == (3, h, w) and (off_grid == off_prog).all(), np.argwhere(off_grid != off_prog)[:4].tolist()
    for i in (0, 1):
        assert 0 < off_grid[i].sum() < w * h, (i, int(off_grid[i].sum()))
    assert not off_grid[2].any()
