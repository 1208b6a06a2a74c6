"""Containment of the SDF-program routes that write a caller's buffers (tests/arena.py): the dense program fill over the width
classes of its launcher, sdfv_program_grid_pass (box launch and scan, cached and nontemporal loads) with an edit box that
touches the grid's last voxel, and the direct march.  Expected values are the numpy restatements': program_ref.run for the
records, program_march_ref.pack for the texel pair, program_pass_ref for what a pass may touch, program_march_ref.march for
the pixels.  (The point-list entry points of programs are in tests/test_gpu_containment_points.py.)"""
import functools
import importlib

import numpy as np
import pytest

import arena as A
import program_march_ref as M
import program_pass_ref as P
import program_ref as R
from program_fill_check import interleave

pytestmark = pytest.mark.gpu
F = np.float32
BB = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


@functools.lru_cache(maxsize=None)
def dense(name, dims):
    """(tex0, tex1) [D, H, W, 4] of the dense fill of a catalogue program over BB: the restated records, packed.  Shared."""
    pkg = importlib.import_module("sdf-viewer_amd")
    PM = importlib.import_module("sdf-viewer_amd.program")
    W, H, D = dims
    rec = R.run(R.catalogue(PM)[name].ops, R.grid_positions(dims, *BB).reshape(-1, 3))
    assert np.isfinite(rec).all()
    t0, t1 = M.pack(rec, M.srgb_table(), F(pkg.AIR_DIST), False)
    t0, t1 = np.ascontiguousarray(t0.reshape(D, H, W, 4)), np.ascontiguousarray(t1.reshape(D, H, W, 4))
    t0.setflags(write=False), t1.setflags(write=False)
    return t0, t1


def layout(vol, kind):
    return interleave(vol).reshape(vol.shape) if kind == "ilv" else np.ascontiguousarray(vol)


def not_yet(a, z0, z1):
    """The other slabs filled, this one holding the complement of every expected bit (tests/test_gpu_containment_fill.py)."""
    b = a.copy()
    b[z0:z1].view(np.uint32)[...] ^= np.uint32(0xFFFFFFFF)
    return b


# launch_program_fill (csrc/program_kernels.hip): always the row-chunk form, tx = 64 for W <= 64, 128 for W <= 128 or with the
# interleaved volume, else 256; rows of any width (the last chunk of a row is partly idle), ty = 256 / tx rows per workgroup.
FILL_DIMS = [(40, 6, 3),    # tx 64, 4 rows per workgroup, H % 4 == 2
             (128, 5, 3),   # tx 128, H odd: the last workgroup of the slab is half empty
             (100, 6, 3),   # tx 128, a partly idle chunk
             (256, 3, 2),   # tx 256
             (257, 3, 5),   # tx 256, two chunks per row, the second one texel wide
             (300, 4, 3),   # tx 256 -- and tx 128 with the interleaved volume: three chunks
             (64, 6, 3)]    # tx 64, full chunks (a one-texel axis has the position 0 / 0, whose NaN payload is open: not here)


@pytest.mark.parametrize("slab", ["whole", "middle"])
@pytest.mark.parametrize("name", ["all_ops", "late_material"])
@pytest.mark.parametrize("dims", FILL_DIMS, ids=["x".join(map(str, d)) for d in FILL_DIMS])
def test_program_fill(pkg, PM, dims, name, slab):
    K = pkg._capi
    W, H, D = dims
    z0, z1 = (0, D) if slab == "whole" else (D // 3, 2 * D // 3)
    r0, r1 = dense(name, dims)
    prog = R.catalogue(PM)[name].build()
    g = pkg.make_grid(dims, *BB, z_begin=z0, z_end=z1)
    for volume in (None, "plain") + (("ilv",) if H % 2 == 0 else ()):
        want_vol = None if volume is None else layout(r0[..., 0], volume)
        arrays = [r0, r1] + ([] if want_vol is None else [want_vol])
        band = A.band_for(*arrays)
        ar = A.Arena(A.arena_bytes(band, *arrays), band=band)
        carve = (lambda a, **kw: ar.output(a.shape, a.dtype, **kw)) if slab == "whole" else (lambda a, **kw: ar.inout(not_yet(a, z0, z1), **kw))
        t0, t1 = carve(r0, align=16, name="tex0"), carve(r1, align=16, name="tex1")
        vol = None if want_vol is None else carve(want_vol, align=8 if volume == "ilv" else 4, name="vol")
        expected = {"tex0": r0, "tex1": r1}
        if vol is not None:
            expected["vol"] = want_vol
        for nt in (1, 2):
            with pkg.options({K.OPT_FILL_NONTEMPORAL: nt}):
                ar.twin(lambda: prog.fill_grid(g, t0[z0:z1], t1[z0:z1], dist=None if vol is None else vol[z0:z1],
                                               flags=K.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0), expected, kinds=("canary", "nan"))


@pytest.mark.parametrize("loads", [1, 2], ids=["scan", "scan_nt"])  # SDFV_OPT_PASS_LOADS: sdfprog_pass_scan / sdfprog_pass_scan_nt
@pytest.mark.parametrize("dims", [(24, 18, 20), (21, 17, 11)])
def test_program_grid_pass(pkg, PM, dims, loads):
    """A grid loaded with all_ops in its lower half and new_voxels' state above, then one pass of late_material with an edit box
    whose upper corner is the grid's last voxel: the box launch covers the box's lattice points up to the last one, the scan
    everything else, refilling what holds AIR_DIST."""
    K = pkg._capi
    W, H, D = dims
    air = F(pkg.AIR_DIST)
    old, new = dense("all_ops", dims), dense("late_material", dims)
    upper = (np.arange(D) >= D // 2)[:, None, None, None]
    before = tuple(np.ascontiguousarray(np.where(upper, air, t)) for t in old)
    cx, cy, cz = P.axis_coords(dims, *BB)
    box = (float(cx[W // 2]), float(cy[H // 3]), float(cz[D // 4]), float(cx[W - 1]), float(cy[H - 1]), float(cz[D - 1]))
    prog = R.catalogue(PM)["late_material"].build()
    g = pkg.make_grid(dims, *BB)
    for step in (1, 2, 4):
        mask = P.update_mask(dims, *BB, step, before[0][..., 0], box, air)
        assert mask[D - 1, H - 1, W - 1] == ((W - 1) % step == 0 and (H - 1) % step == 0 and (D - 1) % step == 0)
        assert mask.any() and not mask.all()
        for volume in (None, "plain") + (("ilv",) if H % 2 == 0 else ()):
            want0, want1, want_vol = P.expected(before, new, mask, air, volume)
            arrays = [want0, want1] + ([] if volume is None else [want_vol])
            ar = A.Arena(A.arena_bytes(A.band_for(*arrays), *arrays), band=A.band_for(*arrays))
            t0, t1 = ar.inout(before[0], align=16, name="tex0"), ar.inout(before[1], align=16, name="tex1")
            expected = {"tex0": want0, "tex1": want1}
            vol = None
            if volume is not None:
                vol = ar.inout(layout(before[0][..., 0], volume), align=8 if volume == "ilv" else 4, name="vol")
                expected["vol"] = layout(want_vol, volume)
            with pkg.options({K.OPT_PASS_LOADS: loads}):
                ar.twin(lambda: prog.grid_pass(g, step, t0, t1, dist=vol, changed_box=box,
                                               flags=K.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0), expected, kinds=("canary", "air"))


@pytest.mark.parametrize("n_cam", [1, 17])
def test_program_raymarch(pkg, PM, n_cam):
    """sdfv_program_raymarch, rows [3, 14) of 33 x 17 images: one camera, and 17 (more than the 16 a launch carries as
    arguments).  The aux record and the depth plane bit for bit, the shaded colour to 1e-4 (include/sdfgrid.h)."""
    name, width, height, y0, y1 = "all_ops", 33, 17, 3, 14
    builder = M.builders(PM)[name]
    prog = builder.build()
    rp = M.render_params(pkg, name)
    pair = M.cameras(pkg, name, width, height)
    views = [M.march(builder.ops, rp, cam, width, height, air_dist=pkg.AIR_DIST, y0=y0, y1=y1) for cam in pair]
    assert all((aux["status"] == 1).any() for aux, _ in views)
    order = [k % 2 for k in range(n_cam)]
    want_aux = np.stack([views[k][0] for k in order])
    want_rgba = np.stack([views[k][1] for k in order])
    shape = (n_cam, y1 - y0, width)
    arrays = [(shape + (4,), np.float32), (shape + (18,), np.float32), (shape, np.float32)]
    band = A.band_for(*arrays)
    ar = A.Arena(A.arena_bytes(band, *arrays), band=band)
    rgba = ar.output(shape + (4,), align=16, name="rgba")
    aux = ar.output(shape + (18,), align=4, name="aux")
    depth = ar.output(shape, align=4, name="depth")
    normal_words = np.zeros(18, bool)
    normal_words[14:17] = True  # sdfv_march_aux.normal: 0 / 0 of a zero tap sum
    expected = {"rgba": A.Approx(want_rgba, 1e-4), "depth": np.ascontiguousarray(want_aux["depth"]),
                "aux": A.Untouched(np.ascontiguousarray(want_aux).view(np.float32).reshape(shape + (18,)), nan_open=normal_words)}
    ar.twin(lambda: prog.render([pair[k] for k in order], width, height, rp=rp, y0=y0, y1=y1, out=rgba, aux_out=aux, depth_out=depth),
            expected, kinds=("canary", "nan"))
