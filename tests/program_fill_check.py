"""Shared by tests/test_gpu_program.py and tests/test_gpu_program_fuzz.py: the dense program fill held, bit for bit, to
sdfv_pack_samples fed the numpy restatement's records (tests/program_ref.py) at every voxel -- with no volume, the plain and the
interleaved one, every non-temporal setting, whole grids and slabs, per Srgba::from policy."""
import numpy as np
import pytest
import torch

import program_ref as R


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    print(f"{what}: {bad.size} of {got.size} words differ")
    assert bad.size == 0, (what, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


def voxel_positions(dims, bb_min, bb_max):
    """idx / (dim - 1) * size + min, three roundings (scene/sdf/mod.rs:179-182), x fastest: [D * H * W, 3]"""
    axes = []
    for a in range(3):
        i = np.arange(dims[a], dtype=np.float32)
        axes.append(((i / (np.float32(dims[a]) - np.float32(1))) * (np.float32(bb_max[a]) - np.float32(bb_min[a]))) + np.float32(bb_min[a]))
    zz, yy, xx = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([xx, yy, zz], axis=-1).reshape(-1, 3).astype(np.float32)


def interleave(vol):
    """texture-order volume [D, H, W], a numpy array or a torch tensor -> the y-interleaved layout as a flat contiguous one: entry
    ((row >> 1) * W + x) * 2 + (row & 1), row = z * H + y.  The one restatement of the layout for every test."""
    D, H, W = vol.shape
    assert H % 2 == 0
    return vol.reshape(D * H // 2, 2, W).swapaxes(1, 2).reshape(-1)


def expected_textures(pkg, grid, dims, samples, srgb, layout):
    """What sdfv_pack_samples leaves on an sdfv_grid_init-ed grid when fed `samples` (numpy [n, 7]) at every voxel."""
    t0, t1 = pkg.alloc_textures(grid)
    pkg.grid_init(grid, t0, t1)
    n = dims[0] * dims[1] * dims[2]
    vol = None if layout is None else torch.full((n,), float(pkg.AIR_DIST), device="cuda")
    with pkg.options({pkg._capi.OPT_EXT_SRGB_QUANT: srgb}):
        pkg.pack_samples(grid, torch.from_numpy(samples).cuda(), t0, t1, dist=vol,
                         flags=pkg._capi.PASS_VOLUME_INTERLEAVED if layout == "ilv" else 0)
    torch.cuda.synchronize()
    return t0.cpu().numpy(), t1.cpu().numpy(), None if vol is None else vol.cpu().numpy()


def fill_equals_packing(pkg, PM, dims, bb_min, bb_max, names, builders=None, srgbs=(0, 1)):
    """builders: name -> Program builder (default: program_ref.catalogue); srgbs: the Srgba::from policies compared."""
    K = pkg._capi
    W, H, D = dims
    grid = pkg.make_grid(dims, bb_min, bb_max)
    pos = voxel_positions(dims, bb_min, bb_max)
    builders = R.catalogue(PM) if builders is None else builders
    for name in names:
        builder = builders[name]
        prog = builder.build()
        samples = R.run(builder.ops, pos)
        # the stress programs do stress, on the reference, before anything is compared (W = 256: the tx256 kernels and, with the
        # interleaved volume, tx128; W = 64: tx64)
        if name == "envelope" and dims in (R.ROW_GRID[0], R.ENVELOPE_GRID_64):
            R.assert_envelope_stresses(builder.ops, pos, W, distinct=min(W, R.ENVELOPE_PLANES))
        if name == "late_material" and dims == R.ROW_GRID[0]:
            R.assert_late_material_stresses(builder.ops, pos, W)
        for srgb in srgbs:
            want = {}
            for layout in (None, "plain") + (("ilv",) if H % 2 == 0 else ()):
                want[layout] = expected_textures(pkg, grid, dims, samples, srgb, layout)
            same_bits(want["plain"][2].reshape(D, H, W), want["plain"][0][..., 0], "the packed volume is tex0.r")
            if H % 2 == 0:
                same_bits(want["ilv"][2], interleave(want["plain"][2].reshape(D, H, W)), "the packed interleaved volume")
            for layout in want:
                for nt in (0, 1, 2):
                    for slabs in (1, 2):
                        t0, t1 = pkg.alloc_textures(grid)
                        t0.fill_(-7.0), t1.fill_(-7.0)
                        vol = None if layout is None else torch.full((D, H, W), -7.0, device="cuda")
                        flags = K.PASS_VOLUME_INTERLEAVED if layout == "ilv" else 0
                        with pkg.options({K.OPT_EXT_SRGB_QUANT: srgb, K.OPT_FILL_NONTEMPORAL: nt}):
                            cuts = [0, D] if slabs == 1 else [0, D // 2, D]
                            for z0, z1 in zip(cuts[:-1], cuts[1:]):
                                g = pkg.make_grid(dims, bb_min, bb_max, z_begin=z0, z_end=z1)
                                prog.fill_grid(g, t0[z0:z1], t1[z0:z1], dist=None if vol is None else vol[z0:z1], flags=flags)
                        torch.cuda.synchronize()
                        what = f"{dims} {name} srgb={srgb} volume={layout} nt={nt} slabs={slabs}"
                        same_bits(t0.cpu().numpy(), want[layout][0], what + " tex0")
                        same_bits(t1.cpu().numpy(), want[layout][1], what + " tex1")
                        if vol is not None:
                            same_bits(vol.cpu().numpy().reshape(-1), want[layout][2], what + " volume")
            if H % 2:  # the interleaved volume pairs rows: an odd height is an argument error, as for the demo's fill
                t0, t1 = pkg.alloc_textures(grid)
                vol = torch.empty((D, H, W), device="cuda")
                with pytest.raises(pkg.SdfvError, match="must be even"):
                    prog.fill_grid(grid, t0, t1, dist=vol, flags=K.PASS_VOLUME_INTERLEAVED)
    assert float(want[None][1][..., 3].min()) == float(want[None][1][..., 3].max()) == float(np.float32(pkg.AIR_DIST))
