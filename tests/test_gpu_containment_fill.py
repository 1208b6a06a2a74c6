"""Containment of the dense fill and its fused volumes (tests/arena.py): every store form of sdfv_fill_grid_commit and of the
step-1 virgin pass that is the fused interleaved fill, each reached by SDFV_OPT_FILL_FORM or by a width the launcher's rule
(launch_fill_dense, csrc/fill_kernels.hip) provably maps to it, over whole grids and over the middle z-slab of a grid whose
other slabs already hold the oracle's texels.  Expected texels are oracle.fill_dense's; poison canary and NaN."""
import functools

import numpy as np
import pytest

import arena as A
from program_fill_check import interleave

pytestmark = pytest.mark.gpu
AUTO, ROWS, FLAT, PAIRED, PAIRROWS = 0, 1, 2, 3, 4  # SDFV_OPT_FILL_FORM

# (kernel, dims, SDFV_OPT_FILL_FORM, volumes).  The launcher's rule, for the comments below: with an interleaved volume the
# form is ilv_paired when forced (3), pairrows when forced (4), else the row-chunk kernel <64> for W <= 64 and <128> above;
# otherwise chunk = 64 / 128 / 256 for W <= 64 / <= 128 / above, and the row-chunk kernel <chunk> runs when W % chunk == 0 or
# form 1 forces it, the flat kernel when form 2 forces it.
DENSE = [
    # <64> stores 4 rows per workgroup: H = 6 leaves the last workgroup of each slice (and of the slab) half empty
    ("rows64", (40, 6, 3), ROWS, (None, "plain", "ilv")),    # W % 64 != 0: forced; lanes 40..63 of every row idle
    ("rows64", (64, 6, 3), AUTO, (None, "plain", "ilv")),    # W % 64 == 0: the launcher's own choice
    # <128> stores 2 rows per workgroup: H = 5 leaves the last one half empty
    ("rows128", (128, 5, 3), AUTO, (None, "plain")),         # W % 128 == 0 (H odd: no interleaved volume)
    ("rows128", (100, 6, 3), AUTO, ("ilv",)),                # 64 < W, interleaved volume: <128> whatever the width
    ("rows128", (100, 6, 3), ROWS, (None, "plain")),
    ("rows256", (256, 3, 2), AUTO, (None, "plain")),         # W % 256 == 0
    ("flat", (33, 5, 7), FLAT, (None, "plain")),             # n_vox = 1155, 4 full workgroups + 131 voxels
    ("flat", (300, 4, 3), FLAT, (None, "plain")),
    ("flat", (1, 9, 4), FLAT, (None, "plain")),              # W = 1: the magic division is not taken
    ("flat", (257, 3, 5), FLAT, (None, "plain")),
    # no bounds test in either ("W is a multiple of kBlock"); ilv_paired pads its grid to groups of 16 workgroups:
    # (256, 6, 3) gives 9 units of two rows -> 32 workgroups, 14 of them padding
    ("pairrows", (256, 2, 1), PAIRROWS, ("ilv",)),
    ("pairrows", (256, 6, 3), PAIRROWS, ("ilv",)),
    ("pairrows", (512, 2, 2), PAIRROWS, ("ilv",)),
    ("ilv_paired", (256, 2, 1), PAIRED, ("ilv",)),
    ("ilv_paired", (256, 6, 3), PAIRED, ("ilv",)),
    ("ilv_paired", (512, 2, 2), PAIRED, ("ilv",)),
]


@functools.lru_cache(maxsize=None)
def oracle_grid(dims):
    """(tex0, tex1, dist, ilv or None) of the whole grid, read-only, shared."""
    import oracle_binding as oracle
    r0, r1 = oracle.fill_dense(oracle.default_params(), dims)
    dist = np.ascontiguousarray(r0[..., 0])
    ilv = interleave(dist).reshape(dist.shape) if dims[1] % 2 == 0 else None
    for a in (r0, r1, dist, ilv):
        if a is not None:
            a.setflags(write=False)
    return r0, r1, dist, ilv


def not_yet(a, z0, z1):
    """The grid before slab [z0, z1) is filled: the other slabs hold `a`, this one the complement of every expected bit, so
    that a store that is skipped, and one that lands a row or a slice off, both show."""
    b = a.copy()
    b[z0:z1].view(np.uint32)[...] ^= np.uint32(0xFFFFFFFF)
    return b


# every case as a whole grid and as the middle slab z in [D // 3, 2 * D // 3) -- which a grid of one slice does not have
RUNS = [(k, d, f, v, slab) for k, d, f, v in DENSE for slab in ("whole", "middle") if slab == "whole" or d[2] // 3 < 2 * d[2] // 3]


@pytest.mark.parametrize("kernel,dims,form,volumes,slab", RUNS, ids=[f"{k}-{'x'.join(map(str, d))}-form{f}-{s}" for k, d, f, _, s in RUNS])
def test_dense_fill_stays_inside_its_textures_and_volume(pkg, kernel, dims, form, volumes, slab):
    K = pkg._capi
    W, H, D = dims
    z0, z1 = (0, D) if slab == "whole" else (D // 3, 2 * D // 3)
    assert z0 < z1
    r0, r1, dist, ilv = oracle_grid(dims)
    prm = pkg.default_params()
    g = pkg.make_grid(dims, z_begin=z0, z_end=z1)
    for volume in volumes:
        want_vol = {None: None, "plain": dist, "ilv": ilv}[volume]
        arrays = [r0, r1] + ([] if want_vol is None else [want_vol])
        band = A.band_for(*arrays)
        ar = A.Arena(A.arena_bytes(band, *arrays), band=band)
        if slab == "whole":
            t0 = ar.output(r0.shape, r0.dtype, align=16, name="tex0")   # "DEVICE pointers, 16-byte aligned"
            t1 = ar.output(r1.shape, r1.dtype, align=16, name="tex1")
            # the plain volume: one float per voxel, 4; the interleaved one: "H even, 8-byte aligned"
            vol = None if want_vol is None else ar.output(want_vol.shape, want_vol.dtype, align=8 if volume == "ilv" else 4, name="vol")
        else:
            t0 = ar.inout(not_yet(r0, z0, z1), align=16, name="tex0")
            t1 = ar.inout(not_yet(r1, z0, z1), align=16, name="tex1")
            vol = None if want_vol is None else ar.inout(not_yet(want_vol, z0, z1), align=8 if volume == "ilv" else 4, name="vol")
        expected = {"tex0": r0, "tex1": r1}
        if vol is not None:
            expected["vol"] = want_vol

        def run():
            if volume == "ilv":  # the fused interleaved fill IS the step-1 pass over a virgin grid (include/sdfgrid.h)
                pkg.fill_grid_pass(prm, g, 1, t0[z0:z1], t1[z0:z1], dist=vol[z0:z1], flags=K.PASS_VIRGIN_GRID | K.PASS_VOLUME_INTERLEAVED)
            else:
                pkg.fill_grid(prm, g, t0[z0:z1], t1[z0:z1], dist=None if vol is None else vol[z0:z1])
        for nt in (1, 2):  # nontemporal and plain stores: separate instantiations of every kernel
            with pkg.options({K.OPT_FILL_FORM: form, K.OPT_FILL_NONTEMPORAL: nt}):
                ar.twin(run, expected, kinds=("canary", "nan"))
