"""Containment of sdfv_slab_fill_step[_commit] (tests/arena.py): the slab's textures -- lower ghost, owned slices, upper ghost(s)
-- and its distance volume are carved from one arena, and a loopback communicator (world 1, periodic: the rank exchanges with
itself) runs every form of the step.  The owned slices must be the oracle's, the ghosts the wrap, and nothing beside the
allocation may change: the plain dense launch, the boundary-first ordered launch (whole, and split between the two streams)
and the copies into the ghosts all address the slab through slice offsets.  (The RCCL transfer itself is not under test.)"""
import functools
import importlib

import numpy as np
import pytest

import arena as A

pytestmark = pytest.mark.gpu
FORMS = ["auto", "side_boundary", "side_boundary_event", "side_boundary_unpacked", "side_boundary_unpacked_event"]

# The smallest slabs tests/test_gpu_slab_comm.py uses for each path: (33, 7, *) rows that fill no workgroup -> fill, then
# exchange; (128, 8, 10) and (256, 4, 7) the row-chunk form of the boundary-first order (W % chunk == 0, H % ty == 0, more than
# two slices); (48, 16, 12) its flat form (a slice is a whole number of workgroups)
CASES = [((33, 7, 9), 0, 2, 1), ((33, 7, 9), 4, 5, 1), ((128, 8, 10), 2, 9, 2), ((256, 4, 7), 0, 7, 1), ((48, 16, 12), 3, 12, 2)]


@pytest.fixture(scope="module")
def par(pkg):
    return importlib.import_module("sdf-viewer_amd.parallel")


@functools.lru_cache(maxsize=None)
def wrapped(dims, z0, z1, halo):
    """[ghost_lo = the last owned slice][owned, the oracle's][ghost_hi = the first `halo` owned slices], both textures."""
    import oracle_binding as oracle
    r0, r1 = oracle.fill_dense(oracle.default_params(), dims, z0=z0, z1=z1)
    idx = [z1 - z0 - 1] + list(range(z1 - z0)) + [k % (z1 - z0) for k in range(halo)]
    w0, w1 = np.ascontiguousarray(r0[idx]), np.ascontiguousarray(r1[idx])
    w0.setflags(write=False), w1.setflags(write=False)
    return w0, w1


@pytest.mark.parametrize("commit", [False, True], ids=["step", "step_commit"])
@pytest.mark.parametrize("dims,z0,z1,halo", CASES)
def test_fill_step_writes_its_slab_and_ghosts_only(pkg, par, dims, z0, z1, halo, commit):
    K = pkg._capi
    if z1 - z0 < halo:
        halo = 1
    w0, w1 = wrapped(dims, z0, z1, halo)
    dist = np.ascontiguousarray(w0[..., 0])
    arrays = [w0, w1] + ([dist] if commit else [])
    band = A.band_for(*arrays)
    ar = A.Arena(A.arena_bytes(band, *arrays), band=band)
    slab = par.SlabTextures(ar.output(w0.shape, align=16, name="tex0"), ar.output(w1.shape, align=16, name="tex1"), z0, z1, 1, halo, halo)
    vol = ar.output(dist.shape, align=4, name="dist") if commit else None
    expected = {"tex0": w0, "tex1": w1}
    if commit:
        expected["dist"] = dist
    prm = pkg.default_params()
    grid = pkg.make_grid(dims, z_begin=z0, z_end=z1)
    forms = {"auto": 0, "side_boundary": K.STEP_SIDE_BOUNDARY, "side_boundary_event": K.STEP_SIDE_BOUNDARY | K.STEP_START_EVENT,
             "side_boundary_unpacked": K.STEP_SIDE_BOUNDARY | K.STEP_UNPACKED,
             "side_boundary_unpacked_event": K.STEP_SIDE_BOUNDARY | K.STEP_UNPACKED | K.STEP_START_EVENT}
    comm = par.SlabComm(pkg, 0, 1, periodic=True, halo_hi=halo)
    try:
        for form in FORMS:
            with pkg.options({K.OPT_SLAB_STEP_FORM: forms[form]}):
                try:
                    ar.twin(lambda: comm.fill_step(prm, grid, slab, dist=vol), expected, kinds=("canary", "nan"))
                except A.ArenaError as e:
                    raise A.ArenaError(f"step form {form!r}:\n{e}") from None
    finally:
        comm.close()


@pytest.mark.parametrize("channels", [4, 1, 18])
@pytest.mark.parametrize("band_height", [16, 8])
def test_bands_scatter_writes_its_bands_rows_only(pkg, band_height, channels):
    """sdfv_bands_scatter moves band set (1, 3) of two 33 x 90 images to its rows of the whole images: bands 1 and 4 of 16 rows,
    bands 1, 4, 7 and 10 of 8 rows (the short last band of either height belongs to another set).  Every other row of `out` is
    another rank's and must keep what it holds.  4 channels take the 16-byte path, 1 and 18 the scalar one (33 is odd)."""
    import ctypes as C
    import torch
    n_cam, width, height, first, step = 2, 33, 90, 1, 3
    rows = np.concatenate([np.arange(b * band_height, min((b + 1) * band_height, height))
                           for b in range(first, -(-height // band_height), step)])
    assert len(rows) == pkg.lib.sdfv_band_rows_ex(height, first, step, band_height)
    rng = np.random.default_rng(channels * band_height)
    part = rng.uniform(0.0, 1.0, (n_cam, len(rows), width, channels)).astype(np.float32)
    want = np.zeros((n_cam, height, width, channels), np.float32)
    want[:, rows] = part
    written = np.zeros(want.shape, bool)
    written[:, rows] = True
    arrays = [part, want]
    band = A.band_for(*arrays)
    ar = A.Arena(A.arena_bytes(band, *arrays), band=band)
    src = ar.input(part, align=4 if channels != 4 else 16, name="part")
    out = ar.output(want.shape, align=4 if channels != 4 else 16, name="out")
    ar.twin(lambda: pkg.check(pkg.lib.sdfv_bands_scatter(C.c_void_p(src.data_ptr()), first, step, band_height, n_cam, width, height,
                                                         channels, C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))),
            {"out": A.Untouched(want, written)}, kinds=("canary", "nan"))
