"""Containment of the LoadingManager passes and of the kernels around them (tests/arena.py): grid states part-way through a load,
taken from the oracle's viewer_update and uploaded, then ONE pass on the device, in place, inside an arena.  The volume a pass
decides on lies next to guard words that hold the canary in one run and AIR_DIST in the other: a 16-byte load one row too far
would see "needs a sample" there and refill other voxels.  Each pass kernel is reached by flags, step, width and the volume's
alignment through the rule of launch_fill_pass (csrc/fill_kernels.hip), stated beside each case."""
import functools

import numpy as np
import pytest

import arena as A
from program_fill_check import interleave

pytestmark = pytest.mark.gpu
KINDS = ("canary", "air")
STEPS = (4, 2, 1)  # oracle.lm_new(dims, 3)


@functools.lru_cache(maxsize=None)
def load_states(dims, edit=False, box=None):
    """{steps done so far: (tex0, tex1)} of a load of the default demo by the oracle's loop: () is new_voxels' state, (4,) the
    state after the first pass, ... -- with edit=True the passes run with other parameters and `box` as the changed box over
    the LOADED grid instead.  Read-only, shared."""
    import oracle_binding as oracle
    prm = oracle.default_params(sphere_radius=0.8, cube_material=1) if edit else oracle.default_params()
    if edit:
        r0, r1 = (a.copy() for a in load_states(dims)[STEPS])
    else:
        r0, r1 = oracle.grid_init(dims)
    lm = oracle.lm_new(dims, len(STEPS))
    states = {(): (r0.copy(), r1.copy())}
    for k, step in enumerate(STEPS):
        n = -(-dims[0] // step) * -(-dims[1] // step) * -(-dims[2] // step)
        assert oracle.viewer_update(prm, dims, lm, r0, r1, changed_box=box, max_iterations=n) == n
        states[STEPS[:k + 1]] = (r0.copy(), r1.copy())
    for a, b in states.values():
        a.setflags(write=False), b.setflags(write=False)
    return states


def voxel_box(dims, lo_idx, hi_idx):
    """A changed box whose faces lie exactly on voxel coordinates (idx / (dim - 1) * size + min, three roundings, over [-1, 1])."""
    def coord(i, n):
        return float(np.float32(np.float32(np.float32(i) / np.float32(n - 1)) * np.float32(2.0)) + np.float32(-1.0))
    return tuple(coord(i, n) for i, n in zip(lo_idx, dims)) + tuple(coord(i, n) for i, n in zip(hi_idx, dims))


WHOLE_BOX = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)  # contains every voxel: the launcher finds that itself and reads nothing


def layout(vol, kind):
    return interleave(vol).reshape(vol.shape) if kind == "ilv" else np.ascontiguousarray(vol)


def run_pass(pkg, dims, before, after, step, *, volume=None, vol_align=16, flags=0, box=None, edit=False, slab=None, options=None):
    """One pass with `step` over the state `before` (in place, in an arena), held to `after`; slab = (z0, z1): the pass runs
    over those slices only, in the middle of the whole grid's arrays, and nothing else of them may change."""
    K = pkg._capi
    z0, z1 = slab or (0, dims[2])
    want0, want1 = before[0].copy(), before[1].copy()
    want0[z0:z1], want1[z0:z1] = after[0][z0:z1], after[1][z0:z1]
    arrays = [want0, want1] + ([] if volume is None else [want0[..., 0]])
    band = A.band_for(*arrays)
    ar = A.Arena(A.arena_bytes(band, *arrays), band=band)
    t0, t1 = ar.inout(before[0], align=16, name="tex0"), ar.inout(before[1], align=16, name="tex1")
    expected = {"tex0": want0, "tex1": want1}
    vol = None
    if volume is not None:
        vol = ar.inout(layout(before[0][..., 0], volume), align=vol_align, name="vol")
        expected["vol"] = layout(want0[..., 0], volume)
    prm = pkg.default_params(sphere_radius=0.8, cube_material=1) if edit else pkg.default_params()
    g = pkg.make_grid(dims, z_begin=z0, z_end=z1)
    fl = flags | (K.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0)
    with pkg.options(options or {}):
        ar.twin(lambda: pkg.fill_grid_pass(prm, g, step, t0[z0:z1], t1[z0:z1], changed_box=box, dist=None if vol is None else vol[z0:z1],
                                           flags=fl), expected, kinds=KINDS)


def boxes_for(dims):
    W, H, D = dims
    return [None, voxel_box(dims, (W // 4, H // 3, D // 4), (W - 2, H - 1, D // 2)), WHOLE_BOX]


@pytest.mark.parametrize("step", STEPS)
def test_per_voxel_pass(pkg, step):
    """fill_pass_kernel: no volume, so no 16-byte loads of one (vol16 false), nothing known, any step."""
    dims = (21, 18, 13)
    done = STEPS[:STEPS.index(step)]
    for box in boxes_for(dims):
        if box is None:
            s = load_states(dims)
            run_pass(pkg, dims, s[done], s[done + (step,)], step)
        else:  # an edit over the loaded grid; the whole box at steps 4 and 2 is the store-only rows form, not fresh
            s = load_states(dims, True, box)
            run_pass(pkg, dims, s[done], s[done + (step,)], step, box=box, edit=True)


@pytest.mark.parametrize("volume", ["plain", "ilv"])
@pytest.mark.parametrize("dims", [(20, 6, 5), (40, 12, 7)])  # W % 4 == 0; 600 and 3360 voxels: no multiple of 256
def test_step_1_quad_pass_and_its_fallback(pkg, dims, volume):
    """fill_pass_quad_kernel: step 1 over a volume at a 16-byte boundary (vol16); at an address that is 8-byte aligned only the
    launcher must take the per-voxel kernel over the volume instead, not misread."""
    done = STEPS[:2]
    for vol_align in (16, 8):
        for box in boxes_for(dims):
            s = load_states(dims) if box is None else load_states(dims, True, box)
            run_pass(pkg, dims, s[done], s[STEPS], 1, volume=volume, vol_align=vol_align, box=box, edit=box is not None)


@pytest.mark.parametrize("volume", [None, "plain", "ilv"])
def test_whole_rows_passes_of_a_flagged_load(pkg, volume):
    """fill_pass_rows_kernel<fresh> and <not fresh>: the caller's flags make every visited voxel required (all_required), steps
    2..8 then store the visited rows whole -- re-storing the texels between lattice points."""
    K = pkg._capi
    dims = (37, 20, 29)
    s = load_states(dims)
    run_pass(pkg, dims, s[()], s[(4,)], 4, volume=volume, vol_align=8, flags=K.PASS_FRESH_GRID | K.PASS_SAME_LOAD)
    run_pass(pkg, dims, s[()], s[(4, 2)], 2, volume=volume, vol_align=8, flags=K.PASS_FRESH_GRID)  # step 2's lattice holds step 4's
    run_pass(pkg, dims, s[(4,)], s[(4, 2)], 2, volume=volume, vol_align=8, flags=K.PASS_SAME_LOAD)
    run_pass(pkg, dims, s[(4,)], s[(4,)], 4, volume=volume, vol_align=8, flags=K.PASS_SAME_LOAD)    # rewrites the bits it holds
    # With a changed box: the flags are knowledge about the LOAD ("same SDF, same parameters, no changed box since"), so a box
    # that changes texels contradicts them and a false flag "overwrites voxels the reference would have kept" (include/sdfgrid.h).
    # What a box can do to these kernels is leave them alone: knowledge makes every visited voxel required whatever the box
    # says, so the same parameters with either box must give the flagged pass's texels (the oracle's state without a box).
    for box in boxes_for(dims)[1:]:
        run_pass(pkg, dims, s[()], s[(4,)], 4, volume=volume, vol_align=8, flags=K.PASS_FRESH_GRID | K.PASS_SAME_LOAD, box=box)
        run_pass(pkg, dims, s[(4,)], s[(4, 2)], 2, volume=volume, vol_align=8, flags=K.PASS_SAME_LOAD, box=box)


@pytest.mark.parametrize("volume", ["plain", "ilv"])  # fill_pass_rows_adaptive_kernel<4> / <2>
@pytest.mark.parametrize("dims,slab", [((40, 12, 29), (7, 22)), ((300, 10, 6), None)])
def test_adaptive_whole_rows_passes(pkg, dims, slab, volume):
    """Nothing known, no box, step 2..8, W % 4 == 0 and the volume at a 16-byte boundary: every wave decides on the 16 bytes (8
    with the interleaved layout) of the volume it reads.  The slab's volume lies between the neighbouring slabs' rows."""
    s = load_states(dims)
    run_pass(pkg, dims, s[()], s[(4,)], 4, volume=volume, slab=slab)
    run_pass(pkg, dims, s[(4,)], s[(4, 2)], 2, volume=volume, slab=slab)
    run_pass(pkg, dims, s[STEPS], s[STEPS], 4, volume=volume, slab=slab)  # a no-op scan of a loaded grid
    # the per-voxel form of the same pass (SDFV_OPT_PASS_FORM 1) reads the volume 4 bytes at a time
    run_pass(pkg, dims, s[(4,)], s[(4, 2)], 2, volume=volume, slab=slab, options={pkg._capi.OPT_PASS_FORM: 1})
    # With a changed box the launcher leaves this kernel (has_box: a box that contains every voxel makes every visited voxel
    # required -- the store-only rows form -- and any other box takes the per-voxel kernel over the volume), so no box reaches
    # the adaptive kernel.  Both routes over the same slab and volume, as an edit of the loaded grid:
    for box in boxes_for(dims)[1:]:
        e = load_states(dims, True, box)
        run_pass(pkg, dims, e[()], e[(4,)], 4, volume=volume, slab=slab, box=box, edit=True)
        run_pass(pkg, dims, e[(4,)], e[(4, 2)], 2, volume=volume, slab=slab, box=box, edit=True)


# ---- the kernels around the passes ----
SMALL = [(5, 3, 2), (70, 4, 3), (257, 2, 2)]  # below a wave; a wave and a bit; a workgroup and one texel


@functools.lru_cache(maxsize=None)
def dense(dims):
    import oracle_binding as oracle
    r0, r1 = oracle.fill_dense(oracle.default_params(), dims)
    r0.setflags(write=False), r1.setflags(write=False)
    return r0, r1


@pytest.mark.parametrize("dims", SMALL)
def test_grid_init_and_commits(pkg, dims):
    W, H, D = dims
    r0, r1 = dense(dims)
    dist = np.ascontiguousarray(r0[..., 0])
    g = pkg.make_grid(dims)
    air = np.full(r0.shape, np.float32(pkg.AIR_DIST), np.float32)
    ar = A.Arena(A.arena_bytes(A.MIN_BAND, r0, r1))
    t0, t1 = ar.output(r0.shape, align=16, name="tex0"), ar.output(r1.shape, align=16, name="tex1")
    ar.twin(lambda: pkg.grid_init(g, t0, t1), {"tex0": air, "tex1": air}, kinds=KINDS)

    ar = A.Arena(A.arena_bytes(A.MIN_BAND, r0, dist))
    src, out = ar.input(r0, align=16, name="tex0"), ar.output(dist.shape, align=4, name="dist")
    ar.twin(lambda: pkg.commit_distance(g, src, dist=out), {"dist": dist}, kinds=KINDS)

    below = np.concatenate([dist[:, 1:], dist[:, -1:]], axis=1)  # d[min(y + 1, H - 1)]: the last row pairs with itself
    pairs = np.ascontiguousarray(np.stack([dist, below], axis=-1))
    ar = A.Arena(A.arena_bytes(A.MIN_BAND, dist, pairs))
    src, out = ar.input(dist, align=4, name="dist"), ar.output(pairs.shape, align=8, name="pairs")
    ar.twin(lambda: pkg.commit_pairs(g, src, pairs=out), {"pairs": pairs}, kinds=KINDS)

    if H % 2 == 0:
        ilv = interleave(dist).reshape(dist.shape)
        ar = A.Arena(A.arena_bytes(A.MIN_BAND, dist, ilv))
        src, out = ar.input(dist, align=4, name="dist"), ar.output(ilv.shape, align=8, name="ilv")
        ar.twin(lambda: pkg.commit_interleaved(g, src, ilv=out), {"ilv": ilv}, kinds=KINDS)


@pytest.mark.parametrize("step", [0, 2, 4])
@pytest.mark.parametrize("dims", SMALL)
def test_grid_init_unvisited(pkg, dims, step):
    """[AIR_DIST; 4] into the rows a pass with `step` does not visit (0: every row), and into those rows of the volume in either
    layout; the visited rows keep what they hold."""
    W, H, D = dims
    r0, r1 = dense(dims)
    air = np.float32(pkg.AIR_DIST)
    y, z = np.arange(H)[None, :], np.arange(D)[:, None]
    visited = np.zeros((D, H), bool) if step == 0 else ((y % step == 0) & (z % step == 0))
    want0, want1 = (np.where(visited[:, :, None, None], r, air) for r in (r0, r1))
    for volume in (None, "plain") + (("ilv",) if H % 2 == 0 else ()):
        arrays = [r0, r1] + ([] if volume is None else [r0[..., 0]])
        ar = A.Arena(A.arena_bytes(A.MIN_BAND, *arrays))
        t0, t1 = ar.inout(r0, align=16, name="tex0"), ar.inout(r1, align=16, name="tex1")
        expected = {"tex0": want0, "tex1": want1}
        vol = None
        if volume is not None:
            vol = ar.inout(layout(r0[..., 0], volume), align=8 if volume == "ilv" else 4, name="vol")
            expected["vol"] = layout(want0[..., 0], volume)
        g = pkg.make_grid(dims)
        ar.twin(lambda: pkg.grid_init_unvisited(g, step, t0, t1, dist=vol, flags=pkg._capi.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0),
                expected, kinds=KINDS)


@pytest.mark.parametrize("volume", [None, "plain", "ilv"])
@pytest.mark.parametrize("arrangement", ["run", "scattered", "beyond"])
def test_pack_samples(pkg, oracle, arrangement, volume):
    """sdfv_pack_samples over the slab z in [1, 4) of a 20 x 6 x 5 grid (360 voxels): a contiguous run from index_base; scattered
    indices that include the slab's last voxel; and one index beyond the slab, which the contract says is skipped.  tex0 is
    written whole, tex1 .rgb only; every other texel keeps new_voxels' state."""
    dims, (z0, z1) = (20, 6, 5), (1, 4)
    W, H, D = dims
    n_vox = W * H * (z1 - z0)
    rng = np.random.default_rng(17)
    base = 0
    if arrangement == "run":
        base, idx = 37, None
        where = base + np.arange(290)           # crosses rows and a slice; a workgroup and 34 records
    else:
        where = np.sort(rng.choice(n_vox - 1, size=257, replace=False))
        where = np.concatenate([where, [n_vox - 1]])            # ... and the slab's last voxel
        rng.shuffle(where)
        if arrangement == "beyond":
            where[100] = n_vox                                   # the first index that is no voxel of the slab
        idx = where.astype(np.uint32)
    samples = rng.uniform(0.0, 1.0, size=(len(where), 7)).astype(np.float32)
    samples[:, 0] = rng.uniform(-0.3, 1.0, size=len(where)).astype(np.float32)   # 0.1 + distance is clamped to [0, 1] on both sides
    samples[5, 1:4] = 0.0                                        # an all-zero colour: the 0.5 grey
    samples[6, 6] = 0.0                                          # occlusion <= 0 -> 1
    air = np.float32(pkg.AIR_DIST)
    want0 = np.full((z1 - z0, H, W, 4), air, np.float32)
    want1 = want0.copy()
    f0, f1 = want0.reshape(-1, 4), want1.reshape(-1, 4)
    for k, v in enumerate(where):
        if v < n_vox:
            p0, p1 = oracle.pack(samples[k])
            f0[v], f1[v, :3] = p0, p1[:3]
    before = np.full_like(want0, air)
    arrays = [before, before, samples] + ([] if volume is None else [before[..., 0]])
    ar = A.Arena(A.arena_bytes(A.MIN_BAND, *arrays, ((len(where),), np.uint32)))
    s = ar.input(samples, align=4, name="samples")               # "n records (4-byte aligned)"
    i = None if idx is None else ar.input(idx, align=4, name="indices")
    t0, t1 = ar.inout(before, align=16, name="tex0"), ar.inout(before, align=16, name="tex1")
    expected = {"tex0": want0, "tex1": want1}
    vol = None
    if volume is not None:
        vol = ar.inout(before[..., 0], align=8 if volume == "ilv" else 4, name="vol")
        expected["vol"] = layout(want0[..., 0], volume)
    g = pkg.make_grid(dims, z_begin=z0, z_end=z1)
    ar.twin(lambda: pkg.pack_samples(g, s, t0, t1, indices=i, index_base=base, dist=vol,
                                     flags=pkg._capi.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0), expected, kinds=KINDS)


@pytest.mark.parametrize("volume", ["plain", "ilv"])
def test_emit_update_points(pkg, volume):
    """sdfv_emit_update_points with its outputs AND its scratch carved from the arena: points 65..84 of the step-2 pass over
    20 x 14 x 17 (10 x 7 lattice points per plane: the run crosses row ends and, at 70, a plane end).  The entries beyond
    `count` are undefined, the scratch is the library's to use -- inside their buffers."""
    import ctypes as C
    import torch
    from test_gpu_viewer_abi import emit_reference
    dims, bmin, bmax, step, cursor, n = (20, 14, 17), (-1.0, -0.5, -0.75), (1.0, 0.5, 0.75), 2, 65, 20
    W, H, D = dims
    rng = np.random.default_rng(7)
    air = np.float32(pkg.AIR_DIST)
    vol = rng.uniform(0.0, 1.0, (D, H, W)).astype(np.float32)
    vol[rng.uniform(size=vol.shape) < 0.4] = air
    box = np.array([-0.2, -0.1, -0.8, 0.6, 0.3, 0.9], np.float32)
    want_p, want_i = emit_reference(dims, bmin, bmax, step, cursor, n, box, vol, air)
    k = len(want_i)
    assert 0 < k < n
    scratch_bytes = pkg.lib.sdfv_emit_update_points_scratch_bytes(n)
    assert scratch_bytes > 0, pkg.lib.sdfv_last_error()
    host_vol = layout(vol, volume).reshape(-1)
    ar = A.Arena(A.arena_bytes(A.MIN_BAND, host_vol, ((n, 3), np.float32), ((n,), np.uint32), ((1,), np.uint32), ((scratch_bytes,), np.uint8)))
    dvol = ar.input(host_vol, align=8 if volume == "ilv" else 4, name="dist")
    pts = ar.output((n, 3), np.float32, align=4, name="points")
    idx = ar.output((n,), np.uint32, align=4, name="indices")
    count = ar.output((1,), np.uint32, align=4, name="count")
    scratch = ar.output((scratch_bytes,), np.uint8, align=16, name="scratch")
    full_p, full_i = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
    full_p[:k], full_i[:k] = want_p, want_i
    beyond = np.arange(n) >= k
    expected = {"points": A.Untouched(full_p, undefined=beyond[:, None]), "indices": A.Untouched(full_i, undefined=beyond),
                "count": np.array([k], np.uint32), "scratch": A.Untouched(np.zeros(scratch_bytes, np.uint8), undefined=True)}
    g = pkg.make_grid(dims, bmin, bmax)
    cb = (C.c_float * 6)(*box)

    def run():
        rc = pkg.lib.sdfv_emit_update_points(C.byref(g), step, cursor, n, cb, dvol.data_ptr(), pkg._capi.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0,
                                             pts.data_ptr(), idx.data_ptr(), count.data_ptr(), scratch.data_ptr(), scratch_bytes,
                                             torch.cuda.current_stream().cuda_stream)
        assert rc == 0, pkg.lib.sdfv_last_error()
    ar.twin(run, expected, kinds=KINDS)
