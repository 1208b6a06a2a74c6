"""Shared by tests/test_gpu_program_pass.py and tests/test_program_pass_cpu.py: what one pass of sdfv_program_grid_pass may touch,
restated in numpy from the header's words (include/sdfgrid.h) -- the pass lattice, update_required on the voxels' positions
(tests/program_ref.py grid_positions: idx / (dim - 1) * size + min in three f32 roundings) -- and the textures it must leave:
where(mask, the dense fill of the new program, what the grid held)."""
import numpy as np

import program_ref as R

F = np.float32
DIMS = (70, 34, 19)                                  # W is no multiple of 64, H is even (the interleaved volume pairs rows)
BB_MIN, BB_MAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
STEPS = (1, 2, 4)


def axis_coords(dims=DIMS, bb_min=BB_MIN, bb_max=BB_MAX):
    """The voxel coordinates per axis, as the fill rounds them: three float32 arrays of W, H and D entries."""
    out = []
    for a in range(3):
        i = np.arange(dims[a], dtype=F)
        out.append(((i / (F(dims[a]) - F(1))) * (F(bb_max[a]) - F(bb_min[a]))) + F(bb_min[a]))
    return out


def lattice(dims, step):
    """[D, H, W] bool: x, y and GLOBAL z are multiples of step."""
    W, H, D = dims
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    return (x % step == 0) & (y % step == 0) & (z % step == 0)


def inside(dims, bb_min, bb_max, box):
    """[D, H, W] bool: the voxel's position lies inside the closed box (None: nowhere; a NaN bound: nowhere)."""
    W, H, D = dims
    if box is None:
        return np.zeros((D, H, W), bool)
    pos = R.grid_positions(dims, bb_min, bb_max).reshape(D, H, W, 3)
    lo, hi = np.array(box[:3], F), np.array(box[3:], F)
    with np.errstate(invalid="ignore"):
        return ((pos >= lo) & (pos <= hi)).all(axis=-1)


def update_mask(dims, bb_min, bb_max, step, tex0_r, box, air):
    """update_required on the pass lattice: tex0.r == AIR_DIST or inside the box."""
    return lattice(dims, step) & ((tex0_r == F(air)) | inside(dims, bb_min, bb_max, box))


def expected(before, dense, mask, air, volume):
    """before, dense: (tex0, tex1) numpy [D, H, W, 4].  With a volume tex1.a of an updated voxel is AIR_DIST (what the dense fill
    writes), without one it keeps what the grid held.  Returns (tex0, tex1, plain volume [D, H, W] = tex0.r)."""
    m = mask[..., None]
    t0 = np.where(m, dense[0], before[0])
    t1 = np.where(m, dense[1], before[1])
    assert (dense[1][..., 3] == F(air)).all()
    if not volume:
        t1[..., 3] = before[1][..., 3]
    return t0, t1, t0[..., 0].copy()


def boxes(step, dims=DIMS, bb_min=BB_MIN, bb_max=BB_MAX):
    """name -> (box, what the mask inside the lattice must be: "some", "none" or "all") for a loaded grid."""
    cx, cy, cz = axis_coords(dims, bb_min, bb_max)
    up, down = (lambda v: np.nextafter(F(v), F(np.inf))), (lambda v: np.nextafter(F(v), F(-np.inf)))
    mid = lambda c, i: (float(c[i]) + float(c[i + 1])) / 2.0                        # noqa: E731
    faces = (cx[8], cy[4], cz[4], cx[48], cy[28], cz[12])                          # all on the step-4 lattice
    out = {
        # 41 voxels wide at step 1: a wave of the box launch spans one row and part of the next
        "generic": ((mid(cx, 9), mid(cy, 4), mid(cz, 2), mid(cx, 50), mid(cy, 21), mid(cz, 12)), "some"),
        "faces": (tuple(float(v) for v in faces), "some"),
        "faces_in": (tuple(float(up(v)) for v in faces[:3]) + tuple(float(down(v)) for v in faces[3:]), "some"),
        "faces_out": (tuple(float(down(v)) for v in faces[:3]) + tuple(float(up(v)) for v in faces[3:]), "some"),
        "partly_outside": ((-2.0, -3.0, -1.5, mid(cx, 30), mid(cy, 17), mid(cz, 9)), "some"),
        # x strictly between two neighbouring lattice planes
        "between": ((float(up(cx[8])), -2.0, -2.0, float(down(cx[8 + step])), 2.0, 2.0), "none"),
        "inverted": ((0.5, -0.5, -0.5, -0.5, 0.5, 0.5), "none"),
        "nan": ((float("nan"), -2.0, -2.0, 2.0, 2.0, 2.0), "none"),
        "everything": ((-2.0, -2.0, -2.0, 2.0, 2.0, 2.0), "all"),
    }
    return out
