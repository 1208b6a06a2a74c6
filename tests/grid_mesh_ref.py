"""Shared by tests/test_grid_mesh_cpu.py and the tests/test_gpu_*grid_mesh*.py files: what is particular to a loaded grid in the
numpy float32 restatement of mesh extraction (include/sdfgrid.h, "Meshing a loaded grid"), written from the header and calling
nothing of the library.

* lattice_of(dims, bb, lod): cells per axis and the mesh's box; unpack(s, lod): the lattice d = s - 0.1f of the published voxels;
* srgb_index / materials: the nearest published voxel of a position and its texels, the sRGB table inverted;
* extract(...): tests/mesh_ref.py's extraction over that lattice, with the lattice's own normals (mesh_ref.lattice_normals) and
  these materials.  The extraction with cells per axis, cell_of and the normals live in tests/mesh_ref.py; the parser of
  srgb_lut.inc is tests/program_march_ref.py's and interleave() is tests/program_fill_check.py's.
Every arithmetic step is one numpy float32 operation on float32 operands."""
import numpy as np

import mesh_ref as MR
from program_march_ref import srgb_table

F = np.float32
DUAL = MR.DUAL
bits = MR.bits
TENTH = F(0.1)                                            # the float the fill adds (scene/sdf/mod.rs:196)
TABLE = srgb_table()


def srgb_index(x):
    """The number of table entries < x, at the most 255, 0 for a NaN -> integer array."""
    x = np.asarray(x, F)
    idx = (TABLE[None, :] < x.reshape(-1, 1)).sum(axis=1)          # the rule as it is written: a count, no search
    return np.minimum(idx, 255).reshape(x.shape)


def srgb_colour(x):
    return srgb_index(x).astype(F) / F(255.0)


def lattice_of(dims, bb, lod):
    """dims = (W, H, D), bb = min.xyz + max.xyz of the grid -> (cells (x, y, z), the mesh's box min.xyz + max.xyz): the upper corner
    is the position of voxel cells * lod as the fill computes it."""
    cells = tuple((int(d) - 1) // int(lod) for d in dims)
    lo, hi = np.array(bb[:3], F), np.array(bb[3:], F)
    top = [F(cells[a] * lod) / (F(dims[a]) - F(1.0)) * (hi[a] - lo[a]) + lo[a] for a in range(3)]
    return cells, tuple(float(v) for v in lo) + tuple(float(v) for v in top)


def unpack(s, lod):
    """s [D, H, W]: the stored distances (tex0.r) -> the lattice d [k, j, i] = s - 0.1f of the voxels (i, j, k) * lod."""
    s = np.asarray(s, F)
    n = [(m - 1) // lod + 1 for m in s.shape]
    return np.ascontiguousarray(s[::lod, ::lod, ::lod][:n[0], :n[1], :n[2]] - TENTH)


def synthetic_grid(dims, bb, lod=1, seed=0):
    """A grid nobody filled: (tex0, tex1) [D, H, W, 4] whose published voxels (every index a multiple of lod) hold a gyroid's
    clamped distance + 0.1, colours that are table entries and seeded material values, and whose other voxels hold [AIR; 4] --
    for the tests that are about where and when the entry points read, not about a fill."""
    import oracle_binding
    rng = np.random.default_rng(seed)
    w, h, d = dims
    ax = [(np.arange(dims[a], dtype=F) / (F(dims[a]) - F(1.0))) * (F(bb[3 + a]) - F(bb[a])) + F(bb[a]) for a in range(3)]
    zz, yy, xx = [v.astype(np.float64) * 4.0 for v in np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")]
    g = 0.3 * (np.sin(xx) * np.cos(yy) + np.sin(yy) * np.cos(zz) + np.sin(zz) * np.cos(xx)) - 0.03
    t0 = np.zeros((d, h, w, 4), F)
    t1 = np.zeros((d, h, w, 4), F)
    t0[..., 0] = np.clip(g.astype(F) + TENTH, F(0), F(1))
    t0[..., 1:] = TABLE[rng.integers(0, 256, size=(d, h, w, 3))]
    t1[..., :3] = rng.uniform(0.0, 1.0, size=(d, h, w, 3)).astype(F)
    air = F(oracle_binding.AIR_DIST)
    t1[..., 3] = air
    zi, yi, xi = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    off = (zi % lod != 0) | (yi % lod != 0) | (xi % lod != 0)
    t0[off] = air
    t1[off] = air
    return t0, t1


# ---- the materials ----
def nearest_voxel(p, box, cells, lod):
    """-> (x, y, z) voxel indices of the nearest published lattice point of each position: q = c + (f > 0.5), voxel = q * lod."""
    c, f = MR.cell_of(p, box, cells)
    return [(c[a] + (f[a] > F(0.5))) * lod for a in range(3)]


def materials(tex0, tex1, bb, lod, p):
    """tex0, tex1 [D, H, W, 4] of the grid over bb, positions p [m, 3] -> [m, 6]: colour (the table inverted), then tex1.rgb."""
    dims = (tex0.shape[2], tex0.shape[1], tex0.shape[0])
    cells, box = lattice_of(dims, bb, lod)
    x, y, z = nearest_voxel(p, box, cells, lod)
    t0, t1 = tex0[z, y, x], tex1[z, y, x]
    out = np.zeros((len(t0), 6), F)
    out[:, :3] = srgb_colour(t0[:, 1:4])
    out[:, 3:] = t1[:, :3]
    return out


def extract(tex0, tex1, bb, lod=1, algorithm=0, with_materials=True):
    """What sdfv_grid_mesh_extract leaves for the grid tex0, tex1 [D, H, W, 4] over bb -> (vertices [V, 12], indices, info)."""
    dims = (tex0.shape[2], tex0.shape[1], tex0.shape[0])
    _, box = lattice_of(dims, bb, lod)
    d = unpack(tex0[..., 0], lod)
    v, idx, info = MR.extract(d, box, algorithm, lambda p: MR.lattice_normals(d, box, p),
                              (lambda p: materials(tex0, tex1, bb, lod, p)) if with_materials else None)
    info["box"] = box
    return v, idx, info
