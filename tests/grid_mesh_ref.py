"""Shared by tests/test_grid_mesh_cpu.py and the tests/test_gpu_*grid_mesh*.py files: a numpy float32 restatement of meshing a
loaded grid (include/sdfgrid.h, "Meshing a loaded grid"), written from the header and calling nothing of the library.

* lattice_of(dims, bb, lod): cells per axis and the mesh's box; unpack(s, lod): the lattice d = s - 0.1f of the published voxels;
* srgb_index / materials: the nearest published voxel of a position and its texels, the sRGB table inverted;
* extract(...): the extraction of tests/lattice_mesh_ref.py and tests/dual_contour_ref.py over a lattice with its own number of
  cells PER AXIS.  Those two modules take a cube (n = d.shape[0] - 1 on every axis); the functions here are theirs with the axis
  each n belongs to written out, and tests/test_grid_mesh_cpu.py holds them to the originals, bit for bit, on cubes.
Every arithmetic step is one numpy float32 operation on float32 operands."""
import os
import re

import numpy as np

import dual_contour_ref as D
import lattice_mesh_ref as L
import program_mesh_ref as M
import program_ref as R

F = np.float32
DUAL = D.DUAL
bits = M.bits
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TENTH = F(0.1)                                            # the float the fill adds (scene/sdf/mod.rs:196)


def srgb_table():
    """The 256 floats of sdf-viewer_amd/csrc/srgb_lut.inc (C99 hexadecimal floats: exact)."""
    text = open(os.path.join(ROOT, "sdf-viewer_amd", "csrc", "srgb_lut.inc")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    t = np.array([float.fromhex(x) for x in re.findall(r"[-+]?0x[0-9a-fA-F.]+p[-+]?\d+", text)], np.float64)
    assert t.shape == (256,) and (t.astype(F) == t).all()
    return t.astype(F)


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


def interleave(vol):
    """[D, H, W] -> the y-interleaved volume as a flat array: entry ((row >> 1) * W + x) * 2 + (row & 1), row = z * H + y."""
    d, h, w = vol.shape
    assert h % 2 == 0
    return np.ascontiguousarray(vol.reshape(d * h // 2, 2, w).transpose(0, 2, 1)).reshape(-1)


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


# ---- the lattice with its own number of cells per axis: d [k, j, i] has (cz + 1, cy + 1, cx + 1) points ----
def cells_of(d):
    return (d.shape[2] - 1, d.shape[1] - 1, d.shape[0] - 1)


def axes_of(cells, bb):
    lo, size = np.array(bb[:3], F), np.array(bb[3:], F) - np.array(bb[:3], F)
    unit = [np.arange(cells[a] + 1, dtype=F) / F(cells[a]) for a in range(3)]
    return unit, lo, size, [unit[a] * size[a] + lo[a] for a in range(3)]


@np.errstate(all="ignore")
def cell_of(p, bb, cells):
    """Steps 1-2 of normal(p) per axis -> (c [3][m] integers, f [3][m] float32)."""
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    lo, size = np.array(bb[:3], F), np.array(bb[3:], F) - np.array(bb[:3], F)
    c, f = [], []
    for a in range(3):
        n = F(cells[a])
        u = (p[:, a] - lo[a]) / size[a] * n
        u = np.where(u > 0, u, F(0))
        u = np.where(u < n, u, n)
        ca = np.minimum(np.floor(u).astype(np.int64), cells[a] - 1)
        c.append(ca)
        f.append(u - ca.astype(F))
    return c, f


@np.errstate(all="ignore")
def normals(d, bb, p):
    """lattice_mesh_ref.normals with cells per axis."""
    d = np.ascontiguousarray(d, F)
    cells = cells_of(d)
    size = np.array(bb[3:], F) - np.array(bb[:3], F)
    c, f = cell_of(p, bb, cells)

    def gradient(a, q):
        hi, low = np.minimum(q[a] + 1, cells[a]), np.maximum(q[a], 1) - 1
        qh, ql = list(q), list(q)
        qh[a], ql[a] = hi, low
        return (d[qh[2], qh[1], qh[0]] - d[ql[2], ql[1], ql[0]]) / (hi - low).astype(F)

    G = []
    for a in range(3):
        g = {(ox, oy, oz): gradient(a, [c[0] + ox, c[1] + oy, c[2] + oz]) for oz in (0, 1) for oy in (0, 1) for ox in (0, 1)}
        x = {(oy, oz): L.lerp(g[0, oy, oz], g[1, oy, oz], f[0]) for oz in (0, 1) for oy in (0, 1)}
        y = {oz: L.lerp(x[0, oz], x[1, oz], f[1]) for oz in (0, 1)}
        G.append(L.lerp(y[0], y[1], f[2]) * (F(cells[a]) / size[a]))
    s = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]
    inv = F(1.0) / np.sqrt(s)
    return np.stack([np.where(s > 0, G[a] * inv, F(0)) for a in range(3)], axis=-1).astype(F)


@np.errstate(all="ignore")
def hermite_positions(d, bb):
    """dual_contour_ref.hermite_positions with cells per axis."""
    unit, lo, size, _ = axes_of(cells_of(d), bb)
    cross, _ = D.crossings(d)
    kk, jj, ii, aa = np.nonzero(cross)
    idx = np.stack([ii, jj, kk], axis=-1)
    rows = np.arange(len(aa))
    nb = idx.copy()
    nb[rows, aa] += 1
    d0, d1 = d[kk, jj, ii], d[nb[:, 2], nb[:, 1], nb[:, 0]]
    t = d0 / (d0 - d1)
    u = np.stack([unit[a][idx[:, a]] for a in range(3)], axis=-1).astype(F)
    ua = u[rows, aa]
    u1 = np.array([unit[a][i + 1] for a, i in zip(aa, idx[rows, aa])], F).reshape(ua.shape)
    u[rows, aa] = ua + t * (u1 - ua)
    return (u * size[None, :] + lo[None, :]).astype(F)


def cell_owner(cells, cell, e):
    """The lattice point that owns edge e of the cells `cell` (flat, x fastest) -> ([i, j, k], axis)."""
    ci, r = cell % cells[0], cell // cells[0]
    cj, ck = r % cells[1], r // cells[1]
    a, s = divmod(int(e), 4)
    o0, o1 = [b for b in range(3) if b != a]
    owner = [ci, cj, ck]
    owner[o0] = owner[o0] + (s & 1)
    owner[o1] = owner[o1] + (s >> 1)
    return owner, a


def triangles(d):
    """lattice_mesh_ref.triangles with cells per axis."""
    cx, cy, cz = cells_of(d)
    inside = d < 0
    cross, vid = D.crossings(d)
    count, edges = M.mc_table()
    case = np.zeros((cz, cy, cx), np.int64)
    for corner in range(8):
        ox, oy, oz = corner & 1, (corner >> 1) & 1, (corner >> 2) & 1
        case |= inside[oz:oz + cz, oy:oy + cy, ox:ox + cx].astype(np.int64) << corner
    case = case.reshape(-1)
    out = []
    for cell in np.nonzero(count[case])[0]:
        for e in edges[case[cell], :3 * count[case[cell]]]:
            owner, a = cell_owner((cx, cy, cz), int(cell), e)
            assert cross[owner[2], owner[1], owner[0], a]
            out.append(vid[owner[2], owner[1], owner[0], a])
    return np.array(out, np.int64), case


@np.errstate(all="ignore")
def solve(d, bb, hermite):
    """dual_contour_ref.solve with cells per axis (the same dict)."""
    cells = cells_of(d)
    cx, cy, cz = cells
    hermite = np.ascontiguousarray(hermite, F)
    _, _, _, axes = axes_of(cells, bb)
    cross, vid = D.crossings(d)
    assert hermite.shape[0] == int(cross.sum())
    all_cells = np.arange(cx * cy * cz)
    present, rec = [], []
    for e in range(12):
        owner, a = cell_owner(cells, all_cells, e)
        present.append(cross[owner[2], owner[1], owner[0], a])
        rec.append(vid[owner[2], owner[1], owner[0], a])
    active = np.any(present, axis=0)
    act = np.nonzero(active)[0]
    ci, r = act % cx, act // cx
    cj, ck = r % cy, r // cy
    present = [p[act] for p in present]
    rec = [np.where(p, r_[act], 0) for p, r_ in zip(present, rec)]
    nv = len(act)
    zero = np.zeros(nv, F)
    c = [zero.copy(), zero.copy(), zero.copy()]
    m = np.zeros(nv, np.int64)
    for e in range(12):
        for b in range(3):
            c[b] = np.where(present[e], c[b] + hermite[rec[e], b], c[b])
        m += present[e]
    c = [c[b] / m.astype(F) for b in range(3)]
    mxx, mxy, mxz, myy, myz, mzz, gx, gy, gz = (zero.copy() for _ in range(9))
    k = np.zeros(nv, np.int64)
    for e in range(12):
        h = hermite[rec[e]]
        nx, ny, nz = h[:, 3], h[:, 4], h[:, 5]
        w = nx * nx + ny * ny + nz * nz
        used = present[e] & (w > F(0.5)) & (w < F(2.0))
        rx, ry, rz = h[:, 0] - c[0], h[:, 1] - c[1], h[:, 2] - c[2]
        b = (nx * rx + ny * ry) + nz * rz
        mxx = np.where(used, mxx + nx * nx, mxx)
        mxy = np.where(used, mxy + nx * ny, mxy)
        mxz = np.where(used, mxz + nx * nz, mxz)
        myy = np.where(used, myy + ny * ny, myy)
        myz = np.where(used, myz + ny * nz, myz)
        mzz = np.where(used, mzz + nz * nz, mzz)
        gx = np.where(used, gx + nx * b, gx)
        gy = np.where(used, gy + ny * b, gy)
        gz = np.where(used, gz + nz * b, gz)
        k += used
    s = F(1.0) / k.astype(F)
    yx, yy, yz = zero.copy(), zero.copy(), zero.copy()
    for _ in range(24):
        tx = gx - ((mxx * yx + mxy * yy) + mxz * yz)
        ty = gy - ((mxy * yx + myy * yy) + myz * yz)
        tz = gz - ((mxz * yx + myz * yy) + mzz * yz)
        yx, yy, yz = yx + s * tx, yy + s * ty, yz + s * tz
    some = k > 0
    y = [np.where(some, yx, zero), np.where(some, yy, zero), np.where(some, yz, zero)]
    pos = np.zeros((nv, 3), F)
    for b, cell in enumerate((ci, cj, ck)):
        pos[:, b] = R.pmax(axes[b][cell], R.pmin(c[b] + y[b], axes[b][cell + 1]))
    cell_vertex = np.cumsum(active) - 1
    kk, jj, ii, aa = np.nonzero(cross)
    idx = np.stack([ii, jj, kk], axis=-1)
    out = []
    for row in range(len(aa)):
        a = int(aa[row])
        o0, o1 = [b for b in range(3) if b != a]
        p = idx[row]
        if not (1 <= p[o0] <= cells[o0] - 1 and 1 <= p[o1] <= cells[o1] - 1):
            continue
        q = []
        for du, dv in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            cc = [int(p[0]), int(p[1]), int(p[2])]
            cc[o0] += du
            cc[o1] += dv
            flat = (cc[2] * cy + cc[1]) * cx + cc[0]
            assert active[flat]
            q.append(int(cell_vertex[flat]))
        flip = (a == 1) != bool(d[p[2], p[1], p[0]] >= 0)
        out += [q[0], q[2], q[1], q[0], q[3], q[2]] if flip else [q[0], q[1], q[2], q[0], q[2], q[3]]
    return dict(pos=pos, idx=np.array(out, np.int64), mass=np.stack(c, axis=-1).astype(F) if nv else np.zeros((0, 3), F),
                used=k, edges=m, cells=act, quads=len(out) // 6)


def extract_lattice(d, bb, algorithm=0):
    """lattice_mesh_ref.extract with cells per axis -> (vertices [V, 12] with zero materials, indices, info)."""
    d = np.ascontiguousarray(d, F)
    assert not np.isnan(d).any() and not (d == 0).any(), "the cases of the tests keep clear of exact zeros and NaNs"
    hp = hermite_positions(d, bb)
    if algorithm == DUAL:
        h = np.zeros((len(hp), 6), F)
        h[:, :3] = hp
        if len(hp):
            h[:, 3:6] = normals(d, bb, hp)
        info = solve(d, bb, h)
        info["hermite"] = h
        pos, idx = info["pos"], info["idx"]
    else:
        assert algorithm == 0
        idx, case = triangles(d)
        pos, info = hp, dict(cases=case)
    v = np.zeros((len(pos), 12), F)
    v[:, :3] = pos
    if len(pos):
        v[:, 3:6] = normals(d, bb, pos)
    return v, idx, info


# ---- the materials ----
def nearest_voxel(p, box, cells, lod):
    """-> (x, y, z) voxel indices of the nearest published lattice point of each position: q = c + (f > 0.5), voxel = q * lod."""
    c, f = cell_of(p, box, cells)
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
    v, idx, info = extract_lattice(d, box, algorithm)
    if with_materials and len(v):
        v[:, 6:] = materials(tex0, tex1, bb, lod, v[:, :3])
    info["lattice"], info["box"] = d, box
    return v, idx, info
