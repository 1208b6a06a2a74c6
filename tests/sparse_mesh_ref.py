"""Shared by the tests of sparse meshing over SDF programs: the numpy float32 restatement of sdfv_program_mesh_extract_sparse,
written from include/sdfgrid.h ("SDF programs: sparse meshing") and calling nothing of the library.  The program machine is
tests/program_ref.py's, normals and materials are tests/program_mesh_ref.py's, the marching-cubes table and the lattice
coordinates tests/mesh_ref.py's.

* refine: the block list level by level, children x fastest, kept iff !(|d| > (L * r) * 1.001f) at the centre lattice point;
* extract: 125 distances per brick, the owned crossing edges in brick, point, axis order, the triangles of the cells whose
  crossing edges all have a brick for an owner;
* active_cells: which cells of the DENSE lattice the surface passes through and how many of them no brick holds -- the condition
  under which the sparse mesh equals the dense one as a set;
* record_set, triangle_set: a mesh as the sets the header's promise speaks of.
Every arithmetic step is one numpy float32 operation on float32 operands."""
import numpy as np

import mesh_ref as MR
import program_mesh_ref as M
import program_ref as R

F = np.float32
CHILD = np.array([(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)], np.int64)                # x fastest
LOCAL = np.array([(l % 5, (l // 5) % 5, l // 25) for l in range(125)], np.int64)                   # a brick's points, x fastest
STRIDE = (1, 5, 25)


def threshold(n, bb, s, L=1.0):
    """t = (L * r) * 1.001f of a block of s cells."""
    size = np.array(bb[3:], F) - np.array(bb[:3], F)
    e = [F(s) / F(n) * size[a] for a in range(3)]
    r = F(0.5) * np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    return (F(L) * r) * F(1.001)


def positions(n, bb, idx):
    """Lattice points idx [m, 3] -> [m, 3] float32: (float)i / (float)n * size + min per axis."""
    axes = MR.axes_of(n, bb)[3]
    return np.stack([axes[a][idx[:, a]] for a in range(3)], axis=-1).astype(F)


@np.errstate(all="ignore")
def refine(ops, n, bb, L=1.0):
    """-> (origins of the bricks [B, 3] in cells, in list order; the stats the call reports but for scratch_bytes)."""
    assert n >= 4 and n & (n - 1) == 0
    blocks, s, tested, kept = np.zeros((1, 3), np.int64), n, [], []
    while s > 4:
        s //= 2
        children = (blocks[:, None, :] + CHILD[None, :, :] * s).reshape(-1, 3)
        keep = np.zeros(0, bool)
        if len(children):
            d = R.run(ops, positions(n, bb, children + s // 2), True)[:, 0]
            keep = ~(np.abs(d) > threshold(n, bb, s, L))
        tested.append(len(children))
        kept.append(int(keep.sum()))
        blocks = children[keep]
    return blocks, dict(levels=len(tested), tested=tested, kept=kept, bricks=len(blocks),
                        evaluations=sum(tested) + 125 * len(blocks))


def edge_crosses(case, e):
    a, s = divmod(int(e), 4)
    o0, o1 = [b for b in range(3) if b != a]
    start = ((s & 1) << o0) | ((s >> 1) << o1)
    return ((case >> start) ^ (case >> (start | (1 << a)))) & 1 == 1


@np.errstate(all="ignore")
def extract(ops, n, bb, materials=False, L=1.0):
    """What sdfv_program_mesh_extract_sparse leaves -> (vertices [V, 12] float32, indices int64, stats)."""
    bricks, stats = refine(ops, n, bb, L)
    B, nb = len(bricks), n // 4
    unit, lo, size, _ = MR.axes_of(n, bb)
    if B == 0:
        return np.zeros((0, 12), F), np.zeros(0, np.int64), stats
    idx = (bricks[:, None, :] + LOCAL[None, :, :]).reshape(-1, 3)
    d = R.run(ops, positions(n, bb, idx), True)[:, 0].reshape(B, 125)
    assert not np.isnan(d).any() and not (d == 0).any(), "the cases of the tests keep clear of exact zeros and NaNs"
    inside = d < 0
    last = bricks // 4 == nb - 1                                                    # [B, 3]
    owned = np.ones((B, 125), bool)
    for a in range(3):
        owned &= (LOCAL[None, :, a] < 4) | last[:, a, None]
    cross = np.zeros((B, 125, 3), bool)
    for a in range(3):
        j = np.nonzero(LOCAL[:, a] < 4)[0]                                          # the +a neighbour is one of the brick's own 125
        cross[:, j, a] = owned[:, j] & (inside[:, j] != inside[:, j + STRIDE[a]])
    vid = (np.cumsum(cross.reshape(-1)) - 1).reshape(cross.shape)
    bi, pi, aa = np.nonzero(cross)                                                  # C order: brick, point, axis
    # edge_position: t = d0 / (d0 - d1), u = u0 + t * (u1 - u0) on the edge's axis, p = u * size + min
    g = bricks[bi] + LOCAL[pi]
    rows = np.arange(len(aa))
    d0, d1 = d[bi, pi], d[bi, pi + np.array(STRIDE)[aa]]
    t = d0 / (d0 - d1)
    u = np.stack([unit[a][g[:, a]] for a in range(3)], axis=-1).astype(F)
    ua = u[rows, aa]
    u1 = np.array([unit[a][i + 1] for a, i in zip(aa, g[rows, aa])], F).reshape(ua.shape)
    u[rows, aa] = ua + t * (u1 - ua)
    pos = (u * size[None, :] + lo[None, :]).astype(F)
    v = np.zeros((len(pos), 12), F)
    v[:, :3] = pos
    if len(pos):
        v[:, 3:6] = M.normals(ops, pos)
        if materials:
            v[:, 6:] = R.run(ops, pos, False)[:, 1:7]
    # triangles: brick by brick, cell by cell (x fastest), only where every crossing edge of the cell is a brick's
    number = {tuple(int(c) for c in b // 4): k for k, b in enumerate(bricks)}
    count, edges = MR.mc_table()
    ins = inside.reshape(B, 5, 5, 5)                                                # [brick, z, y, x]
    case = np.zeros((B, 4, 4, 4), np.int64)
    for corner in range(8):
        ox, oy, oz = corner & 1, (corner >> 1) & 1, (corner >> 2) & 1
        case |= ins[:, oz:oz + 4, oy:oy + 4, ox:ox + 4].astype(np.int64) << corner
    case = case.reshape(B, 64)

    def owner(k, cell, e):
        a, s = divmod(int(e), 4)
        o0, o1 = [b for b in range(3) if b != a]
        l = [cell & 3, (cell >> 2) & 3, cell >> 4]
        l[o0] += s & 1
        l[o1] += s >> 1
        b = [int(c) for c in bricks[k] // 4]
        for axis in range(3):
            if l[axis] == 4 and b[axis] < nb - 1:
                l[axis], b[axis] = 0, b[axis] + 1
        return number.get(tuple(b)), (l[2] * 5 + l[1]) * 5 + l[0], a

    out = []
    for k, cell in zip(*np.nonzero(count[case])):
        cs = int(case[k, cell])
        if any(edge_crosses(cs, e) and owner(k, int(cell), e)[0] is None for e in range(12)):
            continue
        for e in edges[cs, :3 * count[cs]]:
            ob, slot, a = owner(k, int(cell), e)
            assert cross[ob, slot, a]
            out.append(vid[ob, slot, a])
    return v, np.array(out, np.int64), stats


def active_cells(ops, n, bb, L=1.0):
    """-> (cells of the dense lattice with a crossing edge, how many of them lie in no brick)."""
    d = M.lattice(ops, n, bb)[1]
    inside = d < 0
    case = np.zeros((n, n, n), np.int64)
    for corner in range(8):
        ox, oy, oz = corner & 1, (corner >> 1) & 1, (corner >> 2) & 1
        case |= inside[oz:oz + n, oy:oy + n, ox:ox + n].astype(np.int64) << corner
    kk, jj, ii = np.nonzero((case != 0) & (case != 255))
    have = {tuple(int(c) for c in b // 4) for b in refine(ops, n, bb, L)[0]}
    outside = sum((int(i) // 4, int(j) // 4, int(k) // 4) not in have for i, j, k in zip(ii, jj, kk))
    return len(ii), outside


def record_set(v):
    """The vertex records as a sorted list of their 48 bytes."""
    v = np.ascontiguousarray(v, F).reshape(-1, 12)
    return sorted(r.tobytes() for r in v)


def triangle_set(v, idx):
    """The triangles as a sorted list of record triples, each rotated to start at its smallest record."""
    v = np.ascontiguousarray(v, F).reshape(-1, 12)
    rec = [r.tobytes() for r in v]
    out = []
    for a, b, c in np.asarray(idx, np.int64).reshape(-1, 3):
        tri = (rec[a], rec[b], rec[c])
        out.append(min(tri, tri[1:] + tri[:1], tri[2:] + tri[:2]))
    return sorted(out)


def steep_plane(program_module):
    """PLANE(3, 0, 0, -0.3) SPHERE(0.6) INTERSECT over [-1, 1]^3: a plane of slope 3, so L = 1 is a broken promise and L = 3 is not."""
    return program_module.Program((-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)).plane(3.0, 0.0, 0.0, -0.3).sphere(0.6).intersect()


def tiny_sphere(program_module):
    """A sphere of radius 0.07 at (0.3, -0.2, -0.1): four bricks and no vertex at 16 cells, 24 active cells at 32."""
    P = program_module.Program((-1.0, -1.0, -1.0, 1.0, 1.0, 1.0))
    return P.push_affine(program_module.translation(0.3, -0.2, -0.1)).sphere(0.07).pop()


# (program, cells) for which the promise is tested: L = 1 and the program's own box, but for the two stated below
PROMISE = [(name, n) for name in ("single", "anchor", "no_material", "all_ops", "deep", "sixteen", "ties") for n in (8, 16, 32)] + \
          [("single", 64), ("tiny", 16), ("tiny", 32)]
# deep: its POP_SCALE(0.75) rescales the box on top of the value stack only, so the sphere pushed under it keeps the factor 1.25
# of its own POP_SCALE over coordinates stretched by 1 / (0.75 * 1.25): a slope of 4/3 (with L = 1, 9 of its 1245 active cells at
# 32 cells lie outside the bricks).
LIPSCHITZ = {"deep": 1.34}
# ties: its spheres of radius 0.25 about (+-0.5, +-0.5, 0) pass exactly through lattice points of [-1, 1]^3 at every power-of-two
# size, and the dense restatement refuses lattices with exact zeros; over this box it has none.
BOX = {"ties": (-1.0, -1.0, -1.0, 1.03, 1.02, 1.01)}
MATERIALS = ("all_ops", "deep", "ties")


def builder(program_module, name):
    if name == "tiny":
        return tiny_sphere(program_module)
    if name == "steep":
        return steep_plane(program_module)
    return R.catalogue(program_module)[name]


def case(program_module, name):
    """-> (builder, box, L, materials) of a PROMISE program."""
    b = builder(program_module, name)
    return b, BOX.get(name, tuple(b.bb)), LIPSCHITZ.get(name, 1.0), name in MATERIALS
