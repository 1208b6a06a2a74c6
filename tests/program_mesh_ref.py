"""Shared by the tests of meshing over SDF programs: what is particular to a program in the numpy float32 restatement of the
mesh pipeline, written from include/sdfgrid.h ("SDF programs: meshing") and calling nothing of the library.  The extraction
itself -- crossing edges, triangles, dual contouring's solve, the closedness checks, mc_table, bits -- is tests/mesh_ref.py's.

* lattice distances: tests/program_ref.run(ops, pts, True) at u * size + min, u = (float)i / (float)cells;
* normals: normal_default_impl, the four taps and the sums in the header's order, one float32 operation per step;
* materials: columns 1..6 of run(ops, positions, False), on the output vertices;
* postproc: the same columns; the normal recomputed only where |n|^2 < 1e-4.
Every arithmetic step is one numpy float32 operation on float32 operands."""
import functools

import numpy as np

import mesh_ref as MR
import program_ref as R

F = np.float32
DUAL = MR.DUAL
bits = MR.bits


def lattice(ops, n, bb):
    """(unit: [n + 1] lattice coordinates, d: [k, j, i] distances) of the n-cell lattice over bb = min.xyz + max.xyz."""
    d = R.run(ops, MR.lattice_points(n, bb), True)[:, 0].reshape(n + 1, n + 1, n + 1)
    return MR.axes_of(n, bb)[0][0], d


@np.errstate(all="ignore")
def normals(ops, p, eps=0.0):
    """normal_default_impl at p [m, 3] -> [m, 3] float32."""
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    e = F(eps) if eps > 0 else F(0.001)
    me = F(-1.0) * e
    x, y, z = p[:, 0], p[:, 1], p[:, 2]

    def dist(ox, oy, oz):
        return R.run(ops, np.stack([x + ox, y + oy, z + oz], axis=-1), True)[:, 0]

    d1, d2, d3, d4 = dist(e, me, me), dist(me, e, me), dist(me, me, e), dist(e, e, e)
    vx = d1 + -d2 + -d3 + d4
    vy = -d1 + d2 + -d3 + d4
    vz = -d1 + -d2 + d3 + d4
    inv = F(1.0) / np.sqrt(vx * vx + vy * vy + vz * vz)
    return np.stack([vx * inv, vy * inv, vz * inv], axis=-1).astype(F)


def extract(ops, n, bb, materials=False, algorithm=0, zeros_ok=False):
    """What sdfv_program_mesh_extract leaves for n cells over bb -> mesh_ref.extract's (vertices, indices, info)."""
    return MR.extract(lattice(ops, n, bb)[1], bb, algorithm, lambda p: normals(ops, p),
                      (lambda p: R.run(ops, p, False)[:, 1:7]) if materials else None, zeros_ok=zeros_ok)


def postproc(ops, vertices):
    """Mesh::postproc of [m, 12] vertices -> a new array."""
    v = np.array(vertices, F, copy=True)
    if len(v) == 0:
        return v
    nx, ny, nz = v[:, 3] - F(0), v[:, 4] - F(0), v[:, 5] - F(0)
    unset = nx * nx + ny * ny + nz * nz < F(0.0001)
    if unset.any():
        v[unset, 3:6] = normals(ops, v[unset, :3])
    v[:, 6:] = R.run(ops, v[:, :3], False)[:, 1:7]
    return v


@functools.lru_cache(maxsize=None)
def primitive(kind, size):
    """ops of a one-instruction program: ("cube" | "sphere", size)."""
    return ((R.CUBE if kind == "cube" else R.SPHERE, (float(size),)),)
