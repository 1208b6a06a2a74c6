"""Shared by the tests of meshing a sampled lattice (include/sdfgrid.h, "Meshing a sampled lattice"): what is particular to a
caller's lattice in the restatement of mesh extraction -- the distances are GIVEN, the normals are the lattice's own
(mesh_ref.lattice_normals), the material fields zero -- and two lattices to mesh.  The extraction itself, lattice_points and
the normals live in tests/mesh_ref.py."""
import numpy as np

import mesh_ref as MR

F = np.float32
DUAL = MR.DUAL
bits = MR.bits


def extract(d, bb, algorithm=0, zeros_ok=False):
    """What sdfv_lattice_mesh_extract leaves for the lattice d [k, j, i] over bb -> mesh_ref.extract's (vertices, indices, info)."""
    return MR.extract(d, bb, algorithm, lambda p: MR.lattice_normals(d, bb, p), zeros_ok=zeros_ok)


def sphere_lattice(n, bb, radius=0.6):
    """d [k, j, i]: the exact distance to a sphere about the origin, rounded to float32, at the lattice points."""
    p = MR.lattice_points(n, bb).astype(np.float64)
    return (np.linalg.norm(p, axis=1) - radius).astype(F).reshape(n + 1, n + 1, n + 1)


def gyroid_lattice(n, bb, scale=4.0, level=0.1):
    """sin x cos y + sin y cos z + sin z cos x - level at `scale` times the lattice points: a surface that cuts every face of the box."""
    p = MR.lattice_points(n, bb).astype(np.float64) * scale
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    g = np.sin(x) * np.cos(y) + np.sin(y) * np.cos(z) + np.sin(z) * np.cos(x) - level
    return g.astype(F).reshape(n + 1, n + 1, n + 1)
