"""Shared by the tests of meshing the demo tree (sdfv_mesh_extract): what is particular to the demo in the restatement of mesh
extraction -- the lattice's distances (HermiteSource / ScalarSource at the unit-cube lattice points) and the normals, both from
the oracle (tests/oracle_binding.py: source_scalar_many, normal_many).  The extraction itself is tests/mesh_ref.py's; the
vertices' material fields stay Vertex::default()."""
import numpy as np

import mesh_ref as MR

F = np.float32


def demo_lattice(oracle, oprm, n, box, sdf_id=0):
    """box = (min.xyz, max.xyz) -> d [k, j, i]: the oracle's distance at the unit points (float)i / (float)n of the box."""
    ax = np.arange(n + 1, dtype=F) / F(n)
    zz, yy, xx = np.meshgrid(ax, ax, ax, indexing="ij")
    pts = np.stack([xx, yy, zz], axis=-1).reshape(-1, 3)
    return oracle.source_scalar_many(oprm, pts, box[0], box[1], sdf_id).reshape(n + 1, n + 1, n + 1)


def extract_demo(oracle, oprm, n, box, sdf_id=0, algorithm=0):
    """What sdfv_mesh_extract leaves for the demo tree -> mesh_ref.extract's (vertices, indices, info)."""
    return MR.extract(demo_lattice(oracle, oprm, n, box, sdf_id), tuple(box[0]) + tuple(box[1]), algorithm,
                      lambda p: oracle.normal_many(oprm, p, 0.0, sdf_id))
