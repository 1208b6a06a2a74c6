"""Shared by tests/test_program_cast_cpu.py and tests/test_gpu_program_cast.py: a vectorised numpy float32 restatement of the ray
cast over SDF programs (include/sdfgrid.h, sdfv_program_cast_desc), written from the header's per-ray text; it sits on
tests/program_ref.run for the program's value and on tests/program_mesh_ref.normals for normal(p, eps) and calls nothing of the
library.  Every arithmetic step is one float32 numpy operation over the ray array, in the header's order, with a Python loop
over the steps.  Plus the ray sets and the programs the comparisons run on."""
import os
import sys

import numpy as np

import program_march_ref as M
import program_mesh_ref as PMR
import program_ref as R

F = np.float32
RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("t_min", "<f4"), ("dir", "<f4", (3,)), ("t_max", "<f4")])
HIT_DTYPE = np.dtype([("status", "<i4"), ("steps", "<i4"), ("t", "<f4"), ("pos", "<f4", (3,)), ("normal", "<f4", (3,)),
                      ("sample", "<f4", (7,))])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 64
NORMALS, MATERIALS = 1, 2
N_RAYS = 2000


@np.errstate(all="ignore")
def cast(ops, box, rays, flags=NORMALS | MATERIALS, max_steps=0, hit_eps=0.0, normal_eps=0.0):
    """ops: program_ref's [(opcode, operands)]; box: 6 floats; rays: [n, 8] float32 -> HIT_DTYPE array [n]."""
    r = np.ascontiguousarray(rays, F).reshape(-1, 8)
    n = len(r)
    max_steps = int(max_steps) if max_steps else 256
    hit_eps = F(hit_eps) if hit_eps else F(1e-5)
    normal_eps = F(normal_eps) if normal_eps else F(0.001)
    lo, hi = [F(v) for v in box[:3]], [F(v) for v in box[3:]]
    o = [r[:, a].copy() for a in range(3)]
    t_min, t_max = r[:, 3].copy(), r[:, 7].copy()
    d = [r[:, 4 + a].copy() for a in range(3)]
    l = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    u = [v / l for v in d]
    a1 = [(lo[a] - o[a]) / u[a] for a in range(3)]
    a2 = [(hi[a] - o[a]) / u[a] for a in range(3)]
    tnear = np.fmax(np.fmax(np.fmin(a1[0], a2[0]), np.fmin(a1[1], a2[1])), np.fmin(a1[2], a2[2]))
    tfar = np.fmin(np.fmin(np.fmax(a1[0], a2[0]), np.fmax(a1[1], a2[1])), np.fmax(a1[2], a2[2]))
    t0, t1 = np.fmax(t_min, tnear), np.fmin(t_max, tfar)
    crosses = (t1 >= t0) & (tfar >= tnear)

    t = t0.copy()
    status = np.where(crosses, -1, 0).astype(np.int32)
    steps = np.zeros(n, np.int32)
    pos = [np.zeros(n, F) for _ in range(3)]
    dist = np.zeros(n, F)
    marching = crosses.copy()
    for _ in range(max_steps):
        idx = np.flatnonzero(marching)
        if idx.size == 0:
            break
        p = [o[a][idx] + u[a][idx] * t[idx] for a in range(3)]
        v = R.run(ops, np.stack(p, axis=1), distance_only=True)[:, 0]
        for a in range(3):
            pos[a][idx] = p[a]
        dist[idx] = v
        steps[idx] += 1
        hit = v < hit_eps
        status[idx[hit]] = 1
        marching[idx[hit]] = False
        go = idx[~hit]
        t[go] = t[go] + v[~hit]
        left = t[go] > t1[go]
        status[go[left]] = -2
        marching[go[left]] = False

    out = np.zeros(n, HIT_DTYPE)
    out["status"], out["steps"] = status, steps
    out["t"] = np.where(crosses, t, F(0))
    for a in range(3):
        out["pos"][:, a] = pos[a]
    h = np.flatnonzero(status == 1)
    if h.size:
        p = np.stack([pos[a][h] for a in range(3)], axis=1)
        if flags & MATERIALS:
            out["sample"][h] = R.run(ops, p, distance_only=False)
        else:
            out["sample"][h, 0] = dist[h]
        if flags & NORMALS:
            out["normal"][h] = PMR.normals(ops, p, float(normal_eps))
    return out


# ---- the ray sets ----
def rays(seed, box, n=N_RAYS):
    """n seeded rays against `box` (6 floats), every kind in every set, shuffled so that a wave holds several kinds: aimed at the
    box from outside, started inside it (inside the solid, for most programs, some of them), parallel to a box face (a zero
    direction component), skimming just above the box's lower y face shrunk by 0.05 (where the grazed plane of
    program_march_ref.GRAZE lies), missing the box, with [t_min, t_max] windows that end before the box's middle and begin
    behind it, and the rays nothing can be computed for: a zero direction, a NaN origin, a NaN direction.  Directions are not
    normalised.  No origin lies exactly on a face of the box (C leaves the sign of fmaxf(+0, -0) open)."""
    rng = np.random.default_rng([20261021, int(seed)])
    lo, hi = np.array(box[:3], np.float64), np.array(box[3:], np.float64)
    c, half = (lo + hi) / 2, (hi - lo) / 2
    r = np.zeros((n, 8), np.float64)
    kind = rng.integers(0, 8, n)
    kind[:8] = np.arange(8)                              # every kind at least once
    unit = rng.normal(size=(n, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    inside = c + rng.uniform(-0.98, 0.98, (n, 3)) * half
    outside = c + unit * rng.uniform(2.5, 4.0, (n, 1)) * np.linalg.norm(half)
    scale = rng.uniform(0.25, 4.0, (n, 1))               # the direction's length
    r[:, 3], r[:, 7] = 0.0, 100.0
    # 0: aimed at the box from outside
    r[:, :3] = outside
    r[:, 4:7] = (inside - outside) * scale / np.linalg.norm(inside - outside, axis=1, keepdims=True)
    # 1: from inside the box, any direction
    k = kind == 1
    r[k, :3] = inside[k]
    r[k, 4:7] = (unit * scale)[k]
    # 2: parallel to a box face: one direction component is zero (the origin inside or outside the slab of that axis)
    k = np.flatnonzero(kind == 2)
    axis = rng.integers(0, 3, len(k))
    r[k, 4 + axis] = 0.0
    r[k, axis] = np.where(rng.random(len(k)) < 0.7, inside[k, axis], r[k, axis])
    # 3: skimming: parallel to the y faces, a hair above y = lo.y + 0.05, started inside the box
    k = np.flatnonzero(kind == 3)
    r[k, :3] = inside[k]
    r[k, 1] = lo[1] + 0.05 + 10.0 ** rng.uniform(-4.7, -3.0, len(k))
    r[k, 4:7] = (unit * scale)[k]
    r[k, 5] = 0.0
    # 4: missing the box: from outside, turned away from it
    k = kind == 4
    r[k, 4:7] = (unit * scale)[k]
    r[k, 4:7] = np.where(((r[k, 4:7] * (c - r[k, :3])).sum(axis=1) > 0)[:, None], -r[k, 4:7], r[k, 4:7])
    # 5: a window that ends early: t_max between the box's near face and its middle
    k = kind == 5
    reach = np.linalg.norm(c - outside, axis=1)
    r[k, 7] = (reach - rng.uniform(0.2, 1.0, n) * np.linalg.norm(half))[k]
    # 6: a window that begins late: t_min behind the box's middle
    k = kind == 6
    r[k, 3] = (reach + rng.uniform(0.0, 0.8, n) * np.linalg.norm(half))[k]
    # 7: nothing to compute: a zero direction, a NaN origin, a NaN direction, an infinite origin
    k = np.flatnonzero(kind == 7)
    sub = np.arange(len(k)) % 4
    r[k[sub == 0], 4:7] = 0.0
    r[k[sub == 1], :3] = np.nan
    r[k[sub == 2], 4:7] = np.nan
    r[k[sub == 3], :3] = np.inf
    out = r.astype(F)
    assert not ((out[:, :3] == F(lo)) | (out[:, :3] == F(hi))).any()
    return out


def as_rays(a):
    """[n, 8] float32 -> RAY_DTYPE view."""
    return np.ascontiguousarray(a, F).view(RAY_DTYPE).reshape(-1)


def assert_hits_bitwise(got, want, what):
    """Every byte of every record."""
    g = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 16)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 16)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, (what, len(bad), bad[:3].tolist(), [(np.ascontiguousarray(got).view(HIT_DTYPE).reshape(-1)[b],
                                                              np.ascontiguousarray(want).view(HIT_DTYPE).reshape(-1)[b]) for b in bad[:2]])


# ---- the programs: the march catalogue with its boxes (program_march_ref.SCENES, GRAZE among them), and the three models the
# benchmarks time, under the names they have there ----
def spheres8(PM):
    sys.path.insert(0, os.path.join(M.ROOT, "tools"))
    from program_mesh_bench import spheres8 as make
    return make(PM)


def bench_builders(PM):
    """name -> (builder, box): demo3, spheres8, example_sixteen (no surface in its box: a list of misses)."""
    unit = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
    return {"demo3": (PM.Program().cube(0.95).sphere(1.05).subtract(), unit), "spheres8": (spheres8(PM), unit),
            "example_sixteen": (PM.example_sixteen(), unit)}


def scene_box(name):
    lo, hi = M.SCENES[name][:2]
    return tuple(lo) + tuple(hi)
