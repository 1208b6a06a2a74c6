"""Seeded numpy generators of (tex0, tex1) texture pairs for the grid march, and the tables of grids and cameras the march is
rendered with over them (tests/test_march_fields_cpu.py asserts on the oracle alone that each table entry reaches what it is
there for; tests/test_gpu_raymarch_fields.py runs the same entries through every kernel variant).

Every generator takes (dims, bb_min, bb_max, seed), dims = (W, H, D), and returns two float32 [D, H, W, 4] arrays in the
fills' own layout: tex0.r = distance + 0.1, tex0.gba = albedo, tex1 = (metallic, roughness, occlusion, spare) -- the seven
material channels in [0, 1].  Texel (i, j, k) stands at the position the LINEAR sampler gives it, the texel centre
bb_min + (i + 0.5) / n * size, so that the filtered field inside the box is the trilinear interpolant of the formula.

Every value is finite and |tex0.r| <= 1e4.  Non-finite texels are OUT OF SCOPE: what the march does over a NaN or an infinite
distance is not specified anywhere (include/sdfgrid.h has no rule for it) and nothing here feeds it one."""
import numpy as np

F = np.float32

# name -> (dims, bb_min, bb_max): the smallest grids that reach each path of the march kernels
GRIDS = {
    "cube32": ((32, 32, 32), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)),        # hand-written loop, interior fetch (cubic, power of two)
    "box16x32x64": ((16, 32, 64), (-0.5, -1.0, -2.0), (0.5, 1.0, 2.0)),   # hand-written loop through the border fetch only
    "flat8x2x8": ((8, 2, 8), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)),        # a two-texel axis
    "odd20x34x27": ((20, 34, 27), (-1.0, -0.5, -1.0), (1.0, 1.0, 0.75)),  # general / divide variants; H even: interleaved volume
}
IMAGE = (96, 72)
LATTICE_IMAGE = (95, 71)  # odd: the centre row and the centre column hold rays with one direction component exactly 0
SEEDS = {"slow": 11, "steep": 12, "noise": 13, "lattice_x": 14, "lattice_y": 15, "lattice_z": 16, "crossing": 17}


def _geometry(dims, bb_min, bb_max):
    lo, hi = np.array(bb_min, np.float64), np.array(bb_max, np.float64)
    return lo, hi, (lo + hi) / 2, (hi - lo) / 2


def texel_positions(dims, bb_min, bb_max):
    """x, y, z [D, H, W] float64: the texel centres of the sampler."""
    lo, hi, _, _ = _geometry(dims, bb_min, bb_max)
    axes = [lo[a] + (np.arange(dims[a]) + 0.5) / dims[a] * (hi[a] - lo[a]) for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return x, y, z


def _smooth_materials(x, y, z, half, seed):
    """Seven channels in [0, 1] that vary smoothly (and differently) along every axis."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(7):
        k = rng.uniform(1.0, 4.0, size=3) / half
        ph = rng.uniform(0.0, 2 * np.pi)
        out.append(0.5 + 0.5 * np.sin(k[0] * x + k[1] * y + k[2] * z + ph))
    return out


def _assemble(dist, mats):
    t0 = np.stack([0.1 + dist] + list(mats[:3]), axis=-1).astype(F)
    t1 = np.stack(list(mats[3:7]), axis=-1).astype(F)
    for t in (t0[..., 1:], t1):
        np.clip(t, 0.0, 1.0, out=t)
    assert np.isfinite(t0).all() and np.isfinite(t1).all() and np.abs(t0[..., 0]).max() <= 1e4
    return np.ascontiguousarray(t0), np.ascontiguousarray(t1)


SLOW_RADIUS = 1.02
OFF_CENTRE = np.array([0.013, 0.007, -0.011])  # of the shortest half-extent: no texel pair mirrors another (a normal whose four
                                               # taps read equal values is 0 / 0)


def slow(dims, bb_min, bb_max, seed):
    """The exact distance to a sphere that just pokes through the nearest faces, times 1/64: rays crawl and run out of steps
    (a ray arrives within 254 steps only from 0.035 away)."""
    _, _, c, h = _geometry(dims, bb_min, bb_max)
    c = c + OFF_CENTRE * h.min()
    x, y, z = texel_positions(dims, bb_min, bb_max)
    d = (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - SLOW_RADIUS * h.min()) / 64.0
    return _assemble(d, _smooth_materials(x, y, z, h, seed))


def steep(dims, bb_min, bb_max, seed):
    """A gyroid whose value is four times (about) its distance: not 1-Lipschitz, the march overshoots into the solid."""
    _, _, c, h = _geometry(dims, bb_min, bb_max)
    x, y, z = texel_positions(dims, bb_min, bb_max)
    k = 2 * np.pi * 1.25 / h.max()
    qx, qy, qz = k * (x - c[0]), k * (y - c[1]), k * (z - c[2])
    g = np.sin(qx) * np.cos(qy) + np.sin(qy) * np.cos(qz) + np.sin(qz) * np.cos(qx)
    d = 4.0 * (g + 0.55) / (1.2 * k)
    return _assemble(d, _smooth_materials(x, y, z, h, seed))


def noise(dims, bb_min, bb_max, seed):
    """tex0.r uniform in [0.1 - 0.02, 0.1 + 0.25], every other channel uniform in [0, 1], texel by texel."""
    rng = np.random.default_rng(seed)
    shape = (dims[2], dims[1], dims[0], 4)
    t0 = rng.uniform(0.0, 1.0, size=shape).astype(F)
    t1 = rng.uniform(0.0, 1.0, size=shape).astype(F)
    t0[..., 0] = rng.uniform(0.1 - 0.02, 0.1 + 0.25, size=shape[:3]).astype(F)
    return t0, t1


def lattice_plane_index(n):
    return (n - 1) // 2


def lattice(axis):
    """-> generator: tex0.r - 0.1 is the signed distance to the plane through the centres of texel layer (n - 1) // 2 of `axis`."""
    def gen(dims, bb_min, bb_max, seed):
        lo, hi, _, h = _geometry(dims, bb_min, bb_max)
        pos = texel_positions(dims, bb_min, bb_max)
        n = dims[axis]
        plane = lo[axis] + (lattice_plane_index(n) + 0.5) / n * (hi[axis] - lo[axis])
        return _assemble(pos[axis] - plane, _smooth_materials(*pos, h, seed))
    gen.__name__ = "lattice_" + "xyz"[axis]
    return gen


def crossing(dims, bb_min, bb_max, seed):
    """Solid outside a sphere of 1.45 half-extents (the box's corners, but not the middle of its edges: the surface crosses
    all six faces) plus a thin slab across the box (normal to x, holding one texel layer of every grid); the materials vary along both."""
    _, _, c, h = _geometry(dims, bb_min, bb_max)
    c = c + OFF_CENTRE * h.min()
    x, y, z = texel_positions(dims, bb_min, bb_max)
    qx, qy, qz = (x - c[0]) / h[0], (y - c[1]) / h[1], (z - c[2]) / h[2]
    d = h.min() * np.minimum(1.45 - np.sqrt(qx * qx + qy * qy + qz * qz), np.abs(qx - 0.15) - 0.06)
    return _assemble(d, _smooth_materials(x, y, z, h, seed))


FIELDS = {"slow": slow, "steep": steep, "noise": noise, "lattice_x": lattice(0), "lattice_y": lattice(1),
          "lattice_z": lattice(2), "crossing": crossing}
PROGRAM_FIELDS = ("envelope", "deep")  # filled on the device by CompiledProgram.fill_grid
# `deep` is a few blobs well inside the unit box: the fill's two voxel layers of flat8x2x8 stand on the faces y = +-1, where it
# has no solid (smallest distance 0.237) -- no ray over that grid can hit, so that pair is not run.
PROGRAM_ENTRIES = [(n, g) for n in PROGRAM_FIELDS for g in GRIDS if (n, g) != ("deep", "flat8x2x8")]
ENVELOPE_X = 0.15  # (see envelope_cameras)

# The NEAREST path (sdfLODDistBetweenSamples = lod > 1) over `noise` / cube32.  sdfNormal's taps stand h = lod / (N * sqrt(3)) to
# either side of the hit on every axis, 1 / sqrt(3) = 0.577 of a coarse cell apart: a pair snaps to the same coarse texel with
# probability 1 - 0.577 = 0.423 per axis, all four taps read ONE texel -- a zero sum, a NaN normal -- at 0.423^3 = 7.6 % of
# uniformly placed points, whatever the lod.  Hits are not placed uniformly within a cell, so the cap is twice that; and the
# three cameras must leave at least 1000 hits with a finite normal per lod (twice `noise`'s 500-hit condition).
LODS = (2.0, 4.0)
LOD_NAN_CAP = 0.15
LOD_FINITE_HITS = 1000


def make(field, grid):
    dims, lo, hi = GRIDS[grid]
    return FIELDS[field](dims, lo, hi, SEEDS[field])


def fill_program(pkg, PM, name, g):
    """`name` of program_march_ref.builders, filled into a fresh texture pair of grid `g` on the device."""
    import program_march_ref
    prog = program_march_ref.builders(PM)[name].build()
    t0, t1 = pkg.alloc_textures(g)
    prog.fill_grid(g, t0, t1)
    return t0, t1


def program_textures(pkg, PM, name, grid):
    """What that fill writes, from the numpy restatement of the programs (tests/program_ref.py) and of the fills' packing:
    the CPU tests choose and check the program grids' cameras on it; tests/test_gpu_program.py holds the device fill to it."""
    import program_march_ref as M
    import program_ref as R
    dims, lo, hi = GRIDS[grid]
    rec = R.run(M.builders(PM)[name].ops, R.grid_positions(dims, lo, hi))
    t0, t1 = M.pack(rec, M.srgb_table(), F(pkg.lib.sdfv_air_dist()), False)
    shape = (dims[2], dims[1], dims[0], 4)
    return np.ascontiguousarray(t0.reshape(shape)), np.ascontiguousarray(t1.reshape(shape))


# ---- cameras ------------------------------------------------------------------------------------------------------------
def texel_u(x, n, lo, hi):
    """The sampler's float32 texel coordinate of a float32 world coordinate, operation by operation as material.frag's
    restatements take them: ((x - min) / (max - min)) * n - 0.5."""
    x, lo, hi = F(x), F(lo), F(hi)
    return ((x - lo) / (hi - lo)) * F(n) - F(0.5)


def exact_centre(n, lo, hi, i):
    """A float32 coordinate whose float32 texel coordinate is exactly the integer i (interpolation weight exactly 0.0): the
    centre of texel i, or a float32 neighbour of it where the box is not a power of two."""
    x0 = F(lo + (i + 0.5) / n * (hi - lo))
    cands = [x0]
    up = down = x0
    for _ in range(16):
        up, down = np.nextafter(up, F(np.inf)), np.nextafter(down, F(-np.inf))
        cands += [up, down]
    for x in cands:
        if texel_u(x, n, lo, hi) == F(i):
            return float(x)
    raise AssertionError((n, lo, hi, i))


def _axis_up(v):
    return (0.0, 0.0, 1.0) if v == 1 else (0.0, 1.0, 0.0)


def lattice_cameras(axis, grid):
    """Axis-aligned cameras for lattice(axis): they look along the two OTHER axes (rays on the plane's far side leave the box,
    the others meet it), two from outside and one from inside the box.  The eye stands on texel centres in both transverse
    coordinates, so every ray of the image's centre column and centre row keeps one texel coordinate an exact integer.
    What this reaches: a weight of exactly 0.0 -- the lowest value of the cache test "the weight read as an unsigned integer is
    below 0x3f800000" -- held over a whole march on an axis ACROSS the ray, while the other two axes change cell.  What it does
    not reach: a ray that lands on a cell boundary ALONG its march (a weight of exactly 1.0 in the cached cell).  The shader
    starts a ray on a face of the box (u = -0.5) or 0.2 * dir from the eye, and its direction is a normalised float32 vector:
    only the one centre pixel of an odd image marches exactly along an axis, and the texel value 0.1 + k * pitch, rounded, less
    0.1 is not exactly k * pitch either."""
    dims, lo, hi = GRIDS[grid]
    _, _, c, h = _geometry(dims, lo, hi)
    cams = []
    for v, inside in (((axis + 1) % 3, False), ((axis + 2) % 3, False), ((axis + 1) % 3, True)):
        w = 3 - axis - v
        eye = [0.0, 0.0, 0.0]
        eye[axis] = exact_centre(dims[axis], lo[axis], hi[axis], min(lattice_plane_index(dims[axis]) + 2, dims[axis] - 1))
        eye[w] = exact_centre(dims[w], lo[w], hi[w], dims[w] // 2)
        eye[v] = float(c[v] + 0.9 * h[v]) if inside else float(c[v] + h[v] + 1.0 * h.max())
        target = list(eye)
        target[v] = float(c[v] - h[v])
        cams.append(dict(eye=tuple(eye), target=tuple(target), up=_axis_up(v), fovy_degrees=90.0 if inside else 45.0))
    return cams


def envelope_cameras(grid):
    """Over these boxes `envelope` (a union of planes that depends on x alone) is solid everywhere: every ray that samples hits
    on its first sample, and a ray leaves the box (status -2, no sample) only where its chord through the box is shorter than
    the 0.2 the shader steps in before it marches.  The fill clamps tex0.r to [0, 1], so the field is flat -- four equal normal
    taps, 0 / 0 -- outside x in about [-0.04, 0.29] (the narrowest, flat8x2x8's).  The cameras therefore stand close to the
    upper front edge of the box around x = ENVELOPE_X and look up at it from below: they see the faces next to the edge within
    that x range, and the short chords across the edge."""
    dims, lo, hi = GRIDS[grid]
    x, top, front = ENVELOPE_X, hi[1], hi[2]
    outside = dict(eye=(x + 0.02, top - 0.15, front + 0.3), target=(x, top - 0.06, front), fovy_degrees=20.0)
    inside = dict(eye=(x, top - 0.18, front - 0.18), target=(x, top + 0.5, front + 0.5), fovy_degrees=50.0)
    axis = dict(eye=(x, top - 0.1, front + 0.25), target=(x, top - 0.1, front - 1.0), fovy_degrees=34.0)
    return [outside, inside, axis]


def cameras(field, grid):
    """[outside, inside, axis-aligned] camera keywords (pkg.camera_look_at's) for a field over a grid."""
    if field.startswith("lattice_"):
        return lattice_cameras("xyz".index(field[-1]), grid)
    if field == "envelope":
        return envelope_cameras(grid)
    dims, lo, hi = GRIDS[grid]
    _, _, c, h = _geometry(dims, lo, hi)
    v = int(np.flatnonzero(h == h.min())[-1])  # the axis-aligned camera looks along the box's shortest axis (z for a cube)
    if field == "deep":  # (along z: the narrow box cuts a blob more than 0.1 deep at its x face -- clamped flat, a NaN normal)
        v = 2
    outside = dict(eye=tuple(float(x) for x in c + h * np.array([1.7, 1.45, 2.05])), target=tuple(float(x) for x in c))
    inside = dict(eye=tuple(float(x) for x in c + h * np.array([0.3, 0.35, -0.4])),
                  target=tuple(float(x) for x in c + h * np.array([-1.0, -0.5, 1.2])), fovy_degrees=70.0)
    eye = c.copy()
    eye[v] += h[v] + 1.75 * h.max()
    axis = dict(eye=tuple(float(x) for x in eye), target=tuple(float(x) for x in c), up=_axis_up(v))
    if field == "slow":  # from inside: just off the sphere, looking along it (rays into it, past it, and out of the box)
        n, t = np.array([1.0, 1.0, -1.0]) / np.sqrt(3.0), np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
        e = c + (SLOW_RADIUS * h.min() + 0.03) * n
        inside = dict(eye=tuple(float(x) for x in e), target=tuple(float(x) for x in e - n + 1.2 * t), fovy_degrees=90.0)
    return [outside, inside, axis]


def rgba8_cameras():
    """Twelve views of cube32 from around it, alternately from above and below: together they show over a thousand colours of
    `noise` (one view has a few hundred hits)."""
    cams = []
    for k in range(12):
        a = 2 * np.pi * (k + 0.25) / 12
        cams.append(dict(eye=(float(2.1 * np.cos(a)), 1.1 if k % 2 else -0.9, float(2.1 * np.sin(a))), fovy_degrees=60.0))
    return cams


def image_of(field):
    return LATTICE_IMAGE if field.startswith("lattice_") else IMAGE


def oracle_camera(oracle, cam_kw, aspect):
    kw = dict(cam_kw)
    return oracle.camera_look_at(eye=kw.get("eye", (2.5, 3.0, 5.0)), target=kw.get("target", (0, 0, 0)), up=kw.get("up", (0, 1, 0)),
                                 fovy=kw.get("fovy_degrees", 45.0), aspect=aspect, near=kw.get("z_near", 0.1), far=kw.get("z_far", 1000.0))
