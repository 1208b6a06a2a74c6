"""An independent float64 reference for the GRID route of the demo: what the demo fill, the texel lattice, the camera, the
sphere-trace over the trilinear texture and the shading tail MEAN, written from the definitions -- the solids as point sets,
the textbook look-at and GL perspective, the sRGB and tone-mapping formulas -- and not from csrc/, oracle/ or
tests/golden/make_golden.py.  It calls nothing of the library.  The shape follows tests/program_geometry.py, whose error-bound
arithmetic `B` (value of the specified f32 sequence in float64 + a forward bound on the f32 result's error, U = 2^-24 per
operation) it shares.

* `evaluate(prm, points, sdf_id)`: the demo family (0 demo = cube minus sphere, 1 cube, 2 sphere) -> distance, derived bound
  (doubled for the second-order terms), the sample's colour and properties, the two packed texels, and `decided`: false
  wherever a decision of the definition lies within the bound of its threshold.
* `lattice`, `phi`: voxel i of n holds the content of position min + i / (n - 1) * size, but a LINEAR texture fetch places
  texel i at min + (i + 1/2) / n * size.  The field a march sees at p is therefore the lattice interpolant of the SDF at
  phi(p) = c + (p - c) n / (n - 1) per axis (c the box centre), clamped to the box by MirroredRepeat: n / (n - 1)-Lipschitz.
* `camera`, `pixel_rays`, `march_start`: right-handed look-at, GL perspective, the 0.5 bias; the ray through the CENTRE of
  pixel (x, y), row 0 at the top; the shader's start rule.
* `solid_windows` / `first_entry`: closed-form ray entry into {d o phi <= -delta} and {d o phi <= +delta}: phi is affine, so
  the ray stays a line; a box of half side `side -+ delta`, a ball of radius `r +- delta`, the demo an interval difference.
* `cell_bounds`: how far the trilinear interpolant of a hit's cell can lie from d o phi, per hit.
* `shade`, `depth_of`, `unorm8`: the shading tail in float64 with its bound.
* `check_records`: statements C1 .. C7 over one frame of march records, each returning what it found wrong.
"""
import numpy as np

from program_geometry import B, U, f32

T01 = f32(0.1)                                          # the offset the textures store the distance with
AIR_DIST = float(np.float32(0.1) + np.float32(0.001234))  # `1e-1 + 0.001234` evaluated in f32
BRICK_W, BRICK_H, CEMENT = 0.5, 0.25, 0.2
CEMENT_EDGE = CEMENT / 2.0 * BRICK_H                    # 0.025: the cement's half width
BRICK = ((150, 24, 10), 0.2, 0.8, 0.0)                  # colour (of 255), metallic, roughness, occlusion
CEMENT_MAT = ((56, 70, 60), 0.4, 0.5, 1.0)
BLEND = ((0.5, 0.6, 0.7), 0.5, 0.0, 0.0)
KIND_AIR, KIND_BRICK, KIND_CEMENT, KIND_NORMAL, KIND_BLEND = 0, 1, 2, 3, 4
# to_linear in f32: q / 255 (U), + 0.055 (U, constant U), / 1.055 (U, constant U) -> 5 U relative before the power, 2.4 times
# that after it = 12 U; the exponent's own rounding U moves the result by 2.4 U |ln x| <= 2.4 * 2.41 U = 5.8 U (x >= 0.0905);
# powf 1 ulp = 2 U: 19.8 U, doubled like every bound here.  Neighbouring 8-bit codes differ by 3e-4 relative at the least.
TO_LINEAR_REL = 40.0 * U


class Params:
    """The demo's parameters as the f32 the library stores (defaults: sdf/demo/*.rs)."""
    def __init__(self, cube_half_side=0.95, cube_material=0, sphere_radius=1.05, sphere_material=1,
                 max_distance_custom_material=0.05, disable_sphere=0):
        self.side, self.r, self.band = f32(cube_half_side), f32(sphere_radius), f32(max_distance_custom_material)
        self.cube_material, self.sphere_material, self.disable_sphere = int(cube_material), int(sphere_material), int(disable_sphere)

    def kw(self):
        return dict(cube_half_side=self.side, cube_material=self.cube_material, sphere_radius=self.r,
                    sphere_material=self.sphere_material, max_distance_custom_material=self.band, disable_sphere=self.disable_sphere)


def _k(v, like):
    """A compile-time f32 constant with its rounding error against the exact v."""
    r = f32(v)
    return B(np.full(like.v.shape, r), abs(r - float(v)))


def _exact(v, like):
    return B(np.full(like.v.shape, float(v)), 0.0)


class Sample:
    pass


def _brick(u, v):
    """The procedural brick wall at texture coordinate (u, v): rows of height 0.25, every row shifted by a quarter of its number,
    bricks 0.5 wide, cement within 0.025 of a brick's edge.  -> (is cement, decided)"""
    row = np.floor(v.v / BRICK_H)
    s = u + B(row / 4.0, 0.0)                          # the only rounded operation: v / 0.25, floor and / 4 are exact in f32
    bx, by = np.fmod(np.abs(s.v), BRICK_W), np.fmod(np.abs(v.v), BRICK_H)
    cement = (bx < CEMENT_EDGE) | (bx > BRICK_W - CEMENT_EDGE) | (by < CEMENT_EDGE) | (by > BRICK_H - CEMENT_EDGE)
    # the f32 thresholds: f32(0.2) / 2 * 0.25 (within U * 0.025 of 0.025) and W - that, H - that (one rounding each)
    mx = np.minimum(np.abs(bx - CEMENT_EDGE), np.abs(bx - (BRICK_W - CEMENT_EDGE)))
    my = np.minimum(np.abs(by - CEMENT_EDGE), np.abs(by - (BRICK_H - CEMENT_EDGE)))
    return cement, (mx > s.e + U * (BRICK_W + CEMENT_EDGE)) & (my > v.e + U * (BRICK_H + CEMENT_EDGE))


def _material(material, dist, nrm, nrm_decided, X, distance_only):
    """One primitive's sample: air beyond 0.1 (or when only the distance is asked for), else its material at the normal `nrm`
    (three B).  -> Sample(color [n, 3], color_err, props [n, 3], kind, decided)"""
    n = len(dist.v)
    s = Sample()
    air = np.full(n, True) if distance_only else dist.v > T01
    air_decided = np.full(n, True) if distance_only else np.abs(dist.v - T01) > dist.e
    a = [c.abs() for c in nrm]
    if material == 0:                                   # brick, mapped on the plane the normal points out of
        def gt(p, q):
            margin, e = np.abs(p.v - q.v), p.e + q.e
            return p.v > q.v, (margin > e) | (e == 0.0)
        xy, dxy = gt(a[0], a[1])
        xz, dxz = gt(a[0], a[2])
        yz, dyz = gt(a[1], a[2])
        plane = np.where(xy, np.where(xz, 0, 2), np.where(yz, 1, 2))   # 0: u, v = z, y;  1: z, x;  2: x, y
        tri_decided = dxy & np.where(xy, dxz, dyz) & nrm_decided
        pick = lambda i0, i1, i2: B(np.choose(plane, [X[i0].v, X[i1].v, X[i2].v]), np.choose(plane, [X[i0].e, X[i1].e, X[i2].e]))  # noqa: E731
        cement, edge_decided = _brick(pick(2, 2, 0), pick(1, 0, 1))
        col = np.where(cement[:, None], np.array([f32(c / 255.0) for c in CEMENT_MAT[0]]), np.array([f32(c / 255.0) for c in BRICK[0]]))
        props = np.where(cement[:, None], np.array([f32(c) for c in CEMENT_MAT[1:]]), np.array([f32(c) for c in BRICK[1:]]))
        s.color, s.color_err, s.props = col, np.zeros((n, 3)), props
        s.kind, mat_decided = np.where(cement, KIND_CEMENT, KIND_BRICK), tri_decided & edge_decided
    else:                                               # the `normal` material: |n_c| as the colour
        s.color, s.color_err = np.stack([c.v for c in a], axis=1), np.stack([c.e for c in a], axis=1)
        s.props, s.kind, mat_decided = np.zeros((n, 3)), np.full(n, KIND_NORMAL), nrm_decided
    s.color, s.color_err = np.where(air[:, None], 0.0, s.color), np.where(air[:, None], 0.0, s.color_err)
    s.props, s.kind = np.where(air[:, None], 0.0, s.props), np.where(air, KIND_AIR, s.kind)
    s.decided = air_decided & (air | mat_decided)
    return s


def _cube(prm, X):
    """max |p_i| - side, and the axis normals where |p_i| > side (the comparison is exact: its margin is the point's own error)"""
    side = _exact(prm.side, X[0])
    dist = X[0].abs().max(X[1].abs()).max(X[2].abs()) - side
    nrm = [B(np.where(np.abs(c.v) > prm.side, np.sign(c.v), 0.0), 0.0) for c in X]
    decided = np.all([(np.abs(np.abs(c.v) - prm.side) > c.e) | (c.e == 0.0) for c in X], axis=0)
    return dist, nrm, decided


def _sphere(prm, X):
    """|p| - r, and p / |p|"""
    length = (X[0] * X[0] + X[1] * X[1] + X[2] * X[2]).sqrt()
    inv = _exact(1.0, X[0]) / length
    return length - _exact(prm.r, X[0]), [c * inv for c in X], np.full(len(X[0].v), True)


def _quantise(c, ec, srgb_round):
    """trunc(255 c) -- or trunc(255 c + 0.5) -- as an 8-bit code.  A colour that is a known f32 (ec == 0) has ONE product in
    IEEE arithmetic, which is evaluated as such; a computed colour is undecided within its bound of a step."""
    v = 255.0 * c
    exact = ec == 0.0
    v = np.where(exact, np.float32(v).astype(np.float64), v)
    if srgb_round:
        v = np.where(exact, (np.float32(v) + np.float32(0.5)).astype(np.float64), v + 0.5)
    q = np.clip(np.trunc(v), 0.0, 255.0)
    # (colours are |.| or constants, never negative: 0 is no step that can be crossed from below)
    near = (np.abs(v - np.round(v)) <= 255.0 * ec + (3.0 if srgb_round else 2.0) * U * np.abs(v)) & (np.round(v) >= 1.0)
    return q, exact | ~near | (v >= 256.0)


def to_linear(c):
    """sRGB -> linear (IEC 61966-2-1), c in [0, 1]"""
    return np.where(c < 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def evaluate(prm, points, sdf_id=0, distance_only=False, point_err=0.0, srgb_round=False):
    """points [n, 3] float64 (f32 samples: pass them as they are, point_err 0; lattice points: the float64 positions with
    `point_err` [n, 3] = how far the f32 position may lie from them) -> Sample with d, bound [n], color / color_err [n, 3],
    props [n, 3] (metallic, roughness, occlusion), kind [n], tex0 / tex0_err / tex1 [n, 4], decided [n]."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pe = np.broadcast_to(np.asarray(point_err, dtype=np.float64), p.shape)
    X = [B(p[:, i], pe[:, i]) for i in range(3)]
    if sdf_id in (0, 1):
        box, nb, nb_decided = _cube(prm, X)
        sb = _material(prm.cube_material, box, nb, nb_decided, X, distance_only)
    if sdf_id == 2 or (sdf_id == 0 and not prm.disable_sphere):
        sph, ns, ns_decided = _sphere(prm, X)
        ss = _material(prm.sphere_material, sph, ns, ns_decided, X, distance_only)
    if sdf_id == 1 or (sdf_id == 0 and prm.disable_sphere):
        out, dist = sb, box
    elif sdf_id == 2:
        out, dist = ss, sph
    else:
        dist = box.max(sph.neg())
        inter = box.abs() - sph.abs()                  # < 0: the cube's surface is the nearer one
        use_box, gap = inter.v < 0.0, np.abs(inter.v)
        blend = gap <= prm.band
        decided = (np.abs(gap - prm.band) > inter.e) & (blend | ((gap > inter.e) & np.where(use_box, sb.decided, ss.decided)))
        out = Sample()
        w, b3 = use_box[:, None], blend[:, None]
        out.color = np.where(b3, np.array([f32(c) for c in BLEND[0]]), np.where(w, sb.color, ss.color))
        out.color_err = np.where(b3, 0.0, np.where(w, sb.color_err, ss.color_err))
        out.props = np.where(b3, np.array([f32(c) for c in BLEND[1:]]), np.where(w, sb.props, ss.props))
        out.kind = np.where(blend, KIND_BLEND, np.where(use_box, sb.kind, ss.kind))
        out.decided = decided        # (asked for the distance only, the demo still paints the blend: sdf/demo/mod.rs:62-70)
    out.d, out.bound = dist.v, 2.0 * dist.e
    # the texel pair
    shifted = T01 + out.d
    black = (out.color == 0.0).all(axis=1)
    col = np.where(black[:, None], 0.5, out.color)
    q, q_decided = _quantise(col, np.where(black[:, None], 0.0, out.color_err), srgb_round)
    lin = to_linear(q / 255.0)
    occ = np.where(out.props[:, 2] <= 0.0, 1.0, out.props[:, 2])
    out.tex0 = np.concatenate([np.clip(shifted, 0.0, 1.0)[:, None], lin], axis=1)
    out.tex0_err = np.concatenate([(out.bound + 2.0 * U * np.abs(shifted))[:, None], TO_LINEAR_REL * lin], axis=1)
    out.tex1 = np.stack([out.props[:, 0], out.props[:, 1], occ, np.full(len(p), AIR_DIST)], axis=1)
    out.texel_decided = out.decided & q_decided.all(axis=1)
    return out


def normals(prm, points, sdf_id=0):
    """The analytic normals: the axis normals where |p_i| > side, p / |p|, the demo's pick of the nearer surface with the
    sphere's negated (it is a cavity).  -> (n [n, 3], per-component bound [n, 3], decided [n])"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    X = [B(p[:, i], 0.0) for i in range(3)]
    box, nb, _ = _cube(prm, X)
    sph, ns, _ = _sphere(prm, X)
    stack = lambda n: (np.stack([c.v for c in n], axis=1), 2.0 * np.stack([c.e for c in n], axis=1))  # noqa: E731
    if sdf_id == 1:
        return (*stack(nb), np.full(len(p), True))
    if sdf_id == 2:
        return (*stack(ns), np.full(len(p), True))
    gap = box.abs() - sph.abs()
    use_box = (gap.v < 0.0)[:, None]
    (vb, eb), (vs, es) = stack(nb), stack(ns)
    return np.where(use_box, vb, -vs), np.where(use_box, eb, es), np.abs(gap.v) > gap.e


# ---- the lattice and the texture's placement of it ----
def lattice(dims, lo, hi):
    """-> (positions [D * H * W, 3] float64, x fastest, of min + i / (n - 1) * size; bound [.., 3] on the f32 evaluation of it)"""
    axes = []
    for n, a, b in zip(dims, lo, hi):
        i = B(np.arange(n, dtype=np.float64), 0.0)
        f32_sequence = (i / _exact(n - 1.0, i)) * (_exact(f32(b), i) - _exact(f32(a), i)) + _exact(f32(a), i)
        pos = f32(a) + np.arange(n) / (n - 1.0) * (f32(b) - f32(a))
        axes.append((pos, 2.0 * f32_sequence.e + np.abs(f32_sequence.v - pos)))
    zz, yy, xx = np.meshgrid(axes[2][0], axes[1][0], axes[0][0], indexing="ij")
    ez, ey, ex = np.meshgrid(axes[2][1], axes[1][1], axes[0][1], indexing="ij")
    return np.stack([xx, yy, zz], axis=-1).reshape(-1, 3), np.stack([ex, ey, ez], axis=-1).reshape(-1, 3)


def placed(unit_points, lo, hi):
    """Unit-cube points (f32) placed into the box, u * (max - min) + min -> (float64 positions [n, 3], bound [n, 3] on the f32
    evaluation)"""
    u = np.asarray(unit_points, np.float32).astype(np.float64)
    cols = []
    for i in range(3):
        a, b = _exact(f32(lo[i]), B(u[:, i], 0.0)), _exact(f32(hi[i]), B(u[:, i], 0.0))
        cols.append(B(u[:, i], 0.0) * (b - a) + a)
    return np.stack([c.v for c in cols], axis=1), 2.0 * np.stack([c.e for c in cols], axis=1)


def phi(p, dims, lo, hi, clamp=True):
    """Where the content fetched at p was evaluated: c + (p - c) n / (n - 1); MirroredRepeat holds it inside the box."""
    lo, hi, n = np.asarray(lo, np.float64), np.asarray(hi, np.float64), np.asarray(dims, np.float64)
    c = 0.5 * (lo + hi)
    q = c + (np.asarray(p, np.float64) - c) * (n / (n - 1.0))
    return np.clip(q, lo, hi) if clamp else q


# ---- the camera ----
class Camera:
    FIELDS = ("eye", "right", "up", "forward", "tan_half_fovy", "aspect", "bvp")


def camera(eye=(2.5, 3.0, 5.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy=45.0, aspect=1.0, near=0.1, far=1000.0):
    """Right-handed look-at (forward f = normalised target - eye, right s = normalised f x up, up u = s x f; the view matrix has
    rows s, u, -f and translation -(s.e, u.e, -f.e)), the GL perspective (cot(fovy/2) / aspect, cot(fovy/2),
    (far + near) / (near - far), 2 far near / (near - far), -1), and the bias that maps NDC [-1, 1] to [0, 1].  bvp is
    column-major.  Every field comes with a bound on its f32 evaluation: the formulas run through `B` from the f32 inputs."""
    one = B(np.array(1.0), 0.0)
    vec = lambda v: [B(np.array(f32(c)), 0.0) for c in v]  # noqa: E731
    e, t, u0 = vec(eye), vec(target), vec(up)

    def unit(v):
        inv = one / (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]).sqrt()
        return [c * inv for c in v]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def dot(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    f = unit([t[i] - e[i] for i in range(3)])
    s = unit(cross(f, u0))
    u = cross(s, f)
    half = B(np.array(f32(fovy)), 0.0) * _k(np.pi / 180.0, one) * _exact(0.5, one)
    tan = B(np.tan(half.v), (1.0 + np.tan(half.v) ** 2) * half.e + 2.0 * U * np.abs(np.tan(half.v)))   # libm: 1 ulp
    ct = one / tan
    asp, zn, zf = B(np.array(f32(aspect)), 0.0), B(np.array(f32(near)), 0.0), B(np.array(f32(far)), 0.0)
    zero = B(np.array(0.0), 0.0)
    view = [[s[0], s[1], s[2], dot(s, e).neg()], [u[0], u[1], u[2], dot(u, e).neg()],
            [f[0].neg(), f[1].neg(), f[2].neg(), dot(f, e)], [zero, zero, zero, one]]              # [row][column]
    proj = [[ct / asp, zero, zero, zero], [zero, ct, zero, zero],
            [zero, zero, (zf + zn) / (zn - zf), (_exact(2.0, one) * zf * zn) / (zn - zf)], [zero, zero, one.neg(), zero]]
    h = _exact(0.5, one)
    bias = [[h, zero, zero, h], [zero, h, zero, h], [zero, zero, h, h], [zero, zero, zero, one]]

    def matmul(a, b):
        out = []
        for r in range(4):
            row = []
            for c in range(4):
                acc = a[r][0] * b[0][c]
                for k in range(1, 4):
                    acc = acc + a[r][k] * b[k][c]
                row.append(acc)
            out.append(row)
        return out

    m = matmul(bias, matmul(proj, view))
    cam = Camera()
    pack = lambda bs: (np.array([float(b.v) for b in bs]), 2.0 * np.array([float(b.e) for b in bs]))  # noqa: E731
    cam.eye, cam.eye_err = pack(e)
    cam.right, cam.right_err = pack(s)
    cam.up, cam.up_err = pack(u)
    cam.forward, cam.forward_err = pack(f)
    (cam.tan_half_fovy,), (cam.tan_half_fovy_err,) = pack([tan])
    (cam.aspect,), (cam.aspect_err,) = pack([asp])
    cam.bvp, cam.bvp_err = pack([m[r][c] for c in range(4) for r in range(4)])
    cam.near, cam.far = f32(near), f32(far)
    return cam


def orbit_eyes(n, eye0=(2.5, 3.0, 5.0)):
    """camera k of n on the circle of camera 0 around +y"""
    r, a0 = np.hypot(eye0[0], eye0[2]), np.arctan2(eye0[2], eye0[0])
    return [(r * np.cos(a0 + 2.0 * np.pi * k / n), eye0[1], r * np.sin(a0 + 2.0 * np.pi * k / n)) for k in range(n)]


def pixel_rays(cam, width, height):
    """-> (origin [3], unit directions [H, W, 3], bound on a direction's f32 evaluation).  Pixel (x, y) covers
    [x, x + 1] x [y, y + 1] of the image, row 0 at the top; its ray goes through the centre."""
    x = (np.arange(width) + 0.5) / width * 2.0 - 1.0
    y = 1.0 - (np.arange(height) + 0.5) / height * 2.0
    sx, sy = x[None, :, None] * cam.aspect * cam.tan_half_fovy, y[:, None, None] * cam.tan_half_fovy
    d = cam.forward + cam.right * sx + cam.up * sy
    length = np.linalg.norm(d, axis=-1, keepdims=True)
    # the fields' own bounds, scaled as they enter; sx, sy: 5 operations and tan's bound; the sum, the length and the divide
    # (or the second normalisation from the rasterised position): 12 U of a vector of length <= |d|
    err = (cam.forward_err.max() + np.abs(sx) * cam.right_err.max() + np.abs(sy) * cam.up_err.max() +
           (np.abs(sx) + np.abs(sy)) * (5.0 * U + cam.tan_half_fovy_err / cam.tan_half_fovy)) / length + 12.0 * U
    return cam.eye.copy(), d / length, 2.0 * float(err.max())


def ray_box(o, d, lo, hi):
    """Slab intersection of o + t d with the box -> (t_in, t_out); empty where t_in > t_out."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (np.asarray(lo) - o) / d, (np.asarray(hi) - o) / d
    t1, t2 = np.where(np.isnan(t1), -np.inf, t1), np.where(np.isnan(t2), np.inf, t2)
    return np.minimum(t1, t2).max(axis=-1), np.maximum(t1, t2).min(axis=-1)


def march_start(o, d, lo, hi):
    """Where the shader starts a pixel's march (material.frag:133-139): at the fragment of the bounding box -- its entry, or
    its far side when the camera is inside -- unless 0.2 further along the ray is outside the box: then at eye + 0.2 d.
    -> (covered, t_start, t_leave: where the ray leaves the box, start_decided)"""
    t_in, t_out = ray_box(o, d, lo, hi)
    covered = (t_out >= t_in) & (t_out > 0.0)
    t_frag = np.where(t_in > 0.0, t_in, t_out)
    ahead = o + d * (t_frag + 0.2)[..., None]
    oob = np.maximum(np.asarray(lo) - ahead, ahead - np.asarray(hi)).max(axis=-1)
    # (undecided where the f32 evaluation could fall on the other side of 0: a product and a sum per coordinate of the fragment
    # and of the point ahead, on a direction good to a few U: 16 U of the largest coordinate)
    reach = np.abs(np.concatenate([np.asarray(lo, np.float64), np.asarray(hi, np.float64), np.asarray(o, np.float64)])).max()
    return covered, np.where(oob > 0.0, 0.2, t_frag), t_out, np.abs(oob) > 16.0 * U * reach


# ---- ray entry into the eroded and the dilated solid, in phi's coordinates ----
def _ray_ball(O, D, R):
    a, b, c = (D * D).sum(-1), (O * D).sum(-1), (O * O).sum(-1) - R * R
    disc = b * b - a * c
    ok = (disc > 0.0) & (R > 0.0)
    root = np.sqrt(np.where(ok, disc, 0.0))
    return np.where(ok, (-b - root) / a, np.inf), np.where(ok, (-b + root) / a, -np.inf)


def solid_windows(prm, sdf_id, O, D, delta):
    """The parameter intervals in which the line O + t D lies in {d <= delta} (delta < 0: the eroded solid), as up to two
    closed intervals [(a, b), (a2, b2)], empty where a > b.  Cube: the box of half side `side + delta`; sphere: the ball of
    radius r + delta; demo: that box minus the OPEN ball of radius r - delta."""
    empty = (np.full(O.shape[:-1], np.inf), np.full(O.shape[:-1], -np.inf))
    if sdf_id == 2:
        return [_ray_ball(O, D, prm.r + delta), empty]
    h = prm.side + delta
    box = ray_box(O, D, (-h,) * 3, (h,) * 3) if h > 0.0 else empty
    if sdf_id == 1 or prm.disable_sphere:
        return [box, empty]
    c, e = _ray_ball(O, D, prm.r - delta)              # outside the ball: t <= c or t >= e (c = inf: never inside)
    return [(box[0], np.minimum(box[1], c)), (np.maximum(box[0], np.where(np.isfinite(c), e, np.inf)), box[1])]


def first_entry(windows, t0, t1):
    """The first t in [t0, t1] inside the windows -> (t_entry or inf, inside already at t0, length of that stay)"""
    best, inside, stay = np.full(t0.shape, np.inf), np.zeros(t0.shape, bool), np.zeros(t0.shape)
    for a, b in windows:
        lo, hi = np.maximum(a, t0), np.minimum(b, t1)
        ok = (lo <= hi) & (lo < best)
        best, inside, stay = np.where(ok, lo, best), np.where(ok, a <= t0, inside), np.where(ok, hi - lo, stay)
    return best, inside, stay


# ---- scenes ----
class Scene:
    def __init__(self, name, dims, sdf_id, eye, target, width, height, checks, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), **params):
        self.name, self.dims, self.sdf_id, self.eye, self.target = name, tuple(dims), sdf_id, eye, target
        self.width, self.height, self.checks = width, height, set(checks)
        self.lo, self.hi = tuple(f32(v) for v in lo), tuple(f32(v) for v in hi)
        self.prm = Params(**params)
        n = np.asarray(self.dims, np.float64)
        self.h = (np.asarray(self.hi) - np.asarray(self.lo)) / (n - 1.0)      # lattice spacing per axis
        self.diag = float(np.linalg.norm(self.h))
        self.lip = float((n / (n - 1.0)).max())
        self._lat = None

    @property
    def slop(self):
        """What f32 adds to one interpolated distance, against the interpolant of exact lattice data: a texel's own bound (the
        reference's, over this lattice), three levels of mix() (1 - t, two products, a sum: 3 U of values <= 1 each), the
        weights (p01 from a difference and a divide, times n, minus 0.5: 3 U n in texels, times the data's step across a cell
        <= h: 3 U size n / (n - 1) per axis) and the subtraction of the offset (U); the latter three doubled like every bound"""
        size = np.asarray(self.hi) - np.asarray(self.lo)
        return float(self.lattice_eval().tex0_err[:, 0].max()) + 2.0 * U * (9.0 + 1.0 + 3.0 * float(size.sum()) * self.lip)

    def cam(self, **kw):
        args = dict(eye=self.eye, target=self.target, aspect=self.width / self.height)
        args.update(kw)
        return camera(**args)

    def lattice_eval(self):
        """the reference on the whole lattice, once"""
        if self._lat is None:
            pos, err = lattice(self.dims, self.lo, self.hi)
            self._lat = evaluate(self.prm, pos, self.sdf_id, point_err=err)
        return self._lat


ALL = ("C1", "C2", "C3", "C4", "C5", "C6", "C7")
VIEW_AB = dict(eye=(1.5, 1.7, 2.2), target=(0.0, 0.0, 0.0))
VIEW_CD = dict(eye=(1.5, 1.7, 2.2), target=(0.1, -0.05, 0.0))


def scenes():
    no = lambda *drop: [c for c in ALL if c not in drop]  # noqa: E731
    return {
        "a": Scene("a: sphere 0.8 on 32^3", (32, 32, 32), 2, width=96, height=72, checks=ALL, sphere_radius=0.8, **VIEW_AB),
        "b": Scene("b: cube 0.6 on 32^3", (32, 32, 32), 1, width=96, height=72, checks=ALL, cube_half_side=0.6, **VIEW_AB),
        "c": Scene("c: demo on 32^3", (32, 32, 32), 0, width=96, height=72, checks=no("C4"), **VIEW_CD),
        "d": Scene("d: demo on 64^3", (64, 64, 64), 0, width=96, height=72, checks=ALL, **VIEW_CD),
        # (e) and (f) are larger than the 33 x 20 x 12 and 16^3 first planned: there C2 / C3 judged 64 % and 61 % of the hits by
        # the Lipschitz bound, over the cap of 1/3
        "e": Scene("e: demo 0.7 / 0.8 on 49 x 30 x 18 in a shifted box", (49, 30, 18), 0, eye=(1.2, 1.9, 1.6), target=(0.0, 0.1, -0.3),
                   width=61, height=37, checks=no("C3", "C4"), lo=(-1.0, -0.75, -1.25), hi=(1.0, 1.0, 0.5),
                   cube_half_side=0.7, sphere_radius=0.8),
        "f": Scene("f: demo on 64^3 from inside the cavity", (64, 64, 64), 0, eye=(0.2, 0.1, 0.3), target=(1.0, 0.4, -0.2),
                   width=64, height=48, checks=no("C4")),
    }


# ---- the interpolation bound of a hit's cell ----
def _piece(prm, sdf_id, p):
    """(the distance, which smooth piece of the solid's distance function p lies on: 0 .. 5 a face of the cube -- the axis and
    sign of the largest coordinate --, 6 the sphere)"""
    a = np.abs(p)
    axis = a.argmax(axis=-1)
    face = 2 * axis + (np.take_along_axis(p, axis[..., None], -1)[..., 0] < 0.0)
    box, sph = a.max(axis=-1) - prm.side, np.linalg.norm(p, axis=-1) - prm.r
    if sdf_id == 1 or (sdf_id == 0 and prm.disable_sphere):
        return box, face
    if sdf_id == 2:
        return sph, np.full(p.shape[:-1], 6)
    return np.maximum(box, -sph), np.where(box >= -sph, face, 6)


def cell_bounds(sc, hit_pos):
    """For hits at `hit_pos` [k, 3]: q = phi(hit), d(q), and how far the trilinear interpolant I of the lattice data over the
    cell around q (its eight lattice corners; at a face MirroredRepeat repeats the outermost layer, which is the clamp in
    phi) can lie from d(q):  -below <= I - d <= above.
    * all eight corners and q on ONE smooth piece: a face of the cube is linear, I = d; the sphere's |x| is convex with second
      derivatives <= 1 / |x| along every axis, so 0 <= I - d <= sum h_i^2 / (8 min |x|) (successive linear interpolation,
      h^2 / 8 max f'' per axis), min |x| over the cell >= min over the corners - half a diagonal; as the demo's cavity the
      sign turns.
    * otherwise every corner lies within one cell diagonal of q and d is 1-Lipschitz: |I - d| <= diagonal.
    * `above` is about the STORED data, max(d, -0.1) (a texel is clamped at 0): where a corner is clamped the piece is no
      longer smooth and `above` is the diagonal.  `below` is not touched by the clamp, which only raises the interpolant.
    -> (q, d(q), below, above, sharp_below [k] bool, sharp_above [k] bool)"""
    prm, lo, n = sc.prm, np.asarray(sc.lo), np.asarray(sc.dims)
    q = phi(hit_pos, sc.dims, sc.lo, sc.hi)
    i0 = np.clip(np.floor((q - lo) / sc.h), 0, n - 2)
    corners = lo + (i0[:, None, :] + np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)])[None]) * sc.h   # [k, 8, 3]
    dc, pc = _piece(prm, sc.sdf_id, corners)
    dq, pq = _piece(prm, sc.sdf_id, q)
    one = (pc == pq[:, None]).all(axis=1)
    stored = one & (dc.min(axis=1) > -T01)
    rmin = np.maximum(np.linalg.norm(corners, axis=-1).min(axis=1) - 0.5 * sc.diag, 1e-3)      # (a cell at the centre: no bound to speak of)
    curve = (sc.h ** 2).sum() / (8.0 * rmin)
    ball = pq == 6
    convex = sc.sdf_id == 2                              # the ball itself; in the demo the ball is the cavity: -|x| is concave
    above = np.where(stored, np.where(ball & convex, curve, 0.0), sc.diag)
    below = np.where(one, np.where(ball & (not convex), curve, 0.0), sc.diag)
    return q, dq, below, above, one, stored


# ---- the shading tail ----
class _Dev:
    """How one division and one power are evaluated: IEEE divide and libm powf (1 ulp), or a * rcp(b) and exp2(y * log2(x)) on
    the transcendental unit at 1 ulp each (csrc/march_shade.h)."""
    def __init__(self, device):
        self.device = device

    def div(self, a, b):
        r = a / b
        return B(r.v, r.e + 2.0 * U * np.abs(r.v)) if self.device else r    # rcp's ulp on top of the product's rounding

    def pow(self, x, g):
        """x >= 0 to the constant power g (an f32 constant, rounded)"""
        gg = f32(g)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where(x.v > 0.0, np.power(np.maximum(x.v, 1e-300), gg), 0.0)
            lnx = np.where(x.v > 0.0, np.log(np.maximum(x.v, 1e-300)), 0.0)
            slope = np.where(x.v > 0.0, gg * np.power(np.maximum(x.v, 1e-300), gg - 1.0), 0.0)
        # first order; a power below 1 is not Lipschitz at 0, but |a^g - b^g| <= |a - b|^g there
        e_in = np.minimum(np.where(x.v > 0.0, slope * x.e, np.inf), np.power(x.e, gg)) if gg < 1.0 else slope * x.e
        e = e_in + np.abs(v * lnx) * abs(gg - g)                               # the argument's error; the exponent's rounding
        if self.device:   # log2: 1 ulp (2 U |y|), the product U |y|, exp2 of y (1 + eps): 2^y eps |y| ln 2; exp2 itself 1 ulp
            e = e + v * (3.0 * U * np.abs(gg * lnx) + 2.0 * U)
        else:
            e = e + 2.0 * U * v
        return B(v, e)


def shade(raw0, raw1, tint=(1.0, 1.0, 1.0, 1.0), ambient=(1.0, 1.0, 1.0), tone_mapping=2, color_mapping=1, gamma=0.0, device=False):
    """outColor of a hit from its two raw texels: albedo = tex0.gba * tint; the ambient light on a metallic-workflow surface
    contributes occlusion * ambient * mix(albedo, 0, metallic); tone mapping (0 none, 1 Reinhard c / (c + 1), 2 ACES
    (c (2.51 c + 0.03)) / (c (2.43 c + 0.59) + 0.14), 3 filmic with x = max(0, c - 0.004):
    ((x (6.2 x + 0.5)) / (x (6.2 x + 1.7) + 0.06))^2.2), clamped to [0, 1]; colour mapping 1 = linear -> sRGB
    (12.92 c below 0.0031308, 1.055 c^(1/2.4) - 0.055 from there); then c^gamma when gamma > 0.  alpha = tint.a.
    -> (rgba [.., 4] float64, bound [.., 4])"""
    m = _Dev(device)
    raw0, raw1 = np.asarray(raw0, np.float64), np.asarray(raw1, np.float64)
    like = B(raw0[..., 0] * 0.0, 0.0)
    K = lambda v: _k(v, like)   # noqa: E731
    one, zero = _exact(1.0, like), _exact(0.0, like)
    metallic, occ = B(raw1[..., 0], 0.0), B(raw1[..., 2], 0.0)
    out, err = [], []
    for c in range(3):
        albedo = B(raw0[..., 1 + c], 0.0) * _exact(f32(tint[c]), like)
        x = (occ * _exact(f32(ambient[c]), like)) * (albedo * (one - metallic) + zero * metallic)
        if tone_mapping == 1:
            x = m.div(x, x + one)
        elif tone_mapping == 2:
            x = m.div(x * (K(2.51) * x + K(0.03)), x * (K(2.43) * x + K(0.59)) + K(0.14))
        elif tone_mapping == 3:
            y = (x - K(0.004)).max(zero)
            x = m.pow(m.div(y * (K(6.2) * y + K(0.5)), y * (K(6.2) * y + K(1.7)) + K(0.06)), 2.2)
        x = B(np.clip(x.v, 0.0, 1.0), x.e)
        if color_mapping == 1:
            thr = 0.0031308
            low = x * K(12.92)
            high = K(1.055) * m.pow(x, 1.0 / f32(2.4)) - K(0.055)
            # step() and mix(lo, hi, 0 or 1): the selected branch times 1 plus the other times 0; within the bound of the
            # threshold either branch may be taken: the two differ by 6e-8 there, which is added
            near = np.abs(x.v - thr) <= x.e + U * thr
            x = B(np.where(x.v >= thr, high.v, low.v), np.where(x.v >= thr, high.e, low.e) + U * np.abs(high.v) +
                  np.where(near, np.abs(high.v - low.v), 0.0))
        if gamma > 0.0:
            x = m.pow(x, gamma)
        out.append(x.v)
        err.append(2.0 * x.e)
    out.append(np.full(raw0.shape[:-1], f32(tint[3])))
    err.append(np.zeros(raw0.shape[:-1]))
    return np.stack(out, axis=-1), np.stack(err, axis=-1)


def depth_of(cam, pos):
    """gl_FragDepth of a world position: 0.5 ndc_z + 0.5 with ndc_z = clip_z / clip_w of the GL projection, here from the
    float64 look-at and perspective directly (not from bvp).  -> (depth, bound on the f32 evaluation (bvp . p).z / .w)"""
    pos = np.asarray(pos, np.float64)
    z_eye = -((pos - cam.eye) * cam.forward).sum(axis=-1)                   # the view looks down -z
    n, f = cam.near, cam.far
    clip_z, clip_w = (f + n) / (n - f) * z_eye + 2.0 * f * n / (n - f), -z_eye
    depth = 0.5 * clip_z / clip_w + 0.5
    m, me = cam.bvp.reshape(4, 4).T, cam.bvp_err.reshape(4, 4).T            # [row][column]
    P = [B(pos[..., i], 0.0) for i in range(3)]
    row = lambda r: B(m[r, 0] + 0.0 * pos[..., 0], me[r, 0]) * P[0] + B(m[r, 1] + 0.0 * pos[..., 0], me[r, 1]) * P[1] + \
        B(m[r, 2] + 0.0 * pos[..., 0], me[r, 2]) * P[2] + B(m[r, 3] + 0.0 * pos[..., 0], me[r, 3])  # noqa: E731
    quotient = row(2) / row(3)
    assert np.abs(quotient.v - depth).max(initial=0.0) <= 1e-9, "bvp and the projection written out disagree"
    return depth, 2.0 * quotient.e


def unorm8(c, err):
    """float -> 8-bit UNORM: round(255 clamp(c)); decided unless 255 c lies within the bound of a half-integer"""
    v = 255.0 * np.clip(c, 0.0, 1.0)
    return np.floor(v + 0.5), np.abs(v - np.floor(v) - 0.5) > 255.0 * err + 2.0 * U * 255.0


# ---- the statements over one frame of march records ----
class Frame:
    """One camera's records: status, steps [H, W]; hit_pos [H, W, 3]; t, depth [H, W]; raw0, raw1 [H, W, 4]; rgba [H, W, 4]"""
    FIELDS = ("status", "steps", "hit_pos", "t", "raw0", "raw1", "depth")

    def __init__(self, aux, rgba):
        for k in self.FIELDS:
            setattr(self, k, np.array(aux[k]))
        self.rgba = np.array(rgba)

    def copy(self):
        f = Frame.__new__(Frame)
        for k in self.FIELDS + ("rgba",):
            setattr(f, k, getattr(self, k).copy())
        return f


class Report:
    """What check_records found: failures {statement: [message, ...]}, figures {name: number}"""
    def __init__(self):
        self.failures, self.figures = {}, {}

    def fail(self, statement, message):
        self.failures.setdefault(statement, []).append(message)

    def worst(self, name, value):
        self.figures[name] = max(self.figures.get(name, 0.0), float(value))

    def lines(self):
        return [f"{k}: {m}" for k, ms in sorted(self.failures.items()) for m in ms]


def _expect(report, statement, ok, what, *arrays):
    if not ok.all():
        k = int(np.flatnonzero(~ok.reshape(-1))[0])
        detail = ", ".join(f"{np.asarray(a).reshape(len(ok.reshape(-1)), -1)[k]}" for a in arrays)
        report.fail(statement, f"{what}: {int((~ok).sum())} of {ok.size} (first at {k}: {detail})")


def check_records(sc, cam, frame, checks=None, shading=None, device=False, report=None):
    """C1 .. C7 (the statements of tests/test_demo_meaning_cpu.py's docstring) over one frame.  `shading`: the render parameters
    the frame's rgba was shaded with (default: the scene's defaults).  -> Report"""
    rep = Report() if report is None else report
    checks = sc.checks if checks is None else set(checks) & sc.checks
    H, W = frame.status.shape
    o, d, dir_err = pixel_rays(cam, W, H)
    covered, t0, t_leave, start_decided = march_start(o, d, sc.lo, sc.hi)
    hit = frame.status == 1
    hp = frame.hit_pos.astype(np.float64)
    t = frame.t.astype(np.float64)
    size = np.asarray(sc.hi) - np.asarray(sc.lo)
    reach = float(np.abs(np.concatenate([sc.lo, sc.hi, cam.eye])).max())       # the largest coordinate a position can have
    rep.figures["hits"] = int(hit.sum())
    rep.figures["covered"] = int(covered.sum())

    if "C1" in checks:
        # a record's position is start + sum of steps along the pixel's direction, all in f32: the direction's bound over the
        # length travelled from the eye, the start's three operations and every step's two (a product and a sum per
        # coordinate, of magnitudes <= reach) as a vector: sqrt(3) (3 + 2 steps) U reach
        ok_px = hit & start_decided
        along = ((hp - o) * d).sum(axis=-1)
        off = np.linalg.norm(hp - o - along[..., None] * d, axis=-1)
        bound = dir_err * np.abs(along) + np.sqrt(3.0) * (3.0 + 2.0 * frame.steps) * U * 2.0 * reach
        rep.worst("C1 off-ray distance", off[ok_px].max() if ok_px.any() else 0.0)
        _expect(rep, "C1", ~ok_px | (off <= bound), "hit_pos off its own pixel's ray", off, bound)
        # t is the f32 sum of the steps; the travelled length is |hit_pos - start|
        start = o + d * t0[..., None]
        gone = np.linalg.norm(hp - start, axis=-1)
        tb = bound + dir_err * t0 + (2.0 + frame.steps) * U * np.maximum(t, 1.0)
        rep.worst("C1 |t - travelled|", np.abs(t - gone)[ok_px].max() if ok_px.any() else 0.0)
        _expect(rep, "C1", ~ok_px | (np.abs(t - gone) <= tb), "t is not the length travelled from the start point", t, gone, tb)
        _expect(rep, "C1", covered | (frame.status == 0), "a record outside the box's silhouette", frame.status)

    hits = np.flatnonzero(hit.reshape(-1))
    q, dq, below, above, sharp_below, sharp_above = cell_bounds(sc, hp.reshape(-1, 3)[hits])
    later = frame.steps.reshape(-1)[hits] > 1
    if len(hits):
        rep.figures["share of hits C2 judges by the Lipschitz bound"] = float(1.0 - sharp_below.mean())
        rep.figures["share of hits C3 judges by the Lipschitz bound"] = float(1.0 - sharp_above[later].mean()) if later.any() else 0.0
    if "C2" in checks and len(hits):
        rep.worst("C2 d(phi(hit)) - cell bound", (dq - below).max())
        _expect(rep, "C2", dq <= 1e-5 + below + sc.slop, "a hit outside the solid: d(phi(hit_pos)) above 1e-5 + the cell's bound",
                dq, below, hp.reshape(-1, 3)[hits])
    if "C3" in checks and len(hits):
        # the sample before a hit was >= 1e-5 and the step was that sample; the field is lip-Lipschitz along the ray, so the
        # interpolant at the hit is >= -(lip - 1) * step, and step <= min(0.9, t) (a texel holds at most 1, the offset 0.1).
        # The data is max(d, -0.1) (the clamp at 0), itself 1-Lipschitz: the statement is about that
        floor = -(above + (sc.lip - 1.0) * np.minimum(0.9, t.reshape(-1)[hits]) + 1e-5 + sc.slop)
        rep.worst("C3 depth below the surface", (-np.maximum(dq, -T01))[later].max() if later.any() else 0.0)
        _expect(rep, "C3", ~later | (np.maximum(dq, -T01) >= floor), "a hit deeper inside the solid than the overshoot allows",
                dq, floor, hp.reshape(-1, 3)[hits])
    if "C4" in checks:
        delta = sc.diag
        n = np.asarray(sc.dims, np.float64)
        c = 0.5 * (np.asarray(sc.lo) + np.asarray(sc.hi))
        O, D = c + (o - c) * (n / (n - 1.0)), d * (n / (n - 1.0))             # the ray in phi's coordinates (same parameter)
        # phi's clamp moves a point by at most half a cell per axis: where the dilated solid reaches that skin, dilate by
        # half a diagonal more (the eroded solid of these scenes lies inside the lattice)
        extent = (sc.prm.r if sc.sdf_id == 2 else sc.prm.side) + delta
        skin = 0.5 * delta if extent * float(((n - 1.0) / n).max()) >= float((0.5 * size - 0.5 * sc.h).min()) else 0.0
        eps_t = 16.0 * U * reach                                               # what f32 can move a ray parameter by
        # the march goes on until it is more than 1e-4 outside the box
        t_end = ray_box(o, d, np.asarray(sc.lo) - 1e-4 - eps_t, np.asarray(sc.hi) + 1e-4 + eps_t)[1]
        enter, inside, stay = first_entry(solid_windows(sc.prm, sc.sdf_id, O, D, -delta), t0, t_leave)
        # (the stay must be longer than the last step can overshoot the entry by -- see below --, or the march could land behind it)
        overshoot = (sc.lip - 1.0) * np.minimum(0.9, np.where(np.isfinite(enter), enter - t0, 0.0))
        must = covered & start_decided & np.isfinite(enter) & ~inside & (enter > t0 + eps_t) & (stay > overshoot + eps_t)
        near, _, _ = first_entry(solid_windows(sc.prm, sc.sdf_id, O, D, delta + skin + 1e-5 + sc.slop), t0 - eps_t, t_end)
        never = covered & start_decided & ~np.isfinite(near)
        rep.must_hit, rep.never_hit = must, never
        rep.figures["share of covered pixels C4 leaves undecided"] = float(1.0 - (must | never)[covered].mean()) if covered.any() else 1.0
        _expect(rep, "C4", ~must | hit, "a ray that enters the eroded solid is not a hit", frame.status, enter)
        # the last sample before the entry is at most (enter - t') * lip long (d o phi is lip-Lipschitz and -delta at the
        # entry, the interpolant at most delta above it): it lands at most (lip - 1) (enter - t') behind the entry
        late = (t0 + t) - enter - overshoot
        if (must & hit).any():
            rep.figures["C4 latest hit, relative to the entry into the eroded solid"] = float(((t0 + t) - enter)[must & hit].max())
        _expect(rep, "C4", ~(must & hit) | (late <= 1e-5 + sc.slop + 4.0 * U * reach * (2.0 + frame.steps)),
                "a hit later than the entry into the eroded solid", t0 + t, enter)
        _expect(rep, "C4", ~never | ~hit, "a hit on a ray that misses the dilated solid", frame.status)
    if "C5" in checks and len(hits):
        want, bound = depth_of(cam, hp.reshape(-1, 3)[hits])
        got = frame.depth.reshape(-1)[hits].astype(np.float64)
        rep.worst("C5 depth", np.abs(got - want).max())
        _expect(rep, "C5", np.abs(got - want) <= bound, "depth is not 0.5 ndc_z + 0.5 of hit_pos", got, want, bound)
        _expect(rep, "C5", frame.depth[~hit] == 1.0, "depth of a pixel without a hit is not 1", frame.depth[~hit])
    if "C6" in checks and len(hits):
        lat = sc.lattice_eval()
        Wd, Hd, Dd = sc.dims
        u = (hp.reshape(-1, 3)[hits] - np.asarray(sc.lo)) / size * np.asarray(sc.dims) - 0.5   # texel coordinates
        i0 = np.floor(u).astype(np.int64)
        idx = []
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    i = np.clip(i0 + np.array([dx, dy, dz]), 0, np.array(sc.dims) - 1)  # MirroredRepeat one texel out = clamp
                    idx.append((i[:, 2] * Hd + i[:, 1]) * Wd + i[:, 0])
        idx = np.stack(idx, axis=1)                                              # [k, 8]
        all_decided = lat.texel_decided[idx].all(axis=1)
        rep.figures["share of hits whose eight corners are decided"] = float(all_decided.mean())
        vals = np.concatenate([lat.tex0[idx][..., 1:4], lat.tex1[idx][..., 0:3]], axis=-1)          # [k, 8, 6]
        errs = np.concatenate([lat.tex0_err[idx][..., 1:4], np.zeros(idx.shape + (3,))], axis=-1)
        got = np.concatenate([frame.raw0.reshape(-1, 4)[hits][:, 1:4], frame.raw1.reshape(-1, 4)[hits][:, 0:3]], axis=-1).astype(np.float64)
        # a trilinear sample is a convex combination of its corners; three levels of mix() add 9 U of values <= 1, the
        # weights' own error stays inside the interval's span
        lo_, hi_ = (vals - errs).min(axis=1) - 9.0 * U, (vals + errs).max(axis=1) + 9.0 * U
        _expect(rep, "C6", ~all_decided[:, None] | ((got >= lo_) & (got <= hi_)),
                "a material channel outside the span of its cell's eight corners (g, b, a of tex0; r, g, b of tex1)", got, lo_, hi_)
    if "C7" in checks and len(hits):
        want, bound = shade(frame.raw0.reshape(-1, 4)[hits], frame.raw1.reshape(-1, 4)[hits], device=device, **(shading or {}))
        got = frame.rgba.reshape(-1, 4)[hits].astype(np.float64)
        rep.worst("C7 colour", np.abs(got - want).max())
        rep.worst("C7 colour / bound", (np.abs(got - want)[:, :3] / np.maximum(bound[:, :3], 1e-300)).max())
        _expect(rep, "C7", np.abs(got - want) <= bound, "RGBA is not the float64 shading of the record's own texels", got, want, bound)
        _expect(rep, "C7", frame.rgba[~hit] == 0.0, "a pixel without a hit is not transparent black", frame.rgba[~hit])
    return rep


# ---- what the CPU and the GPU tests share: the cases of A, the comparisons, the scenes' hit counts ----
FILL_GRID = (24, 10, 6)
GOLDEN_GRID = dict(dims=(9, 7, 5), lo=(-1.0, -0.5, -1.25), hi=(1.0, 1.0, 1.0))     # tests/golden/grid_9x7x5.npz's box
# hits per scene with the default shading (the oracle's count; the device's is held equal to it by the parity tests)
HITS = {"a": 1525, "b": 1688, "c": 4320, "d": 4451, "e": 565, "f": 1739}
SEEDS = {0: 11, 1: 12, 2: 13}


def surface_points(prm, sdf_id, seed, n=4096):
    """n seeded f32 points within +-0.15 of the family's surfaces: on the cube's faces, around the sphere."""
    rng = np.random.default_rng(seed)
    off = rng.uniform(-0.15, 0.15, n)
    ball = rng.normal(size=(n, 3))
    ball = ball / np.linalg.norm(ball, axis=1, keepdims=True) * (prm.r + off)[:, None]
    face = rng.uniform(-1.0, 1.0, (n, 3)) * (prm.side + 0.15)
    ax = rng.integers(0, 3, n)
    face[np.arange(n), ax] = rng.choice([-1.0, 1.0], n) * (prm.side + off)
    pick = {0: rng.random(n) < 0.5, 1: np.ones(n, bool), 2: np.zeros(n, bool)}[sdf_id]
    return np.where(pick[:, None], face, ball).astype(np.float32)


def case_points(prm, sdf_id):
    """A's points for the samplers: the seeded points around the surfaces and, as the f32 they round to, both lattices"""
    lattices = [lattice(FILL_GRID, (-1.0,) * 3, (1.0,) * 3)[0], lattice(**GOLDEN_GRID)[0]]
    return np.concatenate([surface_points(prm, sdf_id, SEEDS[sdf_id])] + [p.astype(np.float32) for p in lattices])


def cases_a():
    """[(label, Params, sdf_id)]: the defaults (brick cube, `normal` sphere) and the two materials exchanged"""
    out = []
    for sdf_id in (0, 1, 2):
        out.append((f"sdf {sdf_id}, default materials", Params(), sdf_id))
    out.append(("sdf 0, materials exchanged", Params(cube_material=1, sphere_material=0), 0))
    out.append(("sdf 0, 0.7 / 0.8", Params(cube_half_side=0.7, sphere_radius=0.8), 0))
    return out


def compare_samples(label, ref, got7, cap=0.02):
    """got7 [n, 7]: distance, colour, metallic, roughness, occlusion"""
    got = got7.astype(np.float64)
    err = np.abs(got[:, 0] - ref.d)
    k = int(np.argmax(err - ref.bound))
    assert np.isfinite(ref.bound).all() and ref.bound.max() < 1e-5, label
    assert (err <= ref.bound).all(), (label, k, got[k, 0], ref.d[k], ref.bound[k])
    undecided = 1.0 - ref.decided.mean()
    print(f"{label}: {len(got)} samples, {100 * undecided:.2f} % undecided, max distance error / bound = "
          f"{float((err / np.maximum(ref.bound, 1e-300)).max()):.3f}")
    assert undecided <= cap, (label, undecided)
    dec = ref.decided
    assert (np.abs(got[:, 1:4] - ref.color)[dec] <= 2.0 * ref.color_err[dec]).all(), label    # (doubled like the distance's)
    assert (got[dec][:, 1:4][ref.color_err[dec] == 0.0] == ref.color[dec][ref.color_err[dec] == 0.0]).all(), label
    assert (got[:, 4:7][dec] == ref.props[dec]).all(), label


def compare_texels(label, ref, t0, t1, extra=0.0):
    """t0, t1 [n, 4] f32 against the reference's texel pair -> (texels undecided, texels)"""
    t0, t1 = t0.reshape(-1, 4).astype(np.float64), t1.reshape(-1, 4).astype(np.float64)
    tol = ref.tex0_err[:, 0] + extra
    err = np.abs(t0[:, 0] - ref.tex0[:, 0])
    k = int(np.argmax(err - tol))
    assert (err <= tol).all(), (label, k, t0[k, 0], ref.tex0[k, 0], tol[k])
    undecided = 1.0 - ref.texel_decided.mean()
    print(f"{label}: {len(t0)} texels, {100 * undecided:.2f} % undecided, max tex0.r error / bound = {float((err / tol).max()):.3f}")
    dec = ref.texel_decided
    # the colour words are to_linear of an 8-bit code: equal as that code -- within the f32 evaluation's bound of the code's
    # float64 value, two orders of magnitude below the distance to the next code's
    assert (np.abs(t0[:, 1:] - ref.tex0[:, 1:])[dec] <= ref.tex0_err[:, 1:][dec]).all(), label
    assert (t1[dec] == ref.tex1[dec].astype(np.float32).astype(np.float64)).all(), label
    assert (t1[:, 3] == AIR_DIST).all(), label
    return int((~dec).sum()), len(dec)


def pooled(counts, label, cap=0.02):
    """A case is one entry point on one member of the family: the fill's is both lattices together."""
    share = sum(c[0] for c in counts) / sum(c[1] for c in counts)
    print(f"{label}: {100 * share:.2f} % of the texels undecided")
    assert share <= cap, (label, share)


SHADINGS = [dict(tone_mapping=t, color_mapping=c, gamma=g) for t in (0, 1, 2, 3) for c in (0, 1) for g in (0.0, 2.2)]
