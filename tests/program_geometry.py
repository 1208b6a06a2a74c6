"""An independent float64 reference for SDF programs, written from GEOMETRY: what a model means, not how the table in
include/sdfgrid.h computes it.  Shares no code with tests/program_ref.py and calls nothing of the library.

* A scene is a small tree: primitives with their parameters, FORWARD placements (`Rigid`: content rotated by R, then moved by t;
  `Scale`: content scaled by s), hard and smooth CSG, round, shell, a material per primitive.
* `emit(scene, program_module, bb)` turns it into Program builder calls through the public helpers only (translation,
  rigid_inverse, push_scale / pop_scale, push_affine): their conventions are what is under test.
* `evaluate(scene, points)` is the float64 meaning: a child of a placement is evaluated at R^T (p - t) / s and its distance
  multiplied by s; primitive distances are written case by case (box: interior, face, edge, corner; cylinder: interior, side,
  cap, rim; torus: distance to the centre circle minus r; CUBE: the Chebyshev ball).  Parameters and points are the f32-rounded
  ones, as float64.
* Beside every value runs a forward ERROR BOUND for the f32 sequence the header specifies: each f32 operation contributes
  2^-24 |result|; input errors propagate to first order (Lipschitz 1 through + - min max |x|, |y| ex + |x| ey through products,
  e / (2 sqrt) through roots -- capped by sqrt(e), which holds where the first-order term is singular --, the quotient rule
  through the one divide); operands the builder rounds (matrix entries, 1 / s) carry their actual rounding error.  The final
  bound is doubled for the second-order terms.  It is the tests' tolerance: derived, not tuned.
* `known_points(prim, rng, n)`: points whose distance is known by CONSTRUCTION (surface point + t * unit outward normal, t within
  the primitive's reach), independent even of the case analysis above.
"""
import numpy as np

U = 2.0 ** -24


def f32(v):
    return float(np.float32(v))


# ---- the scene tree ----
class Prim:
    def __init__(self, kind, *params, mat=None):
        self.kind, self.params = kind, tuple(f32(v) for v in params)
        self.mat = None if mat is None else tuple(f32(v) for v in mat)


class Rigid:
    """child rotated by R (3 x 3, orthonormal), then moved by t; R = None: moved only."""
    def __init__(self, child, t=(0.0, 0.0, 0.0), R=None):
        self.child, self.t = child, np.array([float(v) for v in t])
        self.R = None if R is None else np.array(R, dtype=np.float64)


class Scale:
    def __init__(self, child, s):
        self.child, self.s = child, f32(s)


class Comb:
    """kind: union, intersect, subtract (a minus b), smooth_union, smooth_subtract (k > 0)"""
    def __init__(self, kind, a, b, k=None):
        self.kind, self.a, self.b, self.k = kind, a, b, None if k is None else f32(k)


class Round:
    def __init__(self, child, r):
        self.child, self.r = child, f32(r)


class Shell:
    def __init__(self, child, t):
        self.child, self.t = child, f32(t)


def union_of(nodes, kind="union", k=None):
    out = nodes[0]
    for n in nodes[1:]:
        out = Comb(kind, out, n, k)
    return out


def rot(axis, degrees):
    """Rotation by `degrees` about a unit axis (Rodrigues), float64."""
    a = np.array(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + s * K + (1.0 - c) * (K @ K)


# ---- the emitter: the tree as Program builder calls ----
def emit(scene, PM, bb=(-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)):
    prog = PM.Program(bb)
    state = {"mat": None}

    def set_material(n):
        """MATERIAL for the first primitive below n, unless it is the current one already (before the frames that place it,
        the way one writes a program by hand)."""
        while not isinstance(n, Prim):
            n = n.a if isinstance(n, Comb) else n.child
        if n.mat != state["mat"]:
            assert n.mat is not None, "a primitive without a material after the first MATERIAL"
            prog.material(*n.mat)
            state["mat"] = n.mat

    def walk(n):
        set_material(n)
        if isinstance(n, Prim):
            getattr(prog, n.kind)(*n.params)
        elif isinstance(n, Rigid):
            prog.push_affine(PM.translation(*n.t) if n.R is None else PM.rigid_inverse(n.R.tolist(), n.t.tolist()))
            walk(n.child)
            prog.pop()
        elif isinstance(n, Scale):
            prog.push_scale(n.s)
            walk(n.child)
            prog.pop_scale(n.s)
        elif isinstance(n, Comb):
            walk(n.a)
            walk(n.b)
            getattr(prog, n.kind)(*(() if n.k is None else (n.k,)))
        elif isinstance(n, Round):
            walk(n.child)
            prog.round(n.r)
        elif isinstance(n, Shell):
            walk(n.child)
            prog.shell(n.t)
        else:
            raise TypeError(n)
    walk(scene)
    return prog


# ---- error-bound arithmetic: (value of the specified f32 sequence in float64, bound on its f32 result's error) ----
class B:
    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)

    @staticmethod
    def op(v, e):                                   # one f32 operation: its own rounding on top of what came in
        return B(v, e + U * np.abs(v))

    def __add__(self, o): return B.op(self.v + o.v, self.e + o.e)
    def __sub__(self, o): return B.op(self.v - o.v, self.e + o.e)
    def __mul__(self, o): return B.op(self.v * o.v, np.abs(o.v) * self.e + np.abs(self.v) * o.e)

    def __truediv__(self, o):
        return B.op(self.v / o.v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v))

    def sqrt(self):
        r = np.sqrt(np.maximum(self.v, 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            first = np.where(r > 0.0, self.e / (2.0 * r), np.inf)
        return B.op(r, np.minimum(first, np.sqrt(self.e)))

    # exact in f32, Lipschitz 1
    def abs(self): return B(np.abs(self.v), self.e)
    def neg(self): return B(-self.v, self.e)
    def max(self, o): return B(np.maximum(self.v, o.v), np.maximum(self.e, o.e))
    def min(self, o): return B(np.minimum(self.v, o.v), np.maximum(self.e, o.e))


def const(v, like):
    """An instruction operand: the f32 the builder stores, with the error of that rounding against the exact `v`."""
    r = f32(v)
    return B(np.full(like.v.shape, r), abs(r - float(v)))


def _len_bound(*c):
    s = c[0] * c[0]
    for k in c[1:]:
        s = s + k * k
    return s.sqrt()


def primitive_bound(kind, a, x, y, z):
    """The error bound of the header's f32 sequence for one primitive at the (already bounded) point."""
    zero = const(0.0, x)
    k = [const(v, x) for v in a]
    if kind == "sphere":
        return (_len_bound(x, y, z) - k[0]).e
    if kind == "cube":
        return (x.abs().max(y.abs()).max(z.abs()) - k[0]).e
    if kind == "box":
        ex, ey, ez = x.abs() - k[0], y.abs() - k[1], z.abs() - k[2]
        return (_len_bound(ex.max(zero), ey.max(zero), ez.max(zero)) + ex.max(ey.max(ez)).min(zero)).e
    if kind == "cylinder":
        dx, dz = _len_bound(x, y) - k[0], z.abs() - k[1]
        return (dx.max(dz).min(zero) + _len_bound(dx.max(zero), dz.max(zero))).e
    if kind == "torus":
        return (_len_bound(_len_bound(x, y) - k[0], z) - k[1]).e
    if kind == "plane":
        return (k[0] * x + k[1] * y + k[2] * z + k[3]).e
    raise ValueError(kind)


# ---- primitive distances, from the geometry ----
def primitive_distance(kind, a, p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    if kind == "sphere":
        return np.sqrt(x * x + y * y + z * z) - a[0]
    if kind == "cube":                               # the ball of the Chebyshev norm, radius h
        return np.max(np.abs(p), axis=1) - a[0]
    if kind == "box":
        q = np.abs(p) - np.array(a[:3])              # signed distance to each pair of face planes
        outside = q > 0.0
        n_out = outside.sum(axis=1)
        qo = np.where(outside, q, 0.0)
        interior = q.max(axis=1)                     # inside: the nearest face, negative
        face = qo.sum(axis=1)                        # beyond one pair of faces: the distance to that face
        edge = np.sqrt((qo * qo).sum(axis=1))        # beyond two: to the edge they share (the third term is 0)
        corner = np.sqrt((q * q).sum(axis=1))        # beyond all three: to the corner
        return np.select([n_out == 0, n_out == 1, n_out == 2], [interior, face, edge], corner)
    if kind == "cylinder":                           # axis z
        side, cap = np.sqrt(x * x + y * y) - a[0], np.abs(z) - a[1]
        return np.select([(side <= 0) & (cap <= 0), (side > 0) & (cap <= 0), (side <= 0) & (cap > 0)],
                         [np.maximum(side, cap), side, cap], np.sqrt(side * side + cap * cap))   # ... else the rim circle
    if kind == "torus":                              # the centre circle has radius R in the plane z = 0
        to_circle = np.sqrt((np.sqrt(x * x + y * y) - a[0]) ** 2 + z * z)
        return to_circle - a[1]
    if kind == "plane":                              # |n| times the signed distance to the plane n . p + d0 = 0
        return a[0] * x + a[1] * y + a[2] * z + a[3]
    raise ValueError(kind)


# ---- the evaluator ----
class Result:
    """d: float64 distance; e: error bound (not yet doubled); mat: index into `materials`; decided: the reference's own margin
    exceeded the operands' bounds at every combinator on the winning path."""
    def __init__(self, d, e, mat, decided):
        self.d, self.e, self.mat, self.decided = d, e, mat, decided


def evaluate(scene, points):
    """points: [n, 3] (their f32 values are what is evaluated) -> (distance [n] float64, bound [n] -- the tolerance, doubled --,
    material [n, 6] float64, decided [n] bool)."""
    p = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    n = len(p)
    materials = [(0.0,) * 6]

    def mat_index(m):
        if m is None:
            return 0
        if m not in materials:
            materials.append(m)
        return materials.index(m)

    def walk(node, q, qb):
        """q: [n, 3] the exact local point; qb: three B, the f32 machine's point with its error against q"""
        if isinstance(node, Prim):
            d = primitive_distance(node.kind, node.params, q)
            e = primitive_bound(node.kind, node.params, *qb)
            return Result(d, e, np.full(n, mat_index(node.mat)), np.ones(n, bool))
        if isinstance(node, Rigid):
            Rm = np.eye(3) if node.R is None else node.R
            q2 = (q - node.t) @ Rm                   # rows: R^T (q - t)
            m3 = -(Rm.T @ node.t)
            qb2 = []
            for i in range(3):
                row = [const(Rm.T[i, j], qb[0]) for j in range(3)] + [const(m3[i], qb[0])]
                qb2.append(row[0] * qb[0] + row[1] * qb[1] + row[2] * qb[2] + row[3])
            qb2 = [B(q2[:, i], qb2[i].e + np.abs(qb2[i].v - q2[:, i])) for i in range(3)]
            return walk(node.child, q2, qb2)
        if isinstance(node, Scale):
            q2 = q / node.s
            inv = const(1.0 / node.s, qb[0])
            qb2 = [c * inv for c in qb]
            qb2 = [B(q2[:, i], qb2[i].e + np.abs(qb2[i].v - q2[:, i])) for i in range(3)]
            r = walk(node.child, q2, qb2)
            out = B(r.d, r.e) * const(node.s, qb[0])
            return Result(r.d * node.s, out.e, r.mat, r.decided)
        if isinstance(node, Round):
            r = walk(node.child, q, qb)
            return Result(r.d - node.r, (B(r.d, r.e) - const(node.r, qb[0])).e, r.mat, r.decided)
        if isinstance(node, Shell):
            r = walk(node.child, q, qb)
            return Result(np.abs(r.d) - node.t, (B(r.d, r.e).abs() - const(node.t, qb[0])).e, r.mat, r.decided)
        if isinstance(node, Comb):
            a, b = walk(node.a, q, qb), walk(node.b, q, qb)
            A, Bb = B(a.d, a.e), B(b.d, b.e)
            if node.kind in ("union", "smooth_union"):
                first, margin = a.d <= b.d, np.abs(a.d - b.d)
            elif node.kind == "intersect":
                first, margin = a.d >= b.d, np.abs(a.d - b.d)
            else:                                    # the subtracts: the material of whichever surface is nearer
                first, margin = np.abs(a.d) < np.abs(b.d), np.abs(np.abs(a.d) - np.abs(b.d))
            if node.kind == "union":
                d, e = np.minimum(a.d, b.d), A.min(Bb).e
            elif node.kind == "intersect":
                d, e = np.maximum(a.d, b.d), A.max(Bb).e
            elif node.kind == "subtract":
                d, e = np.maximum(a.d, -b.d), A.max(Bb.neg()).e
            else:
                k = node.k
                K, quarter, zero = const(k, qb[0]), const(0.25, qb[0]), const(0.0, qb[0])
                other = b.d if node.kind == "smooth_union" else -b.d
                O = Bb if node.kind == "smooth_union" else Bb.neg()
                h = np.maximum(k - np.abs(a.d - other), 0.0) / k
                H = (K - (A - O).abs()).max(zero) / K
                blend = (H * H) * (K * quarter)
                if node.kind == "smooth_union":      # the polynomial smooth minimum: min - h^2 k / 4
                    d, e = np.minimum(a.d, other) - h * h * k / 4.0, (A.min(O) - blend).e
                else:
                    d, e = np.maximum(a.d, other) + h * h * k / 4.0, (A.max(O) + blend).e
            decided = np.where(first, a.decided, b.decided) & (margin > a.e + b.e)
            return Result(d, e, np.where(first, a.mat, b.mat), decided)
        raise TypeError(node)

    qb = [B(p[:, i], 0.0) for i in range(3)]
    r = walk(scene, p, qb)
    table = np.array(materials, dtype=np.float64)
    return r.d, 2.0 * r.e, table[r.mat], r.decided


# ---- what the mesh statements need beside the distance (tests/mesh_geometry.py) ----
def lipschitz(scene):
    """The Lipschitz constant of the scene's distance: 1 through every node (placements are rigid, a scale divides the point and
    multiplies the distance, min, max, their smooth forms, |.| and a constant offset keep it), max(1, |n|) for a plane."""
    if isinstance(scene, Prim):
        return max(1.0, float(np.linalg.norm(scene.params[:3]))) if scene.kind == "plane" else 1.0
    if isinstance(scene, Comb):
        return max(lipschitz(scene.a), lipschitz(scene.b))
    return lipschitz(scene.child)


TETRA = np.array([[1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0], [1.0, 1.0, 1.0]])


def tetra_normal(scene, points, eps=0.001):
    """normal_default_impl as a definition: v = sum_i k_i d(p + k_i e) over the four tetrahedral taps k_i, in float64, the taps at
    the positions f32 arithmetic gives them (p.x + e, p.x + -1.0f * e, each one rounded sum); n = v / |v|.
    -> (n [m, 3] float64, tol_sin [m], decided [m]).  tol_sin bounds the sine of the angle between n and the f32 result: with B
    the evaluator's bound at the taps (the largest of the four), U = 2^-24,
      E = 4 sqrt(3) (B + sqrt(3) U (|p|_inf + e))  +  12 sqrt(3) U (|d(p)| + B + sqrt(3) e)
    (the taps' own errors with their signs, |k_i| = sqrt(3); the three f32 additions per component of terms that are at most
    |d(p)| + B + sqrt(3) e: the derivation of test_program_march_cpu.py's sphere test without its curvature term, since the taps
    ARE the definition here), tol_sin = E / |v|.  decided iff tol_sin < 0.05."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    e = np.float32(eps)
    me = np.float32(-1.0) * e
    v, worst = np.zeros((len(p), 3)), np.zeros(len(p))
    for k in TETRA:
        tap = np.stack([p[:, a] + (e if k[a] > 0 else me) for a in range(3)], axis=1)      # float32 + float32: one rounding
        d, bound, _, _ = evaluate(scene, tap)
        v += k[None, :] * d[:, None]
        worst = np.maximum(worst, bound)
    d0 = evaluate(scene, p)[0]
    length = np.linalg.norm(v, axis=1)
    r3 = np.sqrt(3.0)
    E = 4.0 * r3 * (worst + r3 * U * (np.abs(p.astype(np.float64)).max(axis=1) + float(e))) + \
        12.0 * r3 * U * (np.abs(d0) + worst + r3 * float(e))
    with np.errstate(divide="ignore", invalid="ignore"):
        tol = np.where(length > 0.0, E / length, np.inf)
        n = np.where(length[:, None] > 0.0, v / length[:, None], 0.0)
    return n, tol, tol < 0.05


# ---- points whose distance is known by construction ----
def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def known_points(prim, rng, n, with_normals=False):
    """-> {feature: (points [n, 3] float64, distance [n] float64, lipschitz)}: surface point q + t * unit outward normal, t within
    the primitive's reach, so that the distance there is t (for the plane: |n| t, and the field's Lipschitz constant is |n|).
    with_normals: each entry also carries (unit outward normal [n, 3], margin [n], rho [n]): the direction the point was offset
    along, how far the point lies from where ANOTHER piece of the primitive's surface becomes the nearest one (a ball of that
    radius sees one smooth piece only), and the smallest radius of curvature of the level set through the point (inf: flat)."""
    if with_normals:
        return _known_points_with_normals(prim, rng, n)
    kind, a = prim.kind, prim.params
    sgn = lambda shape: rng.choice(np.array([-1.0, 1.0]), shape)   # noqa: E731
    out = {}

    def offsets(inward, outward=1.5):
        """half of them outside (0 .. outward), half inside (-inward .. 0), some exactly on the surface"""
        t = np.where(rng.random(n) < 0.5, rng.uniform(0.0, outward, n), -rng.uniform(0.0, inward, n) if inward > 0 else 0.0)
        t[:: 16] = 0.0
        return t

    if kind == "sphere":
        d = _unit(rng.normal(size=(n, 3)))
        t = offsets(a[0])
        out["surface"] = (d * (a[0] + t)[:, None], t, 1.0)
    elif kind == "cube":
        # a face of the Chebyshev ball: the offset axis must stay the largest coordinate
        t = offsets(a[0])
        p = rng.uniform(-1.0, 1.0, (n, 3)) * (a[0] + t)[:, None]
        ax = rng.integers(0, 3, n)
        p[np.arange(n), ax] = sgn(n) * (a[0] + t)
        out["face"] = (p, t, 1.0)
    elif kind == "box":
        h = np.array(a[:3])
        inr = h.min()
        # faces: outward from anywhere on the face; inward while this face stays the nearest
        t = offsets(inr)
        room = h[None, :] - np.maximum(-t, 0.0)[:, None]
        p = rng.uniform(-1.0, 1.0, (n, 3)) * room
        ax = rng.integers(0, 3, n)
        p[np.arange(n), ax] = sgn(n) * (h[ax] + t)
        out["face"] = (p, t, 1.0)
        # edges: two axes on the surface, the normal anywhere in the quarter plane between the two face normals
        t = offsets(0.0)
        p = rng.uniform(-1.0, 1.0, (n, 3)) * h
        ax = rng.integers(0, 3, n)                   # the axis ALONG the edge
        phi = rng.uniform(0.0, np.pi / 2, n)
        for k, w in ((1, np.cos(phi)), (2, np.sin(phi))):
            j = (ax + k) % 3
            p[np.arange(n), j] = sgn(n) * (h[j] + t * w)
        out["edge"] = (p, t, 1.0)
        # corners: the normal anywhere in the octant
        t = offsets(0.0)
        d = np.abs(_unit(rng.normal(size=(n, 3))))
        out["corner"] = (sgn((n, 3)) * (h[None, :] + t[:, None] * d), t, 1.0)
    elif kind == "cylinder":
        r, hh = a[0], a[1]
        inr = min(r, hh)
        th = rng.uniform(0.0, 2 * np.pi, n)
        radial = np.stack([np.cos(th), np.sin(th), np.zeros(n)], axis=1)
        t = offsets(inr)
        z = rng.uniform(-1.0, 1.0, n) * (hh - np.maximum(-t, 0.0))
        out["side"] = (radial * (r + t)[:, None] + np.stack([np.zeros(n), np.zeros(n), z], axis=1), t, 1.0)
        t = offsets(inr)
        rho = np.sqrt(rng.random(n)) * (r - np.maximum(-t, 0.0))
        p = radial * rho[:, None]
        p[:, 2] = sgn(n) * (hh + t)
        out["cap"] = (p, t, 1.0)
        t = offsets(0.0)
        phi = rng.uniform(0.0, np.pi / 2, n)
        p = radial * (r + t * np.cos(phi))[:, None]
        p[:, 2] = sgn(n) * (hh + t * np.sin(phi))
        out["rim"] = (p, t, 1.0)
    elif kind == "torus":
        R, r = a[0], a[1]
        th = rng.uniform(0.0, 2 * np.pi, n)
        radial = np.stack([np.cos(th), np.sin(th), np.zeros(n)], axis=1)
        for feature, phi in (("tube", rng.uniform(0.0, 2 * np.pi, n)), ("outer equator", np.zeros(n)), ("inner equator", np.full(n, np.pi))):
            c = np.cos(phi)
            # towards the axis the centre-circle point stays the nearest only up to the axis itself
            reach = np.where(c < -1e-9, 0.9 * R / np.maximum(-c, 1e-9) - r, 1.5)
            t = np.where(rng.random(n) < 0.5, rng.uniform(0.0, 1.0, n) * np.minimum(reach, 1.5), -rng.uniform(0.0, r, n))
            t[:: 16] = 0.0
            w = (r + t)
            p = radial * (R + w * c)[:, None]
            p[:, 2] = w * np.sin(phi)
            out[feature] = (p, t, 1.0)
    elif kind == "plane":
        nrm = np.array(a[:3])
        ln = np.linalg.norm(nrm)
        q = rng.uniform(-1.5, 1.5, (n, 3))
        q = q - ((q @ nrm + a[3]) / (ln * ln))[:, None] * nrm[None, :]      # onto the plane
        t = rng.uniform(-1.5, 1.5, n)
        t[:: 16] = 0.0
        out["plane"] = (q + t[:, None] * (nrm / ln)[None, :], ln * t, ln)
    else:
        raise ValueError(kind)
    return out


def _known_points_with_normals(prim, rng, n):
    """known_points' constructions once more, keeping what each point was built from: q on the surface, the unit outward normal
    m there, p = q + t m.  -> {feature: (points, distance, lipschitz, normal, margin, rho)}"""
    kind, a = prim.kind, prim.params
    sgn = lambda shape: rng.choice(np.array([-1.0, 1.0]), shape)   # noqa: E731
    rows, inf = np.arange(n), np.full(n, np.inf)
    out = {}

    def offsets(inward, outward=0.5):
        t = np.where(rng.random(n) < 0.5, rng.uniform(0.0, outward, n), -rng.uniform(0.0, 0.9 * inward, n) if inward > 0 else 0.0)
        t[:: 16] = 0.0
        return t

    def axis_normal(ax, s):
        m = np.zeros((n, 3))
        m[rows, ax] = s
        return m

    if kind == "sphere":
        m = _unit(rng.normal(size=(n, 3)))
        t = offsets(a[0])
        out["surface"] = (m * (a[0] + t)[:, None], t, 1.0, m, a[0] + t, a[0] + t)
    elif kind == "cube":
        t = offsets(a[0])
        p = rng.uniform(-1.0, 1.0, (n, 3)) * (a[0] + t)[:, None]
        ax, s = rng.integers(0, 3, n), sgn(n)
        p[rows, ax] = s * (a[0] + t)
        others = np.abs(p).copy()
        others[rows, ax] = 0.0
        out["face"] = (p, t, 1.0, axis_normal(ax, s), ((a[0] + t) - others.max(axis=1)) / np.sqrt(2.0), inf)
    elif kind == "box":
        h = np.array(a[:3])
        t = offsets(h.min())
        depth = np.maximum(-t, 0.0)
        p = rng.uniform(-1.0, 1.0, (n, 3)) * (h[None, :] - depth[:, None])
        ax, s = rng.integers(0, 3, n), sgn(n)
        p[rows, ax] = s * (h[ax] + t)
        room = h[None, :] - np.abs(p) - depth[:, None]          # per other axis: how far from where that face (or its edge) is as near
        room[rows, ax] = np.inf
        out["face"] = (p, t, 1.0, axis_normal(ax, s), room.min(axis=1) / np.sqrt(2.0), inf)
        t = offsets(0.0)
        p = rng.uniform(-1.0, 1.0, (n, 3)) * h
        ax = rng.integers(0, 3, n)
        phi = rng.uniform(0.0, np.pi / 2, n)
        m = np.zeros((n, 3))
        for k, w in ((1, np.cos(phi)), (2, np.sin(phi))):
            j, s = (ax + k) % 3, sgn(n)
            p[rows, j] = s * (h[j] + t * w)
            m[rows, j] = s * w
        margin = np.minimum(h[ax] - np.abs(p[rows, ax]), t * np.minimum(np.cos(phi), np.sin(phi)))
        out["edge"] = (p, t, 1.0, m, margin, t)
        t = offsets(0.0)
        dd, s = np.abs(_unit(rng.normal(size=(n, 3)))), sgn((n, 3))
        out["corner"] = (s * (h[None, :] + t[:, None] * dd), t, 1.0, s * dd, (t[:, None] * dd).min(axis=1), t)
    elif kind == "cylinder":
        r, hh = a[0], a[1]
        th = rng.uniform(0.0, 2 * np.pi, n)
        radial = np.stack([np.cos(th), np.sin(th), np.zeros(n)], axis=1)
        t = offsets(min(r, hh))
        depth = np.maximum(-t, 0.0)
        z = rng.uniform(-1.0, 1.0, n) * (hh - depth)
        p = radial * (r + t)[:, None]
        p[:, 2] = z
        out["side"] = (p, t, 1.0, radial, np.minimum((hh - np.abs(z) - depth) / np.sqrt(2.0), r + t), r + t)
        t = offsets(min(r, hh))
        depth = np.maximum(-t, 0.0)
        rho_xy = np.sqrt(rng.random(n)) * (r - depth)
        s = sgn(n)
        p = radial * rho_xy[:, None]
        p[:, 2] = s * (hh + t)
        out["cap"] = (p, t, 1.0, axis_normal(np.full(n, 2), s), (r - rho_xy - depth) / np.sqrt(2.0), inf)
        t = offsets(0.0)
        phi = rng.uniform(0.0, np.pi / 2, n)
        s = sgn(n)
        p = radial * (r + t * np.cos(phi))[:, None]
        p[:, 2] = s * (hh + t * np.sin(phi))
        m = radial * np.cos(phi)[:, None]
        m[:, 2] = s * np.sin(phi)
        out["rim"] = (p, t, 1.0, m, t * np.minimum(np.cos(phi), np.sin(phi)), t)
    elif kind == "torus":
        R, r = a[0], a[1]
        th = rng.uniform(0.0, 2 * np.pi, n)
        radial = np.stack([np.cos(th), np.sin(th), np.zeros(n)], axis=1)
        phi = rng.uniform(0.0, 2 * np.pi, n)
        c = np.cos(phi)
        t = np.where(rng.random(n) < 0.5, rng.uniform(0.0, 0.5, n) * np.where(c < 0.0, 0.5 * (R - r), 1.0), -rng.uniform(0.0, 0.9 * r, n))
        t[:: 16] = 0.0
        w = r + t
        p = radial * (R + w * c)[:, None]
        p[:, 2] = w * np.sin(phi)
        m = radial * c[:, None]
        m[:, 2] = np.sin(phi)
        out["tube"] = (p, t, 1.0, m, np.minimum(w, R + w * c), np.minimum(w, np.abs(R + w * c) / np.maximum(np.abs(c), 1e-12)))
    elif kind == "plane":
        nrm = np.array(a[:3])
        ln = np.linalg.norm(nrm)
        q = rng.uniform(-1.5, 1.5, (n, 3))
        q = q - ((q @ nrm + a[3]) / (ln * ln))[:, None] * nrm[None, :]
        t = rng.uniform(-1.5, 1.5, n)
        out["plane"] = (q + t[:, None] * (nrm / ln)[None, :], ln * t, ln, np.tile(nrm / ln, (n, 1)), inf, inf)
    else:
        raise ValueError(kind)
    return out


def place(node_chain, local_points):
    """local points of the innermost child -> world points, through the forward placements outermost first in `node_chain`
    [(kind, value)]: ("rigid", (R or None, t)) or ("scale", s); also returns the product of the scales."""
    p, scale = np.array(local_points, dtype=np.float64), 1.0
    for kind, v in reversed(node_chain):
        if kind == "scale":
            p, scale = p * f32(v), scale * f32(v)
        else:
            Rm, t = v
            p = (p if Rm is None else p @ np.asarray(Rm, dtype=np.float64).T) + np.asarray(t, dtype=np.float64)
    return p, scale


def wrap(prim, node_chain):
    node = prim
    for kind, v in reversed(node_chain):
        node = Scale(node, v) if kind == "scale" else Rigid(node, v[1], v[0])
    return node


# ---- the scenes the meaning tests run (CPU: the host mirror; GPU: the kernels) ----
def _rot_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]


def _rot_x(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return [[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]


def scene_sixteen():
    """program.py's example_sixteen as a user would describe it: a plate on four pillars, a torus, a tilted cube, a ring of six
    spheres, a bore, a rounded foot, cut by a plane."""
    import math
    s = Prim("box", 0.8, 0.8, 0.1, mat=(0.7, 0.7, 0.75, 0.9, 0.3, 1.0))
    for i in range(4):
        cx, cy = (-0.6 if i & 1 else 0.6), (-0.6 if i & 2 else 0.6)
        s = Comb("union", s, Rigid(Prim("cylinder", 0.08, 0.4, mat=(0.6, 0.3 + 0.1 * i, 0.2, 0.1, 0.7, 1.0)), (cx, cy, 0.45)))
    s = Comb("smooth_union", s, Rigid(Prim("torus", 0.45, 0.08, mat=(0.2, 0.5, 0.8, 0.0, 0.4, 1.0)), (0.0, 0.0, 0.5)), 0.05)
    s = Comb("union", s, Rigid(Scale(Prim("cube", 0.3, mat=(0.9, 0.1, 0.1, 0.3, 0.2, 1.0)), 0.5), (0.0, 0.0, 0.3), _rot_z(45.0)))
    for i in range(6):
        ang = math.radians(60.0 * i)
        ball = Prim("sphere", 0.15, mat=(0.2 + 0.1 * i, 0.8 - 0.1 * i, 0.4, 0.2, 0.5, 1.0))
        s = Comb("smooth_union", s, Rigid(ball, (0.7 * math.cos(ang), 0.7 * math.sin(ang), -0.3)), 0.04)
    s = Comb("subtract", s, Rigid(Prim("cylinder", 0.1, 1.2, mat=(0.3, 0.3, 0.3, 0.0, 0.9, 1.0)), (0.0, 0.0, 0.0), _rot_x(90.0)))
    foot = (0.95, 0.85, 0.2, 1.0, 0.1, 1.0)
    s = Comb("union", s, Rigid(Round(Prim("box", 0.3, 0.3, 0.05, mat=foot), 0.02), (0.0, 0.0, -0.6)))
    return Comb("intersect", s, Prim("plane", 0.0, 0.0, -1.0, 0.95, mat=foot))


def scene_every_opcode():
    a = Rigid(Round(Prim("box", 0.45, 0.3, 0.2, mat=(0.8, 0.2, 0.1, 0.1, 0.6, 0.9)), 0.05), (0.2, -0.1, 0.05), rot((1, 2, 3), 35.0))
    b = Prim("cylinder", 0.22, 0.7, mat=(0.1, 0.1, 0.1, 0.7, 0.2, 0.0))
    c = Scale(Prim("torus", 1.2, 0.3, mat=(0.1, 0.9, 0.3, 0.0, 1.0, 0.5)), 0.5)
    s = Comb("smooth_union", Comb("union", a, b), c, 0.15)
    s = Comb("intersect", s, Prim("plane", 0.0, 0.8, 0.6, -0.55, mat=(0.1, 0.9, 0.3, 0.0, 1.0, 0.5)))
    s = Comb("smooth_subtract", s, Rigid(Prim("sphere", 0.3, mat=(0.5, 0.2, 0.5, 0.3, 0.3, 1.0)), (0.5, 0.1, 0.0)), 0.1)
    return Comb("subtract", s, Rigid(Shell(Prim("cube", 0.3, mat=(0.9, 0.9, 0.2, 0.4, 0.4, 0.4)), 0.04), (-0.45, 0.2, 0.1), _rot_z(20.0)))


def scene_nested_frames():
    """Frames to depth 4 (rigid, scale, rigid, scale) around each kind of solid, unioned."""
    mats = [(0.1 * i, 1.0 - 0.1 * i, 0.5, 0.1 * i, 0.5, 1.0) for i in range(1, 6)]
    prims = [Prim("box", 0.5, 0.3, 0.2, mat=mats[0]), Prim("cylinder", 0.3, 0.6, mat=mats[1]), Prim("torus", 0.5, 0.15, mat=mats[2]),
             Prim("sphere", 0.4, mat=mats[3]), Prim("cube", 0.35, mat=mats[4])]
    spots = [(-0.6, -0.5, 0.1), (0.55, -0.45, -0.2), (0.0, 0.55, 0.3), (-0.6, 0.5, -0.4), (0.6, 0.5, 0.45)]
    nodes = []
    for i, (p, c) in enumerate(zip(prims, spots)):
        inner = Rigid(Scale(p, 1.25 + 0.25 * i), (0.05 * i, -0.03, 0.02 * i), rot((i + 1, 1, 2 - i), 25.0 + 40.0 * i))
        nodes.append(Rigid(Scale(inner, 0.4), c, rot((1, -i, 0.5), -15.0 * (i + 1))))
    return union_of(nodes)


def scene_smooth_blobs():
    mats = [(0.9, 0.1 * i, 0.2, 0.0, 0.1 * i, 1.0) for i in range(7)]
    rng = np.random.default_rng(5)
    nodes = [Rigid(Prim("sphere", 0.2 + 0.03 * i, mat=mats[i]), tuple(rng.uniform(-0.6, 0.6, 3))) for i in range(6)]
    s = union_of(nodes, "smooth_union", 0.2)
    return Comb("smooth_subtract", s, Rigid(Prim("box", 0.25, 0.25, 1.5, mat=mats[6]), (0.1, 0.1, 0.0), rot((0, 1, 0), 30.0)), 0.12)


def scene_rotated_solids():
    a = Rigid(Prim("box", 0.7, 0.5, 0.3, mat=(0.3, 0.6, 0.9, 0.2, 0.4, 0.6)), (0.1, 0.0, -0.1), rot((1, 1, 0), 50.0))
    b = Rigid(Prim("cylinder", 0.45, 0.9, mat=(0.9, 0.6, 0.3, 0.6, 0.4, 0.2)), (-0.1, 0.1, 0.0), rot((0, 1, 1), -70.0))
    c = Rigid(Prim("torus", 0.6, 0.12, mat=(0.5, 0.5, 0.5, 1.0, 0.0, 1.0)), (0.0, 0.0, 0.2), rot((1, 0, 1), 110.0))
    d = Prim("plane", 0.6, -0.3, 1.1, 0.35, mat=(0.0, 0.2, 0.0, 0.0, 0.9, 0.8))       # not a unit normal
    return Comb("subtract", Comb("union", Comb("intersect", a, b), c), d)


def scene_scaled_shells():
    a = Scale(Shell(Prim("sphere", 0.6, mat=(0.2, 0.2, 0.9, 0.1, 0.1, 0.1)), 0.05), 1.5)
    b = Rigid(Scale(Shell(Round(Prim("box", 0.8, 0.6, 0.4, mat=(0.9, 0.2, 0.2, 0.9, 0.9, 0.9)), 0.1), 0.03), 0.75), (0.2, 0.1, 0.0),
              rot((2, -1, 1), 65.0))
    c = Prim("plane", 0.0, 0.0, 1.0, 0.07, mat=(0.2, 0.9, 0.2, 0.5, 0.5, 0.5))
    return Comb("intersect", Comb("union", a, b), c)


def scenes():
    return {"sixteen": scene_sixteen(), "every_opcode": scene_every_opcode(), "nested_frames": scene_nested_frames(),
            "smooth_blobs": scene_smooth_blobs(), "rotated_solids": scene_rotated_solids(), "scaled_shells": scene_scaled_shells()}


# ---- random scenes: trees of the classes above, nested up to the machine's stack limits ----
MAX_VALUES, MAX_FRAMES = 8, 4                          # SDFV_PROGRAM_MAX_VALUES, SDFV_PROGRAM_MAX_FRAMES
RANDOM_SCENES_SEED = 20261019


def stack_needs(node):
    """(values, frames) the emitted program's stacks reach below this node: a Comb evaluates a, keeps it, evaluates b."""
    if isinstance(node, Prim):
        return 1, 0
    if isinstance(node, Comb):
        (va, fa), (vb, fb) = stack_needs(node.a), stack_needs(node.b)
        return max(va, 1 + vb), max(fa, fb)
    v, f = stack_needs(node.child)
    return v, f + isinstance(node, (Rigid, Scale))


def _random_tree(rng, values, frames, prims):
    """A tree whose program needs at most `values` stack slots and `frames` open frames, of about `prims` primitives."""
    u = rng.uniform
    size = lambda: 0.15 + 0.6 * rng.beta(2.0, 2.0)     # noqa: E731
    roll = rng.random()
    if frames > 0 and roll < 0.28:
        if rng.random() < 0.6:
            R3 = None if rng.random() < 0.3 else rot(rng.normal(size=3), u(-180.0, 180.0))
            return Rigid(_random_tree(rng, values, frames - 1, prims), tuple(u(-0.4, 0.4, 3)), R3)
        return Scale(_random_tree(rng, values, frames - 1, prims), u(0.5, 1.6))
    if roll < 0.36:
        return Round(_random_tree(rng, values, frames, prims), u(0.01, 0.12))
    if roll < 0.42:
        return Shell(_random_tree(rng, values, frames, prims), u(0.03, 0.15))
    if values >= 2 and prims >= 2:
        kind = ("union", "intersect", "subtract", "smooth_union", "smooth_subtract")[int(rng.integers(5))]
        k = u(0.03, 0.3) if kind.startswith("smooth") else None
        left = 1 if rng.random() < 0.55 else int(rng.integers(1, prims))   # mostly right-deep: that is what fills the value stack
        return Comb(kind, _random_tree(rng, values, frames, left), _random_tree(rng, values - 1, frames, prims - left), k)
    mat = tuple(np.round(u(0.0, 1.0, 6), 3))
    kind = ("sphere", "cube", "box", "cylinder", "torus", "plane")[int(rng.integers(6))]
    if kind in ("sphere", "cube"):
        return Prim(kind, size(), mat=mat)
    if kind == "box":
        return Prim(kind, size(), size(), size(), mat=mat)
    if kind == "cylinder":
        return Prim(kind, size(), size(), mat=mat)
    if kind == "torus":
        return Prim(kind, u(0.3, 0.8), u(0.08, 0.3), mat=mat)
    nrm = rng.normal(size=3)
    nrm /= np.linalg.norm(nrm)
    return Prim(kind, *nrm, u(-0.4, 0.4), mat=mat)


def random_scenes(seed, n):
    """-> ([(scene, seed of its scene_points)], draws rejected): n random trees of Prim, Rigid, Scale, Comb, Round and Shell.  A
    draw is kept when the REFERENCE ALONE says its comparison decides something -- at most 2 % of the scene's points left out of
    the material comparison and every bound below 1e-4, the two conditions the hand-written scenes are held to -- and redrawn
    otherwise.  Every fourth scene is drawn until it needs all 8 value slots, the one after it until it opens 4 frames."""
    rng = np.random.default_rng(seed)
    kept, rejected = [], 0
    while len(kept) < n:
        i = len(kept)
        for _ in range(400):
            scene = _random_tree(rng, MAX_VALUES, MAX_FRAMES, int(rng.integers(2, 20)))
            v, f = stack_needs(scene)
            if (i % 4 == 0 and v < MAX_VALUES) or (i % 4 == 1 and f < MAX_FRAMES):
                continue                               # (not a rejected draw: a draw of another shape than the one asked for)
            break
        else:
            raise AssertionError("no tree of the shape asked for")
        points_seed = 1000 * int(seed) % 100003 + i
        _, bound, _, decided = evaluate(scene, scene_points(points_seed))
        if 1.0 - decided.mean() <= 0.02 and np.isfinite(bound).all() and bound.max() < 1e-4:
            kept.append((scene, points_seed))
        else:
            rejected += 1
    return kept, rejected


SCENE_SEEDS = {"sixteen": 21, "every_opcode": 22, "nested_frames": 23, "smooth_blobs": 24, "rotated_solids": 25, "scaled_shells": 26}
SCENE_GRID = (12, 10, 8)


def scene_points(seed, n=4096, grid=SCENE_GRID):
    """n seeded points in and around the unit box plus the voxel positions of a small grid over it, as f32."""
    rng = np.random.default_rng(seed)
    axes = [np.linspace(-1.0, 1.0, d) for d in grid]
    zz, yy, xx = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.concatenate([rng.uniform(-1.3, 1.3, (n, 3)), np.stack([xx, yy, zz], axis=-1).reshape(-1, 3)]).astype(np.float32)


FRAME_CHAINS = {
    "bare": [],
    "rotated and moved": [("rigid", (rot((1, 2, -1), 40.0), (0.3, -0.2, 0.1)))],
    "moved": [("rigid", (None, (-0.25, 0.5, 0.125)))],
    "scaled": [("scale", 1.75)],
    "nested to depth 4": [("rigid", (rot((0, 1, 1), 75.0), (0.1, 0.2, -0.3))), ("scale", 0.6),
                          ("rigid", (rot((3, -1, 2), -130.0), (-0.2, 0.05, 0.15))), ("scale", 2.5)],
}

KNOWN_PRIMS = [Prim("sphere", 0.45), Prim("cube", 0.4), Prim("box", 0.5, 0.3, 0.2), Prim("cylinder", 0.3, 0.55),
               Prim("cylinder", 0.6, 0.15), Prim("torus", 0.6, 0.2), Prim("plane", 0.6, 0.0, 0.8, 0.25),
               Prim("plane", 1.5, -2.0, 0.5, -0.4)]


def known_cases(seed=3, n=512):
    """[(label, scene node, world points f32 [n, 3], known distance [n], extra tolerance [n])]: every primitive's feature classes
    under every chain of FRAME_CHAINS.  The extra tolerance is what rounding the world point to f32 moves the answer by:
    Lipschitz constant times the distance between the rounded point and the constructed one."""
    rng = np.random.default_rng(seed)
    out = []
    for prim in KNOWN_PRIMS:
        for chain_name, chain in FRAME_CHAINS.items():
            for feature, (local, dist, lip) in known_points(prim, rng, n).items():
                world, scale = place(chain, local)
                w32 = world.astype(np.float32)
                moved = np.linalg.norm(w32.astype(np.float64) - world, axis=1)
                out.append((f"{prim.kind}{prim.params} {feature}, {chain_name}", wrap(prim, chain), w32, dist * scale, lip * moved))
    return out
