"""What a mesh MEANS: statements M1 .. M7 that any correct extraction of a known solid satisfies, checked against a float64
distance function alone -- no reference mesh, so they hold where no restatement can run (1024 and 2048 cells).  The shape
follows demo_geometry.check_records: a Report, one named statement per failure.  Calls nothing of the library and shares no
code with tests/mesh_ref.py.  ("What a mesh means", has the statements with their derivations.)

`field` is an adapter with
  evaluate(points [m, 3] f32) -> (d [m] float64, bound [m], material [m, 6] float64, decided [m]);
  normal(points) -> (n64 [m, 3], tol_sin [m], decided [m]); a zero n64 is the mesher's "unset" normal;
  L: the Lipschitz constant of d;   inside_box: the outermost lattice layer is decidedly outside (the surface is closed).
ProgramField and DemoField below build it from tests/program_geometry.py and tests/demo_geometry.py.

M1 and the whole-mesh half of M5 are torch: on the device when the mesh is there (int64 keys, sort), on the host otherwise.  The
statements that need the field run in numpy float64, over every vertex or, with sample = (seed, k), over k seeded vertices and k / 8
seeded triangles; M4 and the volume bracket need the whole lattice in float64 and are left out when a sample is given."""
import numpy as np
import torch

import demo_geometry as DG
import program_geometry as PG
from demo_geometry import Report
from program_geometry import U

F = np.float32
DUAL = 4
ALL = ("M1", "M2", "M3", "M4", "M5", "M6", "M7")
NO_NORMALS = ("M1", "M2", "M3", "M4", "M5")            # the lattice route: its normals are another definition
CAP = 0.02


# ---- the lattice ----
def per_axis(cells):
    return (int(cells),) * 3 if np.ndim(cells) == 0 else tuple(int(c) for c in cells)


def tables(cells, bb):
    """Per axis the cells + 1 coordinates (float)i / (float)cells * size + min, each step one numpy float32 operation."""
    out = []
    for a, c in enumerate(per_axis(cells)):
        lo, size = F(bb[a]), F(bb[3 + a]) - F(bb[a])
        t = np.arange(c + 1, dtype=F) / F(c) * size + lo
        assert t.dtype == F and (np.diff(t) > 0).all(), "lattice coordinates that do not increase"
        out.append(t)
    return out


def lattice_positions(tabs):
    zz, yy, xx = np.meshgrid(tabs[2], tabs[1], tabs[0], indexing="ij")
    return np.stack([xx, yy, zz], axis=-1).reshape(-1, 3)


# ---- the adapters ----
class ProgramField:
    """A scene of tests/program_geometry.py over the lattice of `cells` cells of `bb`."""
    def __init__(self, scene, cells, bb):
        self.scene, self.cells, self.bb = scene, per_axis(cells), tuple(float(v) for v in bb)
        self.L = PG.lipschitz(scene)
        self._inside = None

    def evaluate(self, points):
        return PG.evaluate(self.scene, points)

    def normal(self, points):
        return PG.tetra_normal(self.scene, points)

    @property
    def inside_box(self):
        if self._inside is None:
            self._inside = boundary_is_outside(self, self.cells, self.bb)
        return self._inside


class DemoField:
    """The demo family (0 demo, 1 cube, 2 sphere) of tests/demo_geometry.py.  L = 1: a Chebyshev ball's and a ball's distances,
    their max with a negation.  The normal's bound is the one statement A grants sdfv_normal_points: the reference's own
    per-component bound, as a vector's length."""
    L = 1.0

    def __init__(self, prm, sdf_id, cells, bb):
        self.prm, self.sdf_id, self.cells, self.bb = prm, sdf_id, per_axis(cells), tuple(float(v) for v in bb)
        self._inside = None

    @np.errstate(all="ignore")                          # (the ball's normal at its centre, a lattice point)
    def evaluate(self, points):
        s = DG.evaluate(self.prm, np.asarray(points, F).astype(np.float64), self.sdf_id)
        return s.d, s.bound, np.concatenate([s.color, s.props], axis=1), s.decided & (s.color_err == 0.0).all(axis=1)

    @np.errstate(all="ignore")
    def normal(self, points):
        n, ne, decided = DG.normals(self.prm, np.asarray(points, F).astype(np.float64), self.sdf_id)
        return n, np.linalg.norm(ne, axis=1), decided

    @property
    def inside_box(self):
        if self._inside is None:
            self._inside = boundary_is_outside(self, self.cells, self.bb)
        return self._inside


def boundary_is_outside(field, cells, bb, exact_up_to=200_000):
    """Is the outermost lattice layer decidedly outside?  Small lattices: evaluated point by point.  Large ones: the six faces
    are sampled at 65 x 65 points each, and a face is outside where every sample exceeds its bound by L times the half diagonal of
    the patch between samples (no zero within reach); anything less is reported as `not inside`."""
    cells = per_axis(cells)
    if 2 * sum((cells[a] + 1) * (cells[b] + 1) for a, b in ((0, 1), (0, 2), (1, 2))) <= exact_up_to:
        tabs = tables(cells, bb)
        p = lattice_positions(tabs)
        edge = np.zeros(len(p), bool)
        for a in range(3):
            edge |= (p[:, a] == tabs[a][0]) | (p[:, a] == tabs[a][-1])
        d, bound, _, _ = field.evaluate(p[edge])
        return bool((d > bound).all())
    lo, hi = np.array(bb[:3], np.float64), np.array(bb[3:], np.float64)
    for a in range(3):
        o0, o1 = [b for b in range(3) if b != a]
        g0, g1 = np.linspace(lo[o0], hi[o0], 65), np.linspace(lo[o1], hi[o1], 65)
        reach = 0.5 * np.hypot(g0[1] - g0[0], g1[1] - g1[0]) * 1.001 + 1e-6      # (the f32 rounding of the sample points)
        for side in (lo[a], hi[a]):
            p = np.zeros((65 * 65, 3))
            p[:, a] = side
            p[:, o0], p[:, o1] = [g.reshape(-1) for g in np.meshgrid(g0, g1, indexing="ij")]
            d, bound, _, _ = field.evaluate(p.astype(F))
            if not (d - bound > field.L * reach).all():
                return False
    return True


# ---- helpers ----
def _torch(x, dtype=None):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x))
    return t if dtype is None else t.to(dtype)


def _host(t):
    return t.detach().cpu().numpy()


def _expect(rep, statement, ok, what, *arrays):
    ok = np.asarray(ok)
    if not ok.all():
        k = int(np.flatnonzero(~ok.reshape(-1))[0])
        detail = ", ".join(f"{np.asarray(a).reshape(ok.size, -1)[k]}" for a in arrays)
        rep.fail(statement, f"{what}: {int((~ok).sum())} of {ok.size} (first at {k}: {detail})")


def _share(rep, statement, name, undecided, cap=CAP):
    share = float(np.mean(undecided)) if np.size(undecided) else 0.0
    rep.figures[name] = share
    if share > cap:
        rep.fail(statement, f"{name}: {100 * share:.2f} % over the cap of {100 * cap:.0f} %")


def _ratio(rep, name, value, bound):
    if np.size(value):
        rep.worst(name, float((np.asarray(value) / np.maximum(np.asarray(bound), 1e-300)).max()))


def _locate(pos, tabs):
    """pos [V, 3] f32 tensor, tabs: three f32 tensors -> (j [V, 3]: the largest j with tab[j] <= p, clamped into the table;
    on [V, 3]: p equals tab[j] bit for bit; inbox [V, 3])."""
    j, on, inbox = [], [], []
    for a in range(3):
        t, p = tabs[a], pos[:, a].contiguous()
        ja = torch.searchsorted(t, p, right=True) - 1
        ok = (ja >= 0) & (p <= t[-1])                   # (false for a NaN)
        ja = ja.clamp(0, len(t) - 1)
        j.append(ja)
        on.append(ok & (t[ja] == p))
        inbox.append(ok)
    return torch.stack(j, 1), torch.stack(on, 1), torch.stack(inbox, 1)


# ---- the statements ----
def check_mesh(vertices, indices, cells, bb, field, algorithm, with_materials, report=None, sample=None, chi=None,
               statements=ALL):
    """M1 .. M7 over one mesh.  vertices [V, 12] f32 (position, normal, six material fields) and indices [3 T]: numpy arrays or
    torch tensors (host or device).  cells: per axis, or one number; bb = min.xyz + max.xyz; algorithm 0 (marching cubes, also
    the sparse route) or 4 (dual contouring); chi: the Euler characteristic where the model's topology is known by definition.
    -> Report (failures by statement, figures)."""
    rep = Report() if report is None else report
    cells = per_axis(cells)
    dual = algorithm == DUAL
    assert algorithm in (0, DUAL)
    tabs = tables(cells, bb)
    V_t = _torch(vertices)
    I_t = _torch(indices, torch.int64).reshape(-1)
    dev = V_t.device
    nv, nt = int(V_t.shape[0]), int(I_t.shape[0]) // 3
    rep.figures["vertices"], rep.figures["triangles"] = nv, nt
    tt = [torch.from_numpy(t).to(dev) for t in tabs]
    pos = V_t[:, :3].contiguous()
    L = float(field.L)
    h = np.array([float(np.diff(t.astype(np.float64)).max()) for t in tabs])      # the longest edge per axis
    diag = float(np.linalg.norm(h))
    reach = max(abs(float(v)) for v in bb)

    # ---- M1: on the lattice ----
    j, on, inbox = _locate(pos, tt)
    if "M1" in statements and nv:
        if not bool(inbox.all()):
            bad = int((~inbox.all(1)).sum())
            rep.fail("M1", f"{bad} of {nv} vertices outside the box")
    if not dual:
        n_on = on.sum(1)
        at_point = n_on == 3                                      # t rounded onto an end of its edge: the edge is not told
        edge_ok = (n_on == 2) & inbox.all(1)
        axis = (~on).to(torch.int64).argmax(1)
        stride = [1, cells[0] + 1, (cells[0] + 1) * (cells[1] + 1)]
        key = (j[:, 2] * stride[2] + j[:, 1] * stride[1] + j[:, 0]) * 3 + axis
        if "M1" in statements and nv:
            bad = ~(edge_ok | at_point)
            if bool(bad.any()):
                k = int(torch.nonzero(bad)[0])
                rep.fail("M1", f"{int(bad.sum())} of {nv} vertices do not have two coordinates on the lattice "
                               f"(first: vertex {k} at {_host(pos[k])}, {int(n_on[k])} on)")
            ks = torch.sort(key[edge_ok])[0]
            dup = int((ks[1:] == ks[:-1]).sum()) if len(ks) > 1 else 0
            if dup:
                rep.fail("M1", f"{dup} vertices share their lattice edge with another")
            # (t lands on an end of its edge where the distance there is zero within rounding: M2 asks the field)
            rep.figures["M1 vertices on a lattice point"] = int(at_point.sum())
    else:
        # the cells a vertex can be listed for: [j - 1, j] where it lies on a lattice coordinate, else j; clamped to the cells
        cmax = torch.tensor([c - 1 for c in cells], device=dev)
        chi_c = torch.minimum(j, cmax)
        clo = torch.where(on & (j > 0), j - 1, chi_c)
        flat = lambda c: (c[:, 2] * cells[1] + c[:, 1]) * cells[0] + c[:, 0]   # noqa: E731
        kmin, kmax = flat(clo), flat(chi_c)
        if "M1" in statements and nv > 1:
            # vertices come in cell order: some choice of one candidate each increases strictly.  Necessary for that: every
            # vertex has a candidate above the lowest candidates of all before it, and the vertices with one candidate increase
            before = torch.cummax(kmin, 0)[0][:-1]
            late = kmax[1:] <= before
            if bool(late.any()):
                k = int(torch.nonzero(late)[0]) + 1
                rep.fail("M1", f"{int(late.sum())} of {nv} vertices lie in no closed cell after their predecessors' (first: vertex {k})")
            one = kmin == kmax
            ko = kmin[one]
            if len(ko) > 1 and not bool((ko[1:] > ko[:-1]).all()):
                rep.fail("M1", "vertices strictly inside their cells are not in cell order, or two share a cell")

    # ---- the sample ----
    rng = np.random.default_rng(0 if sample is None else sample[0])
    if sample is not None and nv > sample[1]:
        vs = np.sort(rng.choice(nv, sample[1], replace=False))
    else:
        vs = np.arange(nv)
    if sample is not None and nt > sample[1] // 8:             # (a face costs a dozen reference normals, a vertex one)
        ts = np.sort(rng.choice(nt, max(sample[1] // 8, 1), replace=False))
    else:
        ts = np.arange(nt)
    vs_t = torch.from_numpy(vs).to(dev)
    sv = np.ascontiguousarray(_host(V_t[vs_t]), F).reshape(-1, 12)
    sp = sv[:, :3]
    need_field = any(s in statements for s in ("M2", "M3", "M6", "M7"))
    if need_field and len(sp):
        dv, bv, matv, mdec = field.evaluate(sp)
    else:
        dv, bv, matv, mdec = np.zeros(0), np.zeros(0), np.zeros((0, 6)), np.zeros(0, bool)

    # ---- M2, M3 ----
    if not dual and nv and "M2" in statements and bool(at_point.any()):
        # a vertex ON a lattice point: t = d0 / (d0 - d1) rounded to 0 or 1, or u0 + t (u1 - u0) to an end -- the end's distance
        # is below an ulp of the coordinate's share of the edge's: |d| <= bound + L (2 U size + U |p|), doubled twice over
        q = _host(pos[at_point][:65536])
        dq, bq, _, _ = field.evaluate(q)
        size_max = max(float(t[-1]) - float(t[0]) for t in tabs)
        allowed = bq + 8.0 * U * L * (size_max + reach)
        _expect(rep, "M2", np.abs(dq) <= allowed, "a vertex on a lattice point the surface does not pass through", q, dq, allowed)
    if not dual and len(sp) and ("M2" in statements or "M3" in statements):
        sj, sa, sok = _host(j[vs_t]), _host(axis[vs_t]), _host(edge_ok[vs_t])
        sj, sa, spk, dk, bk = sj[sok], sa[sok], sp[sok], dv[sok], bv[sok]
        rows = np.arange(len(sj))
        p0 = np.stack([tabs[a][sj[:, a]] for a in range(3)], axis=1)
        j1 = sj.copy()
        j1[rows, sa] += 1
        p1 = np.stack([tabs[a][j1[:, a]] for a in range(3)], axis=1)
        d0, b0, _, _ = field.evaluate(p0)
        d1, b1, _, _ = field.evaluate(p1)
        both = (np.abs(d0) > b0) & (np.abs(d1) > b1)
        if "M2" in statements:
            _share(rep, "M2", "M2 share of edges with an undecided end", ~both, cap=1.0)
            _expect(rep, "M2", ~both | ((d0 < 0) != (d1 < 0)), "a vertex on an edge whose ends lie on one side of the surface",
                    spk, d0, d1)
        if "M3" in statements:
            crossing = both & ((d0 < 0) != (d1 < 0))
            S = np.abs(d0) + np.abs(d1)
            he = np.linalg.norm(p1.astype(np.float64) - p0.astype(np.float64), axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                # t = d0 / (d0 - d1) from f32 distances within b0, b1 of these: first order, plus the divide's and the
                # subtraction's own roundings; then u0 + t (u1 - u0) and u * size + min: U (2 h + 2 size + |p|) in world units
                dt = (np.abs(d1) * b0 + np.abs(d0) * b1) / (S * S) + 2.0 * U
                size = np.array([float(tabs[a][-1]) - float(tabs[a][0]) for a in range(3)])[sa]
                rounding = 2.0 * L * (dt * he + U * (2.0 * he + 2.0 * size + np.abs(spk[rows, sa].astype(np.float64))))
                limit = np.maximum(np.abs(d0), np.abs(d1)) * np.maximum(L * he / S - 1.0, 0.0) + bk + rounding
            if crossing.any():
                _ratio(rep, "M3 |d(v)| / limit", np.abs(dk)[crossing], limit[crossing])
                rep.worst("M3 excess over the limit without rounding", (np.abs(dk) - (limit - rounding))[crossing].max())
                # the Lipschitz constant is itself part of the statement: S <= L h
                _expect(rep, "M3", ~crossing | (S <= L * he + b0 + b1), "an edge whose end distances differ by more than L times its length",
                        d0, d1, he)
            _expect(rep, "M3", ~crossing | (np.abs(dk) <= limit), "a vertex further from the surface than its edge's end distances allow",
                    spk, dk, limit)
    if dual and len(sp) and "M3" in statements:
        limit = L * diag + bv
        _ratio(rep, "M3 |d(v)| / limit", np.abs(dv), limit)
        _expect(rep, "M3", np.abs(dv) <= limit, "a vertex further from the surface than its cell's diagonal", sp, dv, limit)

    # ---- the whole lattice in float64: M4 and the volume bracket ----
    lattice = None
    if sample is None and ("M4" in statements or "M5" in statements):
        known = getattr(field, "_lattice_signs", None)                    # (one field, several routes: evaluated once)
        lattice_key = (cells, tuple(float(v) for v in bb))
        if known is None or known[0] != lattice_key:
            dl, bl, _, _ = field.evaluate(lattice_positions(tabs))
            field._lattice_signs = known = (lattice_key, dl, bl)
        _, dl, bl = known
        shape = (cells[2] + 1, cells[1] + 1, cells[0] + 1)
        inside, outside = (dl < -bl).reshape(shape), (dl > bl).reshape(shape)
        lattice = (inside, outside)
    if "M4" in statements and lattice is not None:
        inside, outside = lattice
        _share(rep, "M4", "M4 share of lattice points undecided in sign", ~(inside | outside))
        sl = [slice(None)] * 3
        cross = np.zeros(inside.shape + (3,), bool)
        for a in range(3):                               # array axis 2 - a is lattice axis a
            lo_, hi_ = list(sl), list(sl)
            lo_[2 - a], hi_[2 - a] = slice(None, -1), slice(1, None)
            lo_, hi_ = tuple(lo_), tuple(hi_)
            cross[lo_ + (a,)] = (inside[lo_] & outside[hi_]) | (outside[lo_] & inside[hi_])
        rep.figures["M4 decided crossing edges"] = int(cross.sum())
        kk, jj, ii, aa = np.nonzero(cross)
        if not dual:
            have = np.zeros(cross.size, bool)
            have[_host(key[edge_ok])] = True
            # (a vertex that landed on a lattice point stands for every edge that ends there)
            pts = _host(j[at_point])
            near = np.zeros(inside.shape, bool)
            near[pts[:, 2], pts[:, 1], pts[:, 0]] = True
            nb = np.stack([ii, jj, kk], axis=1)
            nb[np.arange(len(aa)), aa] += 1
            ok = have.reshape(cross.shape)[kk, jj, ii, aa] | near[kk, jj, ii] | near[nb[:, 2], nb[:, 1], nb[:, 0]]
            _expect(rep, "M4", ok, "a lattice edge whose ends decidedly differ in sign carries no vertex", np.stack([ii, jj, kk, aa], 1))
        else:
            # a cell with a decided crossing edge is active: some vertex can be listed for it
            active = np.zeros((cells[2], cells[1], cells[0]), bool)
            for a in range(3):
                o0, o1 = [b for b in range(3) if b != a]
                c = cross[..., a]
                for s0 in (0, 1):
                    for s1 in (0, 1):
                        src, dst = [slice(None)] * 3, [slice(None)] * 3
                        src[2 - a], dst[2 - a] = slice(0, cells[a]), slice(0, cells[a])
                        for o, s in ((o0, s0), (o1, s1)):
                            src[2 - o] = slice(s, cells[o] + s)          # the edge's point is the cell's corner offset by s
                        active[tuple(dst)] |= c[tuple(src)]
            covered = np.zeros_like(active)
            lo_c, hi_c = _host(clo), _host(chi_c)
            for ox in (0, 1):
                for oy in (0, 1):
                    for oz in (0, 1):
                        c = np.where(np.array([ox, oy, oz], bool)[None, :], hi_c, lo_c)
                        covered[c[:, 2], c[:, 1], c[:, 0]] = True
            _expect(rep, "M4", ~active | covered, "a cell with a decided crossing edge has no vertex", active)

    # ---- M5: closed, oriented, outward ----
    if "M5" in statements:
        tri = I_t.reshape(-1, 3)
        if nt and (int(tri.min()) < 0 or int(tri.max()) >= nv):
            rep.fail("M5", f"an index outside [0, {nv})")
        else:
            used = torch.zeros(nv, dtype=torch.bool, device=dev)
            if nt:
                used[I_t] = True
            if dual and nv:
                # (an edge on the box's boundary emits no quad: a cell of the outermost layer may keep its vertex to itself)
                used |= ((clo == 0) | (chi_c == cmax)).any(1)
            if not bool(used.all()):
                rep.fail("M5", f"{int((~used).sum())} of {nv} vertices are used by no triangle")
            closed = False
            if nt:
                a_, b_ = tri.reshape(-1), tri[:, [1, 2, 0]].reshape(-1)
                fwd, rev = torch.sort(a_ * nv + b_)[0], torch.sort(b_ * nv + a_)[0]
                twice = int((fwd[1:] == fwd[:-1]).sum())
                closed = bool(torch.equal(fwd, rev))
                if field.inside_box:
                    if not closed:
                        rep.fail("M5", f"{int((fwd != rev).sum())} directed edges without their reverse: the mesh is open or not oriented")
                    if twice and not dual:
                        rep.fail("M5", f"{twice} directed edges are used twice")
                # (dual contouring gives the sheets that cross one cell ONE vertex: its counts are not the surface's)
                if chi is not None and field.inside_box and not dual:
                    got_chi = nv - (3 * nt) // 2 + nt
                    rep.figures["Euler characteristic"] = got_chi
                    if got_chi != chi:
                        rep.fail("M5", f"Euler characteristic {got_chi}, not {chi}")
                p64 = pos.to(torch.float64)
                v0, v1, v2 = p64[tri[:, 0]], p64[tri[:, 1]], p64[tri[:, 2]]
                volume = float((v0 * torch.linalg.cross(v1, v2)).sum() / 6.0)
                rep.figures["signed volume"] = volume
                if field.inside_box and closed:
                    if not volume > 0.0:
                        rep.fail("M5", f"signed volume {volume}: the mesh faces inwards")
                    if lattice is not None:
                        inside, outside = lattice
                        cz, cy, cx = cells[2], cells[1], cells[0]
                        all_in, any_in = np.ones((cz, cy, cx), bool), np.zeros((cz, cy, cx), bool)
                        for oz in (0, 1):
                            for oy in (0, 1):
                                for ox in (0, 1):
                                    s = (slice(oz, oz + cz), slice(oy, oy + cy), slice(ox, ox + cx))
                                    all_in &= inside[s]
                                    any_in |= ~outside[s]
                        cell_volume = np.array([np.diff(t.astype(np.float64)) for t in tabs], dtype=object)
                        vol3 = cell_volume[2][:, None, None] * cell_volume[1][None, :, None] * cell_volume[0][None, None, :]
                        low, high = float((vol3 * all_in).sum()), float((vol3 * any_in).sum())
                        rep.figures["volume bracket"] = (low, high)
                        if not (low * (1.0 - 1e-9) <= volume <= high * (1.0 + 1e-9)):
                            rep.fail("M5", f"signed volume {volume} outside [{low}, {high}]: the cells decidedly inside, the cells not decidedly outside")
                # Faces against the field's normal at their centroid (with a sample: k / 8 seeded triangles; a closed oriented
                # surface faces one way per component, and the signed volume above is over all of it).
                # Dual contouring is left out: its vertex is stated to be in its cell and no more, and a quad of four such
                # vertices may fold (the restated mesh of scaled_shells at 12 cells has two that do); its faces are held by
                # the closed, consistently oriented whole and its positive, bracketed volume.
                if not dual:
                    t3 = _host(p64[tri[torch.from_numpy(ts).to(dev)]])               # [k, 3, 3]
                    fn = np.cross(t3[:, 1] - t3[:, 0], t3[:, 2] - t3[:, 0])
                    big = 0.5 * np.linalg.norm(fn, axis=1) > 1e-12
                    t3, fn = t3[big], fn[big]
                    centre = t3.mean(axis=1)
                    cn, _, cdec = field.normal(centre.astype(F))
                    cdec = cdec & (np.linalg.norm(cn, axis=1) > 0.5)
                    # decided where the SURFACE is one smooth piece across the face and its cell, by the reference alone: its
                    # normals at the face's corners and at the eight corners of the centroid's cell are decided and within 30
                    # degrees of the centroid's.  (A cell coarser than a shell's thickness or a pillar's radius holds two
                    # sheets: what a mesher makes of it faces wherever the lattice's signs send it.)
                    cj = [np.clip(np.searchsorted(tabs[a], centre[:, a].astype(F), side="right") - 1, 0, cells[a] - 1) for a in range(3)]
                    around = [np.stack([tabs[a][cj[a] + o[a]] for a in range(3)], axis=1)
                              for o in ((ox, oy, oz) for oz in (0, 1) for oy in (0, 1) for ox in (0, 1))]
                    for pts in [t3[:, c].astype(F) for c in range(3)] + around:
                        kn, _, kdec = field.normal(pts)
                        cdec &= kdec & ((kn * cn).sum(axis=1) > np.cos(np.radians(30.0)))
                    dots = (fn * cn).sum(axis=1)
                    rep.figures["M5 share of triangles whose centroid normal is undecided"] = float(1.0 - cdec.mean()) if len(cdec) else 0.0
                    _expect(rep, "M5", ~cdec | (dots > 0.0), "a triangle that faces against the surface's normal at its centroid",
                            centre, cn)

    # ---- M6: normals ----
    if "M6" in statements and len(sp):
        got = sv[:, 3:6].astype(np.float64)
        n64, tol, ndec = field.normal(sp)
        # (the demo's cube has no unit normal inside it -- the mesher's "unset" zero -- nor beyond two of its faces: there the
        # reference's components are exact and the record holds them as they are)
        unset = ndec & (np.abs(np.linalg.norm(n64, axis=1) - 1.0) > 1e-9)
        ndec_unit = ndec & ~unset
        length = np.linalg.norm(got, axis=1)
        _share(rep, "M6", "M6 share of normals undecided", ~ndec)
        _expect(rep, "M6", ~unset | (got == n64).all(axis=1), "a normal that is not the reference's where that is no unit vector", sp, got, n64)
        _expect(rep, "M6", ~ndec_unit | (np.abs(length - 1.0) <= 16.0 * U), "a normal that is not of unit length", got, length)
        sine = np.linalg.norm(np.cross(got, n64), axis=1) / np.maximum(length, 1e-300)
        away = (got * n64).sum(axis=1) <= 0.0
        if ndec_unit.any():
            _ratio(rep, "M6 sine / tolerance", sine[ndec_unit], tol[ndec_unit] + 8.0 * U)
            rep.figures["M6 median tolerance"] = float(np.median(tol[ndec_unit]))
        _expect(rep, "M6", ~ndec_unit | ((sine <= tol + 8.0 * U) & ~away), "a normal off the float64 normal of its position", sp, got, n64, tol)

    # ---- M7: materials ----
    if "M7" in statements and len(sp):
        got = np.ascontiguousarray(sv[:, 6:12])
        if with_materials:
            want = np.ascontiguousarray(matv, F)
            _share(rep, "M7", "M7 share of materials undecided", ~mdec)
            _expect(rep, "M7", ~mdec | (got.view(np.uint32) == want.view(np.uint32)).all(axis=1),
                    "material fields that are not the material of the vertex's position", sp, got, want)
        else:
            _expect(rep, "M7", (got.view(np.uint32) == 0).all(axis=1), "material fields set where none were asked for", got)
    return rep


def assert_mesh(label, rep):
    """Print the report's figures, then fail on its first statements."""
    figures = ", ".join(f"{k} = {v:.4g}" if isinstance(v, float) else f"{k} = {v}" for k, v in rep.figures.items())
    print(f"{label}: {figures}")
    assert not rep.failures, (label, rep.lines())


# ---- the models the CPU and the GPU tests share ----
UNIT_BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
ODD_BOX = (-0.9, -0.7, -1.0, 1.0, 0.8, 0.6)             # no cube, not centred
OBLIQUE = dict(t=(0.1, -0.05, 0.15), axis=(1, 2, 3), degrees=35.0, scale=0.8)


def oblique_primitives():
    """{name: (scene, Euler characteristic)}: single primitives scaled, turned about no lattice direction and moved off the
    centre, wholly inside the unit box: topology known by definition."""
    prims = {"sphere": (PG.Prim("sphere", 0.5, mat=(0.2, 0.5, 0.9, 0.1, 0.4, 1.0)), 2),
             "box": (PG.Prim("box", 0.5, 0.35, 0.25, mat=(0.9, 0.5, 0.2, 0.3, 0.6, 0.5)), 2),
             "cylinder": (PG.Prim("cylinder", 0.35, 0.5, mat=(0.3, 0.5, 0.2, 0.7, 0.2, 1.0)), 2),
             "torus": (PG.Prim("torus", 0.5, 0.2, mat=(0.6, 0.1, 0.7, 0.0, 0.9, 0.25)), 0)}
    R = PG.rot(OBLIQUE["axis"], OBLIQUE["degrees"])
    return {f"oblique {k}": (PG.Rigid(PG.Scale(p, OBLIQUE["scale"]), OBLIQUE["t"], R), chi) for k, (p, chi) in prims.items()}


def models():
    """{name: (scene, chi or None)}: the hand-written scenes of program_geometry and the oblique primitives."""
    out = {name: (scene, None) for name, scene in PG.scenes().items()}
    out.update(oblique_primitives())
    return out


def scene_big():
    """The model of the large shapes: a turned torus and a ball, disjoint and inside the unit box; L = 1, chi = 0 + 2."""
    torus = PG.Rigid(PG.Scale(PG.Prim("torus", 0.5, 0.15, mat=(0.8, 0.3, 0.1, 0.2, 0.6, 1.0)), 0.9), (-0.2, 0.1, 0.0),
                     PG.rot((1, 2, 3), 35.0))
    ball = PG.Rigid(PG.Prim("sphere", 0.2, mat=(0.1, 0.4, 0.9, 0.7, 0.3, 0.5)), (0.6, -0.6, 0.55))
    return PG.Comb("union", torus, ball)


BIG_CHI = 2


# ---- two meshes as sets, where they are (the sparse route's promise) ----
def _lexsort(rows):
    """The permutation that sorts the rows of an integer tensor [N, k] lexicographically: stable sorts, last column first."""
    perm = torch.arange(rows.shape[0], device=rows.device)
    for c in reversed(range(rows.shape[1])):
        perm = perm[torch.sort(rows[perm, c], stable=True)[1]]
    return perm


def _canonical(vertices, indices):
    """-> (the records as rows of 12 words, sorted; the triangles over the sorted records' positions, each rotated to start at
    its smallest entry, sorted).  Records that share a position share its place, so their order among themselves is no matter."""
    words = vertices.contiguous().view(torch.int32)
    perm = _lexsort(words[:, :3])
    rows = words[perm]
    first = torch.ones(len(rows), dtype=torch.bool, device=rows.device)
    first[1:] = (rows[1:, :3] != rows[:-1, :3]).any(1)
    place = torch.empty(len(rows), dtype=torch.int64, device=rows.device)
    place[perm] = torch.cumsum(first.to(torch.int64), 0) - 1
    tri = place[indices.to(torch.int64).reshape(-1, 3)]
    n = len(rows) + 1                                    # (the rotation whose first two entries are the smallest pair)
    turn = torch.stack([tri[:, k] * n + tri[:, (k + 1) % 3] for k in range(3)], 1).argmin(1)
    tri = torch.stack([torch.gather(tri, 1, ((turn + k) % 3)[:, None])[:, 0] for k in range(3)], 1)
    return rows, tri[_lexsort(tri)]


def same_mesh_as_a_set(va, ia, vb, ib):
    """Do two meshes hold the same vertex records, word for word, and the same triangles over them?  Torch tensors, compared
    where they are.  -> None or what differs"""
    if va.shape != vb.shape or ia.shape != ib.shape:
        return f"{tuple(va.shape)} vertices and {tuple(ia.shape)} indices against {tuple(vb.shape)} and {tuple(ib.shape)}"
    (ra, ta), (rb, tb) = _canonical(va, ia), _canonical(vb, ib)
    if not torch.equal(ra, rb):
        return f"{int((ra != rb).any(1).sum())} vertex records differ"
    if not torch.equal(ta, tb):
        return f"{int((ta != tb).any(1).sum())} triangles differ"
    return None
