"""CPU tests of what the GRID route MEANS: the oracle (oracle/*.c, to which the kernels are held bit for bit elsewhere) and
the host's sdfv_camera_look_at (the demo's C++ SDF objects sample on the device: tests/test_gpu_demo_meaning.py) against the float64 reference written from the definitions (tests/demo_geometry.py).  Every
tolerance is that reference's derived bound or a cap stated here; the shares the caps limit are the reference's alone and are
printed.  No device needed.

A. or_sample and or_fill_dense of the demo family: the distance within the bound, every other word equal wherever the
   reference decides it (colours that are computed -- the `normal` material -- within their bound; the texel's colour words as
   the 8-bit code they decode).  At most 2 % undecided per case; a case is one entry point on one member of the family (the
   fill's two lattices count together: on the 9 x 7 x 5 one alone the sphere has 8 of 315 texels whose unit normal has a
   component of exactly 1, 2/3 or 1/3, where 255 c is an integer).
B. every field of sdfv_camera_look_at and the oracle's or_camera_look_at within the bound.
C. over scenes (a) .. (f) of demo_geometry.scenes(), for the march records (demo_geometry.check_records):
   C1 hit_pos lies on its own pixel's float64 ray and t is the length travelled from the start point;
   C2 d(phi(hit_pos)) <= 1e-5 + the hit cell's interpolation bound;
   C3 a hit that is not the ray's first sample has d(phi(hit_pos)) >= -(cell bound + (max n/(n-1) - 1) min(0.9, t) + 1e-5);
   C4 a ray that enters the solid eroded by one cell diagonal beyond its start is a hit, no later than that entry (plus the
      overshoot of a Lipschitz constant above 1, which the entry's own derivation carries); a ray that misses the solid
      dilated by one cell diagonal is not a hit;
   C5 depth is 0.5 ndc_z + 0.5 of hit_pos; C6 every material channel lies within the span of its cell's eight corners;
   C7 RGBA is the float64 shading of the record's own texels, for every tone and colour mapping and gamma 0 and 2.2.
   Caps: C2 / C3 judge at most 1/3 of a scene's hits by the Lipschitz bound; C4 leaves at most 1/3 of the covered pixels
   undecided.
D. the checker reports falsified records, each by the statement that names it.
"""
import numpy as np
import pytest

import demo_geometry as G

# ---- A ----
def test_reference_decides_its_own_cases():
    """The caps of A by the reference alone, and that every material and the blend are among what it decides."""
    kinds = set()
    for label, prm, sdf_id in G.cases_a():
        pts = G.surface_points(prm, sdf_id, G.SEEDS[sdf_id])
        assert len(pts) >= 4096
        ref = G.evaluate(prm, pts, sdf_id)
        assert (np.abs(ref.d) <= 0.15 + 1e-6).mean() > 0.45, label              # they do lie around the surfaces
        assert 1.0 - ref.decided.mean() <= 0.02, (label, 1.0 - ref.decided.mean())
        kinds |= set(np.unique(ref.kind[ref.decided]).tolist())
        counts = []
        for grid in (dict(dims=G.FILL_GRID, lo=(-1.0,) * 3, hi=(1.0,) * 3), G.GOLDEN_GRID):
            pos, perr = G.lattice(**grid)
            lat = G.evaluate(prm, pos, sdf_id, point_err=perr)
            assert perr.max() < 2.0 * 4.0 * G.U * 2.25      # four operations on magnitudes up to the box's size, doubled
            counts.append((int((~lat.texel_decided).sum()), len(pos)))
        G.pooled(counts, label)
    assert kinds == {G.KIND_AIR, G.KIND_BRICK, G.KIND_CEMENT, G.KIND_NORMAL, G.KIND_BLEND}


def test_known_values_of_the_reference():
    """The reference at points whose answer is known without it."""
    prm = G.Params()
    pts = np.array([[0.95 + 0.02, 0.8, 0.7],       # just outside the +x face, 0.39 outside the sphere: the wall, mapped (z, y)
                    [1.3, 0.0, 0.0],                # 0.35 outside the cube, 0.25 outside the sphere: air, stored as 0.5 grey
                    [0.6, 0.0, 0.0]])              # deep inside the cube, inside the sphere: the nearer surface is the cube's
    r = G.evaluate(prm, pts.astype(np.float32), 0)
    assert abs(r.d[0] - 0.02) < 1e-6 and r.kind[0] in (G.KIND_BRICK, G.KIND_CEMENT)
    assert abs(r.d[1] - 0.35) < 1e-6 and r.kind[1] == G.KIND_AIR and (r.tex0[1, 1:] == G.to_linear(127.0 / 255.0)).all()
    assert abs(r.d[2] - (1.05 - 0.6)) < 1e-6
    assert abs(G.to_linear(1.0) - 1.0) < 1e-15 and abs(G.to_linear(0.04045) - 0.04045 / 12.92) < 1e-8   # (the standard's branches meet to its constants' digits)
    n, _, _ = G.normals(prm, np.array([[0.97, 0.8, 0.7], [0.0, 0.6, 0.8]], np.float32), 0)
    assert (n[0] == (1.0, 0.0, 0.0)).all() and np.allclose(n[1], (0.0, -0.6, -0.8), atol=1e-7)
    # phi: the first and the last texel centre hold the content of the box's faces
    c = G.phi(np.array([-1.0 + 1.0 / 32, 1.0 - 1.0 / 32, 0.0]), (32, 32, 32), (-1,) * 3, (1,) * 3)
    assert np.allclose(c, (-1.0, 1.0, 0.0), atol=1e-15)


@pytest.mark.parametrize("case", range(len(G.cases_a())))
def test_a_oracle_samples_and_fill(oracle, case):
    label, prm, sdf_id = G.cases_a()[case]
    op = oracle.default_params(**prm.kw())
    pts = G.case_points(prm, sdf_id)
    G.compare_samples(f"or_sample, {label}", G.evaluate(prm, pts, sdf_id), oracle.sample_many(op, pts, sdf_id=sdf_id))
    d_only = oracle.sample_many(op, pts, True, sdf_id=sdf_id)
    G.compare_samples(f"or_sample distance only, {label}", G.evaluate(prm, pts, sdf_id, distance_only=True), d_only)
    assert sdf_id == 0 or (d_only[:, 1:] == 0.0).all()       # the demo paints its blend band even then (sdf/demo/mod.rs:62-70)
    counts = []
    for grid in (dict(dims=G.FILL_GRID, lo=(-1.0,) * 3, hi=(1.0,) * 3), G.GOLDEN_GRID):
        pos, perr = G.lattice(**grid)
        t0, t1 = oracle.fill_dense(op, grid["dims"], grid["lo"], grid["hi"], sdf_id=sdf_id, threads=2)
        counts.append(G.compare_texels(f"or_fill_dense {grid['dims']}, {label}", G.evaluate(prm, pos, sdf_id, point_err=perr), t0, t1))
    G.pooled(counts, f"or_fill_dense, {label}")


def test_a_rounding_policy_of_the_colour_code(oracle):
    """trunc(255 c) against round(255 c): the reference follows the switch, and the two differ where it says so."""
    prm = G.Params()
    pos, perr = G.lattice(G.FILL_GRID, (-1.0,) * 3, (1.0,) * 3)
    trunc, rnd = G.evaluate(prm, pos, 0, point_err=perr), G.evaluate(prm, pos, 0, point_err=perr, srgb_round=True)
    assert (trunc.tex0[:, 1:] != rnd.tex0[:, 1:]).any()
    oracle.L.or_set_ext_variant(oracle.EXT_VARIANTS["srgb_quant_round"])
    try:
        t0, t1 = oracle.fill_dense(oracle.default_params(), G.FILL_GRID, threads=2)
    finally:
        oracle.L.or_set_ext_variant(0)
    G.pooled([G.compare_texels("or_fill_dense, rounding policy", rnd, t0, t1)], "or_fill_dense, rounding policy")


# ---- B ----
def cameras_b(pkg):
    out = [("default", {}), ("off-axis target", dict(eye=(1.5, 1.7, 2.2), target=(0.1, -0.05, 0.0), aspect=96 / 72)),
           ("inside the box", dict(eye=(0.2, 0.1, 0.3), target=(1.0, 0.4, -0.2), aspect=64 / 48)),
           ("near / far 0.1, 1000", dict(near=0.1, far=1000.0, aspect=16 / 9)), ("near / far 0.5, 20", dict(near=0.5, far=20.0, fovy=70.0))]
    return out + [(f"orbit {k} of 8", dict(eye=e, aspect=96 / 72)) for k, e in enumerate(G.orbit_eyes(8))]


def test_b_camera_fields(pkg, oracle):
    worst = 0.0
    for label, kw in cameras_b(pkg):
        ref = G.camera(**kw)
        args = dict(eye=kw.get("eye", (2.5, 3.0, 5.0)), target=kw.get("target", (0.0, 0.0, 0.0)), aspect=kw.get("aspect", 1.0))
        got_pkg = pkg.camera_look_at(fovy_degrees=kw.get("fovy", 45.0), z_near=kw.get("near", 0.1), z_far=kw.get("far", 1000.0), **args)
        got_or = oracle.camera_look_at(fovy=kw.get("fovy", 45.0), near=kw.get("near", 0.1), far=kw.get("far", 1000.0), **args)
        for who, got in (("sdfv_camera_look_at", got_pkg), ("or_camera_look_at", got_or)):
            for field in G.Camera.FIELDS:
                g = np.atleast_1d(np.array(getattr(got, field), dtype=np.float64))
                want, tol = np.atleast_1d(getattr(ref, field)), np.atleast_1d(getattr(ref, field + "_err")) + G.U * np.abs(np.atleast_1d(getattr(ref, field)))
                # (the stored f32's own rounding on top.)  The bound decides something: a wrong sign, a transposed entry or another
                # depth range moves a field by its own magnitude, four orders above this
                assert tol.max() < 3e-5 * max(1.0, np.abs(want).max()), (label, field, tol.max())
                assert (np.abs(g - want) <= tol).all(), (who, label, field, g, want, tol)
                worst = max(worst, float((np.abs(g - want) / np.maximum(tol, 1e-300)).max()))
    # the orbit is the package's orbit
    for cam, eye in zip(pkg.orbit_cameras(8, 96 / 72), G.orbit_eyes(8)):
        assert (np.abs(np.array(cam.eye) - eye) <= G.U * np.abs(eye) + 1e-12).all()      # one rounding to f32
    print(f"camera fields: max error / bound = {worst:.3f}")
    assert worst < 1.0


def test_b_handedness_and_pixel_order():
    """What the conventions mean, on a camera one can check by hand: looking down -z from (0, 0, 5) with +y up, +x is to the
    right; pixel (0, 0) is the top left one; depth grows from 0 at the near plane to 1 at the far plane."""
    cam = G.camera(eye=(0.0, 0.0, 5.0), near=1.0, far=9.0)
    assert np.allclose(cam.forward, (0, 0, -1)) and np.allclose(cam.right, (1, 0, 0)) and np.allclose(cam.up, (0, 1, 0))
    _, d, _ = G.pixel_rays(cam, 4, 2)
    assert d[0, 0, 0] < 0 < d[0, 0, 1] and d[1, 3, 0] > 0 > d[1, 3, 1] and (d[..., 2] < 0).all()
    depth, _ = G.depth_of(cam, np.array([[0.0, 0.0, 4.0], [0.3, -0.2, -4.0], [0.0, 0.0, 0.0]]))
    assert np.allclose(depth[:2], (0.0, 1.0), atol=1e-12) and 0.0 < depth[2] < 1.0


# ---- C ----


_cache = {}                                             # a scene's oracle textures, filled once


def oracle_frame(oracle, sc, shading=None, eye=None):
    op = oracle.default_params(**sc.prm.kw())
    key = ("tex", sc.name)
    if key not in _cache:
        _cache[key] = oracle.fill_dense(op, sc.dims, sc.lo, sc.hi, sdf_id=sc.sdf_id, threads=4)
    t0, t1 = _cache[key]
    rp = oracle.default_render_params(sc.dims, sc.lo, sc.hi)
    for k, v in (shading or {}).items():
        setattr(rp, k, v)
    cam = oracle.camera_look_at(eye=sc.eye if eye is None else eye, target=sc.target, aspect=sc.width / sc.height)
    rgba, aux = oracle.raymarch(rp, t0, t1, cam, sc.width, sc.height, threads=4)
    return G.Frame(aux, rgba)



@pytest.mark.parametrize("name", list("abcdef"))
def test_c_march_records_of_the_oracle(oracle, name):
    sc = G.scenes()[name]
    frame = oracle_frame(oracle, sc)
    rep = G.check_records(sc, sc.cam(), frame)
    print(sc.name, rep.figures)
    assert not rep.failures, rep.lines()
    assert rep.figures["hits"] == G.HITS[name], rep.figures["hits"]
    assert rep.figures["share of hits C2 judges by the Lipschitz bound"] <= 1.0 / 3.0
    if "C3" in sc.checks:
        assert rep.figures["share of hits C3 judges by the Lipschitz bound"] <= 1.0 / 3.0
    if "C4" in sc.checks:
        assert rep.figures["share of covered pixels C4 leaves undecided"] <= 1.0 / 3.0
    # C7 for every shading
    for sh in G.SHADINGS:
        if sh == dict(tone_mapping=2, color_mapping=1, gamma=0.0):
            continue
        f = oracle_frame(oracle, sc, sh)
        r = G.check_records(sc, sc.cam(), f, checks={"C7"}, shading=sh)
        assert not r.failures, (sh, r.lines())
        assert r.figures["C7 colour / bound"] < 1.0


# ---- D ----
def fakes(sc, cam, good, good_report):
    """{name: (falsified frame, the statements one of which must report it)}"""
    out = {}
    f = good.copy()
    for k in G.Frame.FIELDS + ("rgba",):
        setattr(f, k, getattr(good, k)[:, ::-1].copy())
    out["image mirrored left to right"] = (f, {"C1"})
    f = good.copy()
    for k in G.Frame.FIELDS + ("rgba",):
        setattr(f, k, getattr(good, k)[::-1].copy())
    out["image mirrored top to bottom"] = (f, {"C1"})
    # content at texel centres: the hit positions such a march would have are phi(hit) of the real ones ... on the rays that
    # would lead there: rescale about the box centre AND keep C1 out of it by asking for C2 / C3 only
    f = good.copy()
    f.hit_pos = G.phi(good.hit_pos.astype(np.float64), sc.dims, sc.lo, sc.hi, clamp=False).astype(np.float32)
    out["phi omitted"] = (f, {"C2", "C3"})
    f = good.copy()
    f.depth = np.where(good.status == 1, G.depth_of(G.camera(eye=sc.eye, target=sc.target, aspect=sc.width / sc.height, near=0.2),
                                                    good.hit_pos.astype(np.float64))[0], 1.0).astype(np.float32)
    out["depth with the near plane doubled"] = (f, {"C5"})
    f = good.copy()
    f.raw0 = good.raw0[..., [0, 1, 3, 2]].copy()
    out["g and b of raw0 swapped"] = (f, {"C6"})
    f = good.copy()
    f.raw1 = good.raw1[..., [2, 1, 0, 3]].copy()
    out["occlusion and metallic swapped"] = (f, {"C6"})
    f = good.copy()
    lin, _ = G.shade(good.raw0, good.raw1, color_mapping=0)
    f.rgba = np.where((good.status == 1)[..., None], lin, 0.0).astype(np.float32)
    out["sRGB mapping skipped"] = (f, {"C7"})
    # hits dropped inside the eroded solid / added outside the dilated one: every 5th pixel of either kind
    f = good.copy()
    drop = np.zeros(good.status.size, bool)
    drop[np.flatnonzero(good_report.must_hit.reshape(-1))[::5]] = True
    f.status = np.where(drop.reshape(good.status.shape), -2, good.status)
    out["hits dropped inside the eroded solid"] = (f, {"C4"})
    if good_report.never_hit.any():                    # (scene d's dilated cube is the whole box: no ray misses it)
        f = good.copy()
        add = np.zeros(good.status.size, bool)
        add[np.flatnonzero(good_report.never_hit.reshape(-1))[::5]] = True
        f.status = np.where(add.reshape(good.status.shape), 1, good.status)
        out["hits added outside the dilated solid"] = (f, {"C4"})
    return out


@pytest.mark.parametrize("name", ["a", "d"])
def test_d_the_checker_reports_falsified_records(oracle, name):
    sc = G.scenes()[name]
    cam = sc.cam()
    good = oracle_frame(oracle, sc)
    good_report = G.check_records(sc, cam, good)
    assert not good_report.failures
    made = fakes(sc, cam, good, good_report)
    assert len(made) == (9 if name == "a" else 8)
    for label, (fake, statements) in made.items():
        rep = G.check_records(sc, cam, fake)
        print(f"{sc.name}, {label}: reported by {sorted(rep.failures)}")
        assert statements & set(rep.failures), (label, sorted(rep.failures))
        # the statement that names the fake reports it on its own too
        alone = G.check_records(sc, cam, fake, checks=statements)
        assert set(alone.failures) and set(alone.failures) <= statements, (label, sorted(alone.failures))
