"""GPU tests of what the GRID route MEANS: the demo fill, the samplers and every family of march kernels against the float64
reference written from the definitions (tests/demo_geometry.py), through the checker the oracle is held to on the CPU
(tests/test_demo_meaning_cpu.py: statements A and C1 .. C7, the same scenes, the same caps).  Everything runs on the default
stream and is synchronised before it is read.

What differs from the CPU file: tex0.r of the device may carry the one extra rounding of the clamp where it applies; the
shading's pow and divisions are exp2(y * log2(x)) and a * rcp(b) at 1 ulp each (csrc/march_shade.h), from which the C7 bound
is derived (demo_geometry.shade(device=True)) -- not RGBA_TOL; the 8-bit plane equals round(255 * the float64 colour) except
where 255 c lies within that bound of a half-integer, at most 1 % of the hit pixels' channels.

Measured on an MI355X: the file 3.4 s for its 19 cases; slowest samplers[0] 0.27 s, then the march of scene d 0.22 s, f 0.18 s,
a 0.17 s, c 0.14 s (the 17 families of a scene give one and the same set of records, bit for bit, which is checked once).
Device colour against float64 shading over the six scenes: at most 2.1e-7 without tone mapping, 1.7e-7 Reinhard, 2.7e-7 ACES,
3.7e-7 filmic (0.17 of the bound with the defaults); depth 2.6e-7; off-ray distance 6.5e-7 (8.6e-7 from the orbit cameras);
8-bit channels left out 0.05 % at most.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import demo_geometry as G
import march_compare as MC

pytestmark = pytest.mark.gpu
UNIT = dict(lo=(-1.0,) * 3, hi=(1.0,) * 3)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_of(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- fill and samplers ----
@pytest.mark.parametrize("case", range(len(G.cases_a())))
def test_samplers_on_the_device(pkg, case):
    label, prm, sdf_id = G.cases_a()[case]
    dp = pkg.default_params(**prm.kw())
    pts = G.case_points(prm, sdf_id)
    got = host_of(pkg.sample_points(dp, dev(pts), sdf_id=sdf_id))
    G.compare_samples(f"sdfv_sample_points, {label}", G.evaluate(prm, pts, sdf_id), got)
    d_only = host_of(pkg.sample_points(dp, dev(pts), distance_only=True, sdf_id=sdf_id))
    G.compare_samples(f"sdfv_sample_points distance only, {label}", G.evaluate(prm, pts, sdf_id, distance_only=True), d_only)
    assert (d_only[:, 0] == got[:, 0]).all()
    # the demo's own normals: exact on the cube's faces, within the bound's angle on the sphere
    n, ne, decided = G.normals(prm, pts, sdf_id)
    gn = host_of(pkg.normal_points(dp, dev(pts), sdf_id=sdf_id)).astype(np.float64)
    axis = decided & (ne == 0.0).all(axis=1)
    assert sdf_id == 2 or axis.sum() > 256
    assert (gn[axis] == n[axis]).all(), label
    ball = decided & ~axis
    angle = np.linalg.norm(np.cross(gn[ball], n[ball]), axis=1)             # sin of the angle between unit vectors
    print(f"sdfv_normal_points, {label}: {int(axis.sum())} axis normals equal, {int(ball.sum())} sphere normals, "
          f"max angle / bound = {float((angle / np.linalg.norm(ne[ball], axis=1)).max()) if ball.any() else 0.0:.3f}")
    assert (angle <= np.linalg.norm(ne[ball], axis=1)).all() and (np.abs(gn[ball] - n[ball]) <= ne[ball]).all(), label
    assert 1.0 - decided.mean() <= 0.02
    # the mesher's scalar source: unit-cube points placed into the box, u * (max - min) + min, then the distance alone
    for grid in (dict(dims=G.FILL_GRID, **UNIT), G.GOLDEN_GRID):
        u = np.random.default_rng(G.SEEDS[sdf_id] + 100).random((4096, 3)).astype(np.float32)
        where, where_err = G.placed(u, grid["lo"], grid["hi"])
        ref = G.evaluate(prm, where, sdf_id, distance_only=True, point_err=where_err)
        got = host_of(pkg.source_sample_scalar(dp, dev(u), grid["lo"], grid["hi"], sdf_id=sdf_id)).astype(np.float64)
        assert ref.bound.max() < 1e-5 and (np.abs(got - ref.d) <= ref.bound).all(), (label, grid["dims"])


def test_host_sdf_objects_sample_the_demo_family(pkg, host):
    """The viewer host's C++ SDF objects (demo, and its children cube and sphere), which sample on the device."""
    prm = G.Params()
    demo = host.SDF.demo()
    kids = demo.children()
    assert [k.name() for k in kids] == ["DemoCube", "DemoSphere"]
    for sdf, sdf_id in ((demo, 0), (kids[0], 1), (kids[1], 2)):
        pts = G.case_points(prm, sdf_id)
        G.compare_samples(f"host object {sdf.name()}", G.evaluate(prm, pts, sdf_id), sdf.sample_batch(pts))


@pytest.mark.parametrize("case", range(len(G.cases_a())))
def test_fills_on_the_device(pkg, case):
    """sdfv_fill_grid, sdfv_fill_grid_commit with the plain volume, and the fused fill with the y-interleaved one (the step-1
    pass over a fresh allocation).  tex0.r and the volumes: A's bound plus one rounding of the clamp."""
    K = pkg._capi
    label, prm, sdf_id = G.cases_a()[case]
    dp = pkg.default_params(**prm.kw())
    counts = {"sdfv_fill_grid": [], "sdfv_fill_grid_commit": [], "fused fill, interleaved volume": []}
    for grid in (dict(dims=G.FILL_GRID, **UNIT), G.GOLDEN_GRID):
        W, H, D = grid["dims"]
        pos, perr = G.lattice(**grid)
        ref = G.evaluate(prm, pos, sdf_id, point_err=perr)
        extra = G.U * np.abs(ref.tex0[:, 0])
        g = pkg.make_grid(grid["dims"], grid["lo"], grid["hi"])
        for how in counts:
            if how.startswith("fused") and H % 2:
                continue
            t0, t1 = pkg.alloc_textures(g)
            t0.fill_(-7.0), t1.fill_(-7.0)
            vol = torch.full((D, H, W), -7.0, device="cuda")
            if how == "sdfv_fill_grid":
                pkg.check(pkg.lib.sdfv_fill_grid(C.byref(dp), sdf_id, C.byref(g), t0.data_ptr(), t1.data_ptr(), None))
            elif how == "sdfv_fill_grid_commit":
                pkg.fill_grid(dp, g, t0, t1, sdf_id=sdf_id, dist=vol)
            else:
                pkg.fill_grid_pass(dp, g, 1, t0, t1, sdf_id=sdf_id, dist=vol, flags=K.PASS_VIRGIN_GRID | K.PASS_VOLUME_INTERLEAVED)
            h0, h1, v = host_of(t0), host_of(t1), host_of(vol)
            counts[how].append(G.compare_texels(f"{how} {grid['dims']}, {label}", ref, h0, h1, extra=extra))
            if how != "sdfv_fill_grid":
                if how.startswith("fused"):                  # entry ((row >> 1) * W + x) * 2 + (row & 1)
                    v = v.reshape(D * H // 2, W, 2).transpose(0, 2, 1)
                assert (v.reshape(-1) == h0.reshape(-1, 4)[:, 0]).all(), (how, label)
    for how, c in counts.items():
        G.pooled(c, f"{how}, {label}")


def test_fill_follows_the_rounding_policy(pkg):
    K = pkg._capi
    prm = G.Params()
    pos, perr = G.lattice(G.FILL_GRID, **UNIT)
    g = pkg.make_grid(G.FILL_GRID)
    for policy in (0, 1):
        t0, t1 = pkg.alloc_textures(g)
        with pkg.options({K.OPT_EXT_SRGB_QUANT: policy}):
            pkg.fill_grid(pkg.default_params(), g, t0, t1)
        ref = G.evaluate(prm, pos, 0, point_err=perr, srgb_round=bool(policy))
        G.pooled([G.compare_texels(f"fill, SDFV_OPT_EXT_SRGB_QUANT = {policy}", ref, host_of(t0), host_of(t1), extra=G.U)], f"policy {policy}")


# ---- march ----
def device_scene(pkg, sc):
    """The scene's textures and its three acceleration volumes on the device."""
    g = pkg.make_grid(sc.dims, sc.lo, sc.hi)
    t0, t1 = pkg.alloc_textures(g)
    pkg.fill_grid(pkg.default_params(**sc.prm.kw()), g, t0, t1, sdf_id=sc.sdf_id)
    dist = pkg.commit_distance(g, t0)
    pairs = pkg.commit_pairs(g, dist)
    ilv = pkg.commit_interleaved(g, dist) if sc.dims[1] % 2 == 0 else None
    torch.cuda.synchronize()
    return g, t0, t1, dist, pairs, ilv


def device_frames(pkg, oracle, sc, dscene, cameras, mask=0, vols=None, shading=None):
    """-> ([Frame per camera], rgba8 [n, H, W, 4])"""
    g, t0, t1 = dscene[:3]
    rp = pkg.default_render_params(g)
    for k, v in (shading or {}).items():
        setattr(rp, k, v)
    with pkg.options({pkg._capi.OPT_RAYMARCH_DISABLE: mask}):
        rgba, depth, aux, img8 = pkg.raymarch(rp, t0, t1, cameras, sc.width, sc.height, want_aux=True, want_depth=True, rgba8="both",
                                              **(vols or {}))
        torch.cuda.synchronize()
    rgba, depth, img8 = rgba.cpu().numpy(), depth.cpu().numpy(), img8.cpu().numpy()
    recs = MC.aux_to_np(oracle, aux)
    assert (recs["depth"].view(np.uint32) == depth.view(np.uint32)).all()
    return [G.Frame(recs[i], rgba[i]) for i in range(len(rgba))], img8


def check_unorm8(sc, frame, img8, shading, label):
    hit = frame.status == 1
    want, bound = G.shade(frame.raw0[hit], frame.raw1[hit], device=True, **(shading or {}))
    code, decided = G.unorm8(want, bound)
    left_out = 1.0 - decided.mean()
    assert left_out <= 0.01, (label, left_out)
    got = img8[hit].astype(np.float64)
    assert (got == code)[decided].all(), (label, got[~((got == code) | ~decided)][:4])
    assert (np.abs(got - code) <= 1.0).all() and (img8[~hit] == 0).all(), label
    return left_out


@pytest.mark.parametrize("name", list("abcdef"))
def test_march_families_on_the_device(pkg, oracle, name):
    sc = G.scenes()[name]
    cam_ref = sc.cam()
    dscene = device_scene(pkg, sc)
    dist, pairs, ilv = dscene[3:]
    cam = pkg.camera_look_at(eye=sc.eye, target=sc.target, aspect=sc.width / sc.height)
    seen, ran = {}, []
    for variant, mask in MC.variants(pkg._capi).items():
        if variant.startswith("ilv") and ilv is None:            # as march_compare.compare() skips it: H is odd
            continue
        (frame,), img8 = device_frames(pkg, oracle, sc, dscene, cam, mask, MC.volumes_of(variant, dist, pairs, ilv))
        ran.append(variant)
        key = b"".join(getattr(frame, k).tobytes() for k in G.Frame.FIELDS + ("rgba",)) + img8.tobytes()
        if key in seen:                                           # the same records and planes, bit for bit: the same verdict
            continue
        rep = G.check_records(sc, cam_ref, frame, device=True)
        left_out = check_unorm8(sc, frame, img8[0], None, f"{sc.name}, {variant}")
        seen[key] = variant
        print(f"{sc.name}, {variant}: {rep.figures}, rgba8 channels left out {100 * left_out:.2f} %")
        assert not rep.failures, (variant, rep.lines())
        assert rep.figures["hits"] == G.HITS[name], (variant, rep.figures["hits"])
        assert rep.figures["share of hits C2 judges by the Lipschitz bound"] <= 1.0 / 3.0
        assert "C3" not in sc.checks or rep.figures["share of hits C3 judges by the Lipschitz bound"] <= 1.0 / 3.0
        assert "C4" not in sc.checks or rep.figures["share of covered pixels C4 leaves undecided"] <= 1.0 / 3.0
        assert rep.figures["C7 colour / bound"] < 1.0
    assert len(ran) == len(MC.variants(pkg._capi)) - (0 if ilv is not None else 3)
    print(f"{sc.name}: {len(ran)} families, {len(seen)} distinct result(s): {sorted(seen.values())}")
    # C7 and the 8-bit plane under every tone mapping, colour mapping and gamma
    worst = {}
    for sh in G.SHADINGS:
        (frame,), img8 = device_frames(pkg, oracle, sc, dscene, cam, shading=sh)
        rep = G.check_records(sc, cam_ref, frame, checks={"C7"}, shading=sh, device=True)
        assert not rep.failures, (sh, rep.lines())
        assert rep.figures["C7 colour / bound"] < 1.0
        check_unorm8(sc, frame, img8[0], sh, f"{sc.name}, {sh}")
        worst[sh["tone_mapping"]] = max(worst.get(sh["tone_mapping"], 0.0), rep.figures["C7 colour"])
    print(f"{sc.name}: device colour against float64, max per tone mapping: " + ", ".join(f"{t}: {v:.2e}" for t, v in sorted(worst.items())))


def test_camera_batch_on_the_device(pkg, oracle):
    """One batch of the eight orbit cameras over scene (a): C1 and C4 per camera."""
    sc = G.scenes()["a"]
    dscene = device_scene(pkg, sc)
    cams = pkg.orbit_cameras(8, sc.width / sc.height)
    frames, _ = device_frames(pkg, oracle, sc, dscene, cams)
    assert len(frames) == 8
    for k, (frame, eye) in enumerate(zip(frames, G.orbit_eyes(8))):
        rep = G.check_records(sc, G.camera(eye=eye, aspect=sc.width / sc.height), frame, checks={"C1", "C4"}, device=True)
        print(f"orbit camera {k}: {rep.figures}")
        assert not rep.failures, (k, rep.lines())
        assert rep.figures["hits"] > 100 and rep.figures["share of covered pixels C4 leaves undecided"] <= 1.0 / 3.0
