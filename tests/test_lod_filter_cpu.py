"""The lattice filter of a loading grid (SDFV_OPT_RAYMARCH_LOD_FILTER, include/sdfgrid.h) without a GPU: the option itself, the
numpy restatement tests/lod_filter_ref.py pinned to oracle/raymarch.c where the two must agree (L = 1), what the filter promises
(no texel off the lattice is read; a planar field is met where it is), the cameras tests/test_gpu_lod_filter.py uses, and the
resource contract of the new kernels read from the built library."""
import ctypes as C
import os

import numpy as np
import pytest

import lod_filter_ref as LF
import march_fields as MF
from kernel_objects import code_objects, kernel_table  # noqa: F401  (fixture)

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_option_default_roundtrip_refusal(pkg):
    K = pkg._capi
    assert K.OPT_RAYMARCH_LOD_FILTER == 16
    assert pkg.get_option(K.OPT_RAYMARCH_LOD_FILTER) == 0
    pkg.set_option(K.OPT_RAYMARCH_LOD_FILTER, 1)
    try:
        assert pkg.get_option(K.OPT_RAYMARCH_LOD_FILTER) == 1
        with pytest.raises(pkg.SdfvError) as e:
            pkg.set_option(K.OPT_RAYMARCH_LOD_FILTER, 2)
        # refused the way the other plain options refuse theirs: same code, same text apart from the numbers
        with pytest.raises(pkg.SdfvError) as other:
            pkg.set_option(K.OPT_RAYMARCH_KEEP_NORMAL, 2)
        assert e.value.code == other.value.code
        assert str(e.value).replace("16", "#") == str(other.value).replace(str(K.OPT_RAYMARCH_KEEP_NORMAL), "#")
        assert pkg.get_option(K.OPT_RAYMARCH_LOD_FILTER) == 1  # a refused value changes nothing
    finally:
        pkg.set_option(K.OPT_RAYMARCH_LOD_FILTER, 0)
    with pkg.options({K.OPT_RAYMARCH_LOD_FILTER: 1}):
        assert pkg.get_option(K.OPT_RAYMARCH_LOD_FILTER) == 1
    assert pkg.get_option(K.OPT_RAYMARCH_LOD_FILTER) == 0


@pytest.mark.parametrize("lod", [3.0, 1.5, 65536.0])
def test_bad_lod_is_refused_before_a_device_is_asked_for(pkg, lod):
    """Option 1 with a lod that is no power of two in [2, 2^15]: SDFV_ERR_INVALID_ARGUMENT and a message that names the value,
    from the argument checks (no device needed; the buffers are addresses that are never read).  With option 0 the same call
    passes every argument check, as it always did."""
    K, lib = pkg._capi, pkg.lib
    rp = pkg.default_render_params(pkg.make_grid((16, 16, 16)))
    rp.lod_dist_between_samples = lod
    d = K.MarchDesc()
    d.size = C.sizeof(d)
    d.rp = C.pointer(rp)
    d.tex0, d.tex1, d.rgba = 0x10000, 0x20000, 0x30000
    d.cameras, d.n_cameras = (pkg.Camera * 1)(pkg.camera_look_at()), 1
    d.width, d.height, d.y0, d.y1 = 8, 8, 0, 8
    with pkg.options({K.OPT_RAYMARCH_LOD_FILTER: 1}):
        assert lib.sdfv_raymarch_ex(C.byref(d), None) == -1  # SDFV_ERR_INVALID_ARGUMENT
        msg = lib.sdfv_last_error().decode()
        assert "SDFV_OPT_RAYMARCH_LOD_FILTER" in msg and f"lod_dist_between_samples {lod:g} " in msg, msg
    if lib.sdfv_device_count() == 0:  # (with a device the call would launch over these addresses: tests/test_gpu_lod_filter.py has it)
        assert lib.sdfv_raymarch_ex(C.byref(d), None) == -4 and "no HIP device" in lib.sdfv_last_error().decode()


def _equal_oracle(oracle, rp, t0, t1, cam, width, height, what):
    want_rgba, want = oracle.raymarch(rp, t0, t1, cam, width, height, threads=1)
    got, got_rgba = LF.march(rp, t0, t1, cam, width, height, lod=1)
    both_nan = np.isnan(want["normal"]).any(axis=-1) & np.isnan(got["normal"]).any(axis=-1)
    for f in ("status", "steps", "hit_pos", "t", "raw0", "raw1", "normal", "depth"):
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        diff = (g.view(np.uint32) != w.view(np.uint32)).reshape(g.shape[:2] + (-1,)).any(axis=-1)
        if f == "normal":
            diff &= ~both_nan
        assert not diff.any(), (what, f, int(diff.sum()), np.argwhere(diff)[:3].tolist())
    # (numpy's pow and libm's are not the same function: the project's bound for the pow() tail)
    assert np.abs(got_rgba - want_rgba).max() <= 1e-4, what
    assert (want["status"] == 1).sum() > 50, what
    return want


def test_restatement_with_l1_is_the_oracle_golden(oracle):
    """L = 1: s = u, M = N, the indices clamp(m, 0, N - 1) and clamp(m + 1, 0, N - 1) -- the LINEAR clamp footprint, which is
    MirroredRepeat wherever a marching ray or a normal tap can stand (fast_index / fast_normal hold on these grids)."""
    g = np.load(os.path.join(GOLD, "raymarch_12cube_40x30.npz"))
    t0, t1 = np.ascontiguousarray(g["tex0"]), np.ascontiguousarray(g["tex1"])
    W, H = int(g["width"]), int(g["height"])
    rp = oracle.default_render_params((12, 12, 12))
    for k in (0, 1):
        cam = oracle.Camera()
        C.memmove(C.byref(cam), g[f"cam_{k}"].ctypes.data, C.sizeof(cam))
        _equal_oracle(oracle, rp, t0, t1, cam, W, H, f"golden camera {k}")


def test_restatement_with_l1_is_the_oracle_fields(oracle):
    grid = "odd20x34x27"  # no power of two anywhere: the divide, three different sizes
    dims, lo, hi = MF.GRIDS[grid]
    t0, t1 = MF.make("crossing", grid)
    rp = oracle.default_render_params(dims, lo, hi)
    W, H = 40, 30
    statuses = set()
    for kw in MF.cameras("crossing", grid):
        want = _equal_oracle(oracle, rp, t0, t1, MF.oracle_camera(oracle, kw, W / H), W, H, (grid, kw))
        statuses |= set(np.unique(want["status"]).tolist())
    assert {1, -2, 0} <= statuses


# ---- the cases of tests/test_gpu_lod_filter.py, chosen and checked here on the restatement alone -----------------------------
POW2_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))    # XF 1: exact reciprocals
ODD_BOX = ((-0.9, -0.6, -0.75), (1.1, 0.7, 0.45))   # XF 0: extents 2.0 (but min not -max), 1.3, 1.2 -- the IEEE divide
CASES = [  # (dims, L)
    ((9, 7, 5), 2), ((9, 7, 5), 4), ((9, 7, 5), 8),  # L = 8: M = 2, 1, 1 -- a single lattice point on an axis, both clamps
    ((33, 21, 13), 4),
    ((16, 16, 16), 2),
    ((10, 10, 10), 4),                               # the last lattice point (8) is not the last voxel (9)
]
FIELDS = ("slow", "steep", "noise", "crossing")
IMAGES = ((40, 30), (17, 9))
NAN_NORMAL_CAP = 0.01


def case_cameras(lo, hi):
    """[outside, inside (the 0.2 shift), grazing a face] as pkg.camera_look_at keywords."""
    lo, hi = np.array(lo), np.array(hi)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    outside = dict(eye=tuple(float(x) for x in c + h * np.array([1.7, 1.45, 2.05])), target=tuple(float(x) for x in c))
    inside = dict(eye=tuple(float(x) for x in c + h * np.array([0.3, 0.35, -0.4])),
                  target=tuple(float(x) for x in c + h * np.array([-1.0, -0.5, 1.2])), fovy_degrees=70.0)
    # just above the top face, looking along it and slightly down: rays skim the face y = max at a shallow angle
    graze = dict(eye=(float(c[0] + 2.2 * h[0]), float(hi[1] + 0.02 * h[1]), float(c[2] + 0.3 * h[2])),
                 target=(float(c[0] - h[0]), float(hi[1] - 0.25 * h[1]), float(c[2])), fovy_degrees=40.0)
    return [outside, inside, graze]


def case_textures(field, dims, lo, hi, lod):
    """The field over the grid with the off-lattice texels of tex0 and tex1 overwritten by NaN, and the clean pair."""
    t0, t1 = MF.FIELDS[field](dims, lo, hi, MF.SEEDS[field])
    return LF.poison_off_lattice(t0, lod), LF.poison_off_lattice(t1, lod), t0, t1


def all_cases():
    for dims, lod in CASES:
        for bi, (lo, hi) in enumerate((POW2_BOX, ODD_BOX)):
            for field in FIELDS:
                yield dims, lod, bi, lo, hi, field


def reference_for(oracle_or_pkg, dims, lo, hi, lod, field, cam_kw, width, height, clean=False, y0=0, y1=None):
    """The restatement's record for one view of one case; cameras and parameters through the oracle's or the package's own
    constructors (same layout, same bits: tests/test_abi.py)."""
    p0, p1, t0, t1 = case_textures(field, dims, lo, hi, lod)
    if hasattr(oracle_or_pkg, "make_grid"):
        rp = oracle_or_pkg.default_render_params(oracle_or_pkg.make_grid(dims, lo, hi))
        cam = oracle_or_pkg.camera_look_at(aspect=width / height, **cam_kw)
    else:
        rp = oracle_or_pkg.default_render_params(dims, lo, hi)
        cam = MF.oracle_camera(oracle_or_pkg, cam_kw, width / height)
    rp.lod_dist_between_samples = float(lod)
    return LF.march(rp, t0 if clean else p0, t1 if clean else p1, cam, width, height, y0=y0, y1=y1)


# The one combination whose lattice is degenerate: `steep` is a gyroid of period h / 1.25 = 0.8 in the unit box, and the lattice
# points of 10 texels at L = 4 (texel centres 0, 4, 8) stand 4 * 2 / 10 = 0.8 apart -- every lattice point holds the same value,
# the filtered field is a constant, and sdfNormal of a constant is 0 / 0 at every hit, whatever the camera.  The case stays in
# the parity test (NaN-ness compared); the 1 % cap cannot apply to it, and the test below asserts that this is the reason.
CONSTANT_LATTICE = ((10, 10, 10), 4, 0, "steep")


def test_off_lattice_texels_are_never_read_and_cameras_reach_their_purpose(oracle):
    """Over textures whose off-lattice texels are NaN in tex0 and tex1 the restatement gives the record it gives over the clean
    ones, for every case of the GPU test; per view at most 1 % of the hits have a NaN normal; and per grid and lod the views
    together hold hits, rays that leave the box and pixels off the box."""
    per_grid = {}
    for dims, lod, bi, lo, hi, field in all_cases():
        seen, hits = per_grid.setdefault((dims, lod), [set(), 0])
        for (W, H) in IMAGES:
            for ci, kw in enumerate(case_cameras(lo, hi)):
                what = (dims, lod, bi, field, (W, H), ci)
                aux, rgba = reference_for(oracle, dims, lo, hi, lod, field, kw, W, H)
                clean_aux, clean_rgba = reference_for(oracle, dims, lo, hi, lod, field, kw, W, H, clean=True)
                assert aux.tobytes() == clean_aux.tobytes() and rgba.tobytes() == clean_rgba.tobytes(), what
                assert np.isfinite(aux["raw0"]).all() and np.isfinite(aux["raw1"]).all() and np.isfinite(aux["hit_pos"]).all()
                n_hit, n_nan = int((aux["status"] == 1).sum()), int(LF.nan_normal(aux).sum())
                if (dims, lod, bi, field) == CONSTANT_LATTICE:
                    on = ~LF.off_lattice_mask((dims[2], dims[1], dims[0]), lod)
                    values = case_textures(field, dims, lo, hi, lod)[2][..., 0][on]
                    assert values.max() - values.min() <= 1e-6 and n_nan > 0
                else:
                    assert n_nan <= NAN_NORMAL_CAP * n_hit, what + (n_nan, n_hit)
                if (W, H) == IMAGES[0]:
                    seen |= set(np.unique(aux["status"]).tolist())
                    per_grid[(dims, lod)][1] += n_hit
                    assert (aux["status"] != 0).sum() >= 40, what  # every camera sees the box
    for key, (seen, hits) in per_grid.items():
        assert {0, 1, -2, -1} <= seen and hits >= 1000, (key, seen, hits)


def test_cli_lod_filter_flag_refuses_an_unknown_value():
    """`sdf-viewer-gpu app --lod-filter <nearest|linear>`: anything else is a usage error (exit status 2), decided before the
    program looks for a device."""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sdf-viewer_amd", "sdf-viewer-gpu")
    r = subprocess.run([exe, "app", "--lod-filter", "cubic", "demo"], capture_output=True, text=True)
    assert r.returncode == 2 and "--lod-filter" in r.stderr and "cubic" in r.stderr, (r.returncode, r.stderr[:300])
    assert "--lod-filter <nearest|linear>" in r.stderr  # the usage text names the flag


# ---- the filter does what it is for ----------------------------------------------------------------------------------------
PLANE_N = np.array([0.36, 0.80, 0.48])  # |n| = 1
PLANE_C = 0.11
PLANE_DIMS, PLANE_LOD = (33, 33, 33), 8


def voxel_positions(dims, lo, hi):
    """The fill's voxel positions (scene/sdf/mod.rs:142-146: min + i / (n - 1) * size) as x, y, z [D, H, W] float64."""
    axes = [lo[a] + np.arange(dims[a]) / (dims[a] - 1) * (hi[a] - lo[a]) for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return x, y, z


def test_tilted_plane_is_met_where_it_is(oracle):
    """d = n . x - c sampled at the fill's voxel positions, 33^3, L = 8 (lattice points 0, 8, .., 32: M = 5 per axis).

    Trilinear interpolation of an affine field is exact, so the filter reproduces the plane -- displaced by the difference between
    where the fill samples a voxel (min + i / (N - 1) * size) and where the sampler places it (the texel centre,
    min + (i + 0.5) / N * size): at most half a voxel spacing per axis.  A hit is declared within 1e-5 of the filtered zero set.
    So every hit of the restatement lies within ONE voxel spacing (2 / 32 = 0.0625) of the plane, and the worst is better than
    the NEAREST route's (the oracle at lod 8, which reads the same lattice but snaps: blocks 8 voxels wide).  Bound written
    out: |n . hit - c| <= 1e-5 + 0.5 * spacing * (|nx| + |ny| + |nz|) = 0.0513 < 0.0625.

    Measured on this input, worst |n . hit - c| over the three cameras' hits:  lattice filter 0.0180,  NEAREST 0.4144  (2444 hits)."""
    dims, lod = PLANE_DIMS, PLANE_LOD
    lo, hi = POW2_BOX
    x, y, z = voxel_positions(dims, lo, hi)
    d = PLANE_N[0] * x + PLANE_N[1] * y + PLANE_N[2] * z - PLANE_C
    t0 = np.stack([0.1 + d, 0.5 + 0 * d, 0.5 + 0 * d, 0.5 + 0 * d], axis=-1).astype(F)
    t1 = np.full(t0.shape, F(0.5))
    p0, p1 = LF.poison_off_lattice(t0, lod), LF.poison_off_lattice(t1, lod)
    rp = oracle.default_render_params(dims, lo, hi)
    rp.lod_dist_between_samples = float(lod)
    spacing = 2.0 / (dims[0] - 1)
    worst_new = worst_nearest = 0.0
    W, H = 40, 30
    n_hits = 0
    # Cameras INSIDE the box on the plane's air side, 0.67 from it: their rays start 0.2 in front of the eye (main()'s shift), in
    # air, so every hit is a ray arriving at the surface -- a ray that enters the box from outside may enter it inside the solid
    # and "hit" on its first sample, at the face, wherever that is.
    eye = (0.2, 0.7, 0.3)
    for kw in (dict(eye=eye, target=(0.0, -1.0, 0.0), up=(0.0, 0.0, 1.0), fovy_degrees=90.0),
               dict(eye=eye, target=(-1.0, -0.6, 0.4), fovy_degrees=80.0), dict(eye=eye, target=(0.9, -0.3, -1.0), fovy_degrees=80.0)):
        cam = MF.oracle_camera(oracle, kw, W / H)
        aux, _ = LF.march(rp, p0, p1, cam, W, H)
        hit = aux["status"] == 1
        n_hits += int(hit.sum())
        err = np.abs(aux["hit_pos"][hit].astype(np.float64) @ PLANE_N - PLANE_C)
        worst_new = max(worst_new, float(err.max()))
        # NEAREST over the clean textures (its snap may fold onto texel N - 1, which is on this lattice: 32 = 4 * 8)
        _, near = oracle.raymarch(rp, t0, t1, cam, W, H, threads=1)
        nh = near["status"] == 1
        worst_nearest = max(worst_nearest, float(np.abs(near["hit_pos"][nh].astype(np.float64) @ PLANE_N - PLANE_C).max()))
    print(f"worst hit error: lattice filter {worst_new:.4f}, NEAREST {worst_nearest:.4f}, voxel spacing {spacing:.4f}, {n_hits} hits")
    assert n_hits > 500
    assert worst_new <= spacing, (worst_new, spacing)
    assert worst_new < worst_nearest, (worst_new, worst_nearest)


# ---- the resource contract of the new kernels --------------------------------------------------------------------------------
# raymarch_kernel<kMarchLattice = 5, LINEAR = false, XF, SYMM = false, AUX, ASM = false, NORMAL>.  VGPRs as built:
# plain 58, keep-normal 70 / 71, aux 87.  Each is held to the top of the waves-per-SIMD step it lands on -- 512 registers per SIMD
# lane, allocated in blocks of 8: 8 waves up to 64, 7 up to 72, 5 up to 96.
LATTICE_KERNELS = {  # (AUX, NORMAL) -> VGPR ceiling
    (False, False): 64,
    (False, True): 72,
    (True, True): 96,
}


def test_lattice_kernels_resources(code_objects):  # noqa: F811
    table = kernel_table(code_objects)
    b = lambda v: "Lb1E" if v else "Lb0E"  # noqa: E731
    found = 0
    for xf in (0, 1):
        for (aux, normal), ceiling in LATTICE_KERNELS.items():
            name = f"_ZN4sdfv12_GLOBAL__N_115raymarch_kernelILi5ELb0ELi{xf}E{b(False)}{b(aux)}{b(False)}{b(normal)}EEvNS_12RaymarchArgsE"
            k = table[name]
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["lds"] == 0, (name, k)
            assert k["vgpr"] <= ceiling, (name, k["vgpr"], ceiling)
            # ... and that IS its step (8 waves per SIMD is the most there is)
            assert min(8, 512 // ((k["vgpr"] + 7) // 8 * 8)) == 512 // ceiling, (name, k["vgpr"], ceiling)
            found += 1
    assert found == 6
    assert sum("raymarch_kernelILi5E" in n for n in table) == 6  # and no other instantiation of the lattice march
