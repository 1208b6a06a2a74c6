"""CPU tests of the ray cast over SDF programs (include/sdfgrid.h sdfv_program_cast_desc, include/sdfprogram.h
sdfv_program_raycast_host): the layouts, every refusal with its text and order, the host mirror -- the per-ray source the kernel
is built from -- against an independent numpy restatement byte for byte, what a hit MEANS against float64 geometry, and what the
built kernel looks like.  No device needed."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import program_cast_ref as CR
import program_fuzz as PF
import program_geometry as G
import program_march_ref as M
from kernel_objects import code_objects, kernel_table, opcodes  # noqa: F401 (code_objects is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NO_DEVICE = -1, -4
FUZZ_PROGRAMS = 6            # of program_fuzz.corpus(DEFAULT_SEED, ...): the first that change sign in their box


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


def test_struct_sizes(pkg, PM):
    K = pkg._capi
    assert C.sizeof(K.Ray) == 32 and C.sizeof(K.RayHit) == 64 and C.sizeof(K.ProgramCastDesc) == 72
    assert K.ProgramCastDesc.rays.offset == 32 and K.ProgramCastDesc.n.offset == 48 and K.ProgramCastDesc.normal_eps.offset == 68
    assert K.RayHit.pos.offset == 12 and K.RayHit.normal.offset == 24 and K.RayHit.sample.offset == 36
    assert PM.ray_dtype().itemsize == 32 and PM.hit_dtype().itemsize == 64
    assert PM.ray_dtype() == CR.RAY_DTYPE and PM.hit_dtype() == CR.HIT_DTYPE
    assert (K.CAST_NORMALS, K.CAST_MATERIALS) == (1, 2) and pkg.lib.sdfv_abi_version() == 5


# ---- refusals: sdfv_program_raycast_check, the host mirror and the device entry point say the same thing ----
def entry_points(pkg):
    V = importlib.import_module("sdf-viewer_amd.viewer")
    host = V.lib.sdfv_program_raycast_host
    host.restype, host.argtypes = C.c_int, [C.c_void_p]
    return pkg.lib.sdfv_program_raycast_check, host, pkg.lib.sdfv_program_raycast


def test_every_refusal_has_its_text_and_its_place_in_the_order(pkg, PM):
    check, host, dev = entry_points(pkg)
    D = pkg._capi.ProgramCastDesc
    prog = M.builders(PM)["anchor"].build()
    rays = CR.rays(1, (-1, -1, -1, 1, 1, 1), 16)
    hits = np.full(16 * 64, 7, np.uint8).view(CR.HIT_DTYPE)     # every byte 7: a refused call writes nothing
    flat = (C.c_float * 3)(-1.0, 0.5, -1.0), (C.c_float * 3)(1.0, 0.5, 1.0)
    reversed_ = (C.c_float * 3)(-1.0, -1.0, 2.0), (C.c_float * 3)(1.0, 1.0, 1.0)
    nonfinite = (C.c_float * 3)(float("-inf"), -1.0, -1.0), (C.c_float * 3)(1.0, 1.0, 1.0)
    good = (C.c_float * 3)(-1.0, -1.0, -1.0), (C.c_float * 3)(1.0, 1.0, 1.0)

    def box(d, b):
        d.bb_min, d.bb_max = b

    # in the order the header lists them; every edit violates its own rule only
    cases = [
        ("size", lambda d: setattr(d, "size", 64), "sdfv_program_cast_desc.size = 64 is smaller than the descriptor's first version (72)"),
        ("reserved", lambda d: setattr(d, "reserved", 5), "sdfv_program_cast_desc: reserved must be 0"),
        ("program", lambda d: setattr(d, "program", None), "sdfv_program_cast_desc.program is NULL"),
        ("half a box", lambda d: setattr(d, "bb_min", good[0]), "bounding box: bb_min and bb_max are both given or both NULL (the program's box)"),
        ("flat box", lambda d: box(d, flat), "degenerate bounding box on axis 1: [0.5, 0.5]"),
        ("rays NULL", lambda d: setattr(d, "rays", None), "NULL buffer"),
        ("alignment", lambda d: setattr(d, "hits", d.hits + 2), "rays and hits must be 4-byte aligned"),
        ("flags", lambda d: setattr(d, "flags", 4), "unknown flags 0x4"),
        ("max_steps", lambda d: setattr(d, "max_steps", 4097), "max_steps 4097 is outside [1, 4096] (0 = 256)"),
        ("hit_eps", lambda d: setattr(d, "hit_eps", -1.0), "hit_eps = -1: a distance > 0, or 0 for 1e-5"),
        ("normal_eps", lambda d: setattr(d, "normal_eps", float("inf")), "normal_eps = inf: a distance > 0, or 0 for 0.001"),
    ]
    more = [
        (lambda d: box(d, reversed_), "degenerate bounding box on axis 2: [2, 1]"),
        (lambda d: box(d, nonfinite), "degenerate bounding box on axis 0: [-inf, 1]"),
        (lambda d: setattr(d, "hits", None), "NULL buffer"),
        (lambda d: setattr(d, "rays", d.rays + 1), "rays and hits must be 4-byte aligned"),
        (lambda d: setattr(d, "flags", 0x80000001), "unknown flags 0x80000001"),
        (lambda d: setattr(d, "hit_eps", float("nan")), "hit_eps = nan: a distance > 0, or 0 for 1e-5"),
        (lambda d: setattr(d, "normal_eps", -0.5), "normal_eps = -0.5: a distance > 0, or 0 for 0.001"),
    ]

    def fresh():
        d, keep = prog.cast_desc(rays.ctypes.data, hits.ctypes.data, 16)
        return d

    def refused(d, text):
        for fn, args in ((check, (C.byref(d), None)), (host, (C.cast(C.pointer(d), C.c_void_p),)), (dev, (C.byref(d), None))):
            assert fn(*args) == INVALID and pkg.lib.sdfv_last_error().decode() == text, (text, pkg.lib.sdfv_last_error())
        assert (hits.view(np.uint8) == 7).all()

    assert check(None, None) == INVALID and pkg.lib.sdfv_last_error().decode() == "desc is NULL"
    assert host(None) == INVALID and dev(None, None) == INVALID
    for _, edit, text in cases:
        d = fresh()
        edit(d)
        refused(d, text)
    for edit, text in more:
        d = fresh()
        edit(d)
        refused(d, text)
    # two violations at once: the earlier rule of the list is the one reported, for every pair of rules
    for i, (_, first, text) in enumerate(cases):
        for name, second, _ in cases[i + 1:]:
            if (cases[i][0], name) == ("half a box", "flat box"):
                continue                                   # (both edit the box: one descriptor cannot hold the two)
            d = fresh()
            second(d)
            first(d)
            refused(d, text)
    # a longer descriptor: zero beyond what the library knows is accepted, anything else is not
    class Longer(C.Structure):
        _fields_ = [("d", D), ("future", C.c_uint32 * 4)]
    lg = Longer()
    C.memmove(C.byref(lg), C.byref(fresh()), C.sizeof(D))
    lg.d.size = C.sizeof(lg)
    assert check(C.cast(C.pointer(lg), C.POINTER(D)), None) == 0
    lg.future[2] = 9
    assert check(C.cast(C.pointer(lg), C.POINTER(D)), None) == INVALID
    assert pkg.lib.sdfv_last_error().decode() == "sdfv_program_cast_desc.size = 88: this library knows 72 bytes and byte 80 beyond them is not 0"
    # the checked copy carries the defaults; values given are kept
    out = D()
    assert check(C.byref(fresh()), C.byref(out)) == 0
    assert (out.max_steps, np.float32(out.hit_eps), np.float32(out.normal_eps)) == (256, np.float32(1e-5), np.float32(0.001))
    d = fresh()
    d.max_steps, d.hit_eps, d.normal_eps = 4096, 2e-4, 0.01
    assert check(C.byref(d), C.byref(out)) == 0
    assert (out.max_steps, np.float32(out.hit_eps), np.float32(out.normal_eps)) == (4096, np.float32(2e-4), np.float32(0.01))
    assert out.n == 16 and out.rays == rays.ctypes.data
    # n == 0 needs no buffers; without a device the device entry point says so AFTER the checks and computes nothing
    d = fresh()
    d.rays, d.hits, d.n = None, None, 0
    assert check(C.byref(d), None) == 0 and host(C.cast(C.pointer(d), C.c_void_p)) == 0
    if pkg.lib.sdfv_device_count() == 0:
        assert dev(C.byref(fresh()), None) == NO_DEVICE and b"no HIP device" in pkg.lib.sdfv_last_error()
        assert dev(C.byref(d), None) == NO_DEVICE
        assert (hits.view(np.uint8) == 7).all()


# ---- the host mirror against the restatement ----
def fuzz_programs():
    corpus = PF.corpus(PF.DEFAULT_SEED, PF.CORPUS_SIZE)
    picked = [i for i in range(len(corpus)) if PF.changes_sign(*corpus[i])][:FUZZ_PROGRAMS]
    assert len(picked) == FUZZ_PROGRAMS
    return [(f"fuzz{i}", corpus[i][0], corpus[i][1]) for i in picked]


def compared_programs(PM):
    """(name, builder, box, seed of its ray set): the march catalogue with GRAZE, the models the benchmarks time, fuzz programs."""
    out = [(name, b, CR.scene_box(name)) for name, b in M.builders(PM).items()]
    out += [(name, b, box) for name, (b, box) in CR.bench_builders(PM).items()]
    out += [(name, PF.builder(PM, ops, bb), tuple(bb)) for name, ops, bb in fuzz_programs()]
    return [(name, b, box, 100 + i) for i, (name, b, box) in enumerate(out)]


@pytest.fixture(scope="module")
def restated(PM):
    """name -> (rays, the restatement's records): computed once, shared by the tests below."""
    return {name: (CR.rays(seed, box), CR.cast(b.ops, box, CR.rays(seed, box))) for name, b, box, seed in compared_programs(PM)}


def test_host_mirror_equals_the_numpy_restatement_on_every_byte(pkg, PM, restated):
    for name, b, box, _ in compared_programs(PM):
        rays, want = restated[name]
        assert len(rays) == CR.N_RAYS
        got = b.build().cast_host(rays, box=box)
        CR.assert_hits_bitwise(got, want, name)
        assert (got["steps"] <= 256).all()
    # ... with every parameter off its default, the flags singly and not at all, and a structured ray array
    name, b, box, _ = compared_programs(PM)[0]
    rays, want = restated[name]
    prog = b.build()
    for flags in (0, 1, 2, 3):
        got = prog.cast_host(CR.as_rays(rays), normals=bool(flags & 1), materials=bool(flags & 2), box=box)
        CR.assert_hits_bitwise(got, CR.cast(b.ops, box, rays, flags=flags), (name, flags))
        h = got["status"] == 1
        assert h.any() and (flags & 1 or (got["normal"] == 0).all()) and (flags & 2 or (got["sample"][:, 1:] == 0).all())
        for f in ("status", "steps", "t", "pos"):
            assert (got[f].view(np.uint32) == want[f].view(np.uint32)).all(), (flags, f)
    small = tuple(0.7 * v for v in box)
    for kw in (dict(max_steps=1), dict(max_steps=7), dict(max_steps=4096), dict(hit_eps=3e-3, normal_eps=0.02), dict(box=small)):
        args = dict(dict(box=box), **kw)
        CR.assert_hits_bitwise(prog.cast_host(rays, **args), CR.cast(b.ops, args.pop("box"), rays, **args), (name, kw))
    assert len(prog.cast_host(rays[:0], box=box)) == 0


def test_the_ray_sets_are_not_vacuous(PM, restated):
    """Conditions on the restatement alone: every status occurs, each in some set by the hundred; the grazed plane runs rays out
    of steps; example_sixteen and `sixteen` are lists of misses; hits at the first step (rays started inside a solid) and after
    many; records with three and more distinct materials in one 64-ray run."""
    total = {k: 0 for k in (1, 0, -1, -2)}
    for name, (rays, want) in restated.items():
        for k in total:
            total[k] += int((want["status"] == k).sum())
        assert (want["status"] == 0).sum() >= 100 and ((want["status"] == -2).sum() >= 100 or name in ("envelope", "late_material")), name
    assert min(total.values()) >= 100, total
    assert (restated[M.GRAZE][1]["status"] == -1).sum() >= 50
    for name in ("sixteen", "example_sixteen"):
        assert (restated[name][1]["status"] != 1).all()
    w = restated["anchor"][1]
    h = w["status"] == 1
    assert (w["steps"][h] == 1).sum() >= 50 and (w["steps"][h] >= 10).sum() >= 50
    w = restated["deep"][1]
    runs = [len(np.unique(w["sample"][i:i + 64][w["status"][i:i + 64] == 1], axis=0)) for i in range(0, len(w), 64)]
    assert max(runs) >= 3, runs


# ---- meaning: float64 geometry, no reference output ----
def chord_sphere(o, u, r):
    """[t_in, t_out] of the line o + t u through the ball of radius r (NaN where it misses), float64."""
    a, b, c = (u * u).sum(axis=1), (o * u).sum(axis=1), (o * o).sum(axis=1) - r * r
    disc = b * b - a * c
    with np.errstate(invalid="ignore"):
        s = np.sqrt(disc)
    return (-b - s) / a, (-b + s) / a


def chord_cube(o, u, half):
    """... through the Chebyshev ball of radius `half`: the slab test, float64; and the entry face's |cos| of incidence."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-half - o) / u, (half - o) / u
        lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
    axis = np.argmax(lo, axis=1)
    tin, tout = lo.max(axis=1), hi.min(axis=1)
    miss = ~(tout >= tin)
    cos = np.abs(u[np.arange(len(u)), axis]) / np.linalg.norm(u, axis=1)
    return np.where(miss, np.nan, tin), np.where(miss, np.nan, tout), cos


MEANING_SCENES = {
    "sphere": G.Prim("sphere", 0.6, mat=(0.2, 0.5, 0.9, 0.1, 0.4, 1.0)),
    "cube": G.Rigid(G.Prim("cube", 0.4, mat=(0.9, 0.4, 0.1, 0.3, 0.6, 1.0)), t=(0.1, -0.05, 0.15), R=G.rot((1.0, 2.0, 3.0), 35.0)),
}


@pytest.mark.parametrize("which", sorted(MEANING_SCENES))
def test_a_hit_is_where_the_ray_meets_the_solid(pkg, PM, which):
    """SPHERE 0.6 and a translated, rotated CUBE 0.4, 2000 rays each; float64 throughout, the ray being the f32 one the library
    marches: origin o, u = the f32 normalised direction, g(t) = d64(o + u t), [t*, t**] the analytic chord through the (convex)
    solid, theta the incidence at t*.

    The tolerance, derived.  U = 2^-24.  B: program_geometry's bound for the f32 evaluation, taken at the box's corners (every term
    of it is U times a sum of magnitudes that grow with |x|, |y|, |z|: the corner bounds it over the box).  E: the rounding of
    pos = origin + u * t, two operations per axis, sqrt(3) * 2 U (|o|_inf + t).  So the f32 value v at the recorded pos has
    |v - g(t)| <= beta = B + E.
      * from outside: a hit has v < hit_eps, so g(t) < hit_eps + beta; the solid lies behind its tangent plane at t*, so
        g(t) >= (t* - t) cos theta:  t* - t <= (hit_eps + beta) / cos theta;
      * past the surface: the step that led here had v' <= g(t') + beta <= (t* - t') |u| + beta (the surface is no nearer than
        along the ray), |u| <= 1 + 2 U, and t = fl(t' + v'):  t - t* <= delta = beta + 4 U t*;
      * |d64(pos)| <= hit_eps + beta + delta (g is 1-Lipschitz in t up to |u|; pos is within E of o + u t);
      * a ray that left its interval (-2) has no stretch of its chord inside [t0, t1] longer than 2 delta (a landing point at most
        delta behind t* lies inside the solid, where v <= beta < hit_eps is a hit) -- unless the landing point itself is
        beyond t1;
      * a ray that starts inside the solid hits at t0 with its first evaluation."""
    scene = MEANING_SCENES[which]
    b = G.emit(scene, PM)
    box = b.bb
    rays = CR.rays(7 if which == "sphere" else 8, box)
    hits = b.build().cast_host(rays)
    hit_eps = float(np.float32(1e-5))
    corners = np.array([[x, y, z] for x in box[0::3] for y in box[1::3] for z in box[2::3]], np.float32)
    Bc = float(G.evaluate(scene, corners)[1].max())
    assert 0 < Bc < 1e-5
    o = rays[:, :3].astype(np.float64)
    d32 = rays[:, 4:7]
    with np.errstate(all="ignore"):
        u32 = d32 / np.sqrt(d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1] + d32[:, 2] * d32[:, 2])[:, None]
    u = u32.astype(np.float64)
    t = hits["t"].astype(np.float64)
    with np.errstate(all="ignore"):                       # (the rays nothing can be computed for are among them)
        if which == "sphere":
            tin, tout = chord_sphere(o, u, G.f32(0.6))
            x = o + u * tin[:, None]
            cos = np.abs((x * u).sum(axis=1)) / (np.linalg.norm(x, axis=1) * np.linalg.norm(u, axis=1))
        else:
            Rm, tr = scene.R, scene.t
            tin, tout, cos = chord_cube((o - tr) @ Rm, u @ Rm, G.f32(0.4))
    E = np.sqrt(3.0) * 2 * G.U * (np.abs(o).max(axis=1) + np.abs(t))
    beta = Bc + E
    with np.errstate(invalid="ignore"):
        delta = beta + 4 * G.U * np.abs(tin)
    # the interval the march ran in, float64 from the same f32 data (the restatement's formula)
    lo, hi = np.array(box[:3]), np.array(box[3:])
    with np.errstate(all="ignore"):
        a1, a2 = (lo - o) / u, (hi - o) / u
        tnear, tfar = np.fmin(a1, a2).max(axis=1), np.fmax(a1, a2).min(axis=1)
    t0, t1 = np.fmax(rays[:, 3], tnear), np.fmin(rays[:, 7], tfar)
    status = hits["status"]
    assert (hits["steps"] <= 256).all()
    h = np.flatnonzero(status == 1)
    assert len(h) >= 150
    # a hit from outside the solid (its chord begins behind t0 by more than the tolerances)
    with np.errstate(invalid="ignore"):
        outside = h[tin[h] > t0[h] + 2 * (hit_eps + beta[h]) / cos[h]]
    assert len(outside) >= 100 and (cos[outside] > 0).all()
    early, late = tin[outside] - t[outside], t[outside] - tin[outside]
    print(f"{which}: {len(outside)} hits from outside, t* - t max {early.max():.3e}, t - t* max {late.max():.3e}, B {Bc:.2e}")
    assert (early <= (hit_eps + beta[outside]) / cos[outside]).all(), float((early - (hit_eps + beta[outside]) / cos[outside]).max())
    assert (late <= delta[outside]).all(), float((late - delta[outside]).max())
    ref, bound, _, _ = G.evaluate(scene, hits["pos"][outside])
    assert (bound <= Bc).all()
    assert (np.abs(ref) <= hit_eps + beta[outside] + delta[outside]).all()
    ref_all = G.evaluate(scene, hits["pos"][h])[0]
    assert (ref_all < hit_eps + beta[h]).all()
    # a ray that starts inside the solid: t0 inside the chord by more than the bound -> the first evaluation, at t0
    with np.errstate(invalid="ignore"):
        inside = np.flatnonzero((tin + beta < t0) & (t0 < tout - beta) & (t1 >= t0))
    assert len(inside) >= 30
    assert (status[inside] == 1).all() and (hits["steps"][inside] == 1).all()
    assert (np.abs(t[inside] - t0[inside]) <= 4 * G.U * np.abs(t0[inside])).all()
    started_at_t_min = inside[rays[inside, 3] > tnear[inside] + 1e-3]
    assert (hits["t"][started_at_t_min] == rays[started_at_t_min, 3]).all()   # bit for bit where t0 is the caller's t_min
    # a ray that left its interval met nothing in it
    left = np.flatnonzero(status == -2)
    assert len(left) >= 100
    with np.errstate(invalid="ignore"):
        overlap = np.fmin(tout[left], t1[left] - delta[left]) - np.fmax(tin[left], t0[left])
    assert not (overlap > 2 * delta[left]).any(), float(np.nanmax(overlap))


# ---- the built kernel (tests/kernel_objects.py) ----
def test_cast_kernel_keeps_its_state_in_registers(code_objects):
    table = kernel_table(code_objects)
    k = table["sdfprog_cast"]                             # a stable C name, outside the kernel table of the compiled routes
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["lds"] == 0, k
    assert k["vgpr"] <= 80, k                             # the step of 6 waves per SIMD (512 / 80), as the direct march
    assert k["kernarg"] <= 4096
    assert "sdfprogc_cast" not in table and len([n for n in table if n.startswith("sdfprog_cast")]) == 1
    ops = opcodes(k["co"], "sdfprog_cast")
    assert not any(o.startswith(("scratch_", "buffer_", "ds_", "flat_")) for o in ops)
    assert ops.count("global_store_dwordx4 nt") == 4      # the record of an aligned list: four streaming 16-byte stores
    assert not any(o.startswith("v_pk_fma") for o in ops)   # nothing contracted (IEEE divide and sqrt expand to scalar fmas)


def test_cast_headers_compile_as_pedantic_c99(tmp_path):
    import subprocess
    src = tmp_path / "cast_headers.c"
    src.write_text('#include "sdfprogram.h"\n#include "sdfgrid.h"\n'
                   "int main(void) {\n"
                   "    sdfv_prog_op op[1] = {{SDFV_OP_SPHERE, {0, 0, 0}, {0.6f}}};\n"
                   "    float bb[6] = {-1, -1, -1, 1, 1, 1};\n"
                   "    sdfv_ray ray = {{0, 0, 3}, 0, {0, 0, -2}, 100};\n"
                   "    sdfv_ray_hit hit;\n"
                   "    sdfv_program *p = 0;\n"
                   "    sdfv_program_cast_desc d = {0}, out;\n"
                   "    if (sizeof(sdfv_ray) != 32 || sizeof(sdfv_ray_hit) != 64) return 1;\n"
                   "    if (sdfv_program_create(op, 1, bb, &p) != 0) return 2;\n"
                   "    d.size = sizeof(d); d.program = p; d.rays = &ray; d.hits = &hit; d.n = 1;\n"
                   "    d.flags = SDFV_CAST_NORMALS | SDFV_CAST_MATERIALS;\n"
                   "    if (sdfv_program_raycast_check(&d, &out) != 0 || out.max_steps != 256) return 3;\n"
                   "    if (sdfv_program_raycast_host(&d) != 0) return 4;\n"
                   "    if (hit.status != 1 || !(hit.t > 2.39f && hit.t < 2.41f) || !(hit.normal[2] > 0.999f)) return 5;\n"
                   "    sdfv_program_free(p);\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "cast_headers"
    lib_dir = os.path.join(ROOT, "sdf-viewer_amd")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", lib_dir, "-lsdfviewer_host", "-lsdfgrid", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)], timeout=120).returncode == 0
