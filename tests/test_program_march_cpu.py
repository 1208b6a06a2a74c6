"""CPU tests of the direct march of SDF programs (include/sdfgrid.h sdfv_program_march_desc, include/sdfprogram.h
sdfv_program_raymarch_host): the host mirror -- the per-pixel source the kernel is built from -- against an independent numpy
restatement bit for bit, what the rendered points MEAN against the float64 geometric evaluator, the descriptor's rules, and what
the built kernels look like.  No device needed."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import program_geometry as G
import program_march_ref as M
import program_ref as R
from kernel_objects import code_objects, disassembly, kernel_table  # noqa: F401 (code_objects is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NO_DEVICE = -1, -4
RGBA_TOL = 1e-4            # what tests/test_gpu_raymarch.py holds the grid march's rgba to against the oracle: pow() is the one inexact step


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


@pytest.fixture(scope="module")
def restated(pkg, PM):
    """name -> size -> camera index -> policy -> (aux, rgba, material): the numpy restatement of every comparison's frame."""
    air = pkg.lib.sdfv_air_dist()
    out = {}
    for name, b in M.builders(PM).items():
        rp = M.render_params(pkg, name)
        for size in M.SIZES:
            for ci, cam in enumerate(M.cameras(pkg, name, *size)):
                for policy in (0, 1):
                    out[name, size, ci, policy] = M.march(b.ops, rp, cam, size[0], size[1], srgb_round=bool(policy), air_dist=air,
                                                          want_material=True)
    return out


def test_host_mirror_equals_the_numpy_restatement_bitwise(pkg, PM, restated):
    """Every program of the catalogue (sixteen, envelope, late_material, ties and the rest) and the grazed plane, an orbit view
    and a camera inside the box, 160 x 120 and 67 x 41, once per sRGB policy: status, steps, hit_pos, t, raw0, raw1, normal and
    depth as bit patterns; rgba within the grid march's tolerance."""
    worst = 0.0
    try:
        for policy in (0, 1):
            pkg.set_option(pkg._capi.OPT_EXT_SRGB_QUANT, policy)
            for name, b in M.builders(PM).items():
                prog, rp = b.build(), M.render_params(pkg, name)
                for size in M.SIZES:
                    for ci, cam in enumerate(M.cameras(pkg, name, *size)):
                        want_aux, want_rgba, _ = restated[name, size, ci, policy]
                        rgba, aux, depth = prog.render_host(cam, size[0], size[1], rp=rp, want_aux=True, want_depth=True, threads=4)
                        got = M.aux_view(aux[0])
                        M.assert_aux_bitwise(got, want_aux, (name, size, ci, policy))
                        assert (depth[0].view(np.uint32) == want_aux["depth"].view(np.uint32)).all()
                        err = float(np.abs(rgba[0] - want_rgba).max())
                        worst = max(worst, err)
                        assert err <= RGBA_TOL, (name, size, ci, policy, err)
    finally:
        pkg.set_option(pkg._capi.OPT_EXT_SRGB_QUANT, 0)
    print(f"host mirror == restatement bit for bit; max |d rgba| = {worst:.2e}")
    # the two policies do differ somewhere (the comparison saw both)
    assert any((restated[n, M.SIZES[0], 0, 0][0]["raw0"] != restated[n, M.SIZES[0], 0, 1][0]["raw0"]).any() for n in M.SCENES)


def test_the_frames_compared_are_not_vacuous(pkg, PM, restated):
    """Conditions on the restatement alone.  Every scene's orbit view holds at least 5 % hits, 5 % rays that cross the box and leave
    it (-2) and 5 % pixels off the box (0); some pixel of the suite runs out of steps (-1); some 8 x 8 tile holds three materials.
    One scene cannot have hits from ANY camera and is held to the rest: `sixteen` closes with INTERSECT against the plane
    0.95 - z, whose value is positive below z = 0.95 -- where the whole model lies -- so the program's value is positive in the
    whole box (asserted on a lattice here).  It stays in every comparison as the frame of pure misses."""
    out_of_steps, tiles3 = 0, 0
    for name in M.SCENES:
        for size in M.SIZES:
            aux, _, material = restated[name, size, 0, 0]
            st = aux["status"]
            share = {k: float((st == k).mean()) for k in (1, -2, 0)}
            if name == "sixteen":
                pos = R.grid_positions((48, 48, 48), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
                assert R.run(M.builders(PM)[name].ops, pos, distance_only=True)[:, 0].min() >= 0.05
                assert share[1] == 0 and min(share[-2], share[0]) >= 0.05, (name, size, share)
            else:
                assert min(share.values()) >= 0.05, (name, size, share)
        for size in M.SIZES:
            for ci in (0, 1):
                aux, _, material = restated[name, size, ci, 0]
                out_of_steps += int((aux["status"] == -1).sum())
                assert (aux["status"] != -3).all()          # (distances below 1e-5 are never accumulated)
                h, w = material.shape
                for y in range(0, h, 8):
                    for x in range(0, w, 8):
                        m = material[y:y + 8, x:x + 8]
                        tiles3 += len(np.unique(m[m != -2])) >= 3
    assert out_of_steps >= 1 and tiles3 >= 1, (out_of_steps, tiles3)
    assert (restated[M.GRAZE, M.SIZES[0], 1, 0][0]["status"] == -1).any()   # the scene built for it does its part


# ---- meaning: the float64 geometric evaluator ----
def render_scene(pkg, PM, scene, eye, size=(96, 72), normal_h=0.0):
    b = G.emit(scene, PM)
    rp = pkg.default_render_params(pkg.make_grid((256, 256, 256), b.bb[:3], b.bb[3:]))
    cam = pkg.camera_look_at(eye=eye, aspect=size[0] / size[1])
    _, aux = b.build().render_host(cam, size[0], size[1], rp=rp, want_aux=True, threads=4, normal_h=normal_h)
    return M.aux_view(aux[0]), rp


def test_hit_points_lie_on_the_surface_the_program_means(pkg, PM):
    """At every hit pixel the march stopped because the f32 value was below 1e-5; the float64 meaning of the program at hit_pos is
    therefore below 1e-5 + the evaluator's derived f32 bound for that point.  (One-sided: where the solid crosses the box the ray
    starts inside it and the first evaluation is the hit, at any depth.)"""
    hits = 0
    for name, scene in G.scenes().items():
        aux, _ = render_scene(pkg, PM, scene, (1.3, -1.9, 1.6) if name == "sixteen" else (1.5, 1.7, 2.2))
        h = aux["status"] == 1
        if not h.any():
            continue
        p = aux["hit_pos"][h].astype(np.float32)
        ref, bound, _, _ = G.evaluate(scene, p)
        assert np.isfinite(bound).all() and bound.max() < 1e-4
        k = int(np.argmax(ref - bound))
        assert (ref < 1e-5 + bound).all(), (name, p[k], ref[k], bound[k])
        hits += int(h.sum())
    assert hits >= 2000, hits


def test_a_sphere_is_hit_on_its_radius_and_its_normal_points_outwards(pkg, PM):
    """SPHERE r: ||hit_pos| - r| < 1e-5 + bound, and the normal against hit_pos / |hit_pos|.

    The tolerance of the angle, derived (U = 2^-24, R = |hit_pos|, h the tap distance, delta = sqrt(3) h the taps' offset length):
      the taps' sum is  sum_i k_i d(p + k_i h) = 4 h n  +  sum_i k_i rho_i  +  sum_i k_i e_i  + rounding,  since sum_i k_i = 0 and
      sum_i k_i k_i^T = 4 I for the tetrahedron.
      * rho_i, what |p + d| - R - n.d leaves beyond first order: |rho_i| <= T = delta^2 / (2 R) * (1 + delta / (2 R))^2
        (from 1 + x/2 - x^2/8 <= sqrt(1 + x) <= 1 + x/2), so |sum k_i rho_i| <= 4 sqrt(3) T;
      * e_i, the f32 value against the meaning at the tap as evaluated: the evaluator's bound B there, plus the rounding of
        p + k h itself (<= U (|p|_inf + h) per axis, Lipschitz 1: sqrt(3) U (R + h)); |sum k_i e_i| <= 4 sqrt(3) (B + sqrt(3) U (R + h));
      * the three f32 additions per component: each <= U * 4 dmax with dmax = 1e-5 + B + delta; as a vector sqrt(3) * 12 U dmax;
      * the normalisation: a few U in direction, 8 U taken.
      angle <= asin(E / (4 h)) + 8 U  with E the sum of the three vector terms."""
    r = 0.6
    scene = G.Prim("sphere", r, mat=(0.2, 0.5, 0.9, 0.1, 0.4, 1.0))
    for normal_h in (0.0, 0.01):
        aux, rp = render_scene(pkg, PM, scene, (1.5, 1.7, 2.2), normal_h=normal_h)
        h = float(M.normal_h_of(rp.tex_size, rp.lod_dist_between_samples, normal_h))
        hit = aux["status"] == 1
        assert hit.sum() >= 400
        p = aux["hit_pos"][hit].astype(np.float64)
        n = aux["normal"][hit].astype(np.float64)
        _, bound, _, _ = G.evaluate(scene, p.astype(np.float32))
        Rr = np.linalg.norm(p, axis=1)
        assert (np.abs(Rr - G.f32(r)) < 1e-5 + bound).all()
        B = np.zeros(len(p))
        for k in ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1)):
            B = np.maximum(B, G.evaluate(scene, (p + np.array(k) * h).astype(np.float32))[1])
        delta = np.sqrt(3.0) * h
        T = delta ** 2 / (2 * Rr) * (1 + delta / (2 * Rr)) ** 2
        dmax = 1e-5 + B + delta
        E = 4 * np.sqrt(3.0) * T + 4 * np.sqrt(3.0) * (B + np.sqrt(3.0) * G.U * (Rr + h)) + np.sqrt(3.0) * 12 * G.U * dmax
        tol = np.arcsin(np.minimum(1.0, E / (4 * h))) + 8 * G.U
        cosang = np.clip((n * p).sum(axis=1) / (np.linalg.norm(n, axis=1) * Rr), -1.0, 1.0)
        ang = np.arccos(cosang)
        print(f"normal_h {normal_h}: h = {h:.5f}, max angle {ang.max():.2e} rad, tolerance {tol.min():.2e} .. {tol.max():.2e}")
        assert tol.max() < 0.1 and (ang <= tol).all(), (normal_h, float(ang.max()), float(tol.min()))
        assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 4 * G.U * 4


# ---- the descriptor ----
def desc_for(pkg, prog, rp, cam, w=8, h=8, extra=0):
    d, keep = prog.march_desc(cam, w, h, rp=rp)
    buf = (C.c_ubyte * (C.sizeof(d) + extra))()
    C.memmove(buf, C.byref(d), C.sizeof(d))
    return d, buf, keep


def test_descriptor_rules(pkg, PM):
    from importlib import import_module
    V = import_module("sdf-viewer_amd.viewer")
    host = V.lib.sdfv_program_raymarch_host
    host.restype, host.argtypes = C.c_int, [C.c_void_p, C.c_int]
    check = pkg.lib.sdfv_program_raymarch_check
    dev = pkg.lib.sdfv_program_raymarch
    prog = R.catalogue(PM)["anchor"].build()
    rp = M.render_params(pkg, "anchor")
    cam = pkg.camera_look_at(aspect=1.0)
    rgba = np.full((8, 8, 4), 7.0, np.float32)
    D = pkg._capi.ProgramMarchDesc

    def calls(d_bytes):
        """status and message of the three entry points for the descriptor at d_bytes (the device one only where it cannot launch)"""
        out = []
        p = C.cast(d_bytes, C.POINTER(D))
        out.append((check(p, None, None), pkg.lib.sdfv_last_error().decode()))
        out.append((host(C.cast(d_bytes, C.c_void_p), 2), pkg.lib.sdfv_last_error().decode()))
        return out

    def edited(edit, extra=0):
        d, _, keep = desc_for(pkg, prog, rp, cam)
        d.rgba = rgba.ctypes.data
        edit(d)
        buf = (C.c_ubyte * (C.sizeof(d) + extra))()
        C.memmove(buf, C.byref(d), C.sizeof(d))
        return buf, (d, keep)

    # a longer descriptor with a zero tail is accepted, and renders
    buf, keep = edited(lambda d: setattr(d, "size", C.sizeof(D) + 24), extra=24)
    for rc, msg in calls(buf):
        assert rc == 0, msg
    assert (rgba != 7.0).any()
    # ... an unknown non-zero field is not
    buf[C.sizeof(D) + 5] = 1
    for rc, msg in calls(buf):
        assert rc == INVALID and f"byte {C.sizeof(D) + 5}" in msg, msg
    zero_rp = M.render_params(pkg, "anchor")
    zero_rp.tex_size[1] = 0
    dir_rp = M.render_params(pkg, "anchor")
    dir_rp.n_lights = 1
    dir_rp.lights[0].kind = pkg._capi.LIGHT_DIRECTIONAL
    cases = [(lambda d: setattr(d, "program", None), "program"),
             (lambda d: setattr(d, "rgba", None), "rgba and rgba8"),
             (lambda d: setattr(d, "rp", C.pointer(zero_rp)), "normal_h is 0 and rp->tex_size"),
             (lambda d: setattr(d, "rp", C.pointer(dir_rp)), "lights[0] is directional"),
             (lambda d: setattr(d, "reserved", 3), "reserved"),
             (lambda d: setattr(d, "size", C.sizeof(D) - 8), "size"),
             (lambda d: setattr(d, "normal_h", -1.0), "normal_h"),
             (lambda d: setattr(d, "y1", 9), "rows")]
    for edit, word in cases:
        rgba[:] = 7.0
        buf, keep = edited(edit)
        for rc, msg in calls(buf):
            assert rc == INVALID and word in msg, (word, rc, msg)
        assert dev(C.cast(buf, C.POINTER(D)), None) == INVALID and word in pkg.lib.sdfv_last_error().decode()
        assert (rgba == 7.0).all()
    # normal_h > 0 needs no tex_size
    buf, keep = edited(lambda d: (setattr(d, "rp", C.pointer(zero_rp)), setattr(d, "normal_h", 0.004)))
    assert all(rc == 0 for rc, _ in calls(buf))
    # the checked copy and the tap distance
    out, h = D(), C.c_float()
    buf, keep = edited(lambda d: None)
    assert check(C.cast(buf, C.POINTER(D)), C.byref(out), C.byref(h)) == 0
    assert out.width == 8 and out.rgba == rgba.ctypes.data and np.float32(h.value) == M.normal_h_of((256, 256, 256), 1.0)
    # the device entry point computes nothing without a device
    if pkg.lib.sdfv_device_count() == 0:
        rgba[:] = 7.0
        assert dev(C.cast(buf, C.POINTER(D)), None) == NO_DEVICE and b"no HIP device" in pkg.lib.sdfv_last_error()
        assert (rgba == 7.0).all()
    assert pkg.lib.sdfv_abi_version() == 5


def test_host_rows_cameras_and_rgba8_are_those_of_single_full_calls(pkg, PM):
    b = M.builders(PM)["deep"]
    prog, rp = b.build(), M.render_params(pkg, "deep")
    w, h = 67, 41
    cams = list(M.cameras(pkg, "deep", w, h)) * 2
    full = [prog.render_host(c, w, h, rp=rp, want_aux=True, want_depth=True, threads=3) for c in cams]
    rgba, aux, depth = prog.render_host(cams, w, h, rp=rp, want_aux=True, want_depth=True, threads=3, y0=9, y1=30)
    for i, (fr, fa, fd) in enumerate(full):
        assert (rgba[i].view(np.uint32) == fr[0, 9:30].view(np.uint32)).all() and (depth[i].view(np.uint32) == fd[0, 9:30].view(np.uint32)).all()
        assert (aux[i].view(np.uint32) == fa[0, 9:30].view(np.uint32)).all()
    r8 = prog.render_host(cams[0], w, h, rp=rp, rgba8=True)
    want = np.rint(np.clip(full[0][0][0], 0.0, 1.0) * np.float32(255.0)).astype(np.uint32)
    assert (r8[0] == (want[..., 0] | want[..., 1] << 8 | want[..., 2] << 16 | want[..., 3] << 24)).all()


# ---- the built kernels (tests/kernel_objects.py) ----
MARCH_KERNELS = ("sdfprog_march", "sdfprog_march_aux")


def test_march_kernels_keep_their_state_in_registers_and_fetch_instructions_by_scalar_loads(code_objects):
    table = kernel_table(code_objects)
    for name in MARCH_KERNELS:
        k = table[name]                                   # stable C names
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (name, k)
        # built at 78 / 79 VGPRs, the step of 6 waves per SIMD (512 / 80); 81 would drop to 5
        assert k["vgpr"] <= 80, (name, k)
        assert k["kernarg"] <= 4096 and k["lds"] == 1024, (name, k)   # the sRGB table in LDS, as in the fills
        ins = []
        for ln in disassembly(k["co"], name).split("\n"):
            m = re.match(r"\s+(\S+)[^/]*//\s*([0-9A-Fa-f]{12}):[^<]*(?:<[^>+]*\+0x([0-9a-f]+)>)?", ln)
            if m:
                ins.append((m.group(1), int(m.group(2), 16), None if m.group(3) is None else int(m.group(3), 16)))
        ops = [i[0] for i in ins]
        base = ins[0][1]
        # every loop (backward branch) of the kernel: none loads through the vector memory path -- instructions and materials
        # arrive by scalar loads wherever an interpreter or resolve() runs
        back = sorted((base + to, -at) for o, at, to in ins if o.startswith(("s_cbranch", "s_branch")) and to is not None and base + to < at)
        assert back, name
        for lo, hi in back:
            assert not any(o.startswith(("global_load", "flat_load", "buffer_load", "scratch_")) for o, at, _ in ins if lo <= at <= -hi), name
        # the march loop is the outermost loop that starts first: it holds the eighteen instruction bodies, fetches them by wide
        # scalar loads and touches no other memory -- no LDS, no stores
        lo, hi = back[0][0], -back[0][1]
        loop = [o for o, at, _ in ins if lo <= at <= hi]
        assert len(loop) > 200, (name, len(loop))
        assert [o for o in loop if re.match(r"s_load_dwordx(4|8|16)$", o)], (name, "no wide scalar load in the march loop")
        assert not any(o.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_")) for o in loop), name
        # outside it: the sRGB table's staging is the one vector load of the kernel
        assert [o for o in ops if o.startswith(("global_load", "flat_load", "buffer_load"))] == ["global_load_dword"], name
        code = [ln.split("//")[0].split() for ln in disassembly(k["co"], name).split("\n")]
        assert sum(1 for ln in code if ln and ln[0] == "global_store_dwordx4" and "nt" in ln[1:]) == 1, name   # rgba: 16 bytes, streamed
        assert not any(o.startswith("v_pk_fma") for o in ops), name   # nothing contracted (IEEE divide and sqrt expand to scalar fmas)


def test_march_headers_compile_as_pedantic_c99(tmp_path):
    src = tmp_path / "march_headers.c"
    src.write_text('#include "sdfprogram.h"\n#include "sdfgrid.h"\n'
                   "int main(void) {\n"
                   "    sdfv_prog_op op[1] = {{SDFV_OP_SPHERE, {0, 0, 0}, {0.6f}}};\n"
                   "    float bb[6] = {-1, -1, -1, 1, 1, 1}, eye[3] = {2.5f, 3, 5}, at[3] = {0, 0, 0}, up[3] = {0, 1, 0}, h = 0;\n"
                   "    static float rgba[16 * 16 * 4];\n"
                   "    sdfv_program *p = 0;\n"
                   "    sdfv_grid g;\n"
                   "    sdfv_render_params rp;\n"
                   "    sdfv_camera cam;\n"
                   "    sdfv_program_march_desc d = {0}, out;\n"
                   "    if (sdfv_program_create(op, 1, bb, &p) != 0) return 2;\n"
                   "    if (sdfv_grid_from_bb(bb, bb + 3, 64, &g) != 0) return 3;\n"
                   "    sdfv_render_params_default(&rp, &g);\n"
                   "    if (sdfv_camera_look_at(&cam, eye, at, up, 45.0f, 1.0f, 0.1f, 1000.0f) != 0) return 4;\n"
                   "    d.size = sizeof(d); d.program = p; d.rp = &rp; d.cameras = &cam; d.n_cameras = 1;\n"
                   "    d.width = d.height = d.y1 = 16; d.rgba = rgba;\n"
                   "    if (sdfv_program_raymarch_check(&d, &out, &h) != 0 || !(h > 0) || out.width != 16) return 5;\n"
                   "    if (sdfv_program_raymarch_host(&d, 1) != 0) return 6;\n"
                   "    if (!(rgba[(8 * 16 + 8) * 4 + 3] == 1.0f)) return 7;\n"
                   "    sdfv_program_free(p);\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "march_headers"
    lib_dir = os.path.join(ROOT, "sdf-viewer_amd")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), "-L", lib_dir, "-lsdfviewer_host", "-lsdfgrid", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)], timeout=120).returncode == 0
