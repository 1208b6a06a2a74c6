"""Shared by tests/test_program_march_cpu.py and tests/test_gpu_program_march.py: a vectorised numpy float32 restatement of the
direct march of SDF programs (include/sdfgrid.h, sdfv_program_march_desc), written from the header's description and the
shader's per-pixel algorithm; it sits on tests/program_ref.run for the program's value and calls nothing of the library.  Every
arithmetic step is one float32 numpy operation, in the order the per-pixel algorithm takes them.  Plus the scenes, boxes and
cameras the comparisons run on."""
import os
import re

import numpy as np

import program_ref as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUX_DTYPE = np.dtype([("status", "<i4"), ("steps", "<i4"), ("hit_pos", "<f4", (3,)), ("t", "<f4"), ("raw0", "<f4", (4,)),
                      ("raw1", "<f4", (4,)), ("normal", "<f4", (3,)), ("depth", "<f4")])
assert AUX_DTYPE.itemsize == 72
BITWISE_FIELDS = ("status", "steps", "hit_pos", "t", "raw0", "raw1", "normal", "depth")
SIZES = ((160, 120), (67, 41))


def srgb_table():
    """sRGB u8 -> linear, the 256 floats of sdf-viewer_amd/csrc/srgb_lut.inc that the library compiles in (C99 hexadecimal floats:
    exact; held to the oracle's by tests/test_abi.py).  The one parser of that file: tests/grid_mesh_ref.py inverts this table."""
    text = open(os.path.join(ROOT, "sdf-viewer_amd", "csrc", "srgb_lut.inc")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    t = np.array([float.fromhex(x) for x in re.findall(r"[-+]?0x[0-9a-fA-F.]+p[-+]?\d+", text)], np.float64)
    assert t.shape == (256,) and (t.astype(F) == t).all()
    return t.astype(F)


def cam_fields(cam):
    return {k: np.array(getattr(cam, k), F) if hasattr(getattr(cam, k), "__len__") else F(getattr(cam, k))
            for k in ("eye", "right", "up", "forward", "tan_half_fovy", "aspect", "bvp")}


def _len3(x, y, z):
    return np.sqrt(x * x + y * y + z * z)


def _oob(p, lo, hi):
    o = [np.fmax(lo[a] - p[a], p[a] - hi[a]) for a in range(3)]
    return np.fmax(o[0], np.fmax(o[1], o[2]))


def normal_h_of(tex_size, lod, normal_h=0.0):
    if normal_h > 0:
        return F(normal_h)
    s = [F(n) / F(lod) for n in tex_size]
    return F(1) / np.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])


def pack(rec, lut, air_dist, srgb_round):
    """The fill's texel pair for records [n, 7]: scene/sdf/mod.rs:196-208 as sdfgrid.h's fills apply it."""
    d, col, met, rough, occ = rec[:, 0], rec[:, 1:4].copy(), rec[:, 4], rec[:, 5], rec[:, 6]
    col[(col == 0).all(axis=1)] = F(0.5)
    x = F(0.1) + d
    t0 = np.empty((len(rec), 4), F)
    t0[:, 0] = np.where(x < 0, F(0), np.where(x > 1, F(1), x))
    v = col * F(255)
    if srgb_round:
        v = v + F(0.5)
    v = np.fmin(np.fmax(v, F(0)), F(255))
    t0[:, 1:] = lut[v.astype(np.uint32)]
    t1 = np.stack([met, rough, np.where(occ <= 0, F(1), occ), np.full(len(rec), air_dist, F)], axis=1).astype(F)
    return t0, t1


def _mix(a, b, t):
    return a * (F(1) - t) + b * t


def shade(rp, raw0, raw1):
    """material.frag:158-173 with three-d's tone and colour mapping, float32 (pow is the one step that is not exact)."""
    met, occ = raw1[:, 0], raw1[:, 2]
    out = np.empty((len(raw0), 4), F)
    for c in range(3):
        albedo = raw0[:, 1 + c] * F(rp.tint[c])
        lit = occ * F(rp.ambient[c]) * _mix(albedo, F(0), met)
        for l in range(rp.n_lights):
            lit = lit + occ * (F(rp.lights[l].intensity) * F(rp.lights[l].color[c])) * _mix(albedo, F(0), met)
        if rp.tone_mapping == 1:
            lit = lit / (lit + F(1))
        elif rp.tone_mapping == 2:
            lit = (lit * (F(2.51) * lit + F(0.03))) / (lit * (F(2.43) * lit + F(0.59)) + F(0.14))
        elif rp.tone_mapping == 3:
            x = np.fmax(F(0), lit - F(0.004))
            lit = np.power((x * (F(6.2) * x + F(0.5))) / (x * (F(6.2) * x + F(1.7)) + F(0.06)), F(2.2))
        lit = np.fmin(np.fmax(lit, F(0)), F(1))
        if rp.color_mapping == 1:
            sel = (lit >= F(0.0031308)).astype(F)
            lit = _mix(lit * F(12.92), F(1.055) * np.power(lit, F(1) / F(2.4)) - F(0.055), sel)
        if rp.gamma > 0:
            lit = np.power(lit, F(rp.gamma))
        out[:, c] = lit
    out[:, 3] = F(rp.tint[3])
    return out


@np.errstate(all="ignore")
def march(ops, rp, cam, width, height, normal_h=0.0, srgb_round=False, air_dist=None, y0=0, y1=None, want_material=False):
    """-> (aux [rows, width] structured, rgba [rows, width, 4][, material index at the hit [rows, width], -2 where none])."""
    y1 = height if y1 is None else y1
    c = cam_fields(cam)
    lo, hi = [F(v) for v in rp.bounds_min], [F(v) for v in rp.bounds_max]
    ys, xs = np.meshgrid(np.arange(y0, y1), np.arange(width), indexing="ij")
    px, py = xs.ravel().astype(F), ys.ravel().astype(F)
    n = len(px)
    ndc_x = ((px + F(0.5)) / F(width)) * F(2) - F(1)
    ndc_y = F(1) - ((py + F(0.5)) / F(height)) * F(2)
    sx = ndc_x * c["aspect"] * c["tan_half_fovy"]
    sy = ndc_y * c["tan_half_fovy"]
    eye = c["eye"]
    d0 = [c["forward"][a] + c["right"][a] * sx + c["up"][a] * sy for a in range(3)]
    l = _len3(*d0)
    d0 = [v / l for v in d0]
    t1_ = [(lo[a] - eye[a]) / d0[a] for a in range(3)]
    t2_ = [(hi[a] - eye[a]) / d0[a] for a in range(3)]
    tnear = np.fmax(np.fmax(np.fmin(t1_[0], t2_[0]), np.fmin(t1_[1], t2_[1])), np.fmin(t1_[2], t2_[2]))
    tfar = np.fmin(np.fmin(np.fmax(t1_[0], t2_[0]), np.fmax(t1_[1], t2_[1])), np.fmax(t1_[2], t2_[2]))
    covered = (tfar >= tnear) & (tfar > 0)
    tfrag = np.where(tnear > 0, tnear, tfar)
    origin = [eye[a] + d0[a] * tfrag for a in range(3)]
    rd = [origin[a] - eye[a] for a in range(3)]
    l = _len3(*rd)
    rd = [v / l for v in rd]
    shifted = _oob([origin[a] + rd[a] * F(0.2) for a in range(3)], lo, hi) > 0
    origin = [np.where(shifted, eye[a] + rd[a] * F(0.2), origin[a]).astype(F) for a in range(3)]

    pos = [o.copy() for o in origin]
    dist = np.zeros(n, F)
    status = np.where(covered, -1, 0).astype(np.int32)
    steps = np.zeros(n, np.int32)
    marching = covered.copy()
    for _ in range(255):
        idx = np.flatnonzero(marching)
        if idx.size == 0:
            break
        p = [pos[a][idx] for a in range(3)]
        out = _oob(p, lo, hi) > F(1e-4)
        status[idx[out]] = -2
        marching[idx[out]] = False
        idx = idx[~out]
        p = [pos[a][idx] for a in range(3)]
        d = R.run(ops, np.stack(p, axis=1), distance_only=True)[:, 0]
        steps[idx] += 1
        hit = d < F(1e-5)
        status[idx[hit]] = 1
        marching[idx[hit]] = False
        go, dg = idx[~hit], d[~hit]
        dist[go] = dist[go] + dg
        for a in range(3):
            pos[a][go] = pos[a][go] + rd[a][go] * dg
    status[(status == 1) & (dist < 0)] = -3

    aux = np.zeros(n, AUX_DTYPE)
    aux["depth"] = 1
    aux["status"], aux["steps"] = status, np.where(covered, steps, 0)
    for a in range(3):
        aux["hit_pos"][:, a] = np.where(covered, pos[a], F(0))
    aux["t"] = np.where(covered, dist, F(0))
    rgba = np.zeros((n, 4), F)
    material = np.full(n, -2, np.int64)
    h = np.flatnonzero(status == 1)
    if h.size:
        p = np.stack([pos[a][h] for a in range(3)], axis=1)
        rec, m = R.run(ops, p, want_index=True)
        material[h] = m
        lut = srgb_table()
        raw0, raw1 = pack(rec, lut, F(air_dist), srgb_round)
        hh = normal_h_of(rp.tex_size, rp.lod_dist_between_samples, normal_h)
        acc = None
        for k in ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1)):
            q = np.stack([p[:, a] + F(k[a]) * hh for a in range(3)], axis=1)
            d = R.run(ops, q, distance_only=True)[:, 0]
            term = [F(k[a]) * d for a in range(3)]
            acc = term if acc is None else [acc[a] + term[a] for a in range(3)]
        l = _len3(*acc)
        for a in range(3):
            aux["normal"][h, a] = acc[a] / l
        aux["raw0"][h], aux["raw1"][h] = raw0, raw1
        m = c["bvp"]
        hz = m[2] * p[:, 0] + m[6] * p[:, 1] + m[10] * p[:, 2] + m[14]
        hw = m[3] * p[:, 0] + m[7] * p[:, 1] + m[11] * p[:, 2] + m[15]
        aux["depth"][h] = hz / hw
        rgba[h] = shade(rp, raw0, raw1)
    shape = (y1 - y0, width)
    out = (aux.reshape(shape), rgba.reshape(shape + (4,)))
    return out + (material.reshape(shape),) if want_material else out


# ---- scenes: every program of the catalogue, the box it is rendered in, an orbit camera and a camera inside the box ----
# (name of the catalogue entry) -> (bounds_min, bounds_max, orbit eye, inside eye, inside target).  The box is the render
# parameters' (bounds_min / bounds_max), chosen per scene like the cameras, on the restatement alone, so that the orbit view
# holds hits, rays that cross the box and leave it, and pixels off the box (test_program_march_cpu.py asserts the shares).
UNIT = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
CLOSE = (1.125, 1.35, 2.25)
SCENES = {
    "anchor": UNIT + (CLOSE, (0.1, 0.2, 0.3), (1.0, 0.6, -0.4)),
    "no_material": UNIT + (CLOSE, (0.0, 0.1, 0.6), (0.5, 0.0, -0.3)),
    "all_ops": ((-1.0, -0.9, -0.8), (1.0, 0.9, 0.8)) + ((0.09, -2.7, 0.135), (0.6, 0.7, 0.6), (-0.3, -0.2, -0.1)),
    "deep": UNIT + (CLOSE, (0.0, 0.8, 0.8), (0.0, -0.2, -0.3)),
    # (`sixteen` closes with INTERSECT against the plane 0.95 - z: its value is positive in the whole box -- no view of it has a hit)
    "sixteen": UNIT + ((3.0, -4.5, 3.0), (0.9, -0.9, 0.2), (-0.3, 0.2, 0.3)),
    "single": UNIT + (CLOSE, (0.9, 0.8, 0.7), (0.0, 0.0, 0.0)),
    "envelope": ((-1.0, -0.9, -0.8), (1.0, 0.9, 0.8)) + ((0.18, 1.35, 2.475), (0.001, 0.2, 0.3), (0.0, -0.5, -0.6)),
    "late_material": ((-1.0, -0.9, -0.8), (1.0, 0.9, 0.8)) + ((0.18, 1.35, 2.475), (0.3, 0.8, 0.7), (0.2, 0.0, -0.5)),
    "ties": UNIT + (CLOSE, (0.0, 0.0, 0.9), (0.3, 0.2, -0.5)),
    # (inside the unit box `ties_zero` is solid: its sphere has radius 2.  A larger box shows it from outside)
    "ties_zero": ((-3.0, -3.0, -3.0), (3.0, 3.0, 3.0)) + ((3.375, 4.05, 6.75), (2.5, 2.6, 2.4), (0.0, 0.0, 0.0)),
}
GRAZE = "graze"  # one more scene, built for status -1: a plane met at a shallow angle


def builders(PM):
    cat = dict(R.catalogue(PM))
    cat[GRAZE] = PM.Program((-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)).material(0.3, 0.6, 0.9, 0.2, 0.5, 1.0).plane(0.0, 1.0, 0.0, 0.95)
    return cat


SCENES[GRAZE] = UNIT + (CLOSE, (0.9, -0.9495, 0.0), (-1.0, -0.9502, 0.1))


def render_params(pkg, name):
    lo, hi = SCENES[name][:2]
    return pkg.default_render_params(pkg.make_grid((256, 256, 256), lo, hi))


def cameras(pkg, name, width, height):
    """(orbit, inside) for a width x height image."""
    _, _, orbit, eye, target = SCENES[name]
    aspect = width / height
    return pkg.camera_look_at(eye=orbit, aspect=aspect), pkg.camera_look_at(eye=eye, target=target, aspect=aspect, fovy_degrees=70.0)


def aux_view(a):
    """[..., 18] float32 (what the bindings hand out) -> structured sdfv_march_aux array."""
    return np.ascontiguousarray(a).view(AUX_DTYPE).reshape(a.shape[:-1])


def assert_aux_bitwise(got, want, what):
    for f in BITWISE_FIELDS:
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        bad = np.argwhere((g.view(np.uint32) != w.view(np.uint32)).reshape(g.shape[:2] + (-1,)).any(axis=-1))
        assert bad.size == 0, (what, f, len(bad), bad[:3].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:2]])


def lane_utilisation(steps, tile_w, tile_h):
    """sum(steps) / (64 * sum over waves of the wave's max steps) for waves of tile_w x tile_h pixels (tile_w * tile_h = 64) cut
    the way the kernel cuts the image: 16 x 16 workgroup tiles of 8 x 8 waves, or rows of 64."""
    assert tile_w * tile_h == 64
    H, W = steps.shape
    ph, pw = -(-H // tile_h) * tile_h, -(-W // tile_w) * tile_w
    s = np.zeros((ph, pw), np.int64)
    s[:H, :W] = steps
    waves = s.reshape(ph // tile_h, tile_h, pw // tile_w, tile_w).max(axis=(1, 3))
    return float(steps.sum()) / float(64 * waves.sum()) if waves.sum() else 1.0
