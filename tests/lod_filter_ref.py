"""Shared by tests/test_lod_filter_cpu.py and tests/test_gpu_lod_filter.py: a vectorised numpy float32 restatement of the grid
march's whole per-pixel path under the lattice filter (include/sdfgrid.h, SDFV_OPT_RAYMARCH_LOD_FILTER = 1), written from the
header's description and the shader's per-pixel algorithm; it calls nothing of the library.  Every arithmetic step is one
float32 numpy operation, in the order the header states them; the loop keeps a mask per pixel.  Set-up pieces, mix() and the
shading come from tests/program_march_ref.py, fields and cameras from tests/march_fields.py.

With L = 1 the formulas are the LINEAR filter's clamp footprint (s = u, M = N): tests/test_lod_filter_cpu.py holds that case
to oracle/raymarch.c bit for bit, which pins everything here but the division by L and the lattice indices."""
import numpy as np

import march_fields  # noqa: F401  (re-exported: the tests take fields and cameras from here)
from program_march_ref import AUX_DTYPE, F, _len3, _mix, _oob, cam_fields, normal_h_of, shade

TAPS = ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1))  # k.xyy, k.yyx, k.yxy, k.xxx with k = (1, -1)


def lattice_points(n, lod):
    """M = (N + L - 1) / L: what LoadingManager's pass over an axis of n voxels with step L visits."""
    return (int(n) + int(lod) - 1) // int(lod)


def off_lattice_mask(shape_dhw, lod):
    """[D, H, W] bool: True where a texel is NOT on the lattice of step `lod` (some index is no multiple of it)."""
    d, h, w = shape_dhw
    on = (np.arange(d) % lod == 0)[:, None, None] & (np.arange(h) % lod == 0)[None, :, None] & (np.arange(w) % lod == 0)[None, None, :]
    return ~on


def poison_off_lattice(tex, lod, value=np.nan):
    """A copy of tex [D, H, W, 4] whose off-lattice texels hold `value` in all four channels."""
    out = tex.copy()
    out[off_lattice_mask(tex.shape[:3], lod)] = F(value)
    return out


def footprint(p, lo, hi, shape_dhw, lod):
    """The filter's two texel indices and weight per axis at positions p = [x, y, z] (float32 arrays):
    -> ([i0, j0, k0], [i1, j1, k1], [ax, ay, az])."""
    i0, i1, a = [], [], []
    for axis in range(3):
        n = shape_dhw[2 - axis]
        q = (p[axis] - lo[axis]) / (hi[axis] - lo[axis])  # to_p01: the divide (an exact reciprocal gives the same bits)
        u = q * F(n) - F(0.5)
        s = u / F(lod)
        f = np.floor(s)
        a.append(s - f)
        top = lattice_points(n, lod) - 1
        f = np.where(np.isnan(f), F(0), f)
        i0.append(np.clip(f, 0, top).astype(np.int64) * lod)          # clamp(m, 0, M - 1) * L
        i1.append(np.clip(f + F(1), 0, top).astype(np.int64) * lod)   # clamp(m + 1, 0, M - 1) * L
    return i0, i1, a


def sample(tex, p, lo, hi, lod, channel=None):
    """The filtered sample of tex [D, H, W, 4] at p: [n] for one channel, [n, 4] for all."""
    (i0, j0, k0), (i1, j1, k1), (ax, ay, az) = footprint(p, lo, hi, tex.shape[:3], lod)
    t = tex if channel is None else tex[..., channel]
    if channel is None:
        ax, ay, az = ax[:, None], ay[:, None], az[:, None]
    c00, c10 = _mix(t[k0, j0, i0], t[k0, j0, i1], ax), _mix(t[k0, j1, i0], t[k0, j1, i1], ax)
    c01, c11 = _mix(t[k1, j0, i0], t[k1, j0, i1], ax), _mix(t[k1, j1, i0], t[k1, j1, i1], ax)
    return _mix(_mix(c00, c10, ay), _mix(c01, c11, ay), az)


@np.errstate(all="ignore")
def march(rp, tex0, tex1, cam, width, height, y0=0, y1=None, lod=None):
    """-> (aux [rows, width] structured sdfv_march_aux, rgba [rows, width, 4]).  tex0 / tex1: float32 [D, H, W, 4];
    lod: L (default: rp.lod_dist_between_samples, which also sets the normal's tap distance)."""
    y1 = height if y1 is None else y1
    lod = int(rp.lod_dist_between_samples) if lod is None else int(lod)
    assert lod >= 1 and lod & (lod - 1) == 0 and tuple(tex0.shape[:3]) == tuple(int(n) for n in rp.tex_size)[::-1]
    c = cam_fields(cam)
    lo, hi = [F(v) for v in rp.bounds_min], [F(v) for v in rp.bounds_max]
    # the primary ray, the bbox fragment and main()'s ray set-up (material.frag:130-139)
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

    # sdfRaycast(rayOrigin, rayDir, 256), material.frag:92-128: 255 samples at the most
    pos = [o.copy() for o in origin]
    dist = np.zeros(n, F)
    status = np.where(covered, -1, 0).astype(np.int32)
    steps = np.zeros(n, np.int32)
    marching = covered.copy()
    for _ in range(255):
        out = marching & (_oob(pos, lo, hi) > F(1e-4))
        status[out] = -2
        marching &= ~out
        idx = np.flatnonzero(marching)
        if idx.size == 0:
            break
        d = sample(tex0, [pos[a][idx] for a in range(3)], lo, hi, lod, channel=0) - F(1e-1)
        steps[idx] += 1
        hit = d < F(1e-5)
        status[idx[hit]] = 1
        marching[idx[hit]] = False
        go, dg = idx[~hit], d[~hit]
        dist[go] = dist[go] + dg
        for a in range(3):
            pos[a][go] = pos[a][go] + rd[a][go] * dg

    aux = np.zeros(n, AUX_DTYPE)
    aux["depth"] = 1
    aux["status"], aux["steps"] = status, np.where(covered, steps, 0)
    for a in range(3):
        aux["hit_pos"][:, a] = np.where(covered, pos[a], F(0))
    aux["t"] = np.where(covered, dist, F(0))
    rgba = np.zeros((n, 4), F)
    h = np.flatnonzero(status == 1)
    if h.size:
        p = [pos[a][h] for a in range(3)]
        raw0, raw1 = sample(tex0, p, lo, hi, lod), sample(tex1, p, lo, hi, lod)
        hh = normal_h_of(rp.tex_size, rp.lod_dist_between_samples)
        acc = None
        for k in TAPS:  # sdfNormal, material.frag:73-80
            d = sample(tex0, [p[a] + F(k[a]) * hh for a in range(3)], lo, hi, lod, channel=0) - F(1e-1)
            term = [F(k[a]) * d for a in range(3)]
            acc = term if acc is None else [acc[a] + term[a] for a in range(3)]
        l = _len3(*acc)
        for a in range(3):
            aux["normal"][h, a] = acc[a] / l
        aux["raw0"][h], aux["raw1"][h] = raw0, raw1
        m = c["bvp"]
        hz = m[2] * p[0] + m[6] * p[1] + m[10] * p[2] + m[14]
        hw = m[3] * p[0] + m[7] * p[1] + m[11] * p[2] + m[15]
        aux["depth"][h] = hz / hw  # gl_FragDepth, material.frag:180-181
        rgba[h] = shade(rp, raw0, raw1)
    shape = (y1 - y0, width)
    return aux.reshape(shape), rgba.reshape(shape + (4,))


def nan_normal(aux):
    """[rows, width] bool: hits whose restated normal has a NaN component (four taps that read equal values: 0 / 0)."""
    return (aux["status"] == 1) & np.isnan(aux["normal"]).any(axis=-1)


def assert_record_equal(got, want, what, fields=("status", "steps", "hit_pos", "t", "raw0", "raw1", "normal", "depth")):
    """Every field bit for bit; where the wanted normal is NaN only NaN-ness is compared."""
    nn = nan_normal(want)
    for f in fields:
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        diff = (g.view(np.uint32) != w.view(np.uint32)).reshape(g.shape[:2] + (-1,)).any(axis=-1)
        if f == "normal":
            diff &= ~nn
            assert (np.isnan(g).any(axis=-1) == np.isnan(w).any(axis=-1))[nn].all(), (what, "NaN-ness of the normal")
        bad = np.argwhere(diff)
        assert bad.size == 0, (what, f, len(bad), bad[:3].tolist(), [(got[tuple(b)][f], want[tuple(b)][f]) for b in bad[:2]])
