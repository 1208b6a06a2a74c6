"""The comparison shared by the GPU parity tests of the grid march (tests/test_gpu_raymarch.py over the demo fill,
tests/test_gpu_raymarch_fields.py over tests/march_fields.py's textures): every march kernel variant against
oracle/raymarch.c, every aux field bit for bit, the shaded RGBA to RGBA_TOL."""
import numpy as np
import torch

from arena import canary_words

RGBA_TOL = 1e-4


class Canaried:
    """Outputs pre-filled with tests/arena.py's canary: the caching allocator hands a fresh torch.empty the block the previous
    variant just filled correctly, so a variant that skips a tile, a row or a camera would pass on stale results."""

    def __init__(self):
        self.patterns = {}

    def __call__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        if n not in self.patterns:
            self.patterns[n] = torch.from_numpy(canary_words(0, n).view(np.int32)).cuda()
        return self.patterns[n].clone().view(dtype).view(tuple(shape))

    def assert_none_left(self, t, what):
        stale = int((t.reshape(-1).view(torch.int32) == self.patterns[t.numel()]).sum())
        assert stale == 0, f"{what}: {stale} of {t.numel()} words were never written (they still hold the canary)"


def setup_grid(pkg, oracle, dims, bb_min=(-1, -1, -1), bb_max=(1, 1, 1), **kw):
    prm = pkg.default_params(**kw)
    g = pkg.make_grid(dims, bb_min, bb_max)
    t0, t1 = pkg.alloc_textures(g)
    pkg.fill_grid(prm, g, t0, t1)
    torch.cuda.synchronize()
    return g, t0, t1, t0.cpu().numpy(), t1.cpu().numpy()


def aux_to_np(oracle, aux):
    return aux.cpu().numpy().view(oracle.AUX_DTYPE).reshape(aux.shape[:-1])


def variants(K):
    """{name: SDFV_OPT_RAYMARCH_DISABLE mask} of every march kernel family (K = pkg._capi); volumes_of() says which volumes a
    variant is handed."""
    # "fast" / "dist" take the hand-written gfx950 march loop where its specialisation applies (power-of-two grid,
    # symmetric box); "*_c" force the compiler's loop on the same kernels
    # "*_b": the hand-written loop with its interior fetch path switched off (every cell through the clamping fetch)
    return {"fast": 0, "dist": 0, "fast_c": K.RM_NO_ASM_LOOP, "dist_c": K.RM_NO_ASM_LOOP, "general": K.RM_NO_FAST_INDEX,
            "fast_b": K.RM_NO_INTERIOR_FETCH, "dist_b": K.RM_NO_INTERIOR_FETCH,
            # "pairs*": the y-pair volume (two 16-byte gathers per cell), its border fetch for every cell, and a launch
            # whose specialisation does not apply (falls back to the distance volume)
            "pairs": 0, "pairs_b": K.RM_NO_INTERIOR_FETCH, "pairs_c": K.RM_NO_ASM_LOOP,
            # "ilv*": the y-interleaved volume, likewise
            "ilv": 0, "ilv_b": K.RM_NO_INTERIOR_FETCH, "ilv_c": K.RM_NO_ASM_LOOP,
            # without the distance volume beside them (given it, a non-cubic grid marches over that instead)
            "pairs_only": 0, "ilv_only": 0,
            "fast_plain": K.RM_NO_SYMMETRIC | K.RM_NO_POW2_SIZE,
            "fast_div": K.RM_NO_SYMMETRIC | K.RM_NO_POW2_EXTENT}


def volumes_of(variant, dist, pairs, ilv):
    """The dist / pairs / ilv keywords of pkg.raymarch for a variant of variants()."""
    return dict(dist=dist if variant.startswith(("dist", "pairs", "ilv")) and not variant.endswith("_only") else None,
                pairs=pairs if variant.startswith("pairs") else None, ilv=ilv if variant.startswith("ilv") else None)


def compare(pkg, oracle, g, t0, t1, h0, h1, cam_kw, width, height, rp_edit=None, y0=0, y1=None):
    rp = pkg.default_render_params(g)
    if rp_edit:
        rp_edit(rp)
    cam = pkg.camera_look_at(aspect=width / height, **cam_kw)
    orp = oracle.copy_struct(oracle.RenderParams, rp)
    ocam = oracle.copy_struct(oracle.Camera, cam)
    want_rgba, want_aux = oracle.raymarch(orp, h0, h1, ocam, width, height, y0=y0, y1=y1)
    canaried = Canaried()
    dist = pkg.commit_distance(g, t0, dist=canaried(tuple(t0.shape[:-1])))
    canaried.assert_none_left(dist, "commit_distance")
    assert torch.equal(dist, t0[..., 0])
    whole = pkg.make_grid(tuple(int(d) for d in g.dims), tuple(g.bb_min), tuple(g.bb_max))
    pairs = pkg.commit_pairs(whole, dist, pairs=canaried(tuple(dist.shape) + (2,)))  # (d[y], d[min(y + 1, H - 1)]) per texel
    canaried.assert_none_left(pairs, "commit_pairs")
    assert torch.equal(pairs[..., 0], dist) and torch.equal(pairs[:, :-1, :, 1], dist[:, 1:]) and torch.equal(pairs[:, -1, :, 1], dist[:, -1])
    ilv = None
    if int(g.dims[1]) % 2 == 0:  # the y-interleaved volume pairs rows 2p, 2p + 1
        ilv = pkg.commit_interleaved(whole, dist, ilv=canaried(tuple(dist.shape)))
        canaried.assert_none_left(ilv, "commit_interleaved")
        v = ilv.view(dist.shape[0], dist.shape[1] // 2, dist.shape[2], 2)
        assert torch.equal(v[..., 0], dist[:, 0::2]) and torch.equal(v[..., 1], dist[:, 1::2])
    # every march kernel family must reproduce the oracle: the fast march (symmetric-box / fused-scale /
    # reciprocal / divide variants) over tex0.r, the same over the compact distance volume, and the general
    # kernel (full MirroredRepeat, the shader's nested loop)
    K = pkg._capi
    disabled = variants(K)
    rows = (height if y1 is None else y1) - y0
    for variant, mask in disabled.items():
        if variant.startswith("ilv") and ilv is None:
            continue
        # the whole of every output is rendered rows [y0, y1): after the launch no canary may survive anywhere in them
        outs = dict(out=canaried((1, rows, width, 4)), depth_out=canaried((1, rows, width)),
                    aux_out=canaried((1, rows, width, pkg.AUX_FLOATS), torch.int32))
        outs_plain = dict(out=canaried((1, rows, width, 4)), depth_out=canaried((1, rows, width)))
        with pkg.options({K.OPT_RAYMARCH_DISABLE: mask}):
            vols = volumes_of(variant, dist, pairs, ilv)
            use_dist, use_pairs, use_ilv = vols["dist"], vols["pairs"], vols["ilv"]
            rgba, depth, aux = pkg.raymarch(rp, t0, t1, cam, width, height, y0=y0, y1=y1, want_aux=True,
                                            want_depth=True, dist=use_dist, pairs=use_pairs, ilv=use_ilv, **outs)
            # the depth plane without the 72-byte record must be the same plane
            rgba_plain, depth_only = pkg.raymarch(rp, t0, t1, cam, width, height, y0=y0, y1=y1, want_depth=True,
                                                  dist=use_dist, pairs=use_pairs, ilv=use_ilv, **outs_plain)
            torch.cuda.synchronize()
        for name, t in (("rgba", rgba), ("depth", depth), ("aux", aux), ("rgba without aux", rgba_plain), ("depth without aux", depth_only)):
            canaried.assert_none_left(t, f"{variant}: {name}")
        assert torch.equal(depth.view(torch.int32), depth_only.view(torch.int32)), variant
        # the kernel WITHOUT the aux record (the one bench.py times) writes the same RGBA as the one with it
        assert torch.equal(rgba.view(torch.int32), rgba_plain.view(torch.int32)), f"{variant}: aux / no-aux RGBA differ"
        assert torch.equal(depth.view(torch.int32), aux[..., -1]), f"{variant}: depth plane != aux.depth"
        got_rgba = rgba[0].cpu().numpy()
        got_aux = aux_to_np(oracle, aux)[0]
        for field in ("status", "steps"):
            np.testing.assert_array_equal(got_aux[field], want_aux[field], err_msg=f"{variant}:{field}")
        for field in ("hit_pos", "t", "raw0", "raw1", "normal", "depth"):
            np.testing.assert_array_equal(got_aux[field].view(np.uint32), want_aux[field].view(np.uint32),
                                          err_msg=f"{variant}:{field}")
        assert np.abs(got_rgba - want_rgba).max() <= RGBA_TOL, variant
        np.testing.assert_array_equal(got_rgba[..., 3], want_rgba[..., 3])
    return got_rgba, got_aux


def load_textures(pkg, g, tex0, tex1):
    """Host arrays [D, H, W, 4] float32 -> the device texture pair of grid `g` (pkg.alloc_textures)."""
    t0, t1 = pkg.alloc_textures(g)
    assert tuple(t0.shape) == tex0.shape and tuple(t1.shape) == tex1.shape
    t0.copy_(torch.from_numpy(tex0))
    t1.copy_(torch.from_numpy(tex1))
    torch.cuda.synchronize()
    return t0, t1
