"""The grid march, the slab rounds, bands_scatter and the three mesh extractors on the caller's stream (tests/stream_gate.py).

sdfv_raymarch_ex over the 16^3 `steep` volume of tests/test_gpu_containment_march.py, 40 x 30 images, every host argument (the
descriptor, the render parameters, the camera array) the test's own and overwritten on return: one camera over the distance,
the pair and the interleaved volume; 17 host cameras (the camera ring's writer kernels run on the caller's stream in front of
the march); 70 host cameras, staged -- through the ring a launch carries up to 64, so two launches, the first on the caller's
stream, the second on a side stream forked from it and joined back -- and with SDFV_OPT_RAYMARCH_CAMERA_STAGING off -- launches
of 16, so five, dealt to the caller's stream and the three side streams, every side stream forked and joined (what a capture of
the staged case takes too); a device camera array;
the 8-bit plane alone; a band set; and the trilinear filter over the loaded lattice of a loading grid
(SDFV_OPT_RAYMARCH_LOD_FILTER, tests/test_gpu_containment_lod.py's case).  sdfv_raymarch_slab and sdfv_raymarch_slab_round:
the first round of a rank that owns the whole grid of tests/test_gpu_containment_sharded.py, so that the oracle's image of that
grid is the expected one (the image is cleared and marched: a memset and a launch).  Expected pixels are the oracle's and
lod_filter_ref.march's.

The extractors -- mesh_extract, program_mesh_extract, lattice_mesh_extract, 9 cells, marching cubes and dual contouring -- are
documented to synchronise `stream` and are held to THAT: the mesh is the restatement's with the lattice arriving late, the
stream is idle when the call returns, and the host was held for as long as the sleep in front of the call."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import arena as A
import lattice_mesh_ref as LM
import stream_gate as SG
import test_gpu_containment_lod as CL
import test_gpu_containment_march as CM
import test_gpu_containment_sharded as CS
from march_compare import RGBA_TOL
from stream_gate import capture, gate  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
F = np.float32
FIELD, GRID, WIDTH, HEIGHT = "steep", "cube16", 40, 30
DUAL = LM.DUAL
UNIT_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def normal_open(pkg):
    words = np.zeros(pkg.AUX_FLOATS, bool)
    words[CM.AUX_NORMAL] = True  # sdfv_march_aux.normal: 0 / 0 of a zero tap sum
    return words


# ---- sdfv_raymarch_ex ----------------------------------------------------------------------------------------------------------
MARCHES = {  # name: (cameras, "host" | "device", volumes beside the textures, planes, rows[, options])
    "one-dist": (1, "host", ("dist",), ("rgba", "depth", "aux"), None),
    "one-pairs": (1, "host", ("dist", "pairs"), ("rgba",), None),
    "one-ilv": (1, "host", ("dist", "ilv"), ("rgba", "depth"), None),
    "one-textures": (1, "host", (), ("rgba", "aux"), (3, 25)),
    "seventeen-host": (17, "host", ("dist",), ("rgba",), None),
    "seventy-host": (70, "host", ("dist",), ("rgba",), None),           # 64 + 6: the caller's stream and one side stream
    "seventy-host-unstaged": (70, "host", ("dist",), ("rgba",), None, "unstaged"),   # 4 x 16 + 6 over all four streams
    "twenty-device": (20, "device", ("dist",), ("rgba", "depth"), None),
    "rgba8-only": (1, "host", ("dist",), ("rgba8",), None),
    "bands": (2, "host", ("dist",), ("rgba", "depth"), ("bands", 1, 2, 8)),   # bands 1 and 3 of 8 rows; band 3 is the short one
}


def march_case(pkg, name):
    n_cam, where, vols, planes, rows, *opts = MARCHES[name]
    options = {pkg._capi.OPT_RAYMARCH_CAMERA_STAGING: 0} if opts else {}
    dims, lo, hi = CM.GRIDS[GRID]
    h0, h1, dist, pairs, ilv = CM.volume(FIELD, GRID)
    ys = CM.rows_of(HEIGHT, rows)
    if rows is not None and rows[0] == "bands":
        assert len(ys) == pkg.lib.sdfv_band_rows_ex(HEIGHT, *rows[1:])
    view = [k % 3 for k in range(n_cam)]
    kws = CM.camera_kws(GRID)
    want_rgba = np.stack([CM.oracle_image(FIELD, GRID, k, WIDTH, HEIGHT)[0][ys] for k in view])
    want_aux = np.stack([CM.oracle_image(FIELD, GRID, k, WIDTH, HEIGHT)[1][ys] for k in view])
    assert (want_aux["status"] == 1).any(), "the view shows the surface"
    shape = (n_cam, len(ys), WIDTH)
    shapes = {"rgba": (shape + (4,), F, 16), "depth": (shape, F, 4), "aux": (shape + (pkg.AUX_FLOATS,), np.int32, 4),
              "rgba8": (shape + (4,), np.uint8, 4)}
    expected = {"rgba": A.Approx(want_rgba, RGBA_TOL), "rgba8": A.Approx(CM.quantise(want_rgba), 1), "depth": np.ascontiguousarray(want_aux["depth"]),
                "aux": A.Untouched(np.ascontiguousarray(want_aux).view(np.int32).reshape(shapes["aux"][0]), nan_open=normal_open(pkg))}
    host_vols = dict(dist=(dist, 4), pairs=(pairs, 8), ilv=(ilv, 8))
    inputs = {"tex0": (h0, 16), "tex1": (h1, 16), **{v: host_vols[v] for v in vols}}

    def cameras():
        return (pkg.Camera * n_cam)(*[pkg.camera_look_at(aspect=WIDTH / HEIGHT, **kws[k]) for k in view])
    if where == "device":
        inputs["cameras"] = (np.frombuffer(bytes(cameras()), np.uint8).copy(), 4)

    def host():
        h = {"rp": pkg.default_render_params(pkg.make_grid(dims, lo, hi)), "desc": pkg._capi.MarchDesc()}
        if where == "host":
            h["cameras"] = cameras()
        return h

    def call(t, h):
        d = h["desc"]
        d.size, d.rp = C.sizeof(d), C.pointer(h["rp"])
        d.tex0, d.tex1 = t["tex0"].data_ptr(), t["tex1"].data_ptr()
        for v in vols:
            setattr(d, v, t[v].data_ptr())
        d.cameras = C.cast(h["cameras"], C.POINTER(pkg.Camera)) if where == "host" else C.cast(C.c_void_p(t["cameras"].data_ptr()), C.POINTER(pkg.Camera))
        d.n_cameras, d.width, d.height, d.y0, d.y1 = n_cam, WIDTH, HEIGHT, 0, HEIGHT
        if rows is not None and rows[0] == "bands":
            d.band_first, d.band_step, d.band_height = rows[1:]
        elif rows is not None:
            d.y0, d.y1 = rows
        for p in planes:
            setattr(d, p, t[p].data_ptr())
        pkg.check(pkg.lib.sdfv_raymarch_ex(C.byref(d), stream_ptr()))
    return SG.Case(f"raymarch_ex-{name}", call, {p: expected[p] for p in planes}, inputs=inputs, outputs={p: shapes[p] for p in planes}, host=host,
                   poison_around="inputs", options=options)


def lod_case(pkg):
    dims, lod, box = CL.CASES[0]
    lo, hi = box
    p0, p1, views = CL.case("steep", dims, lod, box)
    kw = CL.T.case_cameras(lo, hi)[0]
    want, want_rgba = views[0]
    assert (want["status"] == 1).any()
    shape = (1, CL.HEIGHT, CL.WIDTH)
    expected = {"rgba": A.Approx(want_rgba[None], RGBA_TOL), "depth": np.ascontiguousarray(want["depth"][None]),
                "aux": A.Untouched(np.ascontiguousarray(want).view(np.int32).reshape(shape + (pkg.AUX_FLOATS,)), nan_open=normal_open(pkg))}

    def host():
        rp = pkg.default_render_params(pkg.make_grid(dims, lo, hi))
        rp.lod_dist_between_samples = float(lod)
        return {"rp": rp, "cameras": (pkg.Camera * 1)(pkg.camera_look_at(aspect=CL.WIDTH / CL.HEIGHT, **kw)), "desc": pkg._capi.MarchDesc()}

    def call(t, h):
        d = h["desc"]
        d.size, d.rp, d.tex0, d.tex1 = C.sizeof(d), C.pointer(h["rp"]), t["tex0"].data_ptr(), t["tex1"].data_ptr()
        d.cameras, d.n_cameras, d.width, d.height, d.y0, d.y1 = C.cast(h["cameras"], C.POINTER(pkg.Camera)), 1, CL.WIDTH, CL.HEIGHT, 0, CL.HEIGHT
        d.rgba, d.depth, d.aux = t["rgba"].data_ptr(), t["depth"].data_ptr(), t["aux"].data_ptr()
        pkg.check(pkg.lib.sdfv_raymarch_ex(C.byref(d), stream_ptr()))
    return SG.Case("raymarch_ex-lod-filter", call, expected, inputs={"tex0": (p0, 16), "tex1": (p1, 16)},
                   outputs={"rgba": (shape + (4,), F, 16), "depth": (shape, F, 4), "aux": (shape + (pkg.AUX_FLOATS,), np.int32, 4)}, host=host,
                   poison_around="inputs", options={pkg._capi.OPT_RAYMARCH_LOD_FILTER: 1})


# ---- the slab rounds -----------------------------------------------------------------------------------------------------------
def slab_case(pkg, mode):
    """The first round of the one rank of a world of one: every ray ends here, nothing is handed on, the image is the whole
    grid's.  A pixel whose ray never enters the grid is reported by no rank: its record stays cleared, whatever depth the
    single-GPU march writes there."""
    r0, r1, want_rgba, want_aux = CS.whole_grid()
    W, H, cap = CS.WIDTH, CS.HEIGHT, CS.CAPACITY
    words = np.ascontiguousarray(want_aux).view(np.int32).reshape(H, W, pkg.AUX_FLOATS).copy()
    depth_open = np.zeros(words.shape, bool)
    depth_open[..., 17] = want_aux["status"] == 0
    assert (want_aux["status"] == 1).any()
    head = CS.HEADER_WORDS if mode == "round" else 0
    n_words = head + CS.RAY_WORDS * cap
    empty = np.zeros(n_words, np.int32)
    header = np.zeros(n_words, bool)
    header[:head] = True   # the count (0) and the rest of the header, cleared by the call; no entry is written
    expected = {"rgba": A.Approx(want_rgba, RGBA_TOL), "aux": A.Untouched(words, nan_open=normal_open(pkg), undefined=depth_open),
                "out_down": A.Untouched(empty, written=header), "out_up": A.Untouched(empty, written=header)}
    flag = "counters" if mode == "slab" else "overflow"
    expected[flag] = np.zeros(2 if mode == "slab" else 1, np.int32)

    def host():
        return {"rp": pkg.default_render_params(pkg.make_grid(CS.DIMS, *CS.BB)), "grid": pkg.make_grid(CS.DIMS, *CS.BB),
                "camera": pkg.camera_look_at(eye=CS.EYE, aspect=W / H)}

    def call(t, h):
        p = lambda name: C.c_void_p(t[name].data_ptr())  # noqa: E731
        if mode == "slab":
            pkg.check(pkg.lib.sdfv_raymarch_slab(C.byref(h["rp"]), C.byref(h["grid"]), 0, 0, p("tex0"), p("tex1"), C.byref(h["camera"]), W, H, None, 0,
                                                 p("rgba"), p("aux"), p("out_down"), p("out_up"), cap, p("counters"), stream_ptr()))
        else:
            pkg.check(pkg.lib.sdfv_raymarch_slab_round(C.byref(h["rp"]), C.byref(h["grid"]), 0, 0, p("tex0"), p("tex1"), C.byref(h["camera"]), W, H,
                                                       None, None, 1, p("rgba"), p("aux"), p("out_down"), p("out_up"), cap, p("overflow"), stream_ptr()))
    return SG.Case(f"raymarch_slab{'_round' if mode == 'round' else ''}", call, expected, inputs={"tex0": (r0, 16), "tex1": (r1, 16)},
                   inouts={flag: (expected[flag], 4)},
                   outputs={"rgba": ((H, W, 4), F, 16), "aux": ((H, W, pkg.AUX_FLOATS), np.int32, 4), "out_down": ((n_words,), np.int32, 4),
                            "out_up": ((n_words,), np.int32, 4)}, host=host, poison_around="inputs")


def scatter_case(pkg, channels):
    n_cam, width, height, first, step, bh = 2, 33, 90, 1, 3, 8
    rows = CM.rows_of(height, ("bands", first, step, bh))
    assert len(rows) == pkg.lib.sdfv_band_rows_ex(height, first, step, bh)
    written = np.zeros((n_cam, height, width, channels), bool)
    written[:, rows] = True

    def data(seed):
        part = np.random.default_rng(seed).uniform(0.0, 1.0, (n_cam, len(rows), width, channels)).astype(F)
        want = np.zeros((n_cam, height, width, channels), F)
        want[:, rows] = part
        return part, {"out": A.Untouched(want, written)}
    part, expected = data(channels)
    part2, expected2 = data(channels + 100)
    align = 16 if channels == 4 else 4
    return SG.Case(f"bands_scatter-{channels}",
                   lambda t, h: pkg.check(pkg.lib.sdfv_bands_scatter(C.c_void_p(t["part"].data_ptr()), first, step, bh, n_cam, width, height, channels,
                                                                     C.c_void_p(t["out"].data_ptr()), stream_ptr())),
                   expected, inputs={"part": (part, align)}, outputs={"out": (written.shape, F, align)}, second=({"part": part2}, expected2))


# ---- tests ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MARCHES))
def test_the_march_runs_on_the_callers_stream(pkg, gate, capture, name):
    gate.run(pkg, march_case(pkg, name))
    capture.run(pkg, march_case(pkg, name))


def test_the_lattice_filter_march_runs_on_the_callers_stream(pkg, gate, capture):
    gate.run(pkg, lod_case(pkg))
    capture.run(pkg, lod_case(pkg))


@pytest.mark.parametrize("mode", ["slab", "round"], ids=["sdfv_raymarch_slab", "sdfv_raymarch_slab_round"])
def test_a_slab_round_runs_on_the_callers_stream(pkg, gate, capture, mode):
    gate.run(pkg, slab_case(pkg, mode))
    capture.run(pkg, slab_case(pkg, mode))


@pytest.mark.parametrize("channels", [4, 18])  # the 16-byte path and the scalar one
def test_bands_scatter_runs_on_the_callers_stream(pkg, gate, capture, channels):
    gate.run(pkg, scatter_case(pkg, channels))
    capture.run(pkg, scatter_case(pkg, channels))


# ---- the extractors: documented to synchronise `stream` -------------------------------------------------------------------------
CELLS = 9
LATTICE_BB = (-1.0, -0.75, -1.0, 1.0, 1.0, 0.5)


@functools.lru_cache(maxsize=None)
def wanted_mesh(entry, algorithm):
    """(vertices [V, 12] float32, indices int64) from the restatements, computed once."""
    import oracle_binding as oracle
    pkg, PM = importlib.import_module("sdf-viewer_amd"), importlib.import_module("sdf-viewer_amd.program")  # noqa: N806
    if entry == "lattice":
        v, i, _ = LM.extract(np.ascontiguousarray(LM.gyroid_lattice(CELLS, LATTICE_BB), F), LATTICE_BB, algorithm)
    elif entry == "program":
        import program_mesh_ref as PMR
        import program_ref as R
        b = R.catalogue(PM)["all_ops"]
        v, i, _ = PMR.extract(b.ops, CELLS, b.bb, algorithm=algorithm)
    else:
        import demo_mesh_ref as DM
        v, i, _ = DM.extract_demo(oracle, oracle.params_from(pkg.default_params()), CELLS, UNIT_BOX, 0, algorithm)
    assert len(i) > 0
    return np.ascontiguousarray(v, F), np.asarray(i, np.int64)


@pytest.mark.parametrize("algorithm", [0, DUAL], ids=["marching_cubes", "dual_contouring"])
@pytest.mark.parametrize("entry", ["demo", "program", "lattice"])
def test_the_extractors_synchronise_their_stream(pkg, gate, entry, algorithm):
    import program_ref as R
    want_v, want_i = wanted_mesh(entry, algorithm)
    meshes = []
    builder = R.catalogue(importlib.import_module("sdf-viewer_amd.program"))["all_ops"]
    prog = builder.build() if entry == "program" else None

    def host():
        bb = LATTICE_BB if entry == "lattice" else (tuple(builder.bb) if entry == "program" else UNIT_BOX[0] + UNIT_BOX[1])
        h = {"bb_min": pkg.f3(bb[:3]), "bb_max": pkg.f3(bb[3:])}
        if entry == "demo":
            h["params"] = pkg.default_params()
        return h

    def call(t, h):
        m = pkg._capi.Mesh()
        if entry == "demo":
            rc = pkg.lib.sdfv_mesh_extract(C.byref(h["params"]), pkg.SDF_DEMO, h["bb_min"], h["bb_max"], CELLS, algorithm, C.byref(m), stream_ptr())
        elif entry == "program":
            rc = pkg.lib.sdfv_program_mesh_extract(prog.h, h["bb_min"], h["bb_max"], CELLS, algorithm, 0, C.byref(m), stream_ptr())
        else:
            rc = pkg.lib.sdfv_lattice_mesh_extract(C.c_void_p(t["dist"].data_ptr()), h["bb_min"], h["bb_max"], CELLS, algorithm, 0, C.byref(m), stream_ptr())
        meshes.append(m)   # (converted and freed after the gate: mesh_tensors synchronises the device)
        pkg.check(rc)
    inputs = {"dist": (np.ascontiguousarray(LM.gyroid_lattice(CELLS, LATTICE_BB), F).reshape(-1), 4)} if entry == "lattice" else {}
    try:
        gate.run_synchronous(pkg, SG.Case(f"{entry}_mesh_extract-{algorithm}", call, {}, inputs=inputs, host=host))
    finally:
        got = [pkg.mesh_tensors(m) for m in meshes]
    assert len(got) == 4   # a warm-up and a gated call per poison kind
    for v, i in got:
        v, i = v.cpu().numpy(), i.cpu().numpy().astype(np.int64)
        assert v.shape == want_v.shape and i.shape == want_i.shape
        np.testing.assert_array_equal(i, want_i)
        np.testing.assert_array_equal(LM.bits(v), LM.bits(want_v))
