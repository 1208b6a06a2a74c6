"""What libsdfgrid answers to bad arguments: the status code and the exact sdfv_last_error() text of every argument check an
entry point runs before it asks for a device, and, where an entry point has several checks, which one a call that violates two of
them reports (the checks' order).  tests/golden/api_errors.json holds the answers of the library as recorded from it
(`python tests/test_api_errors_cpu.py --record`); the test replays every case and compares code and text exactly.  No case
reaches a device: buffers are addresses that are never read, only their NULL-ness and alignment count."""
import ctypes as C
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_errors.json")
A = 0x10000                      # a "buffer": 16-byte aligned; A + 4, A + 8 and A + 2 are the misaligned ones
ILV, VIRGIN = 8, 4               # SDFV_PASS_VOLUME_INTERLEAVED, SDFV_PASS_VIRGIN_GRID
NAN, INF = float("nan"), float("inf")
# the two calls whose recorded answer to NULL is 0, not a refusal (a size of nothing; destroying nothing)
ANSWERS_ZERO = ("comm_gather_bands_scratch_bytes/comm_null_is_0_bytes", "slab_comm_destroy/null_is_ok")


def build_cases(pkg):
    """[(name, thunk)]: thunk() makes the call and returns its status."""
    capi, lib = pkg._capi, pkg.lib
    cases = []

    def case(name, fn, *args):
        assert name not in [n for n, _ in cases], name
        cases.append((name, lambda: getattr(lib, fn)(*args)))

    def grid(dims=(4, 4, 4), z=None):
        g = capi.Grid()
        g.dims[:] = dims
        g.bb_min[:] = (-1.0, -1.0, -1.0)
        g.bb_max[:] = (1.0, 1.0, 1.0)
        g.z_begin, g.z_end = z if z else (0, dims[2])
        return C.byref(g)

    def params(**kw):
        p = capi.DemoParams()
        lib.sdfv_demo_params_default(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    def render_params(dims=(4, 4, 4), lights=(), n_lights=None, **kw):
        rp = capi.RenderParams()
        lib.sdfv_render_params_default(C.byref(rp), grid(dims))
        for i, kind in enumerate(lights):
            rp.lights[i].kind = kind
        rp.n_lights = len(lights) if n_lights is None else n_lights
        for k, v in kw.items():
            setattr(rp, k, v)
        return rp

    f3 = C.cast((C.c_float * 3)(-1.0, -1.0, -1.0), C.POINTER(C.c_float))
    box = C.cast((C.c_float * 6)(-1, -1, -1, 1, 1, 1), C.POINTER(C.c_float))
    P, G, ODD, BADG = params(), grid(), grid((4, 5, 4)), grid(z=(3, 9))
    BADSDF, BADMAT = 7, params(cube_material=9)
    cam = capi.Camera()
    CAM = C.pointer(cam)

    # ---- options and the small host-only calls
    case("set_option/unknown", "sdfv_set_option", 999, 0)
    case("set_option/range", "sdfv_set_option", capi.OPT_FILL_NONTEMPORAL, 3)
    case("set_option/range64", "sdfv_set_option", capi.OPT_PASS_INDEX_LIMIT, (1 << 32) + 1)
    case("set_option/waves1", "sdfv_set_option", capi.OPT_RAYMARCH_WAVES_PER_SIMD, 1)
    case("set_option/step_form", "sdfv_set_option", capi.OPT_SLAB_STEP_FORM, 1)
    for name, opt in (("wave_timing", capi.OPT_TUNING_WAVE_TIMING), ("priority_map", capi.OPT_TUNING_PRIORITY_MAP),
                      ("tile_order", capi.OPT_TUNING_TILE_ORDER)):
        case(f"set_option/tuning_{name}", "sdfv_set_option", opt, 0)
    case("get_option/null", "sdfv_get_option", capi.OPT_FILL_FORM, None)
    case("get_option/null+unknown", "sdfv_get_option", 999, None)
    case("get_option/unknown", "sdfv_get_option", 999, C.byref(C.c_uint64()))
    case("grid_from_bb/null", "sdfv_grid_from_bb", f3, None, 8, grid())
    case("grid_from_bb/null_out", "sdfv_grid_from_bb", f3, f3, 8, None)
    case("camera_look_at/null", "sdfv_camera_look_at", None, f3, f3, f3, 45.0, 1.0, 0.1, 10.0)

    # ---- grid init
    case("grid_init/grid_null", "sdfv_grid_init", None, A, A, None)
    case("grid_init/slab", "sdfv_grid_init", BADG, A, A, None)
    case("grid_init/slab_reversed", "sdfv_grid_init", grid(z=(3, 2)), A, A, None)
    case("grid_init/tex_null", "sdfv_grid_init", G, A, None, None)
    case("grid_init/tex0_by4", "sdfv_grid_init", G, A + 4, A, None)
    case("grid_init/tex1_by8", "sdfv_grid_init", G, A, A + 8, None)
    case("grid_init/slab+tex_null", "sdfv_grid_init", BADG, None, None, None)
    case("grid_init/tex_null+by4", "sdfv_grid_init", G, None, A + 4, None)
    fn = "sdfv_grid_init_unvisited_ex"
    case("init_unvisited/grid_null", fn, None, 2, A, A, A, 0, None)
    case("init_unvisited/flags", fn, G, 2, A, A, A, 0x10, None)
    case("init_unvisited/ilv_odd", fn, ODD, 2, A, A, A, ILV, None)
    case("init_unvisited/ilv_by4", fn, G, 2, A, A, A + 4, ILV, None)
    case("init_unvisited/ilv_no_volume_is_allowed", fn, ODD, 2, None, A, None, ILV, None)
    case("init_unvisited/tex_null", fn, G, 2, None, A, A, 0, None)
    case("init_unvisited/step3", fn, G, 3, A, A, A, 0, None)
    case("init_unvisited/tex_by4", fn, G, 2, A, A + 4, A, 0, None)
    case("init_unvisited/dist_by2", fn, G, 2, A, A, A + 2, 0, None)
    case("init_unvisited/slab+flags", fn, BADG, 2, A, A, A, 0x10, None)
    case("init_unvisited/flags+ilv_odd", fn, ODD, 2, A, A, A, ILV | 0x10, None)
    case("init_unvisited/ilv_odd+tex_null", fn, ODD, 2, None, A, A, ILV, None)
    case("init_unvisited/tex_null+step3", fn, G, 3, None, A, A, 0, None)
    case("init_unvisited/step3+tex_by4", fn, G, 3, A + 4, A, A, 0, None)
    case("init_unvisited/tex_by4+dist_by2", fn, G, 2, A + 4, A, A + 2, 0, None)
    case("init_unvisited_plain/step3", "sdfv_grid_init_unvisited", G, 3, A, A, A, None)

    # ---- fills
    fn = "sdfv_fill_grid_commit"
    case("fill_commit/params_null", fn, None, 0, G, A, A, A, None)
    case("fill_commit/sdf_id", fn, P, BADSDF, G, A, A, A, None)
    case("fill_commit/material", fn, BADMAT, 0, G, A, A, A, None)
    case("fill_commit/sphere_material", fn, params(sphere_material=2), 0, G, A, A, A, None)
    case("fill_commit/grid_null", fn, P, 0, None, A, A, A, None)
    case("fill_commit/slab", fn, P, 0, BADG, A, A, A, None)
    case("fill_commit/tex_null", fn, P, 0, G, None, A, A, None)
    case("fill_commit/tex_by8", fn, P, 0, G, A + 8, A, A, None)
    case("fill_commit/dist_by2", fn, P, 0, G, A, A, A + 2, None)
    case("fill_commit/params_null+grid_null", fn, None, BADSDF, None, A, A, A, None)
    case("fill_commit/sdf_id+material", fn, BADMAT, BADSDF, G, A, A, A, None)
    case("fill_commit/material+slab", fn, BADMAT, 0, BADG, A, A, A, None)
    case("fill_commit/slab+tex_null", fn, P, 0, BADG, None, A, A, None)
    case("fill_commit/tex_null+by4", fn, P, 0, G, None, A + 4, A, None)
    case("fill_commit/tex_by4+dist_by2", fn, P, 0, G, A + 4, A, A + 2, None)
    case("fill_grid/tex_null", "sdfv_fill_grid", P, 0, G, A, None, None)
    case("fill_grid/sdf_id", "sdfv_fill_grid", P, BADSDF, G, A, A, None)
    fn = "sdfv_fill_grid_pass_ex"
    case("pass/params_null", fn, None, 0, G, 2, None, A, A, A, 0, None)
    case("pass/sdf_id", fn, P, BADSDF, G, 2, None, A, A, A, 0, None)
    case("pass/material", fn, BADMAT, 1, G, 2, None, A, A, A, 0, None)
    case("pass/slab", fn, P, 0, BADG, 2, None, A, A, A, 0, None)
    case("pass/tex_null", fn, P, 0, G, 2, None, None, A, A, 0, None)
    case("pass/step0", fn, P, 0, G, 0, None, A, A, A, 0, None)
    case("pass/step3", fn, P, 0, G, 3, None, A, A, A, 0, None)
    case("pass/flags", fn, P, 0, G, 2, None, A, A, A, 0x100, None)
    case("pass/ilv_no_volume", fn, P, 0, G, 2, None, A, A, None, ILV, None)
    case("pass/ilv_odd", fn, P, 0, ODD, 2, None, A, A, A, ILV, None)
    case("pass/ilv_by4", fn, P, 0, G, 2, None, A, A, A + 4, ILV, None)
    case("pass/virgin_box", fn, P, 0, G, 2, box, A, A, A, VIRGIN, None)
    case("pass/tex_by4", fn, P, 0, G, 2, None, A, A + 4, A, 0, None)
    case("pass/dist_by2", fn, P, 0, G, 2, None, A, A, A + 2, 0, None)
    case("pass/material+slab", fn, BADMAT, 0, BADG, 2, None, A, A, A, 0, None)
    case("pass/slab+tex_null", fn, P, 0, BADG, 2, None, None, A, A, 0, None)
    case("pass/tex_null+step0", fn, P, 0, G, 0, None, None, A, A, 0, None)
    case("pass/step3+flags", fn, P, 0, G, 3, None, A, A, A, 0x100, None)
    case("pass/flags+ilv_no_volume", fn, P, 0, G, 2, None, A, A, None, 0x100 | ILV, None)
    case("pass/ilv_no_volume+odd", fn, P, 0, ODD, 2, None, A, A, None, ILV, None)
    case("pass/ilv_odd+virgin_box", fn, P, 0, ODD, 2, box, A, A, A, ILV | VIRGIN, None)
    case("pass/virgin_box+tex_by4", fn, P, 0, G, 2, box, A + 4, A, A, VIRGIN, None)
    case("pass/tex_by4+dist_by2", fn, P, 0, G, 2, None, A + 4, A, A + 2, 0, None)
    fn = "sdfv_pack_samples"
    case("pack/grid_null", fn, None, 0, A, A, 4, A, A, A, 0, None)
    case("pack/slab", fn, BADG, 0, A, A, 4, A, A, A, 0, None)
    case("pack/tex_null", fn, G, 0, A, A, 4, A, None, A, 0, None)
    case("pack/samples_null", fn, G, 0, A, None, 4, A, A, A, 0, None)
    case("pack/flags", fn, G, 0, A, A, 4, A, A, A, 1, None)
    case("pack/ilv_no_volume", fn, G, 0, A, A, 4, A, A, None, ILV, None)
    case("pack/ilv_odd", fn, ODD, 0, A, A, 4, A, A, A, ILV, None)
    case("pack/ilv_by4", fn, G, 0, A, A, 4, A, A, A + 4, ILV, None)
    case("pack/tex_by8", fn, G, 0, A, A, 4, A + 8, A, A, 0, None)
    case("pack/dist_by2", fn, G, 0, A, A, 4, A, A, A + 2, 0, None)
    case("pack/samples_by2", fn, G, 0, A, A + 2, 4, A, A, A, 0, None)
    case("pack/indices_by2", fn, G, 0, A + 2, A, 4, A, A, A, 0, None)
    case("pack/slab+tex_null", fn, BADG, 0, A, A, 4, None, A, A, 0, None)
    case("pack/tex_null+samples_null", fn, G, 0, A, None, 4, None, A, A, 0, None)
    case("pack/samples_null+flags", fn, G, 0, A, None, 4, A, A, A, 1, None)
    case("pack/flags+ilv_no_volume", fn, G, 0, A, A, 4, A, A, None, 1 | ILV, None)
    case("pack/ilv_odd+tex_by4", fn, ODD, 0, A, A, 4, A + 4, A, A, ILV, None)
    case("pack/tex_by4+indices_by2", fn, G, 0, A + 2, A, 4, A + 4, A, A, 0, None)

    # ---- points, normals, sources, mesh
    case("sample_points/params_null", "sdfv_sample_points", None, 0, A, 4, 0, A, None)
    case("sample_points/sdf_id", "sdfv_sample_points", P, BADSDF, A, 4, 0, A, None)
    case("sample_points/null_buffer", "sdfv_sample_points", P, 0, None, 4, 0, A, None)
    case("sample_points/sdf_id+null_buffer", "sdfv_sample_points", P, BADSDF, A, 4, 0, None, None)
    case("normal_points/material", "sdfv_normal_points", BADMAT, 0, A, 4, 0.0, 0, A, None)
    case("normal_points/null_buffer", "sdfv_normal_points", P, 0, A, 4, 0.0, 0, None, None)
    case("normal_points/material+null_buffer", "sdfv_normal_points", BADMAT, 0, None, 4, 0.0, 0, A, None)
    for kind in ("scalar", "normal"):
        fn = f"sdfv_source_sample_{kind}"
        case(f"source_{kind}/sdf_id", fn, P, BADSDF, f3, f3, A, 4, A, None)
        case(f"source_{kind}/bb_null", fn, P, 0, f3, None, A, 4, A, None)
        case(f"source_{kind}/null_buffer", fn, P, 0, f3, f3, None, 4, A, None)
        case(f"source_{kind}/sdf_id+bb_null", fn, P, BADSDF, None, f3, A, 4, A, None)
        case(f"source_{kind}/bb_null+null_buffer", fn, P, 0, None, f3, A, 4, None, None)
    case("mesh_postproc/params_null", "sdfv_mesh_postproc", None, 0, A, 3, None)
    case("mesh_postproc/null_buffer", "sdfv_mesh_postproc", P, 0, None, 3, None)
    case("mesh_postproc/by2", "sdfv_mesh_postproc", P, 0, A + 2, 3, None)
    case("mesh_postproc/sdf_id+null_buffer", "sdfv_mesh_postproc", P, BADSDF, None, 3, None)
    case("mesh_postproc/by2_with_n0", "sdfv_mesh_postproc", P, 0, A + 2, 0, None)
    mesh = C.byref(capi.Mesh())
    fn = "sdfv_mesh_extract"
    case("mesh_extract/out_null", fn, P, 0, f3, f3, 8, 0, None, None)
    case("mesh_extract/params_null", fn, None, 0, f3, f3, 8, 0, mesh, None)
    case("mesh_extract/bb_null", fn, P, 0, None, f3, 8, 0, mesh, None)
    case("mesh_extract/algorithm", fn, P, 0, f3, f3, 8, 1, mesh, None)
    case("mesh_extract/voxels0", fn, P, 0, f3, f3, 0, 0, mesh, None)
    case("mesh_extract/voxels1025", fn, P, 0, f3, f3, 1025, 4, mesh, None)
    case("mesh_extract/out_null+params_null", fn, None, 0, f3, f3, 8, 0, None, None)
    case("mesh_extract/sdf_id+bb_null", fn, P, BADSDF, None, None, 8, 0, mesh, None)
    case("mesh_extract/bb_null+algorithm", fn, P, 0, f3, None, 8, 3, mesh, None)
    case("mesh_extract/algorithm+voxels0", fn, P, 0, f3, f3, 0, 2, mesh, None)

    # ---- commits and the volume advice
    fn = "sdfv_commit_distance"
    case("commit_distance/slab", fn, BADG, A, A, None)
    case("commit_distance/null", fn, G, A, None, None)
    case("commit_distance/tex_by4", fn, G, A + 4, A, None)
    case("commit_distance/dist_by2", fn, G, A, A + 2, None)
    case("commit_distance/slab+null", fn, BADG, None, A, None)
    case("commit_distance/tex_by8+dist_by2", fn, G, A + 8, A + 2, None)
    for fn, name in (("sdfv_commit_pairs", "commit_pairs"), ("sdfv_commit_interleaved", "commit_interleaved")):
        case(f"{name}/grid_null", fn, None, A, A, None)
        case(f"{name}/null", fn, G, None, A, None)
        case(f"{name}/dist_by2", fn, G, A + 2, A, None)
        case(f"{name}/out_by4", fn, G, A, A + 4, None)
        case(f"{name}/part", fn, grid(z=(1, 4)), A, A, None)
        case(f"{name}/slab+null", fn, BADG, A, None, None)
        case(f"{name}/null+by4", fn, G, None, A + 4, None)
        case(f"{name}/by4+part", fn, grid(z=(0, 3)), A, A + 4, None)
    case("commit_interleaved/odd", "sdfv_commit_interleaved", ODD, A, A, None)
    case("commit_interleaved/part+odd", "sdfv_commit_interleaved", grid((4, 5, 4), z=(1, 4)), A, A, None)
    case("volume_advice/grid_null", "sdfv_march_volume_advice", None, C.byref(C.c_uint32()))
    case("volume_advice/kind_null", "sdfv_march_volume_advice", G, None)
    case("volume_advice/slab+kind_null", "sdfv_march_volume_advice", BADG, None)

    # ---- the grid march
    def march(name, rp="default", size=None, extra=None, **kw):
        class Wide(C.Structure):  # a caller built against a LATER header: the descriptor with eight bytes this library does not know
            _fields_ = [("d", capi.MarchDesc), ("beyond", C.c_uint8 * 8)]
        w = Wide()
        d = w.d
        d.size = C.sizeof(capi.MarchDesc) if size is None else size
        rp = render_params() if isinstance(rp, str) else rp
        d.rp = C.pointer(rp) if rp is not None else None
        d.tex0, d.tex1, d.rgba, d.cameras = A, A, A, CAM
        d.n_cameras, d.width, d.height, d.y0, d.y1 = 1, 8, 8, 0, 8
        for k, v in kw.items():
            setattr(d, k, v)
        if extra is not None:
            w.beyond[extra] = 1
        cases.append((f"raymarch_ex/{name}", lambda: lib.sdfv_raymarch_ex(C.cast(C.byref(w), C.POINTER(capi.MarchDesc)), None)))

    cases.append(("raymarch_ex/desc_null", lambda: lib.sdfv_raymarch_ex(None, None)))
    march("size_small", size=capi.MarchDesc.depth.offset - 4)
    march("size_beyond", size=C.sizeof(capi.MarchDesc) + 8, extra=5)
    march("reserved", reserved=1)
    march("band_height_without_step", band_height=8)
    march("band_height5", band_step=1, band_height=5)
    march("size_small+reserved", size=8, reserved=1)
    march("size_beyond+reserved", size=C.sizeof(capi.MarchDesc) + 8, extra=0, reserved=1)
    march("reserved+band_height5", reserved=1, band_step=1, band_height=5)
    march("band_height5+rp_null", rp=None, band_step=2, band_height=5)
    march("rp_null", rp=None)
    march("tex_null", tex1=None)
    march("no_colour", rgba=None)
    march("too_many_lights", rp=render_params(n_lights=5))
    march("directional", rp=render_params(lights=(capi.LIGHT_AMBIENT, capi.LIGHT_DIRECTIONAL)))
    march("light_kind", rp=render_params(lights=(7,)))
    march("tex_by4", tex0=A + 4)
    march("rgba_by8", rgba=A + 8)
    march("dist_by2", dist=A + 2)
    march("depth_by2", depth=A + 2)
    march("aux_by2", aux=A + 2)
    march("rgba8_by2", rgba=None, rgba8=A + 2)
    march("pairs_by4", pairs=A + 4)
    march("ilv_by4", ilv=A + 4)
    march("cameras_null", cameras=None)
    march("rows", y0=5, y1=4)
    march("rows_height", y1=9)
    march("empty_texture", rp=render_params((4, 0, 4)))
    march("lod", rp=render_params(lod_dist_between_samples=0.5))
    march("lod_nan", rp=render_params(lod_dist_between_samples=NAN))
    march("texture_too_large", rp=render_params((2048, 2048, 1024)))
    march("tex_null+no_colour", tex0=None, rgba=None)
    march("no_colour+lights", rgba=None, rp=render_params(n_lights=5))
    march("lights+tex_by4", tex0=A + 4, rp=render_params(lights=(capi.LIGHT_DIRECTIONAL,)))
    march("tex_by4+dist_by2", tex1=A + 4, dist=A + 2)
    march("dist_by2+pairs_by4", dist=A + 2, pairs=A + 4)
    march("pairs_by4+cameras_null", pairs=A + 4, cameras=None)
    march("cameras_null+rows", cameras=None, y1=9)
    march("rows+empty_texture", y1=9, rp=render_params((0, 4, 4)))
    march("empty_texture+lod", rp=render_params((0, 4, 4), lod_dist_between_samples=0.5))
    march("lod+texture_too_large", rp=render_params((2048, 2048, 1024), lod_dist_between_samples=0.5))
    march("bands/rows_follow_band_first", band_step=2, band_first=0, band_height=8, cameras=None)
    case("raymarch_host/null", "sdfv_raymarch_host", C.byref(render_params()), A, A, CAM, 1, 8, 8, None, None)
    case("raymarch_host/rp_null", "sdfv_raymarch_host", None, A, A, CAM, 1, 8, 8, A, None)

    # ---- the sharded march
    RP = C.byref(render_params())
    S = grid(z=(1, 3))

    def slab(name, rp=RP, g=S, lo=1, hi=1, tex0=A, tex1=A, camera=CAM, w=8, h=8, in_states=None, n_in=0, rgba=A, down=A, up=A, counters=A):
        case(f"raymarch_slab/{name}", "sdfv_raymarch_slab", rp, g, lo, hi, tex0, tex1, camera, w, h, in_states, n_in, rgba, None,
             down, up, 16, counters, None)

    slab("out_null", up=None)
    slab("counters_null", counters=None)
    slab("n_in_without_states", n_in=3)
    slab("null", camera=None)
    slab("rgba_null", rgba=None)
    slab("slab", g=BADG)
    slab("lights", rp=C.byref(render_params(n_lights=9)))
    slab("tex_by4", tex1=A + 4)
    slab("rgba_by8", rgba=A + 8)
    slab("dims", g=grid((4, 4, 8), z=(1, 3)))
    slab("empty", g=grid(z=(2, 2)), lo=0, hi=0)
    slab("ghost_below", g=grid(z=(0, 2)), lo=1)
    slab("ghost_above", g=grid(z=(2, 4)), hi=1)
    slab("ghost_lo2", g=grid(z=(2, 3)), lo=2)
    slab("ghost_hi3", g=grid((4, 4, 8), z=(1, 3)), rp=C.byref(render_params((4, 4, 8))), hi=3)
    slab("interior_without_ghost", hi=0)
    slab("lod", rp=C.byref(render_params(lod_dist_between_samples=2.0)))
    slab("image", w=65536, h=65536)
    slab("slab_too_large", rp=C.byref(render_params((65536, 65536, 4))), g=grid((65536, 65536, 4), z=(1, 3)))
    slab("out_null+n_in", down=None, n_in=3)
    slab("n_in+null", n_in=3, tex0=None)
    slab("null+slab", rgba=None, g=BADG)
    slab("slab+lights", g=BADG, rp=C.byref(render_params(n_lights=9)))
    slab("lights+tex_by4", rp=C.byref(render_params(lights=(capi.LIGHT_DIRECTIONAL,))), tex0=A + 8)
    slab("tex_by4+dims", tex0=A + 4, g=grid((4, 8, 4), z=(1, 3)))
    slab("dims+empty", g=grid((8, 4, 4), z=(2, 2)))
    slab("empty+ghost", g=grid(z=(4, 4)), hi=1)
    slab("ghost_above+hi3", g=grid(z=(2, 4)), hi=3)
    slab("lo2+interior", g=grid(z=(2, 3)), lo=2, hi=0)
    slab("interior+lod", hi=0, rp=C.byref(render_params(lod_dist_between_samples=2.0)))
    slab("lod+image", rp=C.byref(render_params(lod_dist_between_samples=2.0)), w=65536, h=65536)

    def slab_round(name, in_lo=None, in_hi=None, first=1, down=A, up=A, overflow=A, **kw):
        a = dict(rp=RP, g=S, lo=1, hi=1, tex0=A, tex1=A, camera=CAM, rgba=A)
        a.update(kw)
        case(f"slab_round/{name}", "sdfv_raymarch_slab_round", a["rp"], a["g"], a["lo"], a["hi"], a["tex0"], a["tex1"], a["camera"],
             8, 8, in_lo, in_hi, first, a["rgba"], None, down, up, 16, overflow, None)

    slab_round("buffer_null", down=None)
    slab_round("in_by2", in_lo=A + 2, first=0)
    slab_round("overflow_by2", overflow=A + 2)
    slab_round("first_round_with_rays", in_hi=A)
    slab_round("null", tex0=None)
    slab_round("interior_without_ghost", hi=0)
    slab_round("buffer_null+by2", up=None, down=A + 2)
    slab_round("by2+first_round", in_lo=A + 2)
    slab_round("first_round+null", in_lo=A, rgba=None)

    # ---- the *_host conveniences
    case("fill_grid_host/slab", "sdfv_fill_grid_host", P, 0, BADG, A, A)
    case("fill_grid_host/tex_null", "sdfv_fill_grid_host", P, 0, G, A, None)
    case("fill_grid_host/grid_null+tex_null", "sdfv_fill_grid_host", None, BADSDF, None, None, None)
    case("sample_points_host/null_buffer", "sdfv_sample_points_host", P, 0, None, 4, 0, A)
    case("sample_points_host/sdf_id", "sdfv_sample_points_host", P, BADSDF, A, 4, 0, A)
    case("sample_points_host/null_buffer+params_null", "sdfv_sample_points_host", None, 0, A, 4, 0, None)
    case("normal_points_host/null_buffer", "sdfv_normal_points_host", P, 0, A, 4, 0.0, 0, None)
    case("normal_points_host/material", "sdfv_normal_points_host", BADMAT, 0, A, 4, 0.0, 0, A)
    case("normal_points_host/null_buffer+sdf_id", "sdfv_normal_points_host", P, BADSDF, None, 4, 0.0, 0, A)
    case("mesh_postproc_host/null_buffer", "sdfv_mesh_postproc_host", P, 0, None, 3)
    case("mesh_postproc_host/params_null", "sdfv_mesh_postproc_host", None, 0, A, 3)
    case("mesh_postproc_host/null_buffer+sdf_id", "sdfv_mesh_postproc_host", P, BADSDF, None, 3)

    # ---- SDF programs: what sdfv_program_create rejects (the list of tests/test_program_cpu.py), then the entry points
    SPHERE, CUBE, BOX, PUSH_AFFINE, PUSH_SCALE, POP, POP_SCALE, UNION, SMOOTH_UNION, SMOOTH_SUBTRACT, ROUND, MATERIAL = (
        capi.OP_SPHERE, capi.OP_CUBE, capi.OP_BOX, capi.OP_PUSH_AFFINE, capi.OP_PUSH_SCALE, capi.OP_POP, capi.OP_POP_SCALE,
        capi.OP_UNION, capi.OP_SMOOTH_UNION, capi.OP_SMOOTH_SUBTRACT, capi.OP_ROUND, capi.OP_MATERIAL)
    Sp, Cb, U = (SPHERE, (0.5,)), (CUBE, (0.5,)), (UNION, ())
    ident = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    unit_box = (-1, -1, -1, 1, 1, 1)

    def ops_array(ops, reserved=None):
        arr = (capi.ProgOp * max(len(ops), 1))()
        for i, (op, operands) in enumerate(ops):
            arr[i].op = op
            for k, v in enumerate(operands):
                arr[i].a[k] = v
        if reserved is not None:
            arr[reserved[0]].reserved[reserved[1]] = 1
        return arr

    def create(name, ops, bb=unit_box, n=None, reserved=None, null=()):
        arr = ops_array(ops, reserved)
        out = C.c_void_p()
        case(f"program_create/{name}", "sdfv_program_create", None if "ops" in null else C.cast(arr, C.c_void_p),
             len(ops) if n is None else n, None if "bb" in null else (C.c_float * 6)(*bb), None if "out" in null else C.byref(out))

    create("out_null", [Sp], null=("out",))
    create("ops_null", [Sp], null=("ops",))
    create("bb_null", [Sp], null=("bb",))
    create("n0", [Sp], n=0)
    create("n257", [Sp] + [(MATERIAL, (1, 1, 1))] * 256)
    create("bb_flat", [Sp], bb=(-1, -1, -1, 1, -1, 1))
    create("bb_reversed", [Sp], bb=(-1, -1, -1, 1, 1, -2))
    create("bb_nan", [Sp], bb=(-1, NAN, -1, 1, 1, 1))
    create("bb_inf", [Sp], bb=(-1, -1, -1, INF, 1, 1))
    create("opcode19", [Sp, (19, ()), U])
    create("opcode0", [(0, ())])
    create("opcode_max", [Sp, Cb, (0xffffffff, ())])
    create("reserved", [Sp, Cb, U], reserved=(1, 2))
    create("operand_inf", [Sp, (BOX, (0.1, INF, 0.1)), U])
    create("operand_nan", [(SPHERE, (NAN,))])
    create("operand_last", [(SPHERE, (0.5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -INF))])
    create("smooth_union_k0", [Sp, Cb, (SMOOTH_UNION, (0.0,))])
    create("smooth_subtract_k", [Sp, Cb, (SMOOTH_SUBTRACT, (-0.125,))])
    create("push_scale_s0", [(PUSH_SCALE, (0.0, 1.0)), Sp, (POP_SCALE, (1.0,))])
    create("push_scale_inv", [(PUSH_SCALE, (2.0, -0.5)), Sp, (POP_SCALE, (2.0,))])
    create("pop_scale_s", [(PUSH_SCALE, (2.0, 0.5)), Sp, (POP_SCALE, (-2.0,))])
    create("frame_overflow", [(PUSH_AFFINE, ident)] * 5 + [Sp] + [(POP, ())] * 5)
    create("frame_underflow", [Sp, (POP, ())])
    create("closes_push_scale", [(PUSH_SCALE, (2.0, 0.5)), Sp, (POP, ())])
    create("closes_push_affine", [(PUSH_AFFINE, ident), Sp, (POP_SCALE, (2.0,))])
    create("value_underflow", [Sp, U])
    create("value_underflow_round", [(ROUND, (0.125,))])
    create("value_underflow_pop_scale", [(PUSH_SCALE, (2.0, 0.5)), (POP_SCALE, (2.0,)), Sp])
    create("value_overflow", [Sp] * 9 + [U] * 8)
    create("open_frame", [(PUSH_AFFINE, ident), Sp])
    create("two_values", [Sp, Cb])
    create("no_value", [(MATERIAL, (1, 1, 1))])
    create("out_null+ops_null", [Sp], null=("out", "ops"))
    create("ops_null+n0", [Sp], n=0, null=("ops",))
    create("n0+bb", [Sp], n=0, bb=(1, 1, 1, 0, 0, 0))
    create("bb+opcode", [(0, ())], bb=(-1, -1, 3, 1, 1, 2))
    create("opcode+reserved", [(99, ())], reserved=(0, 0))
    create("reserved+operand", [(SPHERE, (NAN,))], reserved=(0, 1))
    create("operand+k", [Sp, Cb, (SMOOTH_UNION, (0.0, NAN))])
    create("pop_scale_s+frame_underflow", [Sp, (POP_SCALE, (0.0,))])
    create("push_scale_s+frame_overflow", [(PUSH_AFFINE, ident)] * 4 + [(PUSH_SCALE, (0.0, 1.0))])
    create("k+value_underflow", [Sp, (SMOOTH_UNION, (0.0,))])

    one = ops_array([Sp])
    handle = C.c_void_p()
    assert lib.sdfv_program_create(C.cast(one, C.c_void_p), 1, (C.c_float * 6)(*unit_box), C.byref(handle)) == 0
    H = handle.value                                     # (lives as long as the process: one 64-byte program)
    case("program_ops/null", "sdfv_program_ops", None, None, None, None)
    for fn, extra in (("sdfv_program_sample_points", (0,)), ("sdfv_program_normal_points", (0.0,))):
        name = fn[len("sdfv_"):]
        case(f"{name}/program_null", fn, None, A, 4, *extra, A, None)
        case(f"{name}/null_buffer", fn, H, None, 4, *extra, A, None)
        case(f"{name}/points_by2", fn, H, A + 2, 4, *extra, A, None)
        case(f"{name}/out_by2", fn, H, A, 4, *extra, A + 2, None)
        case(f"{name}/program_null+null_buffer", fn, None, A, 4, *extra, None, None)
        case(f"{name}/null_buffer+by2", fn, H, None, 4, *extra, A + 2, None)
    case("program_sample_points_host/program_null", "sdfv_program_sample_points_host", None, A, 4, 0, A)
    case("program_sample_points_host/null_buffer", "sdfv_program_sample_points_host", H, A, 4, 0, None)
    case("program_sample_points_host/program_null+null_buffer", "sdfv_program_sample_points_host", None, None, 4, 0, A)
    fn = "sdfv_program_mesh_extract"
    case("program_mesh_extract/out_null", fn, H, None, None, 8, 0, 0, None, None)
    case("program_mesh_extract/program_null", fn, None, None, None, 8, 0, 0, mesh, None)
    case("program_mesh_extract/half_a_box", fn, H, f3, None, 8, 0, 0, mesh, None)
    case("program_mesh_extract/algorithm", fn, H, None, None, 8, 2, 0, mesh, None)
    case("program_mesh_extract/voxels0", fn, H, None, None, 0, 4, 0, mesh, None)
    case("program_mesh_extract/voxels1025", fn, H, f3, f3, 1025, 0, 0, mesh, None)
    case("program_mesh_extract/flags", fn, H, None, None, 8, 0, 2, mesh, None)
    case("program_mesh_extract/out_null+program_null", fn, None, None, None, 8, 0, 0, None, None)
    case("program_mesh_extract/program_null+half_a_box", fn, None, None, f3, 8, 0, 0, mesh, None)
    case("program_mesh_extract/half_a_box+algorithm", fn, H, None, f3, 8, 1, 0, mesh, None)
    case("program_mesh_extract/algorithm+voxels0", fn, H, None, None, 0, 1, 0, mesh, None)
    case("program_mesh_extract/voxels0+flags", fn, H, None, None, 0, 0, 2, mesh, None)
    for fn, tail in (("sdfv_program_mesh_postproc", (None,)), ("sdfv_program_mesh_postproc_host", ())):
        name = fn[len("sdfv_"):]
        case(f"{name}/program_null", fn, None, A, 3, *tail)
        case(f"{name}/null_buffer", fn, H, None, 3, *tail)
        case(f"{name}/program_null+null_buffer", fn, None, None, 3, *tail)
    case("program_mesh_postproc/by2", "sdfv_program_mesh_postproc", H, A + 2, 3, None)
    fn = "sdfv_program_fill_grid_commit"
    case("program_fill/program_null", fn, None, G, A, A, A, 0, None)
    case("program_fill/slab", fn, H, BADG, A, A, A, 0, None)
    case("program_fill/tex_null", fn, H, G, None, A, A, 0, None)
    case("program_fill/flags", fn, H, G, A, A, A, 4, None)
    case("program_fill/ilv_no_volume", fn, H, G, A, A, None, ILV, None)
    case("program_fill/ilv_odd", fn, H, ODD, A, A, A, ILV, None)
    case("program_fill/ilv_by4", fn, H, G, A, A, A + 4, ILV, None)
    case("program_fill/tex_by4", fn, H, G, A, A + 4, None, 0, None)
    case("program_fill/dist_by2", fn, H, G, A, A, A + 2, 0, None)
    case("program_fill/program_null+grid_null", fn, None, None, A, A, A, 0, None)
    case("program_fill/slab+tex_null", fn, H, BADG, A, None, A, 0, None)
    case("program_fill/tex_null+flags", fn, H, G, None, A, A, 4, None)
    case("program_fill/flags+ilv_no_volume", fn, H, G, A, A, None, 4 | ILV, None)
    case("program_fill/ilv_odd+tex_by4", fn, H, ODD, A + 4, A, A, ILV, None)
    case("program_fill/tex_by4+dist_by2", fn, H, G, A + 4, A, A + 2, 0, None)

    def program_march(name, rp="default", size=None, extra=None, fn="sdfv_program_raymarch_check", **kw):
        class Wide(C.Structure):
            _fields_ = [("d", capi.ProgramMarchDesc), ("beyond", C.c_uint8 * 8)]
        w = Wide()
        d = w.d
        d.size = C.sizeof(capi.ProgramMarchDesc) if size is None else size
        rp = render_params() if isinstance(rp, str) else rp
        d.rp = C.pointer(rp) if rp is not None else None
        d.program, d.rgba, d.cameras = H, A, CAM
        d.n_cameras, d.width, d.height, d.y0, d.y1 = 1, 8, 8, 0, 8
        for k, v in kw.items():
            setattr(d, k, v)
        if extra is not None:
            w.beyond[extra] = 1
        tail = (None, None) if fn.endswith("_check") else (None,)
        cases.append((f"{fn[len('sdfv_'):]}/{name}",
                      lambda: getattr(lib, fn)(C.cast(C.byref(w), C.POINTER(capi.ProgramMarchDesc)), *tail)))

    cases.append(("program_raymarch_check/desc_null", lambda: lib.sdfv_program_raymarch_check(None, None, None)))
    program_march("size_small", size=capi.ProgramMarchDesc.rgba8.offset + 4)
    program_march("size_beyond", size=C.sizeof(capi.ProgramMarchDesc) + 8, extra=7)
    program_march("reserved", reserved=2)
    program_march("program_null", program=None)
    program_march("rp_null", rp=None)
    program_march("no_colour", rgba=None)
    program_march("too_many_lights", rp=render_params(n_lights=5))
    program_march("directional", rp=render_params(lights=(capi.LIGHT_DIRECTIONAL,)))
    program_march("rgba_by4", rgba=A + 4)
    program_march("depth_by2", depth=A + 2)
    program_march("aux_by2", aux=A + 2)
    program_march("rgba8_by2", rgba8=A + 2)
    program_march("cameras_null", cameras=None)
    program_march("rows", y0=3, y1=2)
    program_march("normal_h_negative", normal_h=-1.0)
    program_march("normal_h_nan", normal_h=NAN)
    program_march("no_tap_distance", rp=render_params((0, 0, 0)))
    program_march("size_small+reserved", size=16, reserved=2)
    program_march("reserved+program_null", reserved=2, program=None)
    program_march("program_null+rp_null", program=None, rp=None)
    program_march("rp_null+no_colour", rp=None, rgba=None)
    program_march("no_colour+lights", rgba=None, rp=render_params(n_lights=5))
    program_march("lights+rgba_by4", rgba=A + 4, rp=render_params(lights=(3,)))
    program_march("rgba_by4+aux_by2", rgba=A + 8, aux=A + 2)
    program_march("aux_by2+cameras_null", aux=A + 2, cameras=None)
    program_march("cameras_null+rows", cameras=None, y1=9)
    program_march("rows+normal_h", y1=9, normal_h=-1.0)
    program_march("normal_h+no_tap_distance", normal_h=INF, rp=render_params((0, 0, 0)))
    program_march("reserved", fn="sdfv_program_raymarch", reserved=2)
    program_march("rows", fn="sdfv_program_raymarch", y1=9)

    # ---- the slab communicator: what it checks before it asks for a device or for RCCL (tests/test_gpu_comm_errors.py holds
    # the checks that need a live communicator)
    fn = "sdfv_bands_scatter"
    case("bands_scatter/part_null", fn, None, 0, 1, 16, 1, 8, 8, 4, A, None)
    case("bands_scatter/out_null", fn, A, 0, 1, 16, 1, 8, 8, 4, None, None)
    case("bands_scatter/band_step0", fn, A, 0, 0, 16, 1, 8, 8, 4, A, None)
    case("bands_scatter/channels0", fn, A, 0, 1, 16, 1, 8, 8, 0, A, None)
    case("bands_scatter/part_by2", fn, A + 2, 0, 1, 16, 1, 8, 8, 4, A, None)
    case("bands_scatter/null+channels0", fn, None, 0, 1, 16, 1, 8, 8, 0, A, None)
    case("bands_scatter/band_step0+by2", fn, A, 0, 0, 16, 1, 8, 8, 4, A + 2, None)
    dims3, bounds = (C.c_uint32 * 3)(4, 4, 4), (C.c_uint32 * 2)(0, 4)
    case("comm_gather_bands/comm_null", "sdfv_comm_gather_bands", None, A, 16, 1, 8, 8, 4, 0, A, A, 1024, None)
    case(ANSWERS_ZERO[0], "sdfv_comm_gather_bands_scratch_bytes", None, 0, 16, 1, 8, 8, 4)
    case("comm_gather_cameras/comm_null", "sdfv_comm_gather_cameras", None, A, 1, 8, 8, 4, 0, A, None)
    fn = "sdfv_comm_allgather_slabs"
    case("comm_allgather_slabs/comm_null", fn, None, dims3, bounds, A, A, None, A, A, None, None)
    case("comm_allgather_slabs/comm_null+dims_null", fn, None, None, bounds, A, A, None, A, A, None, None)
    case("comm_allgather_slabs/comm_null+z_bounds_null", fn, None, dims3, None, A, A, None, A, A, None, None)
    case("slab_comm_info/comm_null", "sdfv_slab_comm_info", None, None, None, None)
    case("slab_comm_ranks/comm_null", "sdfv_slab_comm_ranks", None, None, None)
    case("slab_halo_exchange/comm_null", "sdfv_slab_halo_exchange", None, G, A, A, None)
    case("slab_fill_step/comm_null", "sdfv_slab_fill_step", None, P, 0, G, A, A, None)
    case("slab_fill_step_commit/comm_null", "sdfv_slab_fill_step_commit", None, P, 0, G, A, A, A, None)
    case("slab_comm_join/comm_null", "sdfv_slab_comm_join", None, None)

    def slab_march(name, scratch=A, status=A):
        case(f"slab_march/{name}", "sdfv_slab_march", None, RP, S, A, A, CAM, 8, 8, A, None, scratch, 1 << 20, 16, 0, status, None)

    slab_march("comm_null")
    slab_march("comm_null+scratch_null", scratch=None)
    slab_march("comm_null+status_null", status=None)
    case("slab_comm_unique_id/null", "sdfv_slab_comm_unique_id", None)
    ident, handle = (C.c_ubyte * capi.COMM_ID_BYTES)(), C.c_void_p()
    fn = "sdfv_slab_comm_create"
    case("slab_comm_create/id_null", fn, None, 0, 1, 0, C.byref(handle))
    case("slab_comm_create/out_null", fn, ident, 0, 1, 0, None)
    case("slab_comm_create/world0", fn, ident, 0, 0, 0, C.byref(handle))
    case("slab_comm_create/rank_negative", fn, ident, -1, 2, 0, C.byref(handle))
    case("slab_comm_create/rank_is_world", fn, ident, 2, 2, 0, C.byref(handle))
    case("slab_comm_create/flags", fn, ident, 0, 1, 0x80, C.byref(handle))
    case("slab_comm_create/rank+flags", fn, ident, 3, 2, 0x80, C.byref(handle))
    case(ANSWERS_ZERO[1], "sdfv_slab_comm_destroy", None)
    return cases


def run_cases(pkg):
    got = {}
    for name, thunk in build_cases(pkg):
        code = thunk()
        assert name not in got, name
        got[name] = {"code": code, "error": pkg.lib.sdfv_last_error().decode() if code else ""}  # (0 leaves the last message be)
    return got


def test_every_argument_check_answers_with_the_recorded_code_and_text(pkg):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = run_cases(pkg)
    assert sorted(got) == sorted(want)
    # every row is a refusal that needed no device (-4: SDFV_ERR_NO_DEVICE), but for the two that answer 0 by contract
    assert all(v["code"] not in (0, -4) for k, v in want.items() if k not in ANSWERS_ZERO)
    assert all(want[k] == {"code": 0, "error": ""} for k in ANSWERS_ZERO)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import importlib
    with open(GOLDEN, "w") as f:
        json.dump(run_cases(importlib.import_module("sdf-viewer_amd")), f, indent=0, sort_keys=True)
        f.write("\n")
