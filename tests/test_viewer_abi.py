"""CPU tests of the viewer's C ABI (include/sdfviewer.h, exported by libsdfviewer_host.so): the header is plain C, every
function it declares is exported and bound by sdf-viewer_amd/viewer.py and shown in INTEGRATION.md, and the calls refuse
bad arguments -- and, without a GPU, every compute call -- with a status instead of crashing."""
import ctypes as C
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sdfviewer.h")
HOST_LIB = os.path.join(ROOT, "sdf-viewer_amd", "libsdfviewer_host.so")


def viewer_module():
    return importlib.import_module("sdf-viewer_amd.viewer")


def declared_functions():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^[a-z][a-z0-9_ \*]*?\b(sdfv_[a-z0-9_]+)\s*\(", hdr, flags=re.M))


def test_header_is_pedantic_c99(tmp_path):
    src = tmp_path / "use_header.c"
    src.write_text('#include "sdfviewer.h"\n'
                   'static int touch(const sdfv_surface *s) { return s->device_sdf_id == 0; }\n'
                   'int main(void) { sdfv_surface s = {0}; sdfv_load_state st; (void)st; return touch(&s) - 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_and_binding_covers_every_declared_function():
    declared = declared_functions()
    assert len(declared) == 22, sorted(declared)
    syms = subprocess.run(["nm", "-D", "--defined-only", HOST_LIB], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (sdfv_[a-z0-9_]+)", syms))
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(viewer_module().PROTOTYPES), sorted(declared ^ set(viewer_module().PROTOTYPES))
    # the test-only library keeps its own surface: none of these is exported there
    test_syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "sdf-viewer_amd", "libsdfviewer_host_test.so")],
                               capture_output=True, text=True).stdout
    assert not re.search(r" T sdfv_(viewer|scene)_", test_syms)


def test_integration_guide_names_every_viewer_function():
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    missing = sorted(f for f in declared_functions() if f not in guide)
    assert not missing, missing
    assert "## Bind the viewer" in guide or "### Bind the viewer" in guide


def test_abi_version():
    v = viewer_module()
    want = int(re.search(r"#define SDFV_VIEWER_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    assert v.lib.sdfv_viewer_abi_version() == want == 1


def test_calls_refuse_bad_arguments_and_missing_devices_cleanly(pkg):
    v = viewer_module()
    L = v.lib
    INVALID, NO_DEVICE = -1, -4
    bb = v._f6((-1, -1, -1, 1, 1, 1))
    out = C.c_void_p()
    assert L.sdfv_viewer_from_bb(None, 8, 2, C.byref(out)) == INVALID and not out.value
    assert L.sdfv_viewer_new_voxels((C.c_uint32 * 3)(4, 4, 4), bb, 2, 7, C.byref(out)) == INVALID
    assert L.sdfv_viewer_update(None, None, 0, None) == INVALID
    assert L.sdfv_viewer_commit(None) == INVALID and L.sdfv_viewer_state(None, None) == INVALID
    assert L.sdfv_viewer_download(None, None, None) == INVALID and L.sdfv_viewer_render(None, None, 4, 4, None) == INVALID
    assert L.sdfv_viewer_set_stream(None, None) == INVALID and L.sdfv_viewer_set_ingest(None, 1, 0) == INVALID
    assert L.sdfv_viewer_textures(None, None, None, None) == INVALID
    assert L.sdfv_viewer_last_error(None) == b"viewer is NULL" and L.sdfv_scene_last_error(None) == b"scene is NULL"
    L.sdfv_viewer_free(None)
    L.sdfv_scene_free(None)
    empty = v.SurfaceStruct()  # no bounding_box: refused before anything else
    sc = C.c_void_p()
    assert L.sdfv_scene_new(C.byref(empty), v.CLOCK_FN(), None, C.byref(sc)) == INVALID and not sc.value
    assert L.sdfv_scene_render(None, 4, 4, None, None) == INVALID and L.sdfv_scene_set_budget(None, 30, 500) == INVALID
    assert L.sdfv_scene_viewer(None) is None
    loading = C.c_int()
    assert L.sdfv_scene_load_progress(None, C.byref(loading), None, None, 0) == INVALID
    # the emitter's argument checks (libsdfgrid): before any device work
    g = pkg.make_grid((8, 8, 8))
    emit = pkg.lib.sdfv_emit_update_points
    assert emit(C.byref(g), 3, 0, 1, None, 16, 0, 16, 16, 16, 16, 1 << 20, None) == INVALID  # step not a power of two
    assert b"power of two" in pkg.lib.sdfv_last_error()
    assert emit(C.byref(g), 2, 60, 5, None, 16, 0, 16, 16, 16, 16, 1 << 20, None) == INVALID  # beyond the pass's 64 points
    assert emit(C.byref(g), 1, 0, 8, None, 16, 32, 16, 16, 16, 16, 1 << 20, None) == INVALID  # unknown flag
    big = pkg.make_grid((65536, 65536, 1))  # 2^32 voxels: a whole step-1 pass is one point too many for a run
    assert emit(C.byref(big), 1, 0, 1 << 32, None, 16, 0, 16, 16, 16, 16, 1 << 20, None) == INVALID
    assert b"at most 2^32 - 1" in pkg.lib.sdfv_last_error()
    odd = pkg.make_grid((8, 7, 8))
    assert emit(C.byref(odd), 1, 0, 8, None, 16, pkg._capi.PASS_VOLUME_INTERLEAVED, 16, 16, 16, 16, 1 << 20, None) == INVALID
    if pkg.lib.sdfv_device_count() > 0:  # (rocPRIM sizes its scratch for the device it finds)
        assert pkg.lib.sdfv_emit_update_points_scratch_bytes(1 << 20) > 0
        assert emit(C.byref(g), 1, 0, 8, None, 16, 0, 16, 16, 16, 16, 0, None) == INVALID  # no scratch
        assert b"sdfv_emit_update_points_scratch_bytes" in pkg.lib.sdfv_last_error()
    else:
        # no GPU: every compute call says so instead of crashing (no CPU path)
        assert L.sdfv_viewer_from_bb(bb, 8, 2, C.byref(out)) == NO_DEVICE and not out.value
        assert L.sdfv_viewer_new_voxels((C.c_uint32 * 3)(4, 4, 4), bb, 2, 0, C.byref(out)) == NO_DEVICE
        s = v.Surface.from_callbacks(lambda: (-1, -1, -1, 1, 1, 1), sample=lambda p, d: (0.0,) * 7)
        assert L.sdfv_scene_new(C.byref(s.struct), v.CLOCK_FN(), None, C.byref(sc)) == NO_DEVICE and not sc.value
        assert emit(C.byref(g), 1, 0, 8, None, 16, 0, 16, 16, 16, 16, 1 << 20, None) == NO_DEVICE
