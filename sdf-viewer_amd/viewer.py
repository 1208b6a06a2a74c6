"""ctypes binding of include/sdfviewer.h (libsdfviewer_host.so): the viewer and the scene over any SDF given as callbacks.

    surface = Surface.from_callbacks(bounding_box=lambda: (-1, -1, -1, 1, 1, 1), sample=my_sample)
    v = Viewer.new_voxels((64, 64, 64), surface.bounding_box(), loading_passes=3)
    v.update(surface, budget_s=0.03)

Surface.from_torch(bounding_box, fn) builds the device route: fn maps an [n, 3] float32 tensor of positions on the GPU to an
[n, 7] float32 tensor of SDFSample records (distance, r, g, b, metallic, roughness, occlusion), run on the viewer's stream.
"""
import ctypes as C
import os

from . import _capi
from ._capi import DemoParams, Grid, Sample, SdfvError

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsdfviewer_host.so")

ERR_CALLBACK, ERR_INTERNAL = -6, -7
LAYOUT_AUTO, LAYOUT_PLAIN, LAYOUT_INTERLEAVED = 0, 1, 2

FP = C.POINTER(C.c_float)
BBOX_FN = C.CFUNCTYPE(None, C.c_void_p, FP)
SAMPLE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, FP, C.c_int, C.POINTER(Sample))
SAMPLE_BATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, FP, C.c_size_t, C.c_int, C.POINTER(Sample))
CONCURRENCY_FN = C.CFUNCTYPE(C.c_uint32, C.c_void_p)
CHANGED_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, FP)
DEVICE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p)
CLOCK_FN = C.CFUNCTYPE(C.c_uint64, C.c_void_p)


class SurfaceStruct(C.Structure):
    _fields_ = [("user", C.c_void_p), ("bounding_box", BBOX_FN), ("sample", SAMPLE_FN), ("sample_batch", SAMPLE_BATCH_FN),
                ("sample_concurrency", CONCURRENCY_FN), ("changed", CHANGED_FN), ("sample_batch_device", DEVICE_FN),
                ("device_params", C.POINTER(DemoParams)), ("device_sdf_id", C.c_uint32)]


class View(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("target", C.c_float * 3), ("up", C.c_float * 3), ("fovy_degrees", C.c_float),
                ("z_near", C.c_float), ("z_far", C.c_float)]


class LoadState(C.Structure):
    _fields_ = [("remaining", C.c_uint64), ("total_iterations", C.c_uint64), ("passes_left", C.c_uint32),
                ("has_changed_box", C.c_uint32), ("lod_dist_between_samples", C.c_float), ("dims", C.c_uint32 * 3)]


class RenderReport(C.Structure):
    _fields_ = [("cpu_updates", C.c_uint64), ("committed", C.c_uint32), ("last_chunk", C.c_uint32),
                ("request_repaint", C.c_uint32)]


VP, SP = C.c_void_p, C.c_void_p  # sdfv_viewer *, sdfv_scene *
PROTOTYPES = {
    "sdfv_viewer_abi_version": (C.c_uint32, []),
    "sdfv_viewer_from_bb": (C.c_int, [FP, C.c_uint32, C.c_uint32, C.POINTER(VP)]),
    "sdfv_viewer_new_voxels": (C.c_int, [C.POINTER(C.c_uint32), FP, C.c_uint32, C.c_int, C.POINTER(VP)]),
    "sdfv_viewer_update": (C.c_int, [VP, C.POINTER(SurfaceStruct), C.c_uint64, C.POINTER(C.c_size_t)]),
    "sdfv_viewer_commit": (C.c_int, [VP]),
    "sdfv_viewer_state": (C.c_int, [VP, C.POINTER(LoadState)]),
    "sdfv_viewer_textures": (C.c_int, [VP, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(Grid)]),
    "sdfv_viewer_download": (C.c_int, [VP, C.c_void_p, C.c_void_p]),
    "sdfv_viewer_render": (C.c_int, [VP, C.POINTER(View), C.c_uint32, C.c_uint32, C.c_void_p]),
    "sdfv_viewer_set_stream": (C.c_int, [VP, C.c_void_p]),
    "sdfv_viewer_set_ingest": (C.c_int, [VP, C.c_uint32, C.c_size_t]),
    "sdfv_viewer_last_error": (C.c_char_p, [VP]),
    "sdfv_viewer_free": (None, [VP]),
    "sdfv_scene_new": (C.c_int, [C.POINTER(SurfaceStruct), CLOCK_FN, C.c_void_p, C.POINTER(SP)]),
    "sdfv_scene_set_surface": (C.c_int, [SP, C.POINTER(SurfaceStruct), C.c_uint32, C.c_uint32]),
    "sdfv_scene_set_camera": (C.c_int, [SP, C.POINTER(View)]),
    "sdfv_scene_set_budget": (C.c_int, [SP, C.c_uint32, C.c_uint32]),
    "sdfv_scene_render": (C.c_int, [SP, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RenderReport)]),
    "sdfv_scene_load_progress": (C.c_int, [SP, C.POINTER(C.c_int), FP, C.c_char_p, C.c_size_t]),
    "sdfv_scene_viewer": (VP, [SP]),
    "sdfv_scene_last_error": (C.c_char_p, [SP]),
    "sdfv_scene_free": (None, [SP]),
}


def load(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build it with `make -C sdf-viewer_amd/host`")
    lib = C.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    return lib


lib = load()
# include/sdfviewer_mesh.h: the viewer's mesh call, beside sdfviewer.h's (PROTOTYPES is that header's list)
lib.sdfv_viewer_mesh.restype = C.c_int
lib.sdfv_viewer_mesh.argtypes = [VP, C.c_uint32, C.c_uint32, C.POINTER(_capi.Mesh)]


def _check(rc, message):
    if rc != 0:
        raise SdfvError(rc, message.decode() if isinstance(message, bytes) else str(message))


def _f6(v):
    return (C.c_float * 6)(*[float(x) for x in v])


class Surface:
    """An sdfv_surface: `impl SDFSurface` as callbacks.  Keeps the ctypes thunks alive as long as it lives."""

    def __init__(self):
        self.struct = SurfaceStruct()
        self._keep = []
        self._bb = None

    @classmethod
    def from_callbacks(cls, bounding_box, sample=None, sample_batch=None, sample_concurrency=None, changed=None,
                       sample_batch_device=None, device_params=None, device_sdf_id=0):
        """bounding_box() -> 6 floats.  sample(p, distance_only) -> 7 floats (or raises).  sample_batch(points [n, 3] numpy,
        distance_only) -> [n, 7].  changed() -> 6 floats or None.  sample_batch_device(points_ptr, n, out_ptr, stream_ptr)
        -> None (raises on failure): the raw device addresses.  device_params: a DemoParams (the surface is then the demo)."""
        import numpy as np
        s = cls()
        s._bb = tuple(float(x) for x in bounding_box())

        def bb(_user, out):
            for i in range(6):
                out[i] = s._bb[i]
        s._set("bounding_box", BBOX_FN(bb))
        if sample is not None:
            def one(_user, p, distance_only, out):
                try:
                    r = sample((p[0], p[1], p[2]), bool(distance_only))
                except Exception:
                    return 1
                C.memmove(out, (C.c_float * 7)(*[float(x) for x in r]), 28)
                return 0
            s._set("sample", SAMPLE_FN(one))
        if sample_batch is not None:
            def batch(_user, p, n, distance_only, out):
                try:
                    pts = np.ctypeslib.as_array(p, shape=(n, 3)).copy()
                    r = np.ascontiguousarray(sample_batch(pts, bool(distance_only)), dtype=np.float32).reshape(n, 7)
                except Exception:
                    return 1
                C.memmove(out, r.ctypes.data, n * 28)
                return 0
            s._set("sample_batch", SAMPLE_BATCH_FN(batch))
        if sample_concurrency is not None:
            s._set("sample_concurrency", CONCURRENCY_FN(lambda _user: int(sample_concurrency)))
        if changed is not None:
            def ch(_user, out):
                b = changed()
                if b is None:
                    return 0
                for i in range(6):
                    out[i] = float(b[i])
                return 1
            s._set("changed", CHANGED_FN(ch))
        if sample_batch_device is not None:
            def dev(_user, points, n, out, stream):
                try:
                    sample_batch_device(points or 0, n, out or 0, stream or 0)
                except Exception:
                    return 1
                return 0
            s._set("sample_batch_device", DEVICE_FN(dev))
        if device_params is not None:
            s._params = device_params
            s.struct.device_params = C.pointer(device_params)
            s.struct.device_sdf_id = int(device_sdf_id)
        return s

    @classmethod
    def from_torch(cls, bounding_box, fn, **kw):
        """The device route from a Python function over device tensors: fn(points [n, 3] float32 on the GPU) -> [n, 7]
        float32 records, evaluated on the viewer's stream (torch.cuda.ExternalStream), no copy to the host."""
        import torch
        from . import _DeviceArray

        def device_sampler(points_ptr, n, out_ptr, stream_ptr):
            dev = torch.device("cuda", torch.cuda.current_device())
            ext = torch.cuda.ExternalStream(stream_ptr, device=dev) if stream_ptr else torch.cuda.default_stream(dev)
            with torch.cuda.stream(ext):
                pts = torch.as_tensor(_DeviceArray(points_ptr, (n, 3), "<f4"), device=dev)
                out = torch.as_tensor(_DeviceArray(out_ptr, (n, 7), "<f4"), device=dev)
                out.copy_(fn(pts))
        return cls.from_callbacks(bounding_box, sample_batch_device=device_sampler, **kw)

    def _set(self, name, thunk):
        self._keep.append(thunk)
        setattr(self.struct, name, thunk)

    def bounding_box(self):
        return self._bb


class Viewer:
    """SDFViewer through sdfv_viewer_*."""

    def __init__(self, handle, owned=True):
        self.h = handle
        self.owned = owned

    @classmethod
    def from_bb(cls, bb, max_voxels_side, loading_passes):
        h = C.c_void_p()
        rc = lib.sdfv_viewer_from_bb(_f6(bb), int(max_voxels_side), int(loading_passes), C.byref(h))
        _check(rc, "sdfv_viewer_from_bb")
        return cls(h)

    @classmethod
    def new_voxels(cls, dims, bb, loading_passes, layout=LAYOUT_AUTO):
        h = C.c_void_p()
        rc = lib.sdfv_viewer_new_voxels((C.c_uint32 * 3)(*dims), _f6(bb), int(loading_passes), int(layout), C.byref(h))
        _check(rc, "sdfv_viewer_new_voxels")
        return cls(h)

    def update(self, surface, budget_s=0.03, budget_ns=None):
        n = C.c_size_t()
        ns = int(budget_s * 1e9) if budget_ns is None else int(budget_ns)
        rc = lib.sdfv_viewer_update(self.h, C.byref(surface.struct), ns, C.byref(n))
        _check(rc, lib.sdfv_viewer_last_error(self.h))
        return n.value

    def update_rc(self, surface, budget_ns):
        """(status, visited, message) without raising: what the error tests look at."""
        n = C.c_size_t()
        rc = lib.sdfv_viewer_update(self.h, C.byref(surface.struct), int(budget_ns), C.byref(n))
        return rc, n.value, lib.sdfv_viewer_last_error(self.h).decode()

    def commit(self):
        _check(lib.sdfv_viewer_commit(self.h), lib.sdfv_viewer_last_error(self.h))

    def state(self):
        st = LoadState()
        _check(lib.sdfv_viewer_state(self.h, C.byref(st)), "sdfv_viewer_state")
        return dict(remaining=st.remaining, total_iterations=st.total_iterations, passes_left=st.passes_left,
                    has_changed_box=bool(st.has_changed_box), lod=st.lod_dist_between_samples, dims=tuple(st.dims))

    def textures(self):
        t0, t1, g = C.c_void_p(), C.c_void_p(), Grid()
        _check(lib.sdfv_viewer_textures(self.h, C.byref(t0), C.byref(t1), C.byref(g)), lib.sdfv_viewer_last_error(self.h))
        return t0.value, t1.value, g

    def download(self):
        import numpy as np
        d = self.state()["dims"]
        shape = (d[2], d[1], d[0], 4)
        t0, t1 = np.empty(shape, np.float32), np.empty(shape, np.float32)
        _check(lib.sdfv_viewer_download(self.h, t0.ctypes.data, t1.ctypes.data), lib.sdfv_viewer_last_error(self.h))
        return t0, t1

    def mesh(self, algorithm=0, materials=True):
        """sdfv_viewer_mesh: the grid as it is loaded now -> (vertices [n, 12] float32, indices int32) torch tensors on the GPU
        (the library's copy is freed)."""
        from . import mesh_tensors
        m = _capi.Mesh()
        _check(lib.sdfv_viewer_mesh(self.h, int(algorithm), _capi.MESH_WITH_MATERIALS if materials else 0, C.byref(m)),
               lib.sdfv_viewer_last_error(self.h))
        return mesh_tensors(m)

    def render(self, width, height, view=None):
        """-> [height, width, 4] float32 tensor on the GPU."""
        import torch
        img = torch.empty((height, width, 4), dtype=torch.float32, device="cuda")
        _check(lib.sdfv_viewer_render(self.h, C.byref(view) if view is not None else None, width, height, img.data_ptr()),
               lib.sdfv_viewer_last_error(self.h))
        return img

    def set_stream(self, stream_ptr):
        _check(lib.sdfv_viewer_set_stream(self.h, stream_ptr), "sdfv_viewer_set_stream")

    def set_ingest(self, host_threads=0, capacity=0):
        _check(lib.sdfv_viewer_set_ingest(self.h, int(host_threads), int(capacity)), "sdfv_viewer_set_ingest")

    def last_error(self):
        return lib.sdfv_viewer_last_error(self.h).decode()

    def close(self):
        if self.h and self.owned:
            lib.sdfv_viewer_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scene:
    """SDFViewerAppScene through sdfv_scene_*; clock: a callable returning nanoseconds (None = the steady clock)."""

    def __init__(self, surface, clock=None):
        self.surface = surface
        self._clock = CLOCK_FN(lambda _user: int(clock())) if clock is not None else CLOCK_FN()
        h = C.c_void_p()
        _check(lib.sdfv_scene_new(C.byref(surface.struct), self._clock, None, C.byref(h)), "sdfv_scene_new")
        self.h = h

    def set_surface(self, surface, max_voxels_side=0, loading_passes=0):
        self.surface = surface
        _check(lib.sdfv_scene_set_surface(self.h, C.byref(surface.struct), int(max_voxels_side), int(loading_passes)),
               lib.sdfv_scene_last_error(self.h))

    def set_camera(self, view):
        _check(lib.sdfv_scene_set_camera(self.h, C.byref(view)), "sdfv_scene_set_camera")

    def set_budget(self, load_budget_ms=30, commit_interval_ms=500):
        _check(lib.sdfv_scene_set_budget(self.h, int(load_budget_ms), int(commit_interval_ms)), "sdfv_scene_set_budget")

    def render(self, width=0, height=0, draw=False):
        import torch
        img = torch.empty((height, width, 4), dtype=torch.float32, device="cuda") if draw else None
        rep = RenderReport()
        _check(lib.sdfv_scene_render(self.h, width, height, img.data_ptr() if draw else None, C.byref(rep)),
               lib.sdfv_scene_last_error(self.h))
        r = dict(cpu_updates=rep.cpu_updates, committed=bool(rep.committed), last_chunk=bool(rep.last_chunk),
                 request_repaint=bool(rep.request_repaint))
        return (r, img) if draw else r

    def load_progress(self):
        loading, prog, text = C.c_int(), C.c_float(), C.create_string_buffer(256)
        _check(lib.sdfv_scene_load_progress(self.h, C.byref(loading), C.byref(prog), text, 256), "sdfv_scene_load_progress")
        return (prog.value, text.value.decode()) if loading.value else None

    def viewer(self):
        return Viewer(lib.sdfv_scene_viewer(self.h), owned=False)

    def close(self):
        if self.h:
            lib.sdfv_scene_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
