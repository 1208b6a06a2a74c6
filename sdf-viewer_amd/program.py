"""SDF programs (include/sdfgrid.h, "SDF programs"): a caller-defined CSG tree as data, evaluated on the device.

    prog = (Program(bb=(-1, -1, -1, 1, 1, 1))
            .material(0.8, 0.2, 0.1, roughness=0.6)
            .push_affine(translation(0.2, 0.0, 0.0)).box(0.5, 0.3, 0.2).pop()
            .material(0.1, 0.3, 0.9).sphere(0.45)
            .subtract()
            .build())
    t0, t1 = pkg.alloc_textures(grid)
    prog.fill_grid(grid, t0, t1)                       # the dense fill, one launch
    records = prog.sample_points(points)               # [n, 3] CUDA tensor -> [n, 7]
    viewer.update(prog.as_surface())                   # progressive load through sdf-viewer_amd.viewer
    prog2.grid_pass(grid, 1, t0, t1, changed_box=box)  # an edited program over the loaded grid: only the box is re-sampled

Parameters (include/sdfprogram.h, "program editor"): name an operand while building, then edit it by name --

    b = Program().material(0.8, 0.2, 0.1).sphere(0.5)
    b.param("radius", [(len(b.ops) - 1, 0, PARAM_VALUE)], 0.1, 0.9, 0.01, 0.5, box=(-0.9,) * 3 + (0.9,) * 3)
    ed = b.build_editor()
    ed.set("radius", 0.6)                              # a new snapshot; ed.changed() -> the box, once
    ed.update_viewer(viewer)                           # re-samples the box by whole passes (sdfv_viewer_update_program)
    rgba = prog.render(camera, 1920, 1080)             # sphere-traced directly per pixel: no grid
    vertices, indices = prog.mesh(128, materials=True) # marching cubes + Mesh::postproc: [V, 12], [3 * triangles]
    hits = prog.cast(rays)                             # [n, 8] rays -> [n, 16]: status, steps, t, pos, normal, sample per ray

The builder only appends instructions; sdfv_program_create validates them (build() raises SdfvError with the message that
names the offending instruction).
"""
import ctypes as C

from . import _capi
from ._capi import ProgOp, SdfvError, check, lib


PARAM_VALUE, PARAM_NEGATED, PARAM_RECIPROCAL = 0, 1, 2
# the routes CompiledProgram.compile() specialises (SDFV_COMPILE_*)
FILL, POINTS, MARCH = _capi.COMPILE_FILL, _capi.COMPILE_POINTS, _capi.COMPILE_MARCH
MESH = _capi.COMPILE_MESH
PARAM_MAX_TARGETS = 4


class ParamTarget(C.Structure):
    _fields_ = [("op", C.c_uint32), ("operand", C.c_uint32), ("kind", C.c_uint32)]


class ProgramParam(C.Structure):
    """sdfv_program_param"""
    _fields_ = [("id", C.c_uint32), ("name", C.c_char_p), ("description", C.c_char_p), ("min", C.c_float), ("max", C.c_float),
                ("step", C.c_float), ("value", C.c_float), ("n_targets", C.c_uint32), ("targets", ParamTarget * PARAM_MAX_TARGETS),
                ("has_box", C.c_uint32), ("box", C.c_float * 6)]


def ray_dtype():
    """numpy dtype of sdfv_ray (32 bytes)."""
    import numpy as np
    return np.dtype([("origin", "<f4", (3,)), ("t_min", "<f4"), ("dir", "<f4", (3,)), ("t_max", "<f4")])


def hit_dtype():
    """numpy dtype of sdfv_ray_hit (64 bytes); sample = (distance, r, g, b, metallic, roughness, occlusion)."""
    import numpy as np
    return np.dtype([("status", "<i4"), ("steps", "<i4"), ("t", "<f4"), ("pos", "<f4", (3,)), ("normal", "<f4", (3,)),
                     ("sample", "<f4", (7,))])


def hits_view(a):
    """[n, 16] float32 (what CompiledProgram.cast hands out, as numpy) -> the same bytes as a hit_dtype() array [n]."""
    import numpy as np
    return np.ascontiguousarray(a).view(hit_dtype()).reshape(-1)


def translation(tx, ty, tz):
    """The 3 x 4 matrix PUSH_AFFINE wants for content MOVED by (tx, ty, tz): the inverse transform, row-major."""
    return (1.0, 0.0, 0.0, -float(tx), 0.0, 1.0, 0.0, -float(ty), 0.0, 0.0, 1.0, -float(tz))


def rigid_inverse(rotation, t):
    """rotation: 3 x 3 row-major (orthonormal), t: translation of the content -> the inverse as PUSH_AFFINE's 12 floats:
    q' = R^T (q - t)."""
    r = [[float(rotation[i][j]) for j in range(3)] for i in range(3)]
    rt = [[r[j][i] for j in range(3)] for i in range(3)]
    out = []
    for i in range(3):
        out += rt[i] + [-(rt[i][0] * float(t[0]) + rt[i][1] * float(t[1]) + rt[i][2] * float(t[2]))]
    return tuple(out)


class Program:
    """Builder: every method appends one instruction and returns self; build() hands the array to the library."""

    def __init__(self, bb=(-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)):
        self.bb = tuple(float(x) for x in bb)
        self.ops = []
        self.params = []

    def op(self, opcode, *operands):
        """Any instruction by opcode (_capi.OP_*) and operands; the named methods below all come here."""
        assert len(operands) <= 12
        self.ops.append((int(opcode), tuple(float(x) for x in operands)))
        return self

    # primitives
    def sphere(self, r): return self.op(_capi.OP_SPHERE, r)
    def cube(self, h): return self.op(_capi.OP_CUBE, h)
    def box(self, hx, hy, hz): return self.op(_capi.OP_BOX, hx, hy, hz)
    def cylinder(self, r, half_height): return self.op(_capi.OP_CYLINDER, r, half_height)
    def torus(self, major, minor): return self.op(_capi.OP_TORUS, major, minor)
    def plane(self, nx, ny, nz, d): return self.op(_capi.OP_PLANE, nx, ny, nz, d)
    # frames
    def push_affine(self, m12): return self.op(_capi.OP_PUSH_AFFINE, *m12)
    def pop(self): return self.op(_capi.OP_POP)

    def push_scale(self, s):
        import numpy as np
        s = np.float32(s)
        return self.op(_capi.OP_PUSH_SCALE, s, np.float32(1.0) / s)

    def pop_scale(self, s): return self.op(_capi.OP_POP_SCALE, s)
    # combinators
    def union(self): return self.op(_capi.OP_UNION)
    def intersect(self): return self.op(_capi.OP_INTERSECT)
    def subtract(self): return self.op(_capi.OP_SUBTRACT)
    def smooth_union(self, k): return self.op(_capi.OP_SMOOTH_UNION, k)
    def smooth_subtract(self, k): return self.op(_capi.OP_SMOOTH_SUBTRACT, k)
    # on the top value
    def round(self, r): return self.op(_capi.OP_ROUND, r)
    def shell(self, t): return self.op(_capi.OP_SHELL, t)

    def material(self, r, g, b, metallic=0.0, roughness=0.0, occlusion=0.0):
        return self.op(_capi.OP_MATERIAL, r, g, b, metallic, roughness, occlusion)

    def array(self):
        """The instructions as a ctypes array of sdfv_prog_op."""
        arr = (ProgOp * max(len(self.ops), 1))()
        for i, (opcode, operands) in enumerate(self.ops):
            arr[i].op = opcode
            for k, v in enumerate(operands):
                arr[i].a[k] = v
        return arr

    def build(self):
        return CompiledProgram(self.array(), len(self.ops), self.bb)

    def param(self, name, targets, lo, hi, step, value, box=None, description=""):
        """A float parameter of the editor build_editor() makes: `targets` is a list of (instruction index, operand index,
        PARAM_VALUE | PARAM_NEGATED | PARAM_RECIPROCAL), `box` the 6 floats an edit can reach (None: the program's box).  Its id is
        its position in the list."""
        self.params.append(dict(name=str(name), targets=[tuple(int(v) for v in t) for t in targets], lo=float(lo), hi=float(hi),
                                step=float(step), value=float(value), box=None if box is None else tuple(float(v) for v in box),
                                description=str(description)))
        return self

    def build_editor(self):
        return ProgramEditor(self)


def _rotation(axis, degrees):
    import math
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    return [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]] if axis == "z" else [[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]


def example_sixteen():
    """A 16-primitive model with frames and materials, as a Program builder (77 instructions): a plate on four pillars, a torus,
    a tilted cube, a ring of six spheres, a bore, a rounded foot, cut by a plane.  The large program of tools/program_bench.py
    (profiles/program_fill.json's "C") and a member of the tests' catalogue: changing it changes what those numbers mean."""
    import math
    s = Program((-1.0, -1.0, -1.0, 1.0, 1.0, 1.0))
    s.material(0.7, 0.7, 0.75, 0.9, 0.3, 1.0).box(0.8, 0.8, 0.1)                                   # 1: a plate
    for i in range(4):                                                                            # 2..5: four pillars
        cx, cy = (-0.6 if i & 1 else 0.6), (-0.6 if i & 2 else 0.6)
        s.material(0.6, 0.3 + 0.1 * i, 0.2, 0.1, 0.7, 1.0)
        s.push_affine(translation(cx, cy, 0.45)).cylinder(0.08, 0.4).pop().union()
    s.material(0.2, 0.5, 0.8, 0.0, 0.4, 1.0)
    s.push_affine(translation(0.0, 0.0, 0.5)).torus(0.45, 0.08).pop().smooth_union(0.05)            # 6
    s.material(0.9, 0.1, 0.1, 0.3, 0.2, 1.0)
    s.push_affine(rigid_inverse(_rotation("z", 45.0), (0.0, 0.0, 0.3))).push_scale(0.5).cube(0.3).pop_scale(0.5).pop().union()  # 7
    for i in range(6):                                                                            # 8..13: a ring of spheres
        ang = math.radians(60.0 * i)
        s.material(0.2 + 0.1 * i, 0.8 - 0.1 * i, 0.4, 0.2, 0.5, 1.0)
        s.push_affine(translation(0.7 * math.cos(ang), 0.7 * math.sin(ang), -0.3)).sphere(0.15).pop().smooth_union(0.04)
    s.material(0.3, 0.3, 0.3, 0.0, 0.9, 1.0)
    s.push_affine(rigid_inverse(_rotation("x", 90.0), (0.0, 0.0, 0.0))).cylinder(0.1, 1.2).pop().subtract()  # 14: a bore
    s.material(0.95, 0.85, 0.2, 1.0, 0.1, 1.0)
    s.push_affine(translation(0.0, 0.0, -0.6)).box(0.3, 0.3, 0.05).round(0.02).pop().union()        # 15
    s.plane(0.0, 0.0, -1.0, 0.95).intersect()                                                     # 16
    return s


class CompiledProgram:
    """An sdfv_program handle."""

    def __init__(self, ops_array, n, bb):
        h = C.c_void_p()
        check(lib.sdfv_program_create(C.cast(ops_array, C.c_void_p), int(n), (C.c_float * 6)(*[float(x) for x in bb]), C.byref(h)))
        self.h = h
        self._surface = None
        self._owner = None

    @classmethod
    def borrowed(cls, handle, owner):
        """A view of a handle that `owner` owns (a ProgramEditor's snapshot): kept alive with it, never freed here."""
        self = cls.__new__(cls)
        self.h, self._surface, self._owner = C.c_void_p(handle), None, owner
        return self

    def ops(self):
        """(numpy structured copy of the validated instructions, bounding box)."""
        import numpy as np
        p, n, bb = C.c_void_p(), C.c_size_t(), (C.c_float * 6)()
        check(lib.sdfv_program_ops(self.h, C.byref(p), C.byref(n), bb))
        raw = C.string_at(p.value, n.value * 64)
        dt = np.dtype([("op", "<u4"), ("reserved", "<u4", (3,)), ("a", "<f4", (12,))])
        return np.frombuffer(raw, dtype=dt).copy(), tuple(bb)

    def sample_points(self, points, distance_only=False, stream=None, out=None):
        """points: [n, 3] float32 CUDA tensor -> [n, 7] records (distance, r, g, b, metallic, roughness, occlusion); out: optional
        tensor that receives them."""
        import torch
        from . import _dev_ptr, _out_tensor, _stream_ptr
        n = points.shape[0]
        out = _out_tensor(out, (n, 7), torch.float32, points.device, "out")
        check(lib.sdfv_program_sample_points(self.h, _dev_ptr(points, "points") if n else None, n, int(bool(distance_only)),
                                             C.c_void_p(out.data_ptr()) if n else None, _stream_ptr(stream)))
        return out

    def sample_points_host(self, points, distance_only=False):
        """points: [n, 3] float32 numpy array -> [n, 7] numpy array; evaluated on the device."""
        import numpy as np
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.empty((pts.shape[0], 7), np.float32)
        check(lib.sdfv_program_sample_points_host(self.h, pts.ctypes.data, pts.shape[0], int(bool(distance_only)), out.ctypes.data))
        return out

    def mesh(self, n, bb=None, materials=False, stream=None, algorithm=0):
        """sdfv_program_mesh_extract: marching cubes (algorithm 0) or dual contouring (_capi.MESHER_DUAL_CONTOURING_PARTICLE) over
        n^3 cells of `bb` (min.xyz + max.xyz; None: the program's box) -> (vertices [V, 12] float32, indices [3 * triangles]
        int32), copied out of the library's buffers.  materials=True: the vertices leave as mesh_postproc would make them
        (SDFV_MESH_WITH_MATERIALS)."""
        from . import _stream_ptr, f3, mesh_tensors
        m = _capi.Mesh()
        lo, hi = (None, None) if bb is None else (f3(bb[:3]), f3(bb[3:]))
        check(lib.sdfv_program_mesh_extract(self.h, lo, hi, int(n), int(algorithm), _capi.MESH_WITH_MATERIALS if materials else 0, C.byref(m),
                                            _stream_ptr(stream)))
        return mesh_tensors(m)

    def mesh_sparse(self, n, bb=None, materials=False, lipschitz=0.0, stream=None, want_stats=False):
        """sdfv_program_mesh_extract_sparse: marching cubes over n^3 cells (n a power of two, 4 .. 4096) of `bb`, sampling only the
        4-cell bricks that a distance with Lipschitz constant `lipschitz` (0.0: 1) cannot rule out -> (vertices [V, 12] float32,
        indices [3 * triangles] int32), the set mesh(n, bb, materials) returns in another order; with want_stats also a dict
        (levels, tested, kept, bricks, evaluations, scratch_bytes)."""
        from . import _stream_ptr, f3, mesh_tensors
        m, s, d = _capi.Mesh(), _capi.SparseMeshStats(), _capi.SparseMeshDesc()
        s.size, d.size = C.sizeof(s), C.sizeof(d)
        d.program = self.h
        lo, hi = (None, None) if bb is None else (f3(bb[:3]), f3(bb[3:]))
        if bb is not None:
            d.bb_min, d.bb_max = lo, hi
        d.cells, d.algorithm, d.flags = int(n), _capi.MESHER_MARCHING_CUBES, _capi.MESH_WITH_MATERIALS if materials else 0
        d.lipschitz = float(lipschitz)
        d.out, d.stats = C.pointer(m), C.pointer(s)
        check(lib.sdfv_program_mesh_extract_sparse(C.byref(d), _stream_ptr(stream)))
        v, i = mesh_tensors(m)
        if not want_stats:
            return v, i
        return v, i, dict(levels=s.levels, tested=list(s.tested[:s.levels]), kept=list(s.kept[:s.levels]), bricks=s.bricks,
                          evaluations=s.evaluations, scratch_bytes=s.scratch_bytes)

    def normal_points(self, points, eps=0.0, stream=None, out=None):
        """SDFSurface::normal(p, eps) of the program (eps <= 0: None): [n, 3] float32 CUDA tensor -> [n, 3] (out: optional result
        tensor)."""
        import torch
        from . import _dev_ptr, _out_tensor, _stream_ptr
        n = points.shape[0]
        out = _out_tensor(out, (n, 3), torch.float32, points.device, "out")
        check(lib.sdfv_program_normal_points(self.h, _dev_ptr(points, "points") if n else None, n, float(eps),
                                             C.c_void_p(out.data_ptr()) if n else None, _stream_ptr(stream)))
        return out

    def mesh_postproc(self, vertices, stream=None):
        """Mesh::postproc in place over an [n, 12] float32 CUDA tensor of vertices; returns it."""
        from . import VERTEX_FLOATS, _dev_ptr, _stream_ptr
        assert vertices.dim() == 2 and vertices.shape[1] == VERTEX_FLOATS
        n = vertices.shape[0]
        check(lib.sdfv_program_mesh_postproc(self.h, _dev_ptr(vertices, "vertices") if n else None, n, _stream_ptr(stream)))
        return vertices

    def fill_grid(self, grid, tex0, tex1, dist=None, flags=0, stream=None):
        """sdfv_program_fill_grid_commit; flags: _capi.PASS_VOLUME_INTERLEAVED when `dist` is the y-interleaved volume."""
        from . import _dev_ptr, _stream_ptr
        check(lib.sdfv_program_fill_grid_commit(self.h, C.byref(grid), _dev_ptr(tex0, "tex0"), _dev_ptr(tex1, "tex1"),
                                                None if dist is None else _dev_ptr(dist, "dist"), int(flags), _stream_ptr(stream)))

    def grid_pass(self, grid, step, tex0, tex1, dist=None, changed_box=None, flags=0, stream=None):
        """sdfv_program_grid_pass: one LoadingManager pass with this program as the SDF.  changed_box: 6 floats (min.xyz,
        max.xyz) or None; flags: _capi.PASS_* as for pkg.fill_grid_pass."""
        from . import _dev_ptr, _stream_ptr
        box = None if changed_box is None else (C.c_float * 6)(*[float(v) for v in changed_box])
        check(lib.sdfv_program_grid_pass(self.h, C.byref(grid), int(step), box, _dev_ptr(tex0, "tex0"), _dev_ptr(tex1, "tex1"),
                                         None if dist is None else _dev_ptr(dist, "dist"), int(flags), _stream_ptr(stream)))

    def march_desc(self, cameras, width, height, rp=None, normal_h=0.0, y0=0, y1=None):
        """An sdfv_program_march_desc over this program without outputs (and what keeps its pointers alive).  cameras: a
        Camera or a sequence of them; rp: RenderParams (default: the library's defaults for a 256^3 grid over the program's
        box -- the bounds, and the grid whose normal taps normal_h == 0 stands for)."""
        from . import default_render_params, make_grid
        cams = list(cameras) if isinstance(cameras, (list, tuple)) else [cameras]
        arr = (_capi.Camera * max(len(cams), 1))(*cams)
        if rp is None:
            _, bb = self.ops()
            rp = default_render_params(make_grid((256, 256, 256), bb[:3], bb[3:]))
        d = _capi.ProgramMarchDesc()
        d.size = C.sizeof(d)
        d.program = self.h
        d.rp = C.pointer(rp)
        d.cameras = C.cast(arr, C.POINTER(_capi.Camera))
        d.n_cameras, d.width, d.height = len(cams), int(width), int(height)
        d.y0, d.y1 = int(y0), int(height if y1 is None else y1)
        d.normal_h = float(normal_h)
        return d, (arr, rp)

    def render(self, cameras, width, height, rp=None, normal_h=0.0, want_aux=False, want_depth=False, rgba8=False, stream=None,
               y0=0, y1=None, out=None, aux_out=None, depth_out=None):
        """sdfv_program_raymarch: rows [y0, y1) of n_cameras width x height images sphere-traced directly on the device.
        Returns the colour -- [n, rows, width, 4] float32, or [n, rows, width] uint32-as-int32 packed RGBA8 with rgba8=True -- or a
        tuple (colour[, aux: [n, rows, width, 18] float32 view of sdfv_march_aux][, depth: [n, rows, width]]).  out / aux_out /
        depth_out: the caller's tensors for the colour, aux and depth planes (the latter two imply want_aux / want_depth)."""
        import torch
        from . import _out_tensor
        d, keep = self.march_desc(cameras, width, height, rp, normal_h, y0, y1)
        shape = (d.n_cameras, d.y1 - d.y0, d.width)
        dev = torch.device("cuda", torch.cuda.current_device())
        want_aux, want_depth = want_aux or aux_out is not None, want_depth or depth_out is not None
        colour = _out_tensor(out, shape if rgba8 else shape + (4,), torch.int32 if rgba8 else torch.float32, dev, "out")
        aux = _out_tensor(aux_out, shape + (18,), torch.float32, dev, "aux_out") if want_aux else None
        depth = _out_tensor(depth_out, shape, torch.float32, dev, "depth_out") if want_depth else None
        if rgba8:
            d.rgba8 = colour.data_ptr()
        else:
            d.rgba = colour.data_ptr()
        d.aux = aux.data_ptr() if want_aux else None
        d.depth = depth.data_ptr() if want_depth else None
        from . import _stream_ptr
        check(lib.sdfv_program_raymarch(C.byref(d), _stream_ptr(stream)))
        out = (colour,) + ((aux,) if want_aux else ()) + ((depth,) if want_depth else ())
        return out[0] if len(out) == 1 else out

    def render_host(self, cameras, width, height, rp=None, normal_h=0.0, want_aux=False, want_depth=False, rgba8=False, threads=0,
                    y0=0, y1=None):
        """sdfv_program_raymarch_host: the same render on the host (numpy arrays, same shapes; aux as a [..., 18] float32 view),
        by the per-pixel source the kernel is built from; needs no device."""
        import numpy as np
        from . import viewer
        fn = viewer.lib.sdfv_program_raymarch_host
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(_capi.ProgramMarchDesc), C.c_int]
        d, keep = self.march_desc(cameras, width, height, rp, normal_h, y0, y1)
        shape = (d.n_cameras, d.y1 - d.y0, d.width)
        colour = np.empty(shape if rgba8 else shape + (4,), np.uint32 if rgba8 else np.float32)
        aux = np.empty(shape + (18,), np.float32) if want_aux else None
        depth = np.empty(shape, np.float32) if want_depth else None
        if rgba8:
            d.rgba8 = colour.ctypes.data
        else:
            d.rgba = colour.ctypes.data
        d.aux = aux.ctypes.data if want_aux else None
        d.depth = depth.ctypes.data if want_depth else None
        check(fn(C.byref(d), int(threads)))
        out = (colour,) + ((aux,) if want_aux else ()) + ((depth,) if want_depth else ())
        return out[0] if len(out) == 1 else out

    def cast_desc(self, rays_ptr, hits_ptr, n, normals=True, materials=True, max_steps=0, hit_eps=0.0, normal_eps=0.0, box=None):
        """An sdfv_program_cast_desc over this program from raw addresses (and what keeps its box alive).  box: 6 floats
        (min.xyz, max.xyz) or None for the program's."""
        d = _capi.ProgramCastDesc()
        d.size = C.sizeof(d)
        d.program = self.h
        keep = None
        if box is not None:
            keep = (_capi.f3(box[:3]), _capi.f3(box[3:]))
            d.bb_min, d.bb_max = keep
        d.rays, d.hits, d.n = rays_ptr, hits_ptr, int(n)
        d.flags = (_capi.CAST_NORMALS if normals else 0) | (_capi.CAST_MATERIALS if materials else 0)
        d.max_steps, d.hit_eps, d.normal_eps = int(max_steps), float(hit_eps), float(normal_eps)
        return d, keep

    def cast(self, rays, *, normals=True, materials=True, max_steps=0, hit_eps=0.0, normal_eps=0.0, box=None, stream=None,
             out=None):
        """sdfv_program_raycast: rays [n, 8] float32 CUDA tensor (origin.xyz, t_min, dir.xyz, t_max per ray) -> hits [n, 16]
        float32 CUDA tensor, the 64-byte sdfv_ray_hit records (status and steps are int32 bit patterns: hits_view() of the
        tensor's numpy copy names the fields).  max_steps / hit_eps / normal_eps: 0 = the library's 256 / 1e-5 / 0.001; box: the
        6 floats to clip against (None: the program's); out: optional tensor that receives the records."""
        import torch
        from . import _dev_ptr, _out_tensor, _stream_ptr
        if rays.dim() != 2 or rays.shape[1] != 8:
            raise TypeError("rays must be an [n, 8] tensor")
        n = rays.shape[0]
        out = _out_tensor(out, (n, 16), torch.float32, rays.device, "out")
        d, keep = self.cast_desc(_dev_ptr(rays, "rays") if n else None, out.data_ptr() if n else None, n, normals, materials,
                                 max_steps, hit_eps, normal_eps, box)
        check(lib.sdfv_program_raycast(C.byref(d), _stream_ptr(stream)))
        return out

    def cast_host(self, rays, *, normals=True, materials=True, max_steps=0, hit_eps=0.0, normal_eps=0.0, box=None):
        """sdfv_program_raycast_host: the same cast on the host, by the per-ray source the kernel is built from; needs no device.
        rays: [n, 8] float32 numpy array or a RAY_DTYPE structured array -> HIT_DTYPE structured array [n]."""
        import numpy as np
        from . import viewer
        fn = viewer.lib.sdfv_program_raycast_host
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(_capi.ProgramCastDesc)]
        r = np.ascontiguousarray(rays)
        r = r.view(np.float32).reshape(-1, 8) if r.dtype == ray_dtype() else np.ascontiguousarray(r, np.float32).reshape(-1, 8)
        hits = np.empty(len(r), hit_dtype())
        d, keep = self.cast_desc(r.ctypes.data if len(r) else None, hits.ctypes.data if len(r) else None, len(r), normals, materials,
                                 max_steps, hit_eps, normal_eps, box)
        check(fn(C.byref(d)))
        return hits

    def as_surface(self, device_route=True):
        """A viewer.Surface over this program (sdfv_program_as_surface); device_route=False clears sample_batch_device, so
        that the viewer samples through the host callbacks.  The surface keeps the program alive."""
        from . import viewer
        fn = viewer.lib.sdfv_program_as_surface
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(viewer.SurfaceStruct)]
        s = viewer.Surface()
        rc = fn(self.h, C.byref(s.struct))
        if rc != 0:
            raise SdfvError(rc, "sdfv_program_as_surface")
        if not device_route:
            s.struct.sample_batch_device = viewer.DEVICE_FN()
        bb = (C.c_float * 6)()
        s.struct.bounding_box(s.struct.user, bb)
        s._bb = tuple(bb)
        s._keep.append(self)
        return s

    def compile(self, routes=FILL | POINTS | MARCH, arch=None):
        """sdfv_program_compile: a NEW handle whose `routes` (FILL | POINTS | MARCH | MESH) launch kernels compiled for this
        very program at run time; everything else about it is this handle's.  MESH covers mesh(), mesh_sparse(), normals and
        postproc on the device -- the steps that evaluate the program -- and is not part of the default.  arch: None = the
        current device's, or a name such as "gfx950" (needs no device).  Takes of the order of a second per route: for a model that is filled or rendered many
        times, not for an editor's snapshots."""
        h = C.c_void_p()
        check(lib.sdfv_program_compile(self.h, int(routes), None if arch is None else str(arch).encode(), C.byref(h)))
        new = CompiledProgram.__new__(CompiledProgram)
        new.h, new._surface, new._owner = h, None, None
        return new

    def compiled_info(self):
        """sdfv_program_compiled_info as a dict: routes (0 for a plain handle), arch, compile_seconds, code_bytes, launches."""
        info = _capi.CompiledInfo()
        info.size = C.sizeof(info)
        check(lib.sdfv_program_compiled_info(self.h, C.byref(info)))
        return dict(routes=int(info.routes), arch=info.arch.decode(), compile_seconds=float(info.compile_seconds),
                    code_bytes=int(info.code_bytes), launches=int(info.launches))

    def compiled_code(self):
        """The code object of a compiled handle (bytes: an ELF for its architecture)."""
        p, n = C.c_void_p(), C.c_size_t()
        check(lib.sdfv_program_compiled_code(self.h, C.byref(p), C.byref(n), None))
        return C.string_at(p.value, n.value)

    def compiled_source(self):
        """The translation unit sdfv_program_compile generated for this handle (str)."""
        src = C.c_char_p()
        check(lib.sdfv_program_compiled_code(self.h, None, None, C.byref(src)))
        return src.value.decode()

    def close(self):
        if self.h and self._owner is None:
            lib.sdfv_program_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ProgramEditor:
    """An sdfv_program_editor (include/sdfprogram.h): a program whose named operands can be edited.  Every accepted set() makes a
    new snapshot (an immutable sdfv_program); the replaced ones live until trim() or close()."""

    def __init__(self, builder):
        from . import viewer
        self._lib = L = viewer.lib
        L.sdfv_program_editor_create.restype = C.c_int
        L.sdfv_program_editor_create.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(ProgramParam), C.c_size_t,
                                                 C.POINTER(C.c_void_p)]
        L.sdfv_program_editor_free.restype, L.sdfv_program_editor_free.argtypes = None, [C.c_void_p]
        L.sdfv_program_editor_parameters.restype = C.c_int
        L.sdfv_program_editor_parameters.argtypes = [C.c_void_p, C.POINTER(C.POINTER(ProgramParam)), C.POINTER(C.c_size_t)]
        L.sdfv_program_editor_set.restype, L.sdfv_program_editor_set.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_float]
        L.sdfv_program_editor_changed.restype, L.sdfv_program_editor_changed.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float)]
        L.sdfv_program_editor_program.restype, L.sdfv_program_editor_program.argtypes = C.c_void_p, [C.c_void_p]
        L.sdfv_program_editor_trim.restype, L.sdfv_program_editor_trim.argtypes = C.c_int, [C.c_void_p]
        L.sdfv_program_editor_last_error.restype, L.sdfv_program_editor_last_error.argtypes = C.c_char_p, [C.c_void_p]
        L.sdfv_program_editor_as_surface.restype = C.c_int
        L.sdfv_program_editor_as_surface.argtypes = [C.c_void_p, C.POINTER(viewer.SurfaceStruct)]
        L.sdfv_viewer_update_program.restype = C.c_int
        L.sdfv_viewer_update_program.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_size_t)]
        arr = (ProgramParam * max(len(builder.params), 1))()
        for i, p in enumerate(builder.params):
            if len(p["targets"]) > PARAM_MAX_TARGETS:
                raise SdfvError(-1, f"parameter {p['name']}: more than {PARAM_MAX_TARGETS} targets")
            arr[i].id, arr[i].name, arr[i].description = i, p["name"].encode(), p["description"].encode()
            arr[i].min, arr[i].max, arr[i].step, arr[i].value = p["lo"], p["hi"], p["step"], p["value"]
            arr[i].n_targets = len(p["targets"])
            for k, (op, operand, kind) in enumerate(p["targets"]):
                arr[i].targets[k] = ParamTarget(op, operand, kind)
            arr[i].has_box = int(p["box"] is not None)
            for k in range(6):
                arr[i].box[k] = p["box"][k] if p["box"] is not None else 0.0
        h = C.c_void_p()
        rc = L.sdfv_program_editor_create(C.cast(builder.array(), C.c_void_p), len(builder.ops), (C.c_float * 6)(*builder.bb), arr,
                                          len(builder.params), C.byref(h))
        if rc != 0:
            raise SdfvError(rc, L.sdfv_program_editor_last_error(None).decode())
        self.h = h
        self._ids = {p["name"]: i for i, p in enumerate(builder.params)}

    def _id(self, name):
        if isinstance(name, str):
            if name not in self._ids:
                raise SdfvError(-1, f"unknown parameter {name!r}")
            return self._ids[name]
        return int(name)

    def parameters(self):
        """[dict(id, name, description, min, max, step, value, targets, box)] with the current values."""
        p, n = C.POINTER(ProgramParam)(), C.c_size_t()
        check(self._lib.sdfv_program_editor_parameters(self.h, C.byref(p), C.byref(n)))
        return [dict(id=p[i].id, name=p[i].name.decode(), description=p[i].description.decode(), min=p[i].min, max=p[i].max,
                     step=p[i].step, value=p[i].value,
                     targets=[(t.op, t.operand, t.kind) for t in list(p[i].targets)[:p[i].n_targets]],
                     box=tuple(p[i].box) if p[i].has_box else None) for i in range(n.value)]

    def get(self, name):
        return self.parameters()[[q["id"] for q in self.parameters()].index(self._id(name))]["value"]

    def set(self, name, value):
        """set_parameter: raises SdfvError with the reason (out of range, unknown, or the validator's message) and changes nothing
        when the value is refused."""
        rc = self._lib.sdfv_program_editor_set(self.h, self._id(name), float(value))
        if rc != 0:
            raise SdfvError(rc, self._lib.sdfv_program_editor_last_error(self.h).decode())

    def changed(self):
        """The pending box (6 floats) once, then None."""
        out = (C.c_float * 6)()
        return tuple(out) if self._lib.sdfv_program_editor_changed(self.h, out) == 1 else None

    @property
    def program(self):
        """The current snapshot as a CompiledProgram (borrowed: valid until trim() after a later set(), or close())."""
        return CompiledProgram.borrowed(self._lib.sdfv_program_editor_program(self.h), self)

    def trim(self):
        """Frees the replaced snapshots; synchronise the streams that may still run one first."""
        check(self._lib.sdfv_program_editor_trim(self.h))

    def as_surface(self):
        """A viewer.Surface over the current snapshot, whichever it is at each call, with `changed` set."""
        from . import viewer
        s = viewer.Surface()
        rc = self._lib.sdfv_program_editor_as_surface(self.h, C.byref(s.struct))
        if rc != 0:
            raise SdfvError(rc, "sdfv_program_editor_as_surface")
        bb = (C.c_float * 6)()
        s.struct.bounding_box(s.struct.user, bb)
        s._bb = tuple(bb)
        s._keep.append(self)
        return s

    def update_viewer(self, viewer_obj, budget_s=0.03, budget_ns=None):
        """sdfv_viewer_update_program: SDFViewer::update over this editor by whole passes; returns the iterations consumed."""
        n = C.c_size_t()
        ns = int(budget_s * 1e9) if budget_ns is None else int(budget_ns)
        rc = self._lib.sdfv_viewer_update_program(viewer_obj.h, self.h, ns, C.byref(n))
        if rc != 0:
            raise SdfvError(rc, self._lib.sdfv_viewer_last_error(viewer_obj.h).decode())
        return n.value

    def close(self):
        if self.h:
            self._lib.sdfv_program_editor_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
