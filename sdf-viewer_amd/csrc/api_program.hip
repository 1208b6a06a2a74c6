// api_program.hip -- SDF programs: the handle, what sdfv_program_create rejects, and the entry points that evaluate one.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "api_internal.h"
#include "program_cast_kernels.h"
#include "program_handle.h"
#include "program_kernels.h"
#include "program_march_kernels.h"
#include "program_mesh_kernels.h"

using namespace sdfv;

namespace {

const char* program_op_name(uint32_t op) {
    static const char* const names[] = {"?", "SPHERE", "CUBE", "BOX", "CYLINDER", "TORUS", "PLANE", "PUSH_AFFINE", "PUSH_SCALE",
                                        "POP", "POP_SCALE", "UNION", "INTERSECT", "SUBTRACT", "SMOOTH_UNION", "SMOOTH_SUBTRACT",
                                        "ROUND", "SHELL", "MATERIAL"};
    return op <= SDFV_OP_MATERIAL ? names[op] : "?";
}

// Everything sdfgrid.h promises sdfv_program_create rejects.  The stack depths are static: one walk decides them.
int validate_program(const sdfv_prog_op* ops, size_t n, const float bb[6]) {
    if (!ops || !bb) return set_error(SDFV_ERR_INVALID_ARGUMENT, "ops or bb is NULL");
    if (n == 0 || n > SDFV_PROGRAM_MAX_OPS)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "a program has 1 .. %d instructions, not %zu", SDFV_PROGRAM_MAX_OPS, n);
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(bb[i]) || !std::isfinite(bb[3 + i]) || !(bb[3 + i] > bb[i]))
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "degenerate bounding box on axis %d: [%g, %g]", i, bb[i], bb[3 + i]);
    uint32_t values = 0, frames = 0;
    bool scale_frame[SDFV_PROGRAM_MAX_FRAMES] = {};
    for (size_t i = 0; i < n; ++i) {
        const sdfv_prog_op& o = ops[i];
        if (o.op < SDFV_OP_SPHERE || o.op > SDFV_OP_MATERIAL)
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "op %zu: unknown opcode %u", i, o.op);
        const char* name = program_op_name(o.op);
        if (o.reserved[0] | o.reserved[1] | o.reserved[2])
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "op %zu (%s): reserved words must be 0", i, name);
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(o.a[k])) return set_error(SDFV_ERR_INVALID_ARGUMENT, "op %zu (%s): operand %d is not finite", i, name, k);
        // values the instruction takes and leaves, by opcode: the shapes, the frame pushes and POP, POP_SCALE, the five binary
        // operators, ROUND and SHELL, MATERIAL
        static const uint8_t kPops[] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 2, 2, 2, 2, 1, 1, 0};
        static const uint8_t kPushes[] = {0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0};
        static_assert(SDFV_OP_POP_SCALE == 10 && SDFV_OP_UNION == 11 && SDFV_OP_ROUND == 16 && SDFV_OP_MATERIAL == 18, "");
        const uint32_t pops = kPops[o.op], pushes = kPushes[o.op];
        switch (o.op) {
            case SDFV_OP_SMOOTH_UNION: case SDFV_OP_SMOOTH_SUBTRACT:
                if (!(o.a[0] > 0.0f)) return set_error(SDFV_ERR_INVALID_ARGUMENT, "op %zu (%s): k = %g must be > 0", i, name, o.a[0]);
                break;
            case SDFV_OP_PUSH_AFFINE: case SDFV_OP_PUSH_SCALE:
                if (o.op == SDFV_OP_PUSH_SCALE && (!(o.a[0] > 0.0f) || !(o.a[1] > 0.0f)))
                    return set_error(SDFV_ERR_INVALID_ARGUMENT, "op %zu (%s): s = %g and inv_s = %g must be > 0", i, name, o.a[0], o.a[1]);
                if (frames == SDFV_PROGRAM_MAX_FRAMES)
                    return set_error(SDFV_ERR_INVALID_ARGUMENT, "op %zu (%s): frame stack overflow (more than %d open frames)", i, name,
                                SDFV_PROGRAM_MAX_FRAMES);
                scale_frame[frames++] = o.op == SDFV_OP_PUSH_SCALE;
                break;
            case SDFV_OP_POP: case SDFV_OP_POP_SCALE: {
                const bool scale = o.op == SDFV_OP_POP_SCALE;
                if (scale && !(o.a[0] > 0.0f)) return set_error(SDFV_ERR_INVALID_ARGUMENT, "op %zu (%s): s = %g must be > 0", i, name, o.a[0]);
                if (frames == 0) return set_error(SDFV_ERR_INVALID_ARGUMENT, "op %zu (%s): frame stack underflow (no open frame)", i, name);
                if (scale_frame[frames - 1] != scale)
                    return set_error(SDFV_ERR_INVALID_ARGUMENT, "op %zu (%s): closes a %s", i, name, scale ? "PUSH_AFFINE" : "PUSH_SCALE");
                --frames;
                break;
            }
            default:  // nothing but its values to check
                break;
        }
        if (values < pops)
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "op %zu (%s): value stack underflow (needs %u, has %u)", i, name, pops, values);
        values = values - pops + pushes;
        if (values > SDFV_PROGRAM_MAX_VALUES)
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "op %zu (%s): value stack overflow (more than %d values)", i, name,
                        SDFV_PROGRAM_MAX_VALUES);
    }
    if (frames != 0) return set_error(SDFV_ERR_INVALID_ARGUMENT, "op %zu: the program ends with %u open frame(s)", n - 1, frames);
    if (values != 1) return set_error(SDFV_ERR_INVALID_ARGUMENT, "op %zu: the program ends with %u values, not 1", n - 1, values);
    return SDFV_OK;
}

}  // namespace

int sdfv::program_on_device(const sdfv_program* cp, const sdfv_prog_op** out, uint32_t* n_ops, const float** bb) {
    sdfv_program* p = const_cast<sdfv_program*>(cp);
    *n_ops = (uint32_t)p->ops.size();
    if (bb) *bb = p->bb;
    const int dev = current_device();
    if (dev < 0) return set_error(SDFV_ERR_NO_DEVICE, "no current HIP device");
    std::lock_guard<std::mutex> lock(p->mu);
    for (const auto& c : p->device_copies)
        if (c.first == dev) {
            *out = static_cast<const sdfv_prog_op*>(c.second);
            return SDFV_OK;
        }
    void* d = nullptr;
    const size_t bytes = p->ops.size() * sizeof(sdfv_prog_op);
    try {
        p->device_copies.reserve(p->device_copies.size() + 1);  // (so that recording the copy below cannot fail)
    } catch (const std::bad_alloc&) {
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "out of host memory");
    }
    SDFV_HIP(hipMalloc(&d, bytes));
    const hipError_t e = hipMemcpy(d, p->ops.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(e, "hipMemcpy of the program");
    }
    p->device_copies.emplace_back(dev, d);
    *out = static_cast<const sdfv_prog_op*>(d);
    return SDFV_OK;
}

// The prologue of the entry points that run a program over n elements (`names`: the buffers in the alignment message); n == 0 leaves *ops NULL.
static int program_elements_ready(const sdfv_program* p, const void* in, const void* out, size_t n, const char* names,
                                  const sdfv_prog_op** ops, uint32_t* n_ops, sdfv::ProgramKernels* compiled) {
    if (!p) return set_error(SDFV_ERR_INVALID_ARGUMENT, "program is NULL");
    if (int rc = check_point_buffers(in, out, n)) return rc;
    if (int rc = check_word_aligned(names, in, out)) return rc;
    if (int rc = need_device()) return rc;
    if (n == 0) return SDFV_OK;
    // (a compiled handle on the wrong device is refused before its device copy is made)
    if (int rc = program_compiled_kernels(p, SDFV_COMPILE_MESH, compiled)) return rc;
    return program_on_device(p, ops, n_ops);
}

#pragma GCC visibility push(default)
extern "C" {

int sdfv_program_create(const sdfv_prog_op* ops, size_t n, const float bb[6], sdfv_program** out) {
    if (!out) return set_error(SDFV_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (int rc = validate_program(ops, n, bb)) return rc;
    try {  // nothing crosses the C boundary, and a copy that fails takes the half-made handle with it
        std::unique_ptr<sdfv_program> p(new sdfv_program);
        p->ops.assign(ops, ops + n);
        memcpy(p->bb, bb, sizeof(p->bb));
        *out = p.release();
    } catch (const std::bad_alloc&) {
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "out of host memory");  // (the status sdfv_slab_comm_create reports it with)
    }
    return SDFV_OK;
}

void sdfv_program_free(sdfv_program* p) {
    if (!p) return;
    for (const auto& c : p->device_copies) (void)hipFree(c.second);
    program_release_compiled(p);
    delete p;
}

int sdfv_program_ops(const sdfv_program* p, const sdfv_prog_op** ops, size_t* n, float bb[6]) {
    if (!p) return set_error(SDFV_ERR_INVALID_ARGUMENT, "program is NULL");
    if (ops) *ops = p->ops.data();
    if (n) *n = p->ops.size();
    if (bb) memcpy(bb, p->bb, sizeof(p->bb));
    return SDFV_OK;
}

int sdfv_program_sample_points(const sdfv_program* p, const float* points, size_t n, int distance_only, sdfv_sample* out,
                               void* stream) {
    const sdfv_prog_op* dev_ops = nullptr;
    uint32_t n_ops = 0;
    if (!p) return set_error(SDFV_ERR_INVALID_ARGUMENT, "program is NULL");
    if (int rc = check_point_buffers(points, out, n)) return rc;
    if (int rc = check_word_aligned("points and out", points, out)) return rc;
    if (int rc = need_device()) return rc;
    if (n == 0) return SDFV_OK;
    sdfv::ProgramKernels compiled;  // (a compiled handle on the wrong device is refused before its device copy is made)
    if (int rc = program_compiled_kernels(p, SDFV_COMPILE_POINTS, &compiled)) return rc;
    if (int rc = program_on_device(p, &dev_ops, &n_ops)) return rc;
    SDFV_HIP_RETURN(sdfv::launch_program_sample_points(dev_ops, n_ops, points, n, distance_only != 0, out, compiled,
                                                (hipStream_t)stream));
}

int sdfv_program_normal_points(const sdfv_program* p, const float* points, size_t n, float eps, float* out, void* stream) {
    const sdfv_prog_op* dev_ops = nullptr;
    uint32_t n_ops = 0;
    sdfv::ProgramKernels compiled;
    if (int rc = program_elements_ready(p, points, out, n, "points and out", &dev_ops, &n_ops, &compiled)) return rc;
    if (!dev_ops) return SDFV_OK;
    SDFV_HIP_RETURN(sdfv::launch_program_normal_points(dev_ops, n_ops, points, n, eps, out, compiled, (hipStream_t)stream));
}

int sdfv_program_mesh_postproc(const sdfv_program* p, sdfv_vertex* vertices, size_t n, void* stream) {
    const sdfv_prog_op* dev_ops = nullptr;
    uint32_t n_ops = 0;
    sdfv::ProgramKernels compiled;
    if (int rc = program_elements_ready(p, vertices, vertices, n, "vertices", &dev_ops, &n_ops, &compiled)) return rc;
    if (!dev_ops) return SDFV_OK;
    SDFV_HIP_RETURN(sdfv::launch_program_mesh_postproc(dev_ops, n_ops, vertices, n, compiled, (hipStream_t)stream));
}

int sdfv_program_raymarch_check(const sdfv_program_march_desc* desc, sdfv_program_march_desc* checked, float* normal_h) {
    sdfv_program_march_desc d;
    constexpr size_t first_version = offsetof(sdfv_program_march_desc, rgba8) + sizeof(uint32_t*);
    if (int rc = read_sized_desc(desc, first_version, "sdfv_program_march_desc", d)) return rc;
    if (d.reserved != 0) return set_error(SDFV_ERR_INVALID_ARGUMENT, "sdfv_program_march_desc: reserved must be 0");
    if (!d.program) return set_error(SDFV_ERR_INVALID_ARGUMENT, "sdfv_program_march_desc.program is NULL");
    if (!d.rp) return set_error(SDFV_ERR_INVALID_ARGUMENT, "sdfv_program_march_desc.rp is NULL");
    if (!d.rgba && !d.rgba8) return set_error(SDFV_ERR_INVALID_ARGUMENT, "no colour output: rgba and rgba8 are both NULL");
    if (int rc = check_lights(d.rp)) return rc;
    if ((uintptr_t)d.rgba & 15) return set_error(SDFV_ERR_INVALID_ARGUMENT, "rgba must be 16-byte aligned");
    if (int rc = check_word_aligned("depth, aux and rgba8", d.depth, d.aux, d.rgba8)) return rc;
    if (d.n_cameras && !d.cameras) return set_error(SDFV_ERR_INVALID_ARGUMENT, "cameras is NULL");
    if (d.y0 > d.y1 || d.y1 > d.height) return set_error(SDFV_ERR_INVALID_ARGUMENT, "rows [%u,%u) outside height %u", d.y0, d.y1, d.height);
    if (!(d.normal_h >= 0.0f) || !std::isfinite(d.normal_h))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "normal_h = %g: a distance > 0, or 0 to derive it from rp->tex_size", d.normal_h);
    const float h = sdfv::march::normal_tap_distance(*d.rp, d.normal_h);
    if (!(h > 0.0f) || !std::isfinite(h))
        return set_error(SDFV_ERR_INVALID_ARGUMENT,
                    "normal_h is 0 and rp->tex_size = %u x %u x %u with lod_dist_between_samples = %g gives no tap distance: set "
                    "normal_h, or tex_size to the grid whose normals this render is compared with",
                    d.rp->tex_size[0], d.rp->tex_size[1], d.rp->tex_size[2], d.rp->lod_dist_between_samples);
    if (checked) *checked = d;
    if (normal_h) *normal_h = h;
    return SDFV_OK;
}

int sdfv_program_raymarch(const sdfv_program_march_desc* desc, void* stream) {
    sdfv_program_march_desc d;
    float h = 0.0f;
    if (int rc = sdfv_program_raymarch_check(desc, &d, &h)) return rc;
    if (int rc = need_device()) return rc;
    if (d.n_cameras == 0 || d.width == 0 || d.y0 == d.y1) return SDFV_OK;
    sdfv::ProgramMarchArgs a;
    memset(&a, 0, sizeof(a));
    sdfv::ProgramKernels compiled;
    if (int rc = program_compiled_kernels(d.program, SDFV_COMPILE_MARCH, &compiled)) return rc;
    if (int rc = program_on_device(d.program, &a.f.ops, &a.f.n_ops)) return rc;
    a.f.width = d.width;
    a.f.height = d.height;
    a.f.normal_h = h;
    a.f.air_dist = air_dist();
    a.f.srgb_round = g_options.ext_srgb_quant;
    a.f.rp = *d.rp;
    a.y0 = d.y0;
    a.y1 = d.y1;
    const uint64_t pixels_per_cam = (uint64_t)(d.y1 - d.y0) * d.width;
    for (uint32_t c0 = 0; c0 < d.n_cameras; c0 += sdfv::kProgramMarchCameras) {  // the cameras ride in the kernel arguments
        const uint32_t nc = d.n_cameras - c0 < sdfv::kProgramMarchCameras ? d.n_cameras - c0 : sdfv::kProgramMarchCameras;
        a.n_cameras = nc;
        memcpy(a.cameras, d.cameras + c0, nc * sizeof(sdfv_camera));
        point_outputs_at(a, pixels_per_cam, c0, d.rgba, d.rgba8, d.aux, d.depth);
        SDFV_HIP(sdfv::launch_program_march(a, compiled, (hipStream_t)stream));
    }
    return SDFV_OK;
}

int sdfv_program_raycast_check(const sdfv_program_cast_desc* desc, sdfv_program_cast_desc* checked) {
    sdfv_program_cast_desc d;
    if (int rc = read_sized_desc(desc, sizeof(sdfv_program_cast_desc), "sdfv_program_cast_desc", d)) return rc;
    if (d.reserved != 0) return set_error(SDFV_ERR_INVALID_ARGUMENT, "sdfv_program_cast_desc: reserved must be 0");
    if (!d.program) return set_error(SDFV_ERR_INVALID_ARGUMENT, "sdfv_program_cast_desc.program is NULL");
    if ((d.bb_min == nullptr) != (d.bb_max == nullptr))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "bounding box: bb_min and bb_max are both given or both NULL (the program's box)");
    for (int i = 0; d.bb_min && i < 3; ++i)
        if (!std::isfinite(d.bb_min[i]) || !std::isfinite(d.bb_max[i]) || !(d.bb_max[i] > d.bb_min[i]))
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "degenerate bounding box on axis %d: [%g, %g]", i, d.bb_min[i], d.bb_max[i]);
    if (int rc = check_point_buffers(d.rays, d.hits, d.n)) return rc;
    if (int rc = check_word_aligned("rays and hits", d.rays, d.hits)) return rc;
    if (d.flags & ~(SDFV_CAST_NORMALS | SDFV_CAST_MATERIALS)) return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", d.flags);
    if (d.max_steps > 4096) return set_error(SDFV_ERR_INVALID_ARGUMENT, "max_steps %u is outside [1, 4096] (0 = 256)", d.max_steps);
    if (!(d.hit_eps >= 0.0f) || !std::isfinite(d.hit_eps))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "hit_eps = %g: a distance > 0, or 0 for 1e-5", d.hit_eps);
    if (!(d.normal_eps >= 0.0f) || !std::isfinite(d.normal_eps))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "normal_eps = %g: a distance > 0, or 0 for 0.001", d.normal_eps);
    if (d.max_steps == 0) d.max_steps = 256;
    if (d.hit_eps == 0.0f) d.hit_eps = 1e-5f;
    if (d.normal_eps == 0.0f) d.normal_eps = 0.001f;
    if (checked) *checked = d;
    return SDFV_OK;
}

int sdfv_program_raycast(const sdfv_program_cast_desc* desc, void* stream) {
    sdfv_program_cast_desc d;
    if (int rc = sdfv_program_raycast_check(desc, &d)) return rc;
    if (int rc = need_device()) return rc;
    if (d.n == 0) return SDFV_OK;
    sdfv::ProgramCastArgs a;
    memset(&a, 0, sizeof(a));
    const float* bb = nullptr;
    if (int rc = program_on_device(d.program, &a.c.ops, &a.c.n_ops, &bb)) return rc;
    for (int i = 0; i < 3; ++i) {  // (copied: the caller's box is free again when the call returns)
        a.c.bounds_min[i] = d.bb_min ? d.bb_min[i] : bb[i];
        a.c.bounds_max[i] = d.bb_max ? d.bb_max[i] : bb[3 + i];
    }
    a.c.flags = d.flags;
    a.c.max_steps = d.max_steps;
    a.c.hit_eps = d.hit_eps;
    a.c.normal_eps = d.normal_eps;
    a.rays = d.rays;
    a.hits = d.hits;
    a.n = d.n;
    a.rays16 = ((uintptr_t)d.rays & 15) == 0;
    a.hits16 = ((uintptr_t)d.hits & 15) == 0;
    SDFV_HIP_RETURN(sdfv::launch_program_cast(a, (hipStream_t)stream));
}

}  // extern "C"
#pragma GCC visibility pop
