// program_compile.hip -- sdfv_program_compile: one SDF program as gfx kernels of its own, built at run time.
//
// The interpreter (program_eval.h) pays per instruction for a scalar fetch, a dispatch and the stack's register shifts.  With
// the instructions as compile-time constants all three fold away: the switch of prog::step() picks its case at compile time,
// the shifts become register renaming, nothing is fetched.  So this file writes, per program, a translation unit that
//  * holds the instructions as a constexpr sdfv_prog_op array (operands as their 32-bit patterns, never as decimal text),
//  * defines ONE evaluator that calls prog::step() once per instruction on a constant (with a register fence between steps:
//    DESIGN.md 3.6.2), and
//  * defines it as the two evaluator expressions (SDFV_EVAL_ONCE, SDFV_EVAL_LOOPED) of the kernel definitions in
//    program_device.h and, for SDFV_COMPILE_MESH, program_mesh_device.h -- the definitions the library's own kernels are made
//    from -- and invokes one definition per kernel the compiled routes launch (the rows of SDFV_PROGRAM_KERNELS,
//    program_kernels.h), naming it sdfprogc_<stem>, and nothing for a route not asked for,
// and hands it to the run-time compiler (libhiprtc, bound with dlopen on the first compile like RCCL in slab_comm.hip)
// together with the project's headers, embedded in this library as strings by the Makefile (gen_embed_headers.c), and the
// Makefile's code-affecting flags (SDFV_KERNEL_FLAGS).  Same text, same compiler, same flags as hipcc's build of the
// interpreter's kernels: the results are the same bits.  The materials of a result are still fetched through resolve() over
// the handle's device copy of the instructions, as in the interpreter's kernels.
//
// The run-time compiler has its own built-in HIP runtime header and none of libc's: <hip/hip_runtime.h>, <stdint.h>,
// <stddef.h>, <math.h> and <type_traits> are stand-ins below (empty, typedefs, the one trait kernel_common.h uses).
#include <dlfcn.h>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>

#include "program_handle.h"

#ifndef SDFV_KERNEL_FLAGS
#error "SDFV_KERNEL_FLAGS: the Makefile passes the code-affecting flags of the kernels (one string)"
#endif

namespace {

struct EmbeddedHeader {
    const char* name;
    const char* text;
};
#include "build/embedded_headers.inc"

const EmbeddedHeader kStandIns[] = {
    {"hip/hip_runtime.h", "// stand-in: the run-time compiler brings its own runtime header\n"},
    {"stddef.h", "// stand-in: size_t is built in\n"},
    {"math.h", "// stand-in: the device math functions are built in\n"},
    {"stdint.h",
     "#pragma once\n"
     "typedef unsigned char uint8_t;\ntypedef unsigned short uint16_t;\ntypedef unsigned int uint32_t;\ntypedef unsigned long uint64_t;\n"
     "typedef signed char int8_t;\ntypedef short int16_t;\ntypedef int int32_t;\ntypedef long int64_t;\ntypedef unsigned long uintptr_t;\n"},
    {"type_traits",
     "#pragma once\n"
     "namespace std {\n"
     "template <bool B, typename T, typename F> struct conditional { typedef T type; };\n"
     "template <typename T, typename F> struct conditional<false, T, F> { typedef F type; };\n"
     "template <bool B, typename T, typename F> using conditional_t = typename conditional<B, T, F>::type;\n"
     "}\n"},
};

// The specialised kernels by sdfv::ProgramKernel: each row of SDFV_PROGRAM_KERNELS (program_kernels.h) as its name stem, the
// name a handle's code object has it under, and its route.
const struct {
    const char* stem;
    const char* name;
    uint32_t route;
} kKernels[] = {
#define SDFV_X(index, stem, route) {#stem, "sdfprogc_" #stem, route},
    SDFV_PROGRAM_KERNELS(SDFV_X)
#undef SDFV_X
};
static_assert(sizeof(kKernels) / sizeof(kKernels[0]) == sdfv::kProgramKernels, "one row per kernel");
uint32_t route_of(int kernel) { return kKernels[kernel].route; }
// (bit 8 is no route: it stays among the unknown bits)
constexpr uint32_t kAllRoutes = SDFV_COMPILE_FILL | SDFV_COMPILE_POINTS | SDFV_COMPILE_MARCH | SDFV_COMPILE_MESH;

// ---- the run-time compiler: the slice of hiprtc.h this file needs ----
struct Hiprtc {
    void* handle = nullptr;
    int (*CreateProgram)(void**, const char*, const char*, int, const char* const*, const char* const*) = nullptr;
    int (*CompileProgram)(void*, int, const char* const*) = nullptr;
    int (*GetProgramLogSize)(void*, size_t*) = nullptr;
    int (*GetProgramLog)(void*, char*) = nullptr;
    int (*GetCodeSize)(void*, size_t*) = nullptr;
    int (*GetCode)(void*, char*) = nullptr;
    int (*DestroyProgram)(void**) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    const char* load_error = nullptr;
};

template <typename F>
bool bind(void* h, const char* name, F& fn) {
    fn = reinterpret_cast<F>(dlsym(h, name));
    return fn != nullptr;
}

const Hiprtc* hiprtc() {
    static const Hiprtc lib = [] {
        Hiprtc r;
        static std::string message;  // (this initialiser runs once per process)
        const char* path = sdfv::claim_hiprtc_library_path();  // (from here on SDFV_OPT_HIPRTC_LIBRARY is refused)
        if (path && path[0]) {  // SDFV_OPT_HIPRTC_LIBRARY: this file and nothing else
            r.handle = dlopen(path, RTLD_NOW | RTLD_LOCAL);
            if (!r.handle) {
                const char* why = dlerror();
                message = std::string("the library named by SDFV_OPT_HIPRTC_LIBRARY could not be loaded: ") + (why ? why : "dlopen failed");
                r.load_error = message.c_str();
                return r;
            }
        } else {
            // The run-time compiler of the toolchain that built this library first (SDFV_HIPRTC_DEFAULT, from the Makefile: by
            // path, because a process may already hold another libhiprtc.so -- PyTorch bundles one -- and a load by name
            // would hand that one back: another compiler than the interpreter's kernels were built with); then by name.
#ifdef SDFV_HIPRTC_DEFAULT
            r.handle = dlopen(SDFV_HIPRTC_DEFAULT, RTLD_NOW | RTLD_LOCAL);
#endif
            if (!r.handle) r.handle = dlopen("libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
        }
        if (!r.handle) {
            r.load_error = "libhiprtc.so not found (SDFV_OPT_HIPRTC_LIBRARY names another)";
            return r;
        }
        bool ok = true;
        ok = bind(r.handle, "hiprtcCreateProgram", r.CreateProgram) && ok;
        ok = bind(r.handle, "hiprtcCompileProgram", r.CompileProgram) && ok;
        ok = bind(r.handle, "hiprtcGetProgramLogSize", r.GetProgramLogSize) && ok;
        ok = bind(r.handle, "hiprtcGetProgramLog", r.GetProgramLog) && ok;
        ok = bind(r.handle, "hiprtcGetCodeSize", r.GetCodeSize) && ok;
        ok = bind(r.handle, "hiprtcGetCode", r.GetCode) && ok;
        ok = bind(r.handle, "hiprtcDestroyProgram", r.DestroyProgram) && ok;
        ok = bind(r.handle, "hiprtcGetErrorString", r.GetErrorString) && ok;
        if (!ok) r.load_error = "the run-time compiler library lacks a hiprtc entry point";
        return r;
    }();
    return &lib;
}

std::mutex g_compile_mutex;  // compilations are serialised

// ---- the generated translation unit ----
void append(std::string& s, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void append(std::string& s, const char* fmt, ...) {
    char line[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof(line), fmt, ap);
    va_end(ap);
    s += line;
}

std::string generate_source(const std::vector<sdfv_prog_op>& ops, uint32_t routes) {
    std::string s;
    s.reserve(ops.size() * 260 + 4096);
    s += "// generated by sdfv_program_compile: one SDF program, its instructions as constants\n"
         "#include \"program_device.h\"\n";
    if (routes & SDFV_COMPILE_MESH) s += "#include \"program_mesh_device.h\"\n";
    s += "\nnamespace {\n"
         "constexpr float f32(uint32_t bits) { return __builtin_bit_cast(float, bits); }\n";
    append(s, "constexpr uint32_t kOpCount = %zuu;\n", ops.size());
    s += "constexpr sdfv_prog_op kOps[kOpCount] = {\n";
    for (const sdfv_prog_op& o : ops) {
        append(s, "    {%uu, {0u, 0u, 0u}, {", o.op);
        for (int k = 0; k < 12; ++k) {
            uint32_t bits;
            memcpy(&bits, &o.a[k], 4);
            append(s, "f32(0x%08xu)%s", bits, k < 11 ? ", " : "}},\n");
        }
    }
    s += "};\n"
         "// The program at one point: prog::run() of program_eval.h with the loop unrolled and every instruction a constant.\n"
         "// Between two steps the machine's registers pass through an empty asm: what is live there is the machine and nothing\n"
         "// else, as in the interpreter -- unrolled into one block, long programs were otherwise rearranged (subexpressions shared\n"
         "// across dozens of steps, primitives vectorised in pairs) past the interpreter's registers (DESIGN.md 3.6.2).\n"
         "#define SDFV_V(f) \"+v\"(s.f)\n"
         "#define SDFV_FENCE \\\n"
         "    asm volatile(\"\" : SDFV_V(x), SDFV_V(y), SDFV_V(z), SDFV_V(f0x), SDFV_V(f0y), SDFV_V(f0z), SDFV_V(f1x), SDFV_V(f1y), SDFV_V(f1z), \\\n"
         "                 SDFV_V(f2x), SDFV_V(f2y), SDFV_V(f2z), SDFV_V(f3x), SDFV_V(f3y), SDFV_V(f3z)); \\\n"
         "    asm volatile(\"\" : SDFV_V(v0.d), SDFV_V(v1.d), SDFV_V(v2.d), SDFV_V(v3.d), SDFV_V(v4.d), SDFV_V(v5.d), SDFV_V(v6.d), SDFV_V(v7.d), \\\n"
         "                 SDFV_V(v0.m), SDFV_V(v1.m), SDFV_V(v2.m), SDFV_V(v3.m), SDFV_V(v4.m), SDFV_V(v5.m), SDFV_V(v6.m), SDFV_V(v7.m));\n"
         "// One instruction with its first N operands (the ones its opcode reads).  LOOPED = the evaluator sits in a loop (the\n"
         "// march): an operand that is no inline constant lives in an SGPR, the compiler hoists every such constant out of the loop,\n"
         "// and a long program's hundred of them, held across the loop, crowd the kernel's own long-lived scalars out (spilled to\n"
         "// VGPR lanes).  There each operand is its bit pattern OR a zero the compiler cannot see through, made anew per step:\n"
         "// one scalar instruction per operand, the same bits, nothing to hoist.\n"
         "template <bool LOOPED, uint32_t PC, int N>\n"
         "__device__ __forceinline__ void compiled_step(sdfv::prog::Machine& s) {\n"
         "    SDFV_FENCE\n"
         "    if constexpr (LOOPED && N > 0) {\n"
         "        sdfv_prog_op o = kOps[PC];\n"
         "        uint32_t zero = 0u;\n"
         "        asm volatile(\"\" : \"+s\"(zero));\n"
         "#pragma unroll\n"
         "        for (int k = 0; k < N; ++k) o.a[k] = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, kOps[PC].a[k]) | zero);\n"
         "        sdfv::prog::step(s, o, PC);\n"
         "    } else {\n"
         "        sdfv::prog::step(s, kOps[PC], PC);\n"
         "    }\n"
         "}\n"
         "template <bool LOOPED>\n"
         "struct Compiled {\n"
         "    __device__ __forceinline__ sdfv::prog::Value operator()(float px, float py, float pz) const {\n"
         "        sdfv::prog::Machine s;\n"
         "        sdfv::prog::start(s, px, py, pz);\n";
    // operands an opcode reads (program_eval.h step(); MATERIAL's are read by resolve(), from the device copy)
    static const int kOperands[SDFV_OP_MATERIAL + 1] = {0, 1, 1, 3, 2, 2, 4, 12, 2, 0, 1, 0, 0, 0, 1, 1, 1, 1, 0};
    for (size_t pc = 0; pc < ops.size(); ++pc) append(s, "        compiled_step<LOOPED, %zuu, %d>(s);\n", pc, kOperands[ops[pc].op]);
    s += "        return s.v0;\n"
         "    }\n"
         "};\n"
         "}  // namespace\n\n"
         "using namespace sdfv;\n"
         "// the kernels of the routes asked for: the definitions the library's sdfprog_* twins are made from, over this program\n"
         "#define SDFV_EVAL_ONCE(ops, n_ops) Compiled<false>{}\n"
         "#define SDFV_EVAL_LOOPED(ops, n_ops) Compiled<true>{}\n";
    for (int k = 0; k < sdfv::kProgramKernels; ++k)
        if (routes & route_of(k)) append(s, "SDFV_PROGRAM_KERNEL_%s(%s)\n", kKernels[k].stem, kKernels[k].name);
    return s;
}

// The processor of a gcnArchName: "gfx950:sramecc+:xnack-" -> "gfx950".
std::string processor_of(const char* gcn_arch_name) {
    const char* colon = strchr(gcn_arch_name, ':');
    return colon ? std::string(gcn_arch_name, colon) : std::string(gcn_arch_name);
}
int device_processor(int dev, std::string& out) {
    hipDeviceProp_t prop;
    SDFV_HIP(hipGetDeviceProperties(&prop, dev));
    out = processor_of(prop.gcnArchName);
    return SDFV_OK;
}

// source -> code object for `arch`; the compiler's log (its start) into the error message on failure
int compile_source(const std::string& source, const std::string& arch, std::vector<char>& code) {
    std::lock_guard<std::mutex> lock(g_compile_mutex);
    const Hiprtc* rtc = hiprtc();
    if (rtc->load_error) return sdfv::set_error(SDFV_ERR_COMPILE, "run-time compiler: %s", rtc->load_error);
    constexpr int n_embedded = (int)(sizeof(kEmbeddedHeaders) / sizeof(kEmbeddedHeaders[0]));
    constexpr int n_stand_ins = (int)(sizeof(kStandIns) / sizeof(kStandIns[0]));
    const char* names[n_embedded + n_stand_ins];
    const char* texts[n_embedded + n_stand_ins];
    for (int i = 0; i < n_embedded; ++i) names[i] = kEmbeddedHeaders[i].name, texts[i] = kEmbeddedHeaders[i].text;
    for (int i = 0; i < n_stand_ins; ++i) names[n_embedded + i] = kStandIns[i].name, texts[n_embedded + i] = kStandIns[i].text;
    void* prog = nullptr;
    int r = rtc->CreateProgram(&prog, source.c_str(), "sdfv_program.hip", n_embedded + n_stand_ins, texts, names);
    if (r != 0) return sdfv::set_error(SDFV_ERR_COMPILE, "hiprtcCreateProgram: %s", rtc->GetErrorString(r));
    // the Makefile's code-affecting flags, one option per word, and the architecture
    std::vector<std::string> words;
    words.push_back("--offload-arch=" + arch);
    for (const char* p = SDFV_KERNEL_FLAGS; *p;) {
        while (*p == ' ') ++p;
        const char* e = p;
        while (*e && *e != ' ') ++e;
        if (e > p) words.emplace_back(p, e);
        p = e;
    }
    std::vector<const char*> options;
    for (const std::string& w : words) options.push_back(w.c_str());
    r = rtc->CompileProgram(prog, (int)options.size(), options.data());
    int rc = SDFV_OK;
    if (r != 0) {
        size_t n = 0;
        std::string log;
        if (rtc->GetProgramLogSize(prog, &n) == 0 && n > 1) {
            log.resize(n);
            if (rtc->GetProgramLog(prog, &log[0]) != 0) log.clear();
        }
        rc = sdfv::set_error(SDFV_ERR_COMPILE, "compiling for %s failed (%s): %.380s", arch.c_str(), rtc->GetErrorString(r),
                             log.empty() ? "no log" : log.c_str());
    } else {
        size_t n = 0;
        r = rtc->GetCodeSize(prog, &n);
        if (r == 0 && n > 0) {
            code.resize(n);
            r = rtc->GetCode(prog, code.data());
        }
        if (r != 0 || n == 0) rc = sdfv::set_error(SDFV_ERR_COMPILE, "hiprtcGetCode: %s", r ? rtc->GetErrorString(r) : "an empty code object");
    }
    (void)rtc->DestroyProgram(&prog);
    return rc;
}

// The handle's module on device `dev` (loaded on the first use); p->mu is held by the caller.
int load_on_device(sdfv_program* p, int dev, const sdfv::CompiledProgram::Loaded** out) {
    sdfv::CompiledProgram* c = p->compiled;
    for (const auto* l : c->loaded)
        if (l->device == dev) {
            *out = l;
            return SDFV_OK;
        }
    std::unique_ptr<sdfv::CompiledProgram::Loaded> l(new sdfv::CompiledProgram::Loaded);
    memset(l.get(), 0, sizeof(*l));
    l->device = dev;
    c->loaded.reserve(c->loaded.size() + 1);
    SDFV_HIP(hipModuleLoadData(&l->module, c->code.data()));
    for (int k = 0; k < sdfv::kProgramKernels; ++k) {
        if (!(c->routes & route_of(k))) continue;
        const hipError_t e = hipModuleGetFunction(&l->fn[k], l->module, kKernels[k].name);
        if (e != hipSuccess) {
            (void)hipModuleUnload(l->module);
            return sdfv::hip_fail(e, kKernels[k].name);
        }
    }
    *out = l.get();
    c->loaded.push_back(l.release());
    return SDFV_OK;
}

}  // namespace

int sdfv::program_compiled_kernels(const sdfv_program* cp, uint32_t route, ProgramKernels* k) {
    sdfv_program* p = const_cast<sdfv_program*>(cp);
    CompiledProgram* c = p->compiled;
    if (!c || !(c->routes & route)) return SDFV_OK;
    const int dev = current_device();
    if (dev < 0) return set_error(SDFV_ERR_NO_DEVICE, "no current HIP device");
    std::lock_guard<std::mutex> lock(p->mu);
    const CompiledProgram::Loaded* l = nullptr;
    for (const auto* have : c->loaded)
        if (have->device == dev) l = have;
    if (!l) {
        std::string here;
        if (int rc = device_processor(dev, here)) return rc;
        if (here != c->arch)
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "the program was compiled for %s and the current device %d is %s: compile it for this device, or use a plain handle",
                             c->arch.c_str(), dev, here.c_str());
        if (int rc = load_on_device(p, dev, &l)) return rc;
    }
    k->fn = l->fn;
    k->launches = &c->launches;
    return SDFV_OK;
}

void sdfv::program_release_compiled(sdfv_program* p) {
    if (!p->compiled) return;
    for (auto* l : p->compiled->loaded) {
        (void)hipModuleUnload(l->module);
        delete l;
    }
    delete p->compiled;
    p->compiled = nullptr;
}

using namespace sdfv;
#pragma GCC visibility push(default)
extern "C" {

int sdfv_program_compile(const sdfv_program* p, uint32_t routes, const char* arch, sdfv_program** out) {
    if (!out) return set_error(SDFV_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (!p) return set_error(SDFV_ERR_INVALID_ARGUMENT, "program is NULL");
    if (routes == 0) return set_error(SDFV_ERR_INVALID_ARGUMENT, "routes is 0: name at least one of SDFV_COMPILE_FILL, _POINTS, _MARCH, _MESH");
    if (routes & ~kAllRoutes) return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown route bits 0x%x", routes & ~kAllRoutes);
    if (arch && (!arch[0] || strlen(arch) >= sizeof(sdfv_compiled_info::arch) || strchr(arch, ' ')))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "arch is not a processor name such as \"gfx950\"");
    const int dev = current_device();
    std::string here;  // the current device's processor, if there is a device
    if (dev >= 0 && device_processor(dev, here) != SDFV_OK) here.clear();
    if (!arch && here.empty()) return set_error(SDFV_ERR_NO_DEVICE, "arch is NULL and there is no current HIP device to take it from");
    try {
        std::unique_ptr<sdfv_program, void (*)(sdfv_program*)> q(new sdfv_program, sdfv_program_free);
        q->ops = p->ops;
        memcpy(q->bb, p->bb, sizeof(q->bb));
        q->compiled = new CompiledProgram;
        CompiledProgram& c = *q->compiled;
        c.routes = routes;
        c.arch = arch ? processor_of(arch) : here;
        c.source = generate_source(q->ops, routes);
        const auto t0 = std::chrono::steady_clock::now();
        if (int rc = compile_source(c.source, c.arch, c.code)) return rc;
        c.compile_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (c.arch == here) {  // ready before the first covered call, which may then be captured into a graph
            const sdfv_prog_op* dev_ops = nullptr;
            uint32_t n_ops = 0;
            if (int rc = program_on_device(q.get(), &dev_ops, &n_ops)) return rc;
            std::lock_guard<std::mutex> lock(q->mu);
            const CompiledProgram::Loaded* l = nullptr;
            if (int rc = load_on_device(q.get(), dev, &l)) return rc;
        }
        *out = q.release();
    } catch (const std::bad_alloc&) {
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "out of host memory");
    }
    return SDFV_OK;
}

int sdfv_program_compiled_info(const sdfv_program* p, sdfv_compiled_info* info) {
    if (!p) return set_error(SDFV_ERR_INVALID_ARGUMENT, "program is NULL");
    if (!info) return set_error(SDFV_ERR_INVALID_ARGUMENT, "info is NULL");
    if (info->size < sizeof(sdfv_compiled_info))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "sdfv_compiled_info.size = %u is smaller than the structure (%zu)", info->size, sizeof(sdfv_compiled_info));
    const uint32_t size = info->size;
    memset(info, 0, sizeof(*info));
    info->size = size;
    if (const CompiledProgram* c = p->compiled) {
        info->routes = c->routes;
        snprintf(info->arch, sizeof(info->arch), "%s", c->arch.c_str());
        info->compile_seconds = c->compile_seconds;
        info->code_bytes = c->code.size();
        info->launches = c->launches.load(std::memory_order_relaxed);
    }
    return SDFV_OK;
}

int sdfv_program_compiled_code(const sdfv_program* p, const void** code, size_t* bytes, const char** source) {
    if (!p) return set_error(SDFV_ERR_INVALID_ARGUMENT, "program is NULL");
    if (!p->compiled) return set_error(SDFV_ERR_INVALID_ARGUMENT, "a plain handle has no code object: sdfv_program_compile makes a compiled one");
    if (code) *code = p->compiled->code.data();
    if (bytes) *bytes = p->compiled->code.size();
    if (source) *source = p->compiled->source.c_str();
    return SDFV_OK;
}

}  // extern "C"
#pragma GCC visibility pop
