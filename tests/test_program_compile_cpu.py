"""CPU tests of sdfv_program_compile (include/sdfgrid.h, "SDF programs compiled to kernels of their own"): the interface is
declared, exported and bound; a program compiles for gfx950 with no device; the code object holds exactly the kernels of the
routes asked for, within the registers the interpreter's kernels are held to; the generated source states operands as bit
patterns; the same program gives the same code object, twice and from four threads at once; every promised error; the run-time
compiler library is loaded on the first compile only; the host mirror does not care whether a handle is compiled.  What the
specialised kernels COMPUTE is tests/test_gpu_program_compile*.py's."""
import ctypes as C
import importlib
import os
import re
import struct
import subprocess
import sys
import threading

import numpy as np
import pytest

import program_compile_cases as CC
import program_fuzz as Z
import program_geometry as G
import program_ref as R
from kernel_objects import LLVM_TOOLS, have_llvm_tools, kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sdf-viewer_amd", "libsdfgrid.so")
FILL_KERNELS = ["sdfprogc_fill_tx64", "sdfprogc_fill_tx64_nt", "sdfprogc_fill_tx128", "sdfprogc_fill_tx128_nt", "sdfprogc_fill_tx256",
                "sdfprogc_fill_tx256_nt"]
POINTS_KERNELS = ["sdfprogc_sample_points", "sdfprogc_sample_points_staged"]
MARCH_KERNELS = ["sdfprogc_march", "sdfprogc_march_aux"]
ERR_INVALID, ERR_NO_DEVICE, ERR_COMPILE = -1, -4, -6


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


def deepest_of_corpus():
    """The program of the fuzz corpus whose value and frame stacks get deepest (ties: the longest)."""
    best = None
    for ops, bb in Z.corpus(Z.DEFAULT_SEED, Z.CORPUS_SIZE):
        v = f = vmax = fmax = 0
        for ins in ops:
            op = ins[0]
            v += Z.PUSHES_VALUES.get(op, 0) - Z.POPS_VALUES.get(op, 0)
            f += (op in Z.PUSHES) - (op in Z.POPS)
            vmax, fmax = max(vmax, v), max(fmax, f)
        key = (vmax + fmax, len(ops))
        if best is None or key > best[0]:
            best = (key, ops, bb)
    assert best[0][0] >= 8 + 4 - 2, best[0]   # the corpus reaches (nearly) the deepest stacks the instruction set allows
    return best[1], best[2]


def builders(PM):
    deep_ops, deep_bb = deepest_of_corpus()
    return {"demo3": PM.Program().cube(0.95).sphere(1.05).subtract(),
            "every_opcode": G.emit(G.scene_every_opcode(), PM),
            "example_sixteen": PM.example_sixteen(),
            "fuzz_deepest": Z.builder(PM, deep_ops, deep_bb)}


def kernels_of(code, tmp_path, tag):
    co = tmp_path / f"{tag}.co"
    co.write_bytes(code)
    notes = subprocess.run([f"{LLVM_TOOLS}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    return kernel_table([(co, notes)])


# ---- declared, exported, bound ----
def test_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "sdfgrid.h")).read()
    for text in ("int sdfv_program_compile(", "int sdfv_program_compiled_info(", "int sdfv_program_compiled_code(",
                 "#define SDFV_COMPILE_FILL   1u", "#define SDFV_COMPILE_POINTS 2u", "#define SDFV_COMPILE_MARCH  4u",
                 "SDFV_ERR_COMPILE = -6", "SDFV_OPT_HIPRTC_LIBRARY = 17"):
        assert text in header, text
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    for name in ("sdfv_program_compile", "sdfv_program_compiled_info", "sdfv_program_compiled_code"):
        assert f" T {name}\n" in nm, name
        assert name in pkg._capi.PROTOTYPES, name
    K = pkg._capi
    assert (K.COMPILE_FILL, K.COMPILE_POINTS, K.COMPILE_MARCH, K.ERR_COMPILE, K.OPT_HIPRTC_LIBRARY) == (1, 2, 4, -6, 17)
    assert pkg.lib.sdfv_abi_version() == 5
    dynamic = subprocess.run(["readelf", "-d", LIB], check=True, capture_output=True, text=True).stdout
    assert "NEEDED" in dynamic and "hiprtc" not in dynamic.lower(), dynamic


# ---- compiling without a device, the kernels and what they need ----
@pytest.mark.skipif(not have_llvm_tools(), reason="LLVM binary tools not installed")
@pytest.mark.parametrize("name", ["demo3", "every_opcode", "example_sixteen", "fuzz_deepest"])
def test_compiles_for_gfx950_without_a_device(pkg, PM, tmp_path, name):
    """Every route of four programs: the code object is an ELF whose kernels are exactly the routes' variants, and none of them
    needs more than the interpreter's kernel of the same variant is held to (tests/test_program_cpu.py: 72 VGPRs for tx256 and
    the samplers, 80 for tx64 / tx128; tests/test_program_march_cpu.py: 80 for the march), no scratch, no spill.

    As built: 37-45 VGPRs for every fill and sampler, 47-67 VGPRs and 46-54 SGPRs for the march kernels whatever the program
    (DESIGN.md 3.6.2 has the table and how the march's operands are kept from being hoisted out of its loops)."""
    every_route_compiles_within_the_interpreters_registers(PM, builders(PM)[name].build(), tmp_path, name)


def every_route_compiles_within_the_interpreters_registers(PM, plain, tmp_path, name):
    for routes, want in ((PM.FILL, FILL_KERNELS), (PM.POINTS, POINTS_KERNELS), (PM.MARCH, MARCH_KERNELS),
                         (PM.FILL | PM.POINTS | PM.MARCH, FILL_KERNELS + POINTS_KERNELS + MARCH_KERNELS)):
        c = plain.compile(routes, arch="gfx950")
        info = c.compiled_info()
        code = c.compiled_code()
        assert info["routes"] == routes and info["arch"] == "gfx950" and info["launches"] == 0
        assert info["code_bytes"] == len(code) and info["compile_seconds"] > 0.0
        assert code[:4] == b"\x7fELF"
        table = kernels_of(code, tmp_path, f"{name}_{routes}")
        assert sorted(table) == sorted(want)
        for kernel, k in table.items():
            ceiling = 72 if ("tx256" in kernel or "sample_points" in kernel) else 80
            print(f"{name} {kernel}: {k['vgpr']} VGPRs, {k['sgpr']} SGPRs, LDS {k['lds']}")
            assert k["vgpr"] <= ceiling, (kernel, k)
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (kernel, k)
        ops_c, bb_c = c.ops()
        ops_p, bb_p = plain.ops()
        assert ops_c.tobytes() == ops_p.tobytes() and bb_c == bb_p    # the same instructions and box


@pytest.mark.skipif(not have_llvm_tools(), reason="LLVM binary tools not installed")
@pytest.mark.parametrize("name", ["tiny_k", "pow2_k", "identities", "subnormal_sizes"])
def test_the_folding_programs_compile_for_every_route(pkg, PM, tmp_path, name):
    """tests/program_compile_cases.py's programs of subnormal, zero, signed-zero and power-of-two operands: the same kernels
    within the same resources as the programs above."""
    every_route_compiles_within_the_interpreters_registers(PM, CC.folding_programs(PM)[name].build(), tmp_path, name)


# ---- the same program, the same code object: twice, and from four threads at once ----
THREAD_PROGRAMS = ("anchor", "all_ops", "late_material", "ties")


def test_compiling_twice_gives_the_same_bytes(PM):
    plain = R.catalogue(PM)["all_ops"].build()
    first, second = (plain.compile(arch="gfx950").compiled_code() for _ in range(2))
    assert first[:4] == b"\x7fELF" and first == second


def test_four_threads_compile_what_a_serial_compile_gives(pkg, PM):
    """Compilations are serialised inside the library (one run-time compiler, one mutex): four host threads that each compile a
    program of their own twice, at the same time, get the code objects a serial compile of the same program gives, byte for
    byte, and no error text."""
    plains = {n: R.catalogue(PM)[n].build() for n in THREAD_PROGRAMS}
    serial = {n: p.compile(PM.FILL, arch="gfx950").compiled_code() for n, p in plains.items()}
    assert len(set(serial.values())) == len(serial)                  # four different code objects
    got, errors = {}, []

    def work(name):
        try:
            got[name] = [plains[name].compile(PM.FILL, arch="gfx950").compiled_code() for _ in range(2)]
            got[name].append(pkg.lib.sdfv_last_error().decode())
        except Exception as e:  # noqa: BLE001
            errors.append((name, repr(e)))

    threads = [threading.Thread(target=work, args=(n,), daemon=True) for n in THREAD_PROGRAMS]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120.0)                                                # (eight compiles of about half a second each)
    assert not any(t.is_alive() for t in threads), "a compiling thread did not come back"
    assert not errors, errors
    for name in THREAD_PROGRAMS:
        a, b, error_text = got[name]
        assert a == serial[name] and b == serial[name] and error_text == "", name


# ---- the generated source ----
def bits(v):
    return "f32(0x%08xu)" % struct.unpack("<I", struct.pack("<f", v))[0]


def test_generated_source_states_operands_as_bit_patterns(PM):
    tiny = float(np.float32(1e-42))                                  # a subnormal
    one_ulp = float(np.nextafter(np.float32(0.1), np.float32(1.0)))
    def program(r):
        return PM.Program().material(0.1, -0.0, tiny).sphere(r).build()
    a, b, c = (program(r).compile(PM.POINTS, arch="gfx950") for r in (0.1, 0.1, one_ulp))
    src = a.compiled_source()
    assert src == b.compiled_source()                                # the same program, the same text
    assert src != c.compiled_source()                                # one ulp in one operand, another text
    for v, pattern in ((0.1, "f32(0x3dcccccdu)"), (-0.0, "f32(0x80000000u)"), (tiny, bits(tiny))):
        assert bits(v) == pattern and pattern in src, pattern
    assert bits(one_ulp) == "f32(0x3dccccceu)" and bits(one_ulp) in c.compiled_source() and bits(one_ulp) not in src
    assert not re.search(r"\d\.\d", src.split("kOps[kOpCount] = {")[1].split("\n};")[0])  # no decimal text among the operands
    assert "sdfprogc_sample_points" in src and "sdfprogc_fill" not in src and "sdfprogc_march" not in src


# ---- errors ----
def test_errors(pkg, PM):
    lib = pkg.lib
    plain = PM.Program().sphere(0.5).build()

    def compile_rc(p, routes, arch, with_out=True):
        out = C.c_void_p(0xdead)
        rc = lib.sdfv_program_compile(p, routes, arch, C.byref(out) if with_out else None)
        return rc, lib.sdfv_last_error().decode(), out.value

    rc, msg, out = compile_rc(plain.h, 0, b"gfx950")
    assert rc == ERR_INVALID and "routes is 0" in msg and out is None
    rc, msg, out = compile_rc(plain.h, 8 | 1, b"gfx950")
    assert rc == ERR_INVALID and "unknown route bits 0x8" in msg and out is None
    rc, msg, out = compile_rc(None, 1, b"gfx950")
    assert rc == ERR_INVALID and "program is NULL" in msg and out is None
    rc, msg, _ = compile_rc(plain.h, 1, b"gfx950", with_out=False)
    assert rc == ERR_INVALID and "out is NULL" in msg
    rc, msg, out = compile_rc(plain.h, 1, b"gfx000")
    assert rc == ERR_COMPILE and "gfx000" in msg and len(msg) > len("gfx000") and out is None
    if pkg.lib.sdfv_device_count() == 0:
        rc, msg, out = compile_rc(plain.h, 1, None)
        assert rc == ERR_NO_DEVICE and out is None
    # a plain handle: routes 0, no code
    assert plain.compiled_info() == dict(routes=0, arch="", compile_seconds=0.0, code_bytes=0, launches=0)
    code, n = C.c_void_p(1), C.c_size_t(1)
    assert lib.sdfv_program_compiled_code(plain.h, C.byref(code), C.byref(n), None) == ERR_INVALID
    assert "plain handle" in lib.sdfv_last_error().decode()
    assert lib.sdfv_program_compiled_code(None, None, None, None) == ERR_INVALID
    info = pkg._capi.CompiledInfo()
    info.size = C.sizeof(info) - 8
    assert lib.sdfv_program_compiled_info(plain.h, C.byref(info)) == ERR_INVALID
    assert "sdfv_compiled_info.size" in lib.sdfv_last_error().decode()
    assert lib.sdfv_program_compiled_info(None, C.byref(info)) == ERR_INVALID
    assert lib.sdfv_program_compiled_info(plain.h, None) == ERR_INVALID
    # either output of compiled_code may be NULL
    c = plain.compile(PM.POINTS, arch="gfx950")
    assert lib.sdfv_program_compiled_code(c.h, None, None, None) == 0
    assert lib.sdfv_program_compiled_code(c.h, C.byref(code), None, None) == 0 and C.string_at(code.value, 4) == b"\x7fELF"


# ---- the run-time compiler library: loaded by the first compile, named by a process-wide option ----
SUBPROCESS = r'''
import ctypes as C, sys
lib = C.CDLL(%(lib)r)                      # (the library alone: PyTorch would bring a libhiprtc.so of its own into the maps)
lib.sdfv_last_error.restype = C.c_char_p
lib.sdfv_set_option.argtypes = [C.c_uint32, C.c_uint64]
lib.sdfv_get_option.argtypes = [C.c_uint32, C.POINTER(C.c_uint64)]
lib.sdfv_program_create.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_void_p)]
lib.sdfv_program_compile.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.POINTER(C.c_void_p)]
lib.sdfv_program_ops.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_float)]
OPT = 17
def mapped():
    return [l for l in open("/proc/self/maps") if "hiprtc" in l]
op = (C.c_uint32 * 16)(1)                  # SPHERE ...
C.cast(op, C.POINTER(C.c_float))[4] = 0.5  # ... of radius 0.5
plain, out = C.c_void_p(), C.c_void_p(1)
assert lib.sdfv_program_create(op, 1, (C.c_float * 6)(-1, -1, -1, 1, 1, 1), C.byref(plain)) == 0
assert mapped() == [], mapped()
value = C.c_uint64()
assert lib.sdfv_get_option(OPT, C.byref(value)) == 0 and C.string_at(value.value) == b""
if %(bad_path)r:
    buf = C.create_string_buffer(b"/nonexistent/libhiprtc.so")
    assert lib.sdfv_set_option(OPT, C.addressof(buf)) == 0
    buf.value = b"overwritten"             # (the library keeps its own copy)
    assert lib.sdfv_get_option(OPT, C.byref(value)) == 0 and C.string_at(value.value) == b"/nonexistent/libhiprtc.so"
    assert lib.sdfv_program_compile(plain, 2, b"gfx950", C.byref(out)) == -6 and out.value is None
    assert b"SDFV_OPT_HIPRTC_LIBRARY" in lib.sdfv_last_error(), lib.sdfv_last_error()
    assert mapped() == []
    n = C.c_size_t()
    assert lib.sdfv_program_ops(plain, None, C.byref(n), None) == 0 and n.value == 1   # the plain handle's host calls still work
else:
    assert lib.sdfv_program_compile(plain, 2, b"gfx950", C.byref(out)) == 0 and out.value, lib.sdfv_last_error()
    assert mapped() != []
assert lib.sdfv_set_option(OPT, 0) == -1 and b"already been loaded" in lib.sdfv_last_error()
print("ok")
'''


@pytest.mark.parametrize("bad_path", [True, False])
def test_hiprtc_library_option_and_lazy_load(bad_path):
    code = SUBPROCESS % dict(lib=LIB, bad_path=bad_path)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-1500:]


# ---- the host mirror ----
def test_host_mirror_is_untouched_by_compiling(pkg, PM):
    """sdfv_program_raymarch_host over a compiled handle and over its source: the same records, bit for bit (24 x 16)."""
    cam = pkg.camera_look_at(eye=(1.9, 2.3, 3.8), target=(0.0, 0.0, 0.0), aspect=24 / 16)
    for name in ("demo3", "example_sixteen"):
        plain = builders(PM)[name].build()
        compiled = plain.compile(PM.MARCH, arch="gfx950")
        a = plain.render_host(cam, 24, 16, want_aux=True, want_depth=True, threads=2)
        b = compiled.render_host(cam, 24, 16, want_aux=True, want_depth=True, threads=2)
        if name == "demo3":
            assert (a[1].view(np.int32)[..., 0] == 1).any()          # some pixels hit
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        assert compiled.compiled_info()["launches"] == 0
