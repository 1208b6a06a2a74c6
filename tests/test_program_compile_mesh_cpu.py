"""CPU tests of the mesh route of sdfv_program_compile (include/sdfgrid.h, SDFV_COMPILE_MESH = 16): the route bit is declared and
bound and its neighbours stay refused; a program compiled for gfx950 with no device holds exactly the nine kernels of the route,
and none of them without it; each of them needs no scratch, no spill, no more VGPRs than the interpreter's kernel of the same
variant in the built library and exactly its kernel-argument bytes (one argument array feeds both launches: a mismatch would be
a fault on the device); the same program gives the same code object twice.  What the kernels COMPUTE is
tests/test_gpu_program_compile_mesh.py's."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

import program_compile_cases as CC
from kernel_objects import LLVM_TOOLS, code_objects, have_llvm_tools, kernel_table  # noqa: F401 (code_objects: a fixture)
from test_program_compile_cpu import FILL_KERNELS, MARCH_KERNELS, POINTS_KERNELS, builders

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1
MESH_KERNELS = ["sdfprogc_mesh_lattice", "sdfprogc_mesh_vertices", "sdfprogc_mesh_vertices_mat", "sdfprogc_normal_points",
                "sdfprogc_normal_points_staged", "sdfprogc_mesh_postproc", "sdfprogc_mesh_postproc_unaligned",
                "sdfprogc_sparse_refine", "sdfprogc_sparse_bricks"]
MESH_WORDS = ("sdfprogc_mesh", "sdfprogc_sparse", "sdfprogc_normal")
OTHER_WORDS = ("sdfprogc_fill", "sdfprogc_sample", "sdfprogc_march")
PROGRAMS = ["demo3", "every_opcode", "example_sixteen", "fuzz_deepest", "tiny_k", "pow2_k", "identities", "subnormal_sizes"]


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


@pytest.fixture(scope="module")
def plains(PM):
    b = dict(builders(PM))
    b.update(CC.folding_programs(PM))
    return {name: b[name].build() for name in PROGRAMS}


@pytest.fixture(scope="module")
def mesh_compiled(PM, plains):
    """name -> the handle compiled with MESH alone for gfx950 (no device needed)."""
    return {name: p.compile(PM.MESH, arch="gfx950") for name, p in plains.items()}


def kernels_of(code, tmp_path, tag):
    co = tmp_path / f"{tag}.co"
    co.write_bytes(code)
    notes = subprocess.run([f"{LLVM_TOOLS}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    return kernel_table([(co, notes)])


# ---- the route bit ----
def test_route_bit_is_declared_and_bound(pkg, PM):
    header = open(os.path.join(ROOT, "include", "sdfgrid.h")).read()
    for text in ("#define SDFV_COMPILE_FILL   1u", "#define SDFV_COMPILE_POINTS 2u", "#define SDFV_COMPILE_MARCH  4u",
                 "#define SDFV_COMPILE_MESH 16u"):
        assert text in header, text
    assert pkg._capi.COMPILE_MESH == 16 and PM.MESH == 16
    assert pkg.lib.sdfv_abi_version() == 5
    assert C.sizeof(pkg._capi.CompiledInfo) == 64
    import inspect
    assert inspect.signature(PM.CompiledProgram.compile).parameters["routes"].default == PM.FILL | PM.POINTS | PM.MARCH


def test_neighbouring_bits_stay_refused(pkg, PM):
    lib = pkg.lib
    plain = PM.Program().sphere(0.5).build()

    def compile_rc(routes):
        out = C.c_void_p(0xdead)
        rc = lib.sdfv_program_compile(plain.h, routes, b"gfx950", C.byref(out))
        return rc, lib.sdfv_last_error().decode(), out.value

    for routes, names in ((8, "0x8"), (8 | 16, "0x8"), (32, "0x20"), (16 | 32, "0x20")):
        rc, msg, out = compile_rc(routes)
        assert rc == ERR_INVALID and f"unknown route bits {names}" in msg and out is None, (routes, rc, msg)
    rc, msg, out = compile_rc(16)
    assert rc == 0 and out, msg
    lib.sdfv_program_free(C.c_void_p(out))


# ---- the kernels of the route ----
@pytest.mark.skipif(not have_llvm_tools(), reason="LLVM binary tools not installed")
@pytest.mark.parametrize("name", PROGRAMS)
def test_mesh_route_kernels_and_resources(pkg, PM, plains, mesh_compiled, code_objects, tmp_path, name):  # noqa: F811
    """compile(MESH) holds exactly the nine kernels; each within its interpreted twin's VGPRs (the library's kernel, read from
    the built libsdfgrid.so), with no scratch and no spill, and with the twin's kernel-argument bytes."""
    library = kernel_table(code_objects)
    c = mesh_compiled[name]
    info = c.compiled_info()
    code = c.compiled_code()
    assert info["routes"] == PM.MESH and info["arch"] == "gfx950" and info["launches"] == 0
    assert info["code_bytes"] == len(code) and info["compile_seconds"] > 0.0 and code[:4] == b"\x7fELF"
    table = kernels_of(code, tmp_path, name)
    assert sorted(table) == sorted(MESH_KERNELS)
    src = c.compiled_source()
    assert all(w in src for w in MESH_WORDS) and not any(w in src for w in OTHER_WORDS)
    for kernel in MESH_KERNELS:
        k, twin = table[kernel], library[kernel.replace("sdfprogc_", "sdfprog_")]
        print(f"{name:16s} {kernel:34s} {k['vgpr']:3d} VGPRs (interpreter {twin['vgpr']:3d}), {k['sgpr']:3d} SGPRs "
              f"(interpreter {twin['sgpr']:3d}), LDS {k['lds']}, kernarg {k['kernarg']}")
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (kernel, k)
        assert k["vgpr"] <= twin["vgpr"], (kernel, k, twin)
        assert k["kernarg"] == twin["kernarg"], (kernel, k, twin)
    ops_c, bb_c = c.ops()
    ops_p, bb_p = plains[name].ops()
    assert ops_c.tobytes() == ops_p.tobytes() and bb_c == bb_p


@pytest.mark.skipif(not have_llvm_tools(), reason="LLVM binary tools not installed")
@pytest.mark.parametrize("name", ["demo3", "identities"])
def test_all_routes_hold_the_union(PM, plains, tmp_path, name):
    c = plains[name].compile(PM.FILL | PM.POINTS | PM.MARCH | PM.MESH, arch="gfx950")
    assert sorted(kernels_of(c.compiled_code(), tmp_path, name)) == sorted(FILL_KERNELS + POINTS_KERNELS + MARCH_KERNELS + MESH_KERNELS)
    assert c.compiled_info()["routes"] == 23


@pytest.mark.parametrize("name", PROGRAMS)
def test_no_mesh_kernel_without_the_bit(PM, plains, name):
    """The source generated for the three older routes names no mesh kernel and does not read the mesh bodies."""
    src = plains[name].compile(PM.FILL | PM.POINTS | PM.MARCH, arch="gfx950").compiled_source()
    assert not any(w in src for w in MESH_WORDS) and "program_mesh_device.h" not in src
    assert all(w in src for w in OTHER_WORDS)


def test_compiling_the_mesh_route_twice_gives_the_same_bytes(PM, plains, mesh_compiled):
    again = plains["every_opcode"].compile(PM.MESH, arch="gfx950")
    first = mesh_compiled["every_opcode"].compiled_code()
    assert first[:4] == b"\x7fELF" and first == again.compiled_code()
    assert mesh_compiled["every_opcode"].compiled_source() == again.compiled_source()
