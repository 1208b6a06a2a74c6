"""CPU tests of the one table of the SDF-program kernels (SDFV_PROGRAM_KERNELS in csrc/program_kernels.h): every route of
sdfv_program_compile has rows; a handle compiled for gfx950 holds exactly the table's names, per route and for all four; each of
the nineteen compiled kernels takes its explicit arguments at the offsets and sizes of its interpreted twin in the built library
(ProgramKernels::launch hands both ONE argument array: a mismatch would be a wild kernel-argument read on the device); and the
kernels are stated nowhere else -- not as text in program_compile.hip, not as a second launch in the launchers."""
import importlib
import os
import re

import pytest

import program_geometry as G
from kernel_objects import bare_code_object, code_objects, have_llvm_tools, kernel_args, kernel_table  # noqa: F401 (code_objects: a fixture)
from test_program_compile_cpu import FILL_KERNELS, MARCH_KERNELS, POINTS_KERNELS, kernels_of
from test_program_compile_mesh_cpu import MESH_KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdf-viewer_amd", "csrc")
ROUTE_BITS = {"SDFV_COMPILE_FILL": 1, "SDFV_COMPILE_POINTS": 2, "SDFV_COMPILE_MARCH": 4, "SDFV_COMPILE_MESH": 16}
ALL_ROUTES = 23                                                      # kAllRoutes of program_compile.hip
LAUNCHERS = ("program_kernels.hip", "program_march_kernels.hip", "program_mesh_kernels.hip", "sparse_mesh_kernels.hip")


def source(name):
    return open(os.path.join(CSRC, name)).read()


def table_rows():
    """[(enum name, stem, route bit)] in the table's order."""
    text = source("program_kernels.h")
    body = text.split("#define SDFV_PROGRAM_KERNELS(X)")[1].split("\n\n")[0]
    return [(index, stem, ROUTE_BITS[route]) for index, stem, route in re.findall(r"X\((\w+),\s*(\w+),\s*(\w+)\)", body)]


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


def test_every_route_has_rows_and_the_order_stands():
    rows = table_rows()
    assert len(rows) == 19 and len({r[0] for r in rows}) == 19 and len({r[1] for r in rows}) == 19
    assert sum(ROUTE_BITS.values()) == ALL_ROUTES
    for bit in ROUTE_BITS.values():
        assert any(route == bit for _, _, route in rows), bit
    assert {route for _, _, route in rows} == set(ROUTE_BITS.values())
    # a handle keeps its kernels by index: the names in the order they have had since the routes were added
    assert ["sdfprogc_" + stem for _, stem, _ in rows] == FILL_KERNELS + POINTS_KERNELS + MARCH_KERNELS + MESH_KERNELS
    assert "kProgramKernels == 19" in source("program_kernels.h")   # the static_assert on the row count


@pytest.mark.skipif(not have_llvm_tools(), reason="LLVM binary tools not installed")
def test_a_compiled_handle_holds_exactly_the_tables_names(PM, tmp_path):
    rows = table_rows()
    plain = PM.Program().cube(0.95).sphere(1.05).subtract().build()
    for routes in (1, 2, 4, 16, ALL_ROUTES):
        c = plain.compile(routes, arch="gfx950")
        want = sorted("sdfprogc_" + stem for _, stem, route in rows if route & routes)
        assert sorted(kernels_of(c.compiled_code(), tmp_path, f"routes{routes}")) == want, routes
        lines = re.findall(r"^SDFV_PROGRAM_KERNEL_(\w+)\((\w+)\)$", c.compiled_source(), re.M)
        assert sorted(name for _, name in lines) == want and all(name == "sdfprogc_" + stem for stem, name in lines), routes


@pytest.mark.skipif(not have_llvm_tools(), reason="LLVM binary tools not installed")
@pytest.mark.parametrize("name", ["demo3", "every_opcode"])
def test_every_pair_takes_its_arguments_at_the_same_offsets(PM, code_objects, tmp_path, name):  # noqa: F811
    program = {"demo3": lambda: PM.Program().cube(0.95).sphere(1.05).subtract(),
               "every_opcode": lambda: G.emit(G.scene_every_opcode(), PM)}[name]()
    code = program.build().compile(ALL_ROUTES, arch="gfx950").compiled_code()
    co = tmp_path / f"{name}.co"
    co.write_bytes(code)
    compiled = kernel_table(bare_code_object(co))
    compiled_args, library_args, library = kernel_args(bare_code_object(co)), kernel_args(code_objects), kernel_table(code_objects)
    rows = table_rows()
    assert len(rows) == 19
    for _, stem, _ in rows:
        mine, twin = "sdfprogc_" + stem, "sdfprog_" + stem
        print(f"{name:14s} {stem:24s} kernarg {compiled[mine]['kernarg']:4d}  args {compiled_args[mine]}")
        assert compiled_args[mine], mine                             # every one of them takes arguments
        assert compiled_args[mine] == library_args[twin], (stem, compiled_args[mine], library_args[twin])
        assert compiled[mine]["kernarg"] == library[twin]["kernarg"], stem


def test_the_kernels_are_stated_nowhere_else():
    text = source("program_compile.hip")
    literals = re.findall(r'"(?:[^"\\\n]|\\.)*"', text)
    assert literals and not any("__global__" in s for s in literals)
    for name in LAUNCHERS:
        assert "hipLaunchKernelGGL(sdfprog_" not in source(name), name
        assert "bool mine" not in source(name), name
