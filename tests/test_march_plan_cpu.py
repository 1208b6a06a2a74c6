"""The launch plan of the grid march on the CPU: csrc/march_plan.cpp (which kernel variant, which volume, the tile order with its
box-first rectangle, the occupancy cap, how a batch of cameras is cut into launches) and the kernel's workgroup-to-tile mapping
(csrc/march_tile_order.h), compiled by g++ as they stand into tests/c/march_plan_check.cpp.  The expectations are DESIGN.md
3.3's; the program prints every case that fails."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_march_plan_selects_instantiated_kernels_and_renders_every_tile_once(tmp_path):
    csrc = os.path.join(ROOT, "sdf-viewer_amd", "csrc")
    exe = tmp_path / "march_plan_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I", csrc, os.path.join(ROOT, "tests", "c", "march_plan_check.cpp"),
                           os.path.join(csrc, "march_plan.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-4000:], r.stderr[-2000:])
