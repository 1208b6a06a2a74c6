"""The host routes to the mesh of a loaded grid: SDFViewer::mesh (tests/c/grid_mesh_host.cpp, linked against the product
library), sdfv_viewer_mesh through viewer.py, and `sdf-viewer-gpu app ... --mesh-out`, for a provider library behind the per-point ABI and for the demo."""
import os
import subprocess

import numpy as np
import pytest
import torch

import grid_mesh_ref as G
from test_gpu_lattice_mesh import parse_ply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EXE = os.path.join(ROOT, "sdf-viewer_amd", "sdf-viewer-gpu")
GYROID_BOX = (-1.0, -0.5, -0.75, 1.0, 0.5, 0.75)            # tests/c/gyroid_provider.c's bounds


def build_host(tmp_path):
    lib = os.path.join(ROOT, "sdf-viewer_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "grid_mesh_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(rocm, "include"), "-I", os.path.join(lib, "host"),
                           os.path.join(ROOT, "tests", "c", "grid_mesh_host.cpp"), "-o", str(exe), "-L", lib, "-lsdfviewer_host",
                           "-lsdfgrid", "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib"),
                           "-Wl,-rpath," + lib, "-ldl", "-pthread"])
    return exe


def test_sdf_viewer_mesh_is_the_c_call_on_the_viewer_s_textures(gyroid_provider, tmp_path):
    """tests/c/grid_mesh_host.cpp, on a 17^3 viewer that keeps the plain volume and on a 17 x 18 x 17 one pinned to the
    interleaved volume: SDFViewer::mesh equals sdfv_grid_mesh_extract made by hand on the viewer's textures after a full load of
    the gyroid provider, after its load stopped at lod 2 (the call with lod = 2), and for the demo stopped at lod 2, whose virgin
    rows are materialised first, and loaded to the end.  The mesh it leaves has the provider's colours."""
    exe = build_host(tmp_path)
    prefix = tmp_path / "host"
    r = subprocess.run([str(exe), gyroid_provider, str(prefix)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "grid_mesh_host ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    v = np.fromfile(str(prefix) + ".v.bin", F).reshape(-1, 12)
    i = np.fromfile(str(prefix) + ".i.bin", np.uint32)
    assert v.shape[0] > 100 and i.shape[0] % 3 == 0 and i.max() == v.shape[0] - 1
    idx = np.rint(v[:, 6:9].astype(np.float64) * 255.0)
    assert (v[:, 6:9] == (idx.astype(F) / F(255.0))).all() and len(np.unique(idx, axis=0)) > 4      # 8-bit colours, several of them
    lo, hi = np.array(GYROID_BOX[:3], F), np.array(GYROID_BOX[3:], F)
    # (the provider's distance at the box's lowest corner is a NaN: "not inside", and the up to three crossing edges that end there
    # interpolate to a NaN coordinate, as on every route that meshes this provider)
    off = np.isnan(v[:, :3])
    assert off.any(axis=1).sum() <= 3 and (off | ((v[:, :3] >= lo) & (v[:, :3] <= hi))).all()


@pytest.mark.parametrize("algorithm", [0, G.DUAL], ids=["marching_cubes", "dual_contouring"])
def test_the_viewer_s_c_call_is_the_grid_call_on_its_textures(pkg, algorithm):
    """sdfv_viewer_mesh (include/sdfviewer_mesh.h, viewer.py's Viewer.mesh) over a callback surface sampled on the device: after
    the first update of three passes (lod 4 or below published) and after the whole load it equals sdfv_grid_mesh_extract on
    sdfv_viewer_textures' pointers at sdfv_viewer_state's lod; without materials the material words are zero."""
    import importlib
    V = importlib.import_module("sdf-viewer_amd.viewer")  # noqa: N806
    bb = (-1.0, -0.5, -0.75, 1.0, 0.5, 0.75)

    def sample(p):                                           # two spheres, a colour and material that vary with the point
        d = torch.minimum(p.norm(dim=1) - 0.45, (p - torch.tensor([0.5, 0.1, 0.2], device=p.device)).norm(dim=1) - 0.3)
        return torch.stack([d, 0.5 + 0.5 * p[:, 0], 0.25 + 0.0 * d, (p[:, 2] > 0).float(), 0.5 + p[:, 1], 0.125 + 0.0 * d, 1.0 + 0.0 * d], dim=1)
    surface = V.Surface.from_torch(lambda: bb, sample)
    viewer = V.Viewer.new_voxels((21, 12, 17), bb, 3, V.LAYOUT_INTERLEAVED)
    seen = []
    for _ in range(200):
        visited = viewer.update(surface, budget_ns=1)
        viewer.commit()
        lod = int(viewer.state()["lod"])
        if lod not in seen and lod <= 4:
            seen.append(lod)
            t0p, t1p, grid = viewer.textures()
            shape = (int(grid.dims[2]), int(grid.dims[1]), int(grid.dims[0]), 4)
            t0 = torch.as_tensor(pkg._DeviceArray(t0p, shape, "<f4"), device="cuda")
            t1 = torch.as_tensor(pkg._DeviceArray(t1p, shape, "<f4"), device="cuda")
            for materials in (True, False):
                want = pkg.grid_mesh_extract(grid, t0, t1, lod=lod, algorithm=algorithm, materials=materials)
                got = viewer.mesh(algorithm, materials)
                assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1]), (lod, materials)
                assert (got[0][:, 6:] != 0).any().item() == materials
            if lod == 1:
                assert got[0].shape[0] > 100
        if visited == 0:
            break
    assert seen and seen[-1] == 1, seen
    viewer.close()


def dumped_textures(pkg, prefix, bb, max_voxels_side):
    grid = pkg.grid_from_bb(bb[:3], bb[3:], max_voxels_side)
    shape = (int(grid.dims[2]), int(grid.dims[1]), int(grid.dims[0]), 4)
    t0 = np.fromfile(prefix + ".tex0.f32", F).reshape(shape)
    t1 = np.fromfile(prefix + ".tex1.f32", F).reshape(shape)
    return grid, t0, t1


def assert_ply_is_the_mesh(ply_path, v, i):
    verts, faces = parse_ply(open(ply_path).read())
    assert v.shape[0] > 100 and verts.shape[0] == v.shape[0] and faces.shape[0] * 3 == i.shape[0]
    np.testing.assert_array_equal(verts[:, :6].astype(F), v[:, :6])
    want_bytes = np.clip(np.trunc(v[:, 6:9] * F(255.9999)), 0, 255)                               # (c * 255.9999) as u8, mesh.rs:106-108
    np.testing.assert_array_equal(verts[:, 6:9], want_bytes)
    np.testing.assert_array_equal(want_bytes, np.rint(v[:, 6:9].astype(np.float64) * 255.0))      # ... the byte the fill quantised to
    np.testing.assert_array_equal(verts[:, 9:].astype(F), v[:, 9:])
    np.testing.assert_array_equal(faces[:, 1:].reshape(-1), i)


@pytest.mark.parametrize("sdf", ["url", "demo"])
def test_cli_app_writes_the_ply_of_the_loaded_grid(pkg, gyroid_provider, tmp_path, sdf):
    """`sdf-viewer-gpu app --mesh-out FILE [--mesher NAME] ...`: the PLY's vertices, colour bytes and faces are those of
    sdfv_grid_mesh_extract over the textures the same run dumps; an existing file is refused before anything is loaded."""
    out, prefix = tmp_path / "grid.ply", str(tmp_path / "dump")
    tail = ["url", "file://" + gyroid_provider] if sdf == "url" else ["demo", "-s", "0.9"]
    mesher = ["--mesher", "dual-contouring-particle-based-minimization"] if sdf == "demo" else []
    cmd = [EXE, "app", "--max-voxels-side", "24", "--loading-passes", "2", "--width", "32", "--height", "24", "--out", str(tmp_path / "f.ppm"),
           "--dump-textures", prefix, "--mesh-out", str(out)] + mesher + tail
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Meshed the loaded grid" in r.stderr, (r.returncode, r.stderr)
    bb = GYROID_BOX if sdf == "url" else (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
    grid, t0, t1 = dumped_textures(pkg, prefix, bb, 24)
    v, i = pkg.grid_mesh_extract(grid, torch.from_numpy(t0).cuda(), torch.from_numpy(t1).cuda(), algorithm=G.DUAL if sdf == "demo" else 0,
                                 materials=True)
    assert_ply_is_the_mesh(out, v.cpu().numpy(), i.cpu().numpy().astype(np.int64))
    again = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert again.returncode == 1 and "Output file already exists" in again.stderr and "Loaded" not in again.stderr
    bad = subprocess.run([EXE, "app", "--mesh-out", str(tmp_path / "x.ply"), "--mesher", "cubes", "demo"], capture_output=True, text=True,
                         timeout=60)
    assert bad.returncode == 2 and "is not a mesher" in bad.stderr and not os.path.exists(tmp_path / "x.ply")
