"""CPU tests of meshing a loaded grid (include/sdfgrid.h, "Meshing a loaded grid"): the numpy restatement the GPU tests compare
against (tests/grid_mesh_ref.py over tests/mesh_ref.py) -- the extraction on a lattice that is no cube (every route's bits are
pinned by tests/test_mesh_ref_pins.py), the table inversion, the round trip of the golden grid's colours through the oracle's 8-bit quantisation and the PLY byte rule --, what
the two entry points refuse without a device, and what the built kernels look like.  No device needed."""
import ctypes as C
import os
import re

import numpy as np

import grid_mesh_ref as G
import lattice_mesh_ref as L
import mesh_ref as MR
from program_fill_check import interleave
from kernel_objects import code_objects, disassembly, kernel_table  # noqa: F401 (code_objects is a fixture)

INVALID, NO_DEVICE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F = np.float32
BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
SLAB_BOX = (-1.0, -0.5, -0.75, 1.0, 0.5, 0.75)


# ---- the restatement ----
def test_a_lattice_that_is_no_cube_gives_a_closed_surface_inside_its_box():
    """A sphere on 8 x 6 x 4 cells of a box with three different sides: both algorithms give a closed, oriented surface whose
    vertices lie within a cell's diagonal of the sphere, and unit normals."""
    cells, bb = (8, 6, 4), (-1.0, -0.9, -0.8, 1.0, 0.9, 0.8)
    _, _, _, axes = MR.axes_of(cells, bb)
    zz, yy, xx = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    d = (np.sqrt(xx.astype(np.float64) ** 2 + yy ** 2 + zz ** 2) - 0.6).astype(F)
    assert d.shape == (5, 7, 9) and MR.cells_of(d) == cells
    for algorithm in (0, G.DUAL):
        v, i, _ = L.extract(d, bb, algorithm)
        assert v.shape[0] > 20 and i.shape[0] % 3 == 0 and i.max() == v.shape[0] - 1
        MR.assert_closed_and_oriented(i)
        r = np.linalg.norm(v[:, :3].astype(np.float64), axis=1)
        assert np.abs(r - 0.6).max() < 0.5 * np.linalg.norm([2.0 / 8, 1.8 / 6, 1.6 / 4])
        assert np.abs(np.linalg.norm(v[:, 3:6].astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_lattice_of_and_unpack_follow_the_published_voxels():
    """dims 12 at lod 2 and 4: the step does not divide dim - 1, the lattice stops at voxel 10 and 8 and the box's upper corner is
    that voxel's position; at lod 1 the box is the grid's; the off-lattice voxels play no part."""
    bb = (-1.0, -0.5, -1.25, 1.0, 1.0, 1.0)
    for lod, cells, last in ((1, 11, 11), (2, 5, 10), (4, 2, 8)):
        c, box = G.lattice_of((12, 12, 12), bb, lod)
        assert c == (cells,) * 3 and box[:3] == bb[:3]
        for a in range(3):
            want = F(last) / F(11.0) * (F(bb[3 + a]) - F(bb[a])) + F(bb[a])
            assert F(box[3 + a]) == want
        if lod == 1:
            assert box == bb
    s = np.arange(12 ** 3, dtype=F).reshape(12, 12, 12)
    d = G.unpack(s, 4)
    assert d.shape == (3, 3, 3) and d[2, 1, 2] == s[8, 4, 8] - F(0.1)
    c, _ = G.lattice_of((9, 7, 5), bb, 2)
    assert c == (4, 3, 2) and G.unpack(np.zeros((5, 7, 9), F), 2).shape == (3, 4, 5)
    vol = np.arange(4 * 6 * 5, dtype=F).reshape(4, 6, 5)
    ilv = interleave(vol)
    for z, y, x in ((0, 0, 0), (1, 3, 2), (3, 5, 4), (2, 4, 1)):
        row = z * 6 + y
        assert ilv[((row >> 1) * 5 + x) * 2 + (row & 1)] == vol[z, y, x]


# ---- the table inversion ----
def test_the_table_inversion_is_the_identity_on_the_table_monotone_between_and_total():
    t = G.TABLE
    assert (np.diff(t.astype(np.float64)) > 0).all() and t[0] == 0 and t[255] == 1
    assert (G.srgb_index(t) == np.arange(256)).all()
    # between two entries: the upper one's index; just above an entry likewise, just below it its own
    mid = ((t[:-1].astype(np.float64) + t[1:]) / 2).astype(F)
    assert (G.srgb_index(mid) == np.arange(1, 256)).all()
    assert (G.srgb_index(np.nextafter(t[:-1], F(2))) == np.arange(1, 256)).all()
    assert (G.srgb_index(np.nextafter(t[1:], F(-1))) == np.arange(1, 256)).all()
    x = np.sort(np.random.default_rng(1).uniform(-0.5, 1.5, 5000).astype(F))
    assert (np.diff(G.srgb_index(x)) >= 0).all()
    with np.errstate(invalid="ignore"):
        assert G.srgb_index(F(np.nan)) == 0 and G.srgb_index(F(-1.0)) == 0 and G.srgb_index(F(-0.0)) == 0
        assert G.srgb_index(F(-np.inf)) == 0
    assert G.srgb_index(F(1.5)) == 255 and G.srgb_index(F(np.inf)) == 255 and G.srgb_index(np.nextafter(F(1), F(2))) == 255
    assert G.srgb_colour(t[255]) == F(1.0) and G.srgb_colour(t[128]) == F(128) / F(255)


def ply_byte(c):
    """(c * 255.9999) as u8, meshers/mesh.rs:106-108: f32 product, saturating truncation."""
    return np.clip(np.trunc(np.asarray(c, F) * F(255.9999)), 0, 255).astype(np.int64)


def test_the_golden_grid_s_colours_come_back_as_the_oracle_s_8_bit_colours(oracle):
    """tests/golden/grid_9x7x5.npz: every voxel's tex0.gba inverts to the byte the oracle quantises that voxel's sample to (a black
    sample as the grid's 0.5 grey), and the reference's PLY rule turns the vertex colour idx / 255 into the same byte again."""
    g = np.load(os.path.join(GOLD, "grid_9x7x5.npz"))
    dims = tuple(int(d) for d in g["dims"])
    ints = {"cube_material", "sphere_material", "disable_sphere"}
    keys = ["cube_half_side", "cube_material", "sphere_radius", "sphere_material", "max_distance_custom_material", "disable_sphere"]
    seen = set()
    for k, row in enumerate(g["params"]):
        prm = oracle.default_params(**{name: (int(v) if name in ints else float(v)) for name, v in zip(keys, row)})
        axes = [np.array([oracle.L.or_voxel_coord(i, dims[a], float(g["bb_min"][a]), float(g["bb_max"][a])) for i in range(dims[a])], F)
                for a in range(3)]
        zz, yy, xx = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
        s = oracle.sample_many(prm, np.stack([xx, yy, zz], axis=-1).reshape(-1, 3))
        colour = np.where((s[:, 1:4] != 0).any(axis=1, keepdims=True), s[:, 1:4], F(0.5))
        want = np.array([[oracle.L.or_srgb_quantize(float(c)) for c in px] for px in colour], np.int64)
        t0 = g[f"tex0_{k}"].reshape(-1, 4)
        got = G.srgb_index(t0[:, 1:4])
        assert (got == want).all(), k
        assert (G.TABLE[got] == t0[:, 1:4]).all()                     # (the texels hold table entries: the inversion is exact)
        assert (ply_byte(G.srgb_colour(t0[:, 1:4])) == want).all(), k
        seen.update(np.unique(want).tolist())
    assert len(seen) >= 4                                             # more than one colour took part
    assert (ply_byte(np.arange(256, dtype=F) / F(255.0)) == np.arange(256)).all()   # ... and the PLY rule holds for every byte


def test_the_restated_materials_take_the_nearest_published_voxel():
    """Positions at known places of a 9 x 7 x 5 grid whose texels encode their own voxel: f = 0.5 stays at c, anything above goes
    to c + 1, outside the box clamps, at lod 2 the voxel is twice the lattice point."""
    bb = (-1.0, -0.5, -1.25, 1.0, 1.0, 1.0)
    dims = (9, 7, 5)
    t0 = np.zeros((5, 7, 9, 4), F)
    t1 = np.zeros((5, 7, 9, 4), F)
    zz, yy, xx = np.meshgrid(np.arange(5), np.arange(7), np.arange(9), indexing="ij")
    t0[..., 1], t0[..., 2], t0[..., 3] = G.TABLE[xx], G.TABLE[yy + 100], G.TABLE[zz + 200]
    t1[..., 0], t1[..., 1], t1[..., 2] = xx, yy, zz
    for lod in (1, 2):
        cells, box = G.lattice_of(dims, bb, lod)
        lo, size = np.array(box[:3], np.float64), np.array(box[3:], np.float64) - np.array(box[:3], np.float64)
        u = np.array([(1.5, 0.25, 0.75), (1.51, 2.49, 0.0), (-3.0, 9.0, 1.0), (cells[0], cells[1], cells[2]), (0.49, 0.51, 1.75)])
        u = np.minimum(u, np.array(cells) + 5.0)
        p = (u / np.array(cells) * size + lo).astype(F)
        m = G.materials(t0, t1, bb, lod, p)
        want = np.array([(1, 0, 1), (2, 2, 0), (0, cells[1], 1), cells, (0, 1, 2)]) * lod
        want = np.minimum(want, np.array(cells) * lod)
        assert (m[:, 3:] == want).all(), (lod, m[:, 3:], want)
        assert (m[:, 0] == (want[:, 0] / F(255)).astype(F)).all() and (m[:, 2] == ((want[:, 2] + 200) / F(255)).astype(F)).all()


# ---- the ABI ----
def test_both_entry_points_are_declared_exported_and_bound(pkg):
    names = ("sdfv_grid_mesh_extract", "sdfv_grid_vertex_materials")
    header = open(os.path.join(ROOT, "include", "sdfgrid.h")).read()
    raw = C.CDLL(pkg._capi.LIB_PATH)
    for name in names:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in pkg._capi.PROTOTYPES and getattr(raw, name)
    assert "Meshing a loaded grid" in header
    assert callable(pkg.grid_mesh_extract) and callable(pkg.grid_vertex_materials)
    assert pkg.lib.sdfv_abi_version() == 5     # additive: the version stays


def test_the_viewer_s_mesh_call_is_declared_exported_and_bound(pkg, tmp_path):
    """include/sdfviewer_mesh.h beside sdfviewer.h (as sdfv_viewer_update_program lives in sdfprogram.h): plain C, exported by the
    product library and by nothing else, bound by viewer.py, shown in INTEGRATION.md; NULL arguments are refused and the mesh
    handed in is zeroed."""
    import importlib
    import subprocess
    src = tmp_path / "use_header.c"
    src.write_text('#include "sdfviewer_mesh.h"\nint main(void) { sdfv_mesh m; return sdfv_viewer_mesh(0, 0, 0, &m) == SDFV_ERR_INVALID_ARGUMENT ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    header = open(os.path.join(ROOT, "include", "sdfviewer_mesh.h")).read()
    assert re.search(r"^int sdfv_viewer_mesh\(sdfv_viewer \*v, uint32_t algorithm, uint32_t flags, sdfv_mesh \*out\);", header, re.M)
    for lib, exported in (("libsdfviewer_host.so", True), ("libsdfviewer_host_test.so", False)):
        syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "sdf-viewer_amd", lib)], capture_output=True, text=True).stdout
        assert (" T sdfv_viewer_mesh" in syms) == exported, lib
    assert "sdfv_viewer_mesh" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    V = importlib.import_module("sdf-viewer_amd.viewer")  # noqa: N806
    assert callable(V.Viewer.mesh) and V.lib.sdfv_viewer_abi_version() == 1
    m = pkg._capi.Mesh()
    m.vertices, m.indices, m.n_vertices, m.n_indices = 1, 1, 7, 7
    assert V.lib.sdfv_viewer_mesh(None, 0, 1, C.byref(m)) == INVALID
    assert (m.vertices, m.indices, m.n_vertices, m.n_indices) == (None, None, 0, 0)
    assert V.lib.sdfv_viewer_mesh(None, 0, 1, None) == INVALID


def test_every_refusal_comes_before_the_device_check(pkg):
    lib, K = pkg.lib, pkg._capi
    m = K.Mesh()
    A = 4096                                              # any non-NULL, 16-byte aligned address: nothing reads it before the device check

    def grid(dims=(9, 8, 5), z_begin=0, z_end=None):
        return pkg.make_grid(dims, (-1, -1, -1), (1, 1, 1), z_begin, z_end)

    def extract(g=None, tex0=A, tex1=A, dist=None, volume_flags=0, lod=1, algorithm=0, flags=1, out=m):
        g = grid() if g is None else g
        m.vertices, m.indices, m.n_vertices, m.n_indices = 1, 1, 7, 7
        rc = lib.sdfv_grid_mesh_extract(C.byref(g), tex0, tex1, dist, volume_flags, lod, algorithm, flags,
                                        None if out is None else C.byref(out), None)
        return rc, lib.sdfv_last_error()

    def cleared():
        return (m.vertices, m.indices, m.n_vertices, m.n_indices) == (None, None, 0, 0)

    def refused(text, **kw):
        rc, msg = extract(**kw)
        assert rc == INVALID and text in msg and cleared(), (kw, rc, msg)

    assert extract(out=None) == (INVALID, b"out is NULL")
    assert lib.sdfv_grid_mesh_extract(None, A, A, None, 0, 1, 0, 0, C.byref(m), None) == INVALID and lib.sdfv_last_error() == b"grid is NULL"
    # a slab
    refused(b"meshing takes a whole grid", g=grid(z_begin=1))
    refused(b"meshing takes a whole grid", g=grid(z_end=4))
    refused(b"meshing takes a whole grid", g=grid(z_begin=2, z_end=4))
    refused(b"outside depth", g=grid(z_end=6))                                     # (check_grid's own)
    # pointers
    refused(b"texture pointer is NULL", tex0=None)
    refused(b"texture pointer is NULL", tex1=None)                                # materials need tex1 ...
    refused(b"16-byte aligned", tex0=A + 4)
    refused(b"16-byte aligned", tex1=A + 8)
    refused(b"4-byte aligned", dist=A + 2)
    # flags
    for flags in (2, 3, 0x80000000):
        refused(b"unknown flags 0x%x" % flags, flags=flags)
    for vf in (1, 4, 16, 9):
        refused(b"unknown flags 0x%x" % vf, volume_flags=vf, dist=A)
    refused(b"SDFV_PASS_VOLUME_INTERLEAVED without a volume", volume_flags=8)
    refused(b"must be even", volume_flags=8, dist=A, g=grid((9, 7, 5)))
    refused(b"8-byte aligned", volume_flags=8, dist=A + 4)
    # lod
    for lod in (0, 3, 6, 12, 0xffffffff):
        refused(b"lod %u is not a power of two" % lod, lod=lod)
    # cells
    refused(b"0 cells along axis 0", g=grid((1, 8, 5)))
    refused(b"0 cells along axis 2", g=grid((9, 8, 0), z_end=0))
    refused(b"0 cells along axis 1", g=grid((9, 8, 5)), lod=8)
    refused(b"1025 cells along axis 0", g=grid((1026, 8, 5)))
    refused(b"outside [1, 1024]", g=grid((9, 8, 2051)), lod=2)
    # a lattice of 2^32 points or more cannot be reached within 1024 cells per axis (1025^3 < 2^32): the check is there for the day
    # the limit moves; algorithm
    for algorithm in (1, 2, 3, 5):
        assert extract(algorithm=algorithm) == (INVALID, b"Unsupported algorithm %d" % algorithm) and cleared()

    def mats(g=None, tex0=A, tex1=A, lod=1, vertices=A, n=5):
        g = grid() if g is None else g
        return lib.sdfv_grid_vertex_materials(C.byref(g), tex0, tex1, lod, vertices, n, None), lib.sdfv_last_error()

    assert lib.sdfv_grid_vertex_materials(None, A, A, 1, A, 5, None) == INVALID and lib.sdfv_last_error() == b"grid is NULL"
    for kw, text in ((dict(g=grid(z_begin=1)), b"meshing takes a whole grid"), (dict(tex0=None), b"texture pointer is NULL"),
                     (dict(tex1=None), b"texture pointer is NULL"), (dict(tex1=A + 4), b"16-byte aligned"),
                     (dict(lod=3), b"lod 3 is not a power of two"), (dict(lod=16), b"0 cells along axis"),
                     (dict(vertices=None), b"NULL buffer"), (dict(vertices=A + 2), b"4-byte aligned"),
                     (dict(n=2 ** 32), b"too many for one launch")):
        rc, msg = mats(**kw)
        assert rc == INVALID and text in msg, (kw, rc, msg)
    if lib.sdfv_device_count() == 0:
        for algorithm in (0, 4):
            for flags, tex1 in ((0, None), (0, A), (1, A)):
                rc, msg = extract(algorithm=algorithm, flags=flags, tex1=tex1)
                assert rc == NO_DEVICE and b"no HIP device" in msg and cleared()
        assert extract(g=grid((9, 8, 5), z_end=0))[0] == NO_DEVICE          # z_end 0: the whole grid
        assert extract(dist=A, volume_flags=8)[0] == NO_DEVICE
        v = np.full((5, 12), 7.0, F)
        assert mats(vertices=v.ctypes.data)[0] == NO_DEVICE and (v == 7.0).all()
    assert mats(vertices=None, n=0)[0] in (0, NO_DEVICE)                    # an empty request needs no buffer


# ---- the built kernels (tests/kernel_objects.py) ----
KERNELS = ("grid_lattice_copy", "grid_lattice_volume", "grid_lattice_tex0", "grid_vertex_materials", "grid_normals_materials")


def stream_of(k, name):
    return [ln.split("//")[0].split()[0] for ln in disassembly(k["co"], name).split("\n") if ln.split("//")[0].split()]


def dwords(op):
    m = re.search(r"dwordx(\d)", op)
    return int(m.group(1)) if m else 1


def test_grid_mesh_kernels_keep_the_resource_ceilings(code_objects):
    """no scratch, no spill, at most 64 VGPRs -- the 8-waves-per-SIMD step lattice_normals is held to.  LDS: the
    256-entry table in the two material kernels, none in the unpack.  The unpack reads one dword (nontemporal) and stores one;
    the material kernels gather two texels and search the table with at most 24 LDS reads; nothing is contracted."""
    table = kernel_table(code_objects)
    assert sorted(n for n in table if n.startswith("grid_")) == sorted(KERNELS)
    for name in KERNELS:
        k = table[name]
        print(name, {a: b for a, b in k.items() if a != "co"})
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (name, k)
        assert k["vgpr"] <= 64, (name, k)
        assert k["kernarg"] <= 256, (name, k)
        assert k["lds"] == (1024 if "materials" in name else 0), (name, k)
        ops = stream_of(k, name)
        assert not any(o.startswith(("scratch_", "buffer_", "flat_")) for o in ops), name
        assert not any(o.startswith("v_pk_fma") for o in ops), name
    for name in KERNELS[:3]:
        ops = [ln.split("//")[0].split() for ln in disassembly(table[name]["co"], name).split("\n") if ln.split("//")[0].split()]
        mem = [o for o in ops if o[0].startswith("global_")]
        assert [o[0] for o in mem] == ["global_load_dword", "global_store_dword"], (name, mem)
        assert "nt" in mem[0] and "nt" not in mem[1], (name, mem)              # read once, stored for the count that follows
    # the table entry, the position, (the corner loop's round,) and the two texels, of which the compiler loads the live 12 bytes
    for name, stored, loaded in (("grid_vertex_materials", 6, 1 + 3 + 6), ("grid_normals_materials", 9, 1 + 3 + 12 + 6)):
        ops = stream_of(table[name], name)
        assert sum(dwords(o) for o in ops if o.startswith("global_store")) == stored, (name, ops)
        assert sum(dwords(o) for o in ops if o.startswith("global_load")) == loaded, (name, ops)
        # 8 probes per channel; the first is the same entry for all three
        assert 8 <= sum(1 for o in ops if o.startswith(("ds_read_b32", "ds_load_b32"))) <= 24, name
        assert sum(1 for o in ops if o.startswith("s_barrier")) == 1, name
