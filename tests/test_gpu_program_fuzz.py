"""GPU tests over seeded random SDF programs (tests/program_fuzz.py): the same interpreter source is inlined into the dense fills,
the point samplers, normal_points, the direct march, the mesh and dual-contouring kernels and the pass kernels, and the compiler
schedules its register stacks differently in each -- so every route runs the corpus, or its share of it, against the numpy
restatement the route already has, bit for bit.  What the corpus reaches is asserted on the CPU
(tests/test_program_fuzz_cpu.py); tools/soak.sh re-seeds these tests.  Every failure message carries the seed, the program's
index and the program as builder calls."""
import contextlib
import importlib

import numpy as np
import pytest
import torch

import program_fuzz as Z
import program_march_ref as M
import program_mesh_ref as MR
import program_pass_ref as P
import program_ref as R
from program_fill_check import fill_equals_packing, interleave, same_bits
from test_gpu_dual_contour import assert_mesh_equal as assert_dual_mesh_equal
from test_gpu_program_march import RGBA_TOL
from test_gpu_program_mesh import assert_mesh_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


@pytest.fixture(scope="module")
def corpus():
    return Z.corpus(Z.seed(), Z.size())


@pytest.fixture(scope="module")
def extreme():
    return Z.extreme_corpus(Z.seed(), Z.size())


@pytest.fixture(scope="module")
def shared(corpus):
    """The 13 or more programs the routes with a costly restatement run: one of every length, all with a surface in their box."""
    picked = Z.share(corpus)
    assert len(picked) >= 13
    return picked


@contextlib.contextmanager
def explained(index, ops, bb, kind="corpus"):
    """Puts the seed, the index and the program in front of whatever assertion fails inside."""
    try:
        yield
    except AssertionError as e:
        raise AssertionError(Z.label(Z.seed(), index, ops, bb, kind) + str(e)) from e


def records_equal(got, want, decided, what):
    """Bit for bit where the restated distance is a number, a NaN where it is a NaN (the huge points of program_ref.points() make
    some), the material wherever the restatement's compares had numbers to compare."""
    gb, wb = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert gb.shape == wb.shape, what
    number = ~np.isnan(want[:, 0])
    bad = np.flatnonzero((gb[:, 0] != wb[:, 0]) & number)
    assert bad.size == 0, (what, "distances", bad[:4], got[bad[:4]], want[bad[:4]])
    assert np.isnan(got[~number, 0]).all(), (what, "a distance that is NaN")
    bad = np.flatnonzero((gb[:, 1:] != wb[:, 1:]).any(axis=1) & decided)
    assert bad.size == 0, (what, "materials", bad[:4], got[bad[:4]], want[bad[:4]])


@pytest.mark.timeout(600)
def test_the_samplers_equal_the_restatement_on_both_corpora(pkg, PM, corpus, extreme):
    """The whole ordinary corpus on program_ref.points() (the staged kernel and its scalar tail), a ragged 191-point slice and a
    slice whose buffer is not 16-byte aligned (the scalar kernel alone); the whole extreme corpus on program_ref.odd_batch()
    under the header's rule for NaN."""
    pts = R.points()
    dev = torch.from_numpy(pts).cuda()
    ragged = dev[64:64 + 191].contiguous()
    flat = torch.empty(3 * 512 + 1, device="cuda")
    flat[1:] = dev[3:3 + 512].reshape(-1)
    unaligned = flat[1:].view(512, 3)
    assert dev.data_ptr() % 16 == 0 and unaligned.data_ptr() % 16 != 0 and len(pts) > 256 and len(pts) % 256
    for i, (ops, bb) in enumerate(corpus):
        with explained(i, ops, bb):
            prog = Z.builder(PM, ops, bb).build()
            for distance_only in (False, True):
                want, decided = R.run(ops, pts, distance_only, want_decided=True)
                records_equal(prog.sample_points(dev, distance_only).cpu().numpy(), want, decided, f"d_only={distance_only}")
                records_equal(prog.sample_points(ragged, distance_only).cpu().numpy(), want[64:64 + 191], decided[64:64 + 191], "ragged")
                records_equal(prog.sample_points(unaligned, distance_only).cpu().numpy(), want[3:3 + 512], decided[3:3 + 512], "unaligned")
    odd, ordinary = R.odd_batch()
    odd_dev = torch.from_numpy(odd).cuda()
    nans = numbers = 0
    for i, (ops, bb) in enumerate(extreme):
        with explained(i, ops, bb, "extreme_corpus"):
            prog = Z.builder(PM, ops, bb).build()
            for distance_only in (False, True):
                want, decided = R.run(ops, odd, distance_only, want_decided=True)
                R.assert_records_under_the_nan_rule(prog.sample_points(odd_dev, distance_only).cpu().numpy(), want, decided, ordinary,
                                                    f"d_only={distance_only}", both_kinds=False)
            nans += int(np.isnan(want[:, 0]).sum())
            numbers += int((~np.isnan(want[~ordinary, 0])).sum())
    torch.cuda.synchronize()
    assert nans > 0 and numbers > 0                        # over the corpus the batches hold both kinds at odd points


FILL_GRIDS = (((70, 6, 4), (0, 1)),                        # one full wave and a ragged one per row; both Srgba::from policies
              ((256, 4, 2), (0,)))                         # four waves per row


@pytest.mark.timeout(600)
@pytest.mark.parametrize("dims,srgbs", FILL_GRIDS)
def test_the_dense_fill_equals_packing_the_restated_samples_on_the_corpus(pkg, PM, corpus, dims, srgbs):
    """fill_equals_packing of tests/program_fill_check.py (no volume, the plain and the interleaved one, every non-temporal
    setting, whole and in two slabs) for every program of the corpus, over its own box."""
    for i, (ops, bb) in enumerate(corpus):
        with explained(i, ops, bb):
            fill_equals_packing(pkg, PM, dims, bb[:3], bb[3:], ("fuzz",), builders={"fuzz": Z.builder(PM, ops, bb)}, srgbs=srgbs)


@pytest.mark.timeout(600)
def test_a_pass_of_one_program_over_a_grid_loaded_with_another(pkg, PM, corpus):
    """Consecutive programs A, B of the corpus share a box: the 70 x 34 x 19 grid holds A's dense fill, then one pass of B at
    steps 4, 2 and 1, with the generic box and with none, for the three forms of the volume -- where(mask, B's fill, A's) with
    the mask restated (tests/program_pass_ref.py).  As in tests/test_gpu_program_pass.py a pair is compared only if no stored
    voxel of A or B equals AIR_DIST in the restatement (such a voxel reads as not loaded)."""
    K = pkg._capi
    air = np.float32(pkg.AIR_DIST)
    lut = M.srgb_table()
    pairs = [(i, i + 1) for i in range(0, len(corpus) - 1, 2)]
    assert len(pairs) >= 13 and all(corpus[a][1] == corpus[b][1] for a, b in pairs)
    skipped = differing = 0
    W, H, D = P.DIMS
    for ia, ib in pairs:
        bb = corpus[ia][1]
        lo, hi = bb[:3], bb[3:]
        pos = R.grid_positions(P.DIMS, lo, hi)
        stored = [M.pack(R.run(corpus[k][0], pos), lut, air, False)[0][:, 0] for k in (ia, ib)]
        if any((s == air).any() for s in stored):
            skipped += 1
            continue
        with explained(ib, corpus[ib][0], bb, f"over [{ia}], corpus"):
            grid = pkg.make_grid(P.DIMS, lo, hi)
            dense = []
            for k in (ia, ib):
                t0, t1 = pkg.alloc_textures(grid)
                Z.builder(PM, *corpus[k]).build().fill_grid(grid, t0, t1)
                torch.cuda.synchronize()
                dense.append((t0.cpu().numpy(), t1.cpu().numpy()))
            same_bits(dense[0][0][..., 0].reshape(-1), stored[0], "A's fill stores the restated distance")
            before, B = dense[0], Z.builder(PM, *corpus[ib]).build()
            differs = (dense[0][0].view(np.uint32) != dense[1][0].view(np.uint32)).any(-1) | (dense[0][1].view(np.uint32) != dense[1][1].view(np.uint32)).any(-1)
            inbox = P.inside(P.DIMS, lo, hi, P.boxes(1, P.DIMS, lo, hi)["generic"][0])
            differing += bool((differs & inbox).any() and (differs & ~inbox).any())     # a wrong mask would show, either way
            for step in (4, 2, 1):
                for box in (P.boxes(step, P.DIMS, lo, hi)["generic"][0], None):
                    mask = P.update_mask(P.DIMS, lo, hi, step, before[0][..., 0], box, air)
                    assert mask.any() == (box is not None) and not mask.all()
                    for volume in ("plain", "ilv", None):
                        want = P.expected(before, dense[1], mask, air, volume)
                        t0, t1 = torch.from_numpy(before[0].copy()).cuda(), torch.from_numpy(before[1].copy()).cuda()
                        plain = before[0][..., 0].copy()
                        vol = None if volume is None else torch.from_numpy(interleave(plain) if volume == "ilv" else plain.reshape(-1)).cuda()
                        B.grid_pass(grid, step, t0, t1, dist=vol, changed_box=box, flags=K.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0)
                        torch.cuda.synchronize()
                        what = f"step {step} box {box} volume {volume}"
                        same_bits(t0.cpu().numpy(), want[0], what + " tex0")
                        same_bits(t1.cpu().numpy(), want[1], what + " tex1")
                        if volume:
                            same_bits(vol.cpu().numpy(), interleave(want[2]) if volume == "ilv" else want[2].reshape(-1), what + " volume")
    print(f"{len(pairs)} pairs, {skipped} skipped for a stored AIR_DIST, {differing} whose fills differ inside the box and outside it")
    assert 4 * skipped <= len(pairs) and 4 * differing >= 3 * (len(pairs) - skipped)


@pytest.mark.timeout(600)
def test_the_direct_march_equals_its_restatement_on_the_corpus(pkg, PM, corpus, shared):
    """sdfv_program_raymarch against tests/program_march_ref.py: one 43 x 27 frame (neither a multiple of 8) from an orbit camera
    and from a close one; every field of the march record and the depth bit for bit, rgba within the march's tolerance."""
    w, h = Z.MARCH_SIZE
    assert w % 8 and h % 8
    air = pkg.lib.sdfv_air_dist()
    frames = mixed = 0
    for i in shared:
        ops, bb = corpus[i]
        with explained(i, ops, bb):
            prog, rp = Z.builder(PM, ops, bb).build(), Z.render_params(pkg, bb)
            for ci, cam in enumerate(Z.march_cameras(pkg, bb)):
                want_aux, want_rgba = M.march(ops, rp, cam, w, h, air_dist=air)
                rgba, aux, depth = prog.render(cam, w, h, rp=rp, want_aux=True, want_depth=True)
                torch.cuda.synchronize()
                rgba, aux, depth = rgba.cpu().numpy(), aux.cpu().numpy(), depth.cpu().numpy()
                M.assert_aux_bitwise(M.aux_view(aux[0]), want_aux, f"camera {ci}")
                assert (depth[0].view(np.uint32) == want_aux["depth"].view(np.uint32)).all(), f"camera {ci} depth"
                err = float(np.abs(rgba[0] - want_rgba).max())
                assert err <= RGBA_TOL, (f"camera {ci} rgba", err)
                frames += 1
                mixed += bool((want_aux["status"] == 1).any() and (want_aux["status"] == -2).any())
    print(f"{frames} frames, {mixed} with hits and with rays that leave the box")
    assert 4 * mixed >= 3 * frames


def restated_meshes(ops, bb, materials, sizes=(7, 9)):
    """{(n, algorithm): (vertices, indices)} from the two restatements, or None where they do not apply: a lattice with an exact
    zero or a NaN (tests/mesh_ref.py extract refuses those), a marching-cubes normal that is not finite
    (tests/test_gpu_program_mesh.py compares them bit for bit) or a dual-contouring position that is not
    (tests/test_gpu_dual_contour.py asserts it)."""
    out = {}
    for n in sizes:
        _, d = MR.lattice(ops, n, bb)
        if np.isnan(d).any() or (d == 0).any():
            return None
        out[n, 0] = MR.extract(ops, n, bb, materials)[:2]
        out[n, MR.DUAL] = MR.extract(ops, n, bb, materials, MR.DUAL)[:2]
        if not np.isfinite(out[n, 0][0][:, 3:6]).all() or not np.isfinite(out[n, MR.DUAL][0][:, :3]).all():
            return None
    return out


@pytest.mark.timeout(600)
def test_marching_cubes_and_dual_contouring_equal_their_restatements_on_the_corpus(pkg, PM, corpus):
    """mesh(n, algorithm=0) and mesh(n, algorithm=4) against tests/program_mesh_ref.py (over tests/mesh_ref.py) at 7 and 9
    cells over the program's box, the materials fused on every other program: the first 16 programs of the corpus, in the
    order of program_fuzz.share, that the restatements apply to."""
    meshed = nonempty = 0
    for i in Z.share(corpus, count=len(corpus)):
        ops, bb = corpus[i]
        materials = meshed % 2 == 1
        want = restated_meshes(ops, bb, materials)
        if want is None:
            continue
        with explained(i, ops, bb):
            prog = Z.builder(PM, ops, bb).build()
            for (n, algorithm), (want_v, want_i) in want.items():
                v, idx = prog.mesh(n, materials=materials, algorithm=algorithm)
                if len(want_v) == 0:
                    assert tuple(v.shape) == (0, 12) and tuple(idx.shape) == (0,), (n, algorithm)
                    continue
                check = assert_mesh_equal if algorithm == 0 else assert_dual_mesh_equal
                check(v.cpu().numpy(), idx.cpu().numpy().astype(np.int64), want_v, want_i, (n, algorithm, materials))
        meshed += 1
        nonempty += any(len(v) for v, _ in want.values())
        if meshed == 16:
            break
    print(f"{meshed} programs meshed, {nonempty} with a non-empty restated mesh")
    assert meshed >= 13 and 4 * nonempty >= 3 * meshed


@pytest.mark.timeout(600)
@pytest.mark.parametrize("eps", [0.0, 0.01])
def test_normal_points_equal_the_restatement_on_the_corpus(pkg, PM, corpus, shared, eps):
    """sdfv_program_normal_points against program_mesh_ref.normals (the restatement of test_normal_points_against_the_restatement)
    on the first 1000 of program_ref.points(): bit for bit where a component is a number, a NaN where it is a NaN."""
    pts = R.points()[:1000]
    dev = torch.from_numpy(pts).cuda()
    for i in shared:
        ops, bb = corpus[i]
        with explained(i, ops, bb):
            want = MR.normals(ops, pts, eps)
            number = ~np.isnan(want)
            got = Z.builder(PM, ops, bb).build().normal_points(dev, eps).cpu().numpy()
            assert (MR.bits(got)[number] == MR.bits(want)[number]).all(), "components that are numbers"
            assert np.isnan(got[~number]).all(), "components that are NaN"
