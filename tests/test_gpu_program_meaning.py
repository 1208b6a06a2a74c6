"""GPU tests of what SDF programs MEAN: the point sampler and the dense fill of sdfv_program_* against the float64 reference
written from geometry (tests/program_geometry.py), on points of known distance and on whole scenes, within that reference's
derived error bound.  (Device and host mirror are held bitwise equal by tests/test_gpu_program.py; the CPU tests of meaning,
tests/test_program_meaning_cpu.py, hold the host mirror to the same reference.)"""
import importlib

import numpy as np
import pytest
import torch

import program_geometry as G
import program_ref as R

pytestmark = pytest.mark.gpu
FILL_GRID = (24, 10, 6)                      # a small grid over the unit box: tx64 rows, H even for the interleaved volume


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


def within(got, ref, tol, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    k = int(np.argmax(err - tol))
    print(f"{what}: max error / bound = {float((err / np.maximum(tol, 1e-300)).max()):.3f}")
    assert np.isfinite(tol).all() and (err <= tol).all(), (what, k, float(np.asarray(got).reshape(-1)[k]), float(ref[k]), float(tol[k]))


@pytest.mark.timeout(600)
def test_primitives_at_points_of_known_distance_on_the_device(pkg, PM):
    cases = G.known_cases()
    assert len(cases) >= 80
    for label, node, pts, known, extra in cases:
        prog = G.emit(node, PM).build()
        _, bound, _, _ = G.evaluate(node, pts)
        got = prog.sample_points(torch.from_numpy(pts).cuda(), True).cpu().numpy()
        assert (bound + extra < 1e-4).all(), label
        within(got[:, 0], known, bound + extra, label)


@pytest.mark.timeout(900)
def test_scenes_on_the_device_equal_the_float64_reference_within_its_bound(pkg, PM):
    scenes_on_the_device(pkg, PM, [(name, scene, G.SCENE_SEEDS[name]) for name, scene in G.scenes().items()])


@pytest.mark.timeout(900)
def test_random_scenes_on_the_device_equal_the_float64_reference_within_its_bound(pkg, PM):
    """program_geometry.random_scenes -- trees nested up to the stack limits, kept or redrawn by the reference alone -- through the
    sampler and the 24 x 10 x 6 fill, as the hand-written scenes are."""
    kept, rejected = G.random_scenes(G.RANDOM_SCENES_SEED, 8)
    print(f"random scenes: {len(kept)} kept, {rejected} draws rejected")
    assert len(kept) >= 8 and rejected <= len(kept)
    assert max(G.stack_needs(s)[0] for s, _ in kept) == G.MAX_VALUES and max(G.stack_needs(s)[1] for s, _ in kept) == G.MAX_FRAMES
    scenes_on_the_device(pkg, PM, [(f"random_scenes({G.RANDOM_SCENES_SEED})[{i}]", scene, seed) for i, (scene, seed) in enumerate(kept)])


def scenes_on_the_device(pkg, PM, cases):
    """cases: [(name, scene, seed of its scene_points)]"""
    K = pkg._capi
    W, H, D = FILL_GRID
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    grid = pkg.make_grid(FILL_GRID, lo, hi)
    vox = R.grid_positions(FILL_GRID, lo, hi)
    for name, scene, points_seed in cases:
        builder = G.emit(scene, PM)
        prog = builder.build()
        # the sampler, on the scene's points: distance within the bound, material where the reference decides it
        pts = G.scene_points(points_seed)
        ref, bound, mat, decided = G.evaluate(scene, pts)
        assert 1.0 - decided.mean() <= 0.02 and bound.max() < 1e-4, name
        got = prog.sample_points(torch.from_numpy(pts).cuda()).cpu().numpy()
        within(got[:, 0], ref, bound, f"scene {name}, sample_points")
        wrong = np.flatnonzero(decided & (got[:, 1:].astype(np.float64) != mat).any(axis=1))
        assert wrong.size == 0, (name, pts[wrong[:4]], got[wrong[:4]], mat[wrong[:4]])
        # the dense fill: tex0.r = clamp(f32(0.1) + d, 0, 1), one more f32 rounding on top of the bound (a clamp is Lipschitz 1)
        ref, bound, _, _ = G.evaluate(scene, vox)
        shifted = float(np.float32(0.1)) + ref
        want, tol = np.clip(shifted, 0.0, 1.0), bound + 2.0 * G.U * np.abs(shifted)
        assert 0.05 < ((want > 0.0) & (want < 1.0)).mean()                      # the clamp leaves something to compare
        for layout in ("plain", "ilv"):
            t0, t1 = pkg.alloc_textures(grid)
            t0.fill_(-7.0), t1.fill_(-7.0)
            vol = torch.full((D, H, W), -7.0, device="cuda")
            prog.fill_grid(grid, t0, t1, dist=vol, flags=K.PASS_VOLUME_INTERLEAVED if layout == "ilv" else 0)
            torch.cuda.synchronize()
            within(t0[..., 0].cpu().numpy().reshape(-1), want, tol, f"scene {name}, tex0.r of the fill, {layout} volume")
            v = vol.cpu().numpy()
            if layout == "ilv":                                                  # entry ((row >> 1) * W + x) * 2 + (row & 1)
                v = v.reshape(D * H // 2, W, 2).transpose(0, 2, 1)
            within(v.reshape(-1), want, tol, f"scene {name}, the {layout} volume of the fill")
