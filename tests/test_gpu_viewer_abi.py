"""GPU tests of the viewer's C ABI (include/sdfviewer.h) and of its device-sampled route: the emitter kernel against a numpy
restatement of LoadingManager order + positions + update_required, a torch device callback loaded through
sdfv_viewer_update against the oracle's loop fed the same function, a failing callback, and the scene's scheduling with an
injected clock.  Each test runs under its own time limit."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

from program_fill_check import interleave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    return importlib.import_module("sdf-viewer_amd.viewer")


def coords(dims, bb_min, bb_max):
    """idx as f32 / (dim - 1) * size + min, three separately rounded f32 steps (scene/sdf/mod.rs:179-182)"""
    out = []
    for a in range(3):
        i = np.arange(dims[a], dtype=np.float32)
        dm1 = np.float32(dims[a]) - np.float32(1)
        size = np.float32(bb_max[a]) - np.float32(bb_min[a])
        out.append(((i / dm1) * size) + np.float32(bb_min[a]))
    return out


def emit_reference(dims, bb_min, bb_max, step, cursor, n, box, vol, air):
    W, H, D = dims
    nx, ny = -(-W // step), -(-H // step)
    c = np.arange(cursor, cursor + n, dtype=np.int64)
    x, y, z = (c % nx) * step, (c // nx % ny) * step, (c // (nx * ny)) * step
    flat = (z * H + y) * W + x
    cx, cy, cz = coords(dims, bb_min, bb_max)
    px, py, pz = cx[x], cy[y], cz[z]
    req = vol.reshape(-1)[flat] == air
    if box is not None:
        req |= (px >= box[0]) & (px <= box[3]) & (py >= box[1]) & (py <= box[4]) & (pz >= box[2]) & (pz <= box[5])
    pts = np.stack([px, py, pz], axis=1)[req]
    return pts, flat[req].astype(np.uint32)


@pytest.mark.timeout(300)
def test_emitter_equals_loading_manager_order_positions_and_update_required(pkg):
    rng = np.random.default_rng(7)
    air = np.float32(pkg.AIR_DIST)
    cases = [((20, 13, 17), (-1.0, -0.5, -0.75), (1.0, 0.5, 0.75), False),
             ((16, 14, 12), (-2.0, -1.0, 0.25), (0.5, 1.5, 3.0), True),
             ((33, 32, 9), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), True),
             ((7, 5, 3), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), False)]
    checked = 0
    for dims, bmin, bmax, ilv in cases:
        W, H, D = dims
        vol = rng.uniform(0.0, 1.0, (D, H, W)).astype(np.float32)
        vol[rng.uniform(size=vol.shape) < 0.4] = air
        dev_vol = torch.from_numpy(interleave(vol) if ilv else vol.reshape(-1)).cuda()
        g = pkg.make_grid(dims, bmin, bmax)
        for _ in range(12):
            step = int(2 ** rng.integers(0, 4))
            total = (-(-W // step)) * (-(-H // step)) * (-(-D // step))
            cursor = int(rng.integers(0, total))
            n = int(rng.integers(0, total - cursor + 1))
            box = None
            if rng.uniform() < 0.6:
                lo = rng.uniform(bmin, bmax).astype(np.float32)
                hi = (lo + rng.uniform(0.0, 1.0, 3)).astype(np.float32)
                box = np.concatenate([lo, hi]).astype(np.float32)
            want_p, want_i = emit_reference(dims, bmin, bmax, step, cursor, n, box, vol, air)
            pts = torch.full((max(n, 1), 3), float("nan"), device="cuda")
            idx = torch.full((max(n, 1),), 0xFFFFFFF, dtype=torch.int32, device="cuda")
            count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            scratch_bytes = pkg.lib.sdfv_emit_update_points_scratch_bytes(max(n, 1))
            scratch = torch.empty(max(scratch_bytes, 1), dtype=torch.uint8, device="cuda")
            cb = (C.c_float * 6)(*box) if box is not None else None
            flags = pkg._capi.PASS_VOLUME_INTERLEAVED if ilv else 0
            rc = pkg.lib.sdfv_emit_update_points(C.byref(g), step, cursor, n, cb, dev_vol.data_ptr(), flags, pts.data_ptr(),
                                                 idx.data_ptr(), count.data_ptr(), scratch.data_ptr(), scratch_bytes,
                                                 torch.cuda.current_stream().cuda_stream)
            assert rc == 0, pkg.lib.sdfv_last_error()
            torch.cuda.synchronize()
            k = int(count.item())
            assert k == len(want_i), (dims, step, cursor, n, box)
            np.testing.assert_array_equal(idx[:k].cpu().numpy().view(np.uint32), want_i)
            np.testing.assert_array_equal(pts[:k].cpu().numpy().view(np.uint32), want_p.view(np.uint32))
            checked += k
    assert checked > 1000


# ---- a union of axis-aligned boxes: subtraction, abs, max and min only, so host and device round identically ----
BOXES = np.array([[-0.4, -0.1, 0.0, 0.45, 0.3, 0.5], [0.35, 0.2, -0.3, 0.3, 0.25, 0.35]], np.float32)  # centre, half size
BB = (-1.0, -0.6, -0.8, 1.0, 0.6, 0.8)


def boxes_np(p, half_scale):
    d = None
    for b in BOXES:
        q = np.abs(p - b[:3]) - b[3:] * half_scale
        e = np.maximum(np.maximum(q[..., 0], q[..., 1]), q[..., 2])
        d = e if d is None else np.minimum(d, e)
    out = np.zeros(p.shape[:-1] + (7,), np.float32)
    out[..., 0] = d
    out[..., 1] = np.where(p[..., 0] > 0, np.float32(0.9), np.float32(0.0))
    out[..., 2] = np.where(p[..., 1] > 0, np.float32(0.4), np.float32(0.0))
    out[..., 3] = np.where(p[..., 2] > 0, np.float32(1.5), np.float32(0.0))  # (0, 0, 0) occurs: the 0.5 grey default
    out[..., 4] = np.float32(0.25)
    out[..., 5] = np.where(p[..., 0] > p[..., 2], np.float32(0.75), np.float32(0.1))
    out[..., 6] = np.where(p[..., 1] > np.float32(0.2), np.float32(0.0), np.float32(0.6))
    return out


def boxes_torch(p, half_scale):
    b = torch.as_tensor(BOXES, device=p.device)
    q = (p[:, None, :] - b[None, :, :3]).abs() - b[None, :, 3:] * half_scale
    d = q.amax(dim=2).amin(dim=1)
    z = torch.zeros_like(d)
    out = torch.stack([d, torch.where(p[:, 0] > 0, z + 0.9, z), torch.where(p[:, 1] > 0, z + 0.4, z),
                       torch.where(p[:, 2] > 0, z + 1.5, z), z + 0.25, torch.where(p[:, 0] > p[:, 2], z + 0.75, z + 0.1),
                       torch.where(p[:, 1] > 0.2, z, z + 0.6)], dim=1)
    return out


@pytest.mark.timeout(600)
@pytest.mark.parametrize("dims,layout", [((24, 18, 20), 1), ((24, 18, 20), 2), ((21, 17, 11), 1)])
def test_torch_device_callback_loads_like_the_oracle_loop(V, oracle, dims, layout):
    state = {"scale": np.float32(1.0), "changed": None}

    def changed():
        b, state["changed"] = state["changed"], None
        return b
    surf = V.Surface.from_torch(lambda: BB, lambda p: boxes_torch(p, float(state["scale"])), changed=changed)
    v = V.Viewer.new_voxels(dims, BB, 3, layout=layout)
    stream = torch.cuda.Stream()
    v.set_stream(stream.cuda_stream)
    r0, r1 = oracle.grid_init(dims)
    lm = oracle.lm_new(dims, 3)

    @oracle.SAMPLE_FN
    def ref_sample(_user, p, _distance_only, out):
        s = boxes_np(np.array([p[0], p[1], p[2]], np.float32), state["scale"])
        for i in range(7):
            out[i] = s[i]

    def step_and_compare(box):
        n = v.update(surf, budget_ns=0)  # one small run per call: every intermediate state is compared
        assert n > 0
        assert oracle.viewer_update_fn(ref_sample, dims, lm, r0, r1, changed_box=box, max_iterations=n, bb_min=BB[:3],
                                       bb_max=BB[3:]) == n
        t0, t1 = v.download()
        np.testing.assert_array_equal(t0.view(np.uint32), r0.view(np.uint32))
        np.testing.assert_array_equal(t1.view(np.uint32), r1.view(np.uint32))

    steps = 0
    while v.state()["remaining"]:
        step_and_compare(None)
        steps += 1
    assert steps >= 3 and v.state()["lod"] == 1.0
    # an edit that reports a box: the reference's 3-pass reload (scene/sdf/mod.rs:146-156) with the box applied
    state["scale"] = np.float32(0.75)
    box = (-1.0, -0.6, -0.8, 0.1, 0.6, 0.8)
    state["changed"] = box
    lm = oracle.lm_new(dims, 3)
    step_and_compare(box)
    assert v.state()["has_changed_box"]
    while v.state()["remaining"]:
        step_and_compare(box)
    # a callback that fails: the call returns an error naming it, the textures keep what the last complete run left, and a
    # later update finishes the load to the same bits
    state["scale"] = np.float32(0.5)
    state["changed"] = box
    lm = oracle.lm_new(dims, 3)
    good = v.download()
    bad = V.Surface.from_torch(lambda: BB, lambda p: (_ for _ in ()).throw(RuntimeError("refused")), changed=changed)
    rc, n, msg = v.update_rc(bad, 0)
    assert rc == V.ERR_CALLBACK and n == 0 and "sample_batch_device" in msg, (rc, n, msg)
    now = v.download()
    np.testing.assert_array_equal(now[0].view(np.uint32), good[0].view(np.uint32))
    np.testing.assert_array_equal(now[1].view(np.uint32), good[1].view(np.uint32))
    while v.state()["remaining"]:
        step_and_compare(box)
    v.close()


@pytest.mark.timeout(600)
def test_device_route_keeps_a_30ms_budget_over_several_runs(V, oracle):
    """A device callback that costs 2 us per point (a host sleep inside it, the way a slow caller kernel would block the run):
    every 30 ms call ends near its budget although the first run of 4096 points costs 8 ms -- each run is timed to its end and
    the next one sized for the largest cost per sample seen -- calls span several runs and pass boundaries, and every state is
    the oracle's at the same visited count."""
    import time
    dims = (96, 80, 72)
    cost_per_point = 2e-6

    def slow(p):
        time.sleep(p.shape[0] * cost_per_point)
        return boxes_torch(p, 1.0)
    surf = V.Surface.from_torch(lambda: BB, slow)
    v = V.Viewer.new_voxels(dims, BB, 3, layout=1)
    r0, r1 = oracle.grid_init(dims)
    lm = oracle.lm_new(dims, 3)

    @oracle.SAMPLE_FN
    def ref_sample(_user, p, _distance_only, out):
        s = boxes_np(np.array([p[0], p[1], p[2]], np.float32), np.float32(1.0))
        for i in range(7):
            out[i] = s[i]
    took, visits = [], []
    while v.state()["remaining"]:
        t = time.perf_counter()
        n = v.update(surf, budget_s=0.030)
        took.append(time.perf_counter() - t)
        visits.append(n)
        assert oracle.viewer_update_fn(ref_sample, dims, lm, r0, r1, max_iterations=n, bb_min=BB[:3], bb_max=BB[3:]) == n
    t0, t1 = v.download()
    np.testing.assert_array_equal(t0.view(np.uint32), r0.view(np.uint32))
    np.testing.assert_array_equal(t1.view(np.uint32), r1.view(np.uint32))
    assert len(visits) >= 10 and max(visits) > 4096, visits  # (more than one run per call)
    assert max(took) < 0.045, sorted(took)[-5:]
    assert sorted(took)[len(took) // 2] > 0.020, took  # (the calls do use their budget)


@pytest.mark.timeout(300)
def test_a_failure_after_some_runs_reports_what_those_runs_visited(V, oracle):
    """One call, runs of at most 3000 points, the third sampling call fails: the call returns SDFV_ERR_CALLBACK with *visited =
    the iterations of the two runs packed before it, the textures are the oracle's at that count, and a later call finishes."""
    dims = (40, 30, 20)
    calls = {"n": 0}

    def flaky(p):
        calls["n"] += 1
        if calls["n"] == 3:
            raise RuntimeError("refused")
        return boxes_torch(p, 1.0)
    surf = V.Surface.from_torch(lambda: BB, flaky)
    v = V.Viewer.new_voxels(dims, BB, 3, layout=2)
    v.set_ingest(capacity=3000)
    r0, r1 = oracle.grid_init(dims)
    lm = oracle.lm_new(dims, 3)

    @oracle.SAMPLE_FN
    def ref_sample(_user, p, _distance_only, out):
        s = boxes_np(np.array([p[0], p[1], p[2]], np.float32), np.float32(1.0))
        for i in range(7):
            out[i] = s[i]
    rc, n, msg = v.update_rc(surf, 10 ** 10)
    assert rc == V.ERR_CALLBACK and "sample_batch_device" in msg, (rc, msg)
    assert n == 10 * 8 * 5 + 3000, n  # the step-4 pass (one run), one run of the step-2 pass; the next run failed
    assert oracle.viewer_update_fn(ref_sample, dims, lm, r0, r1, max_iterations=n, bb_min=BB[:3], bb_max=BB[3:]) == n
    t0, t1 = v.download()
    np.testing.assert_array_equal(t0.view(np.uint32), r0.view(np.uint32))
    np.testing.assert_array_equal(t1.view(np.uint32), r1.view(np.uint32))
    assert v.state()["total_iterations"] == n
    n2 = v.update(surf, budget_s=10.0)
    assert oracle.viewer_update_fn(ref_sample, dims, lm, r0, r1, max_iterations=n2, bb_min=BB[:3], bb_max=BB[3:]) == n2
    assert v.state()["remaining"] == 0
    t0, t1 = v.download()
    np.testing.assert_array_equal(t0.view(np.uint32), r0.view(np.uint32))
    np.testing.assert_array_equal(t1.view(np.uint32), r1.view(np.uint32))


@pytest.mark.timeout(600)
def test_host_callbacks_load_like_the_oracle_loop_and_a_failure_drops_its_run(V, oracle):
    dims = (20, 16, 14)
    fail_at = {"left": -1}

    def sample_batch(pts, _d):
        if fail_at["left"] >= 0:
            fail_at["left"] -= len(pts)
            if fail_at["left"] < 0:
                raise RuntimeError("refused")
        return boxes_np(pts.astype(np.float32), np.float32(1.0))
    surf = V.Surface.from_callbacks(lambda: BB, sample_batch=sample_batch)
    v = V.Viewer.new_voxels(dims, BB, 3, layout=1)
    r0, r1 = oracle.grid_init(dims)
    lm = oracle.lm_new(dims, 3)

    @oracle.SAMPLE_FN
    def ref_sample(_user, p, _distance_only, out):
        s = boxes_np(np.array([p[0], p[1], p[2]], np.float32), np.float32(1.0))
        for i in range(7):
            out[i] = s[i]
    n = v.update(surf, budget_ns=0)
    oracle.viewer_update_fn(ref_sample, dims, lm, r0, r1, max_iterations=n, bb_min=BB[:3], bb_max=BB[3:])
    fail_at["left"] = 0  # the next sample_batch call fails (a call's first run is one voxel)
    rc, n_bad, msg = v.update_rc(surf, 0)
    assert rc == V.ERR_CALLBACK and n_bad == 0 and "sample_batch" in msg, (rc, msg)
    t0, t1 = v.download()
    np.testing.assert_array_equal(t0.view(np.uint32), r0.view(np.uint32))
    np.testing.assert_array_equal(t1.view(np.uint32), r1.view(np.uint32))
    fail_at["left"] = -1
    n = v.update(surf, budget_s=10.0)
    assert oracle.viewer_update_fn(ref_sample, dims, lm, r0, r1, max_iterations=n, bb_min=BB[:3], bb_max=BB[3:]) == n
    assert v.state()["remaining"] == 0
    t0, t1 = v.download()
    np.testing.assert_array_equal(t0.view(np.uint32), r0.view(np.uint32))
    np.testing.assert_array_equal(t1.view(np.uint32), r1.view(np.uint32))


@pytest.mark.timeout(300)
def test_scene_frame_scheduling_with_an_injected_clock(V, pkg, oracle):
    """test_gpu_host.py::test_scene_frame_scheduling through sdfv_scene_*: the demo handed over as device_params."""
    clock = {"ns": 0}
    prm = pkg.default_params()
    demo = V.Surface.from_callbacks(lambda: (-1, -1, -1, 1, 1, 1), device_params=prm)
    sc = V.Scene(demo, clock=lambda: clock["ns"])
    assert sc.viewer().state()["dims"] == (32, 32, 32)
    sc.set_surface(demo, max_voxels_side=24, loading_passes=3)
    assert sc.viewer().state()["dims"] == (24, 24, 24) and sc.load_progress() is None
    sc.set_budget(0, 500)
    passes = [6 ** 3, 12 ** 3, 24 ** 3]
    assert sc.render() == dict(cpu_updates=passes[0], committed=True, last_chunk=False, request_repaint=True)
    assert sc.viewer().state()["lod"] == 4.0
    prog, text = sc.load_progress()
    total = sum(passes)
    assert abs(prog - passes[0] / total) < 1e-6
    assert text == f"Loading SDF {100 * passes[0] / total:.2f}% (2 levels of detail left, evaluations: {passes[0]} / {total})"
    clock["ns"] += 100_000_000
    assert sc.render() == dict(cpu_updates=passes[1], committed=False, last_chunk=False, request_repaint=True)
    assert sc.viewer().state()["lod"] == 2.0
    clock["ns"] += 450_000_000
    assert sc.render() == dict(cpu_updates=passes[2], committed=True, last_chunk=False, request_repaint=True)
    assert sc.render() == dict(cpu_updates=0, committed=True, last_chunk=True, request_repaint=True)
    assert sc.viewer().state()["lod"] == 1.0 and sc.load_progress() is None
    r, img = sc.render(96, 54, draw=True)
    assert r == dict(cpu_updates=0, committed=False, last_chunk=False, request_repaint=False)
    torch.cuda.synchronize()
    dims = (24, 24, 24)
    r0, r1 = oracle.fill_dense(oracle.default_params(), dims)
    want, _ = oracle.raymarch(oracle.default_render_params(dims), r0, r1, oracle.camera_look_at(aspect=96 / 54), 96, 54,
                              want_aux=False)
    assert np.abs(img.cpu().numpy() - want).max() <= 1e-4
    sc.close()


@pytest.mark.timeout(900)
def test_plain_c_host(tmp_path):
    """tests/c/viewer_host.c: C11, no C++ -- the viewer's ABI against the oracle's loop (liboracle.so)."""
    exe = tmp_path / "viewer_host"
    lib = os.path.join(ROOT, "sdf-viewer_amd")
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(ROOT, "oracle"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c", "viewer_host.c"), "-o", str(exe), "-L", lib, "-lsdfviewer_host", "-lsdfgrid",
           "-L", os.path.join(ROOT, "oracle"), "-loracle", "-L", "/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(ROOT, "oracle"), "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=800)
    assert r.returncode == 0 and r.stdout.strip().endswith("viewer_host ok"), r.stdout[-3000:] + r.stderr[-3000:]
