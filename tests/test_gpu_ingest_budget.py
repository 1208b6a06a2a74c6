"""The ingest path's time budget and its failure modes, with providers unlike the uniform gyroid: a provider whose cost per sample
jumps mid-pass (tests/c/gyroid_provider.c -DGYROID_COST_NS: 10 us per point in the upper third of the box) must not make one
update(sdf, 30 ms) call run for hundreds of milliseconds, and an SDF whose sample() throws on the calling thread must not leave
voxels behind that the host believes loaded and the device never received (tests/c/ingest_throw.cpp).  Every state is still
the oracle's loop advanced by the returned count, bit for bit."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

from test_gpu_ingest import RefViewer, assert_viewer_equals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COST = 10e-6            # s per sample where p.z > 0.25
BUDGET = 0.030          # the reference's frame budget
CALL_LIMIT = 0.100      # budget + one gather (2048 samples ~ 20 ms) + slack
DIMS = (96, 48, 72)
SLOW_Z = 0.25


@pytest.fixture(scope="module")
def slow_gyroid(tmp_path_factory):
    """The gyroid fixture with a 10 us cost per point above z = 0.25 whose edit reports the box z in [0.25, 0.75] (the same gcc line
    as conftest._build_provider)."""
    out = tmp_path_factory.mktemp("slow_gyroid") / "libslow_gyroid.so"
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall",
                           "-Wextra", "-Werror", f"-DGYROID_COST_NS={int(COST * 1e9)}", "-DGYROID_EDIT_HIGH_Z", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "gyroid_provider.c"), "-o", str(out), "-lm"])
    return str(out)


def lattice(n, step):
    return np.arange(0, n, step)


def z_coords(bb):
    """f32 z coordinate of every voxel, as update() computes it (scene/sdf/mod.rs:179-182)."""
    d = DIMS[2]
    z = np.arange(d, dtype=np.float32) / np.float32(d - 1)
    return z * np.float32(bb[5] - bb[2]) + np.float32(bb[2])


def slow_samples_fresh(bb):
    """A fresh load samples every voxel once, whatever the number of passes (a later pass skips what an earlier one loaded)."""
    return DIMS[0] * DIMS[1] * int((z_coords(bb) > SLOW_Z).sum())


def slow_samples_box_edit(bb, steps=(4, 2, 1)):
    """A box edit re-samples every box voxel of every pass lattice that holds it (the box test, not the mirror, lets it through)."""
    z = z_coords(bb)
    return sum(len(lattice(DIMS[0], s)) * len(lattice(DIMS[1], s)) * int((z[lattice(DIMS[2], s)] >= SLOW_Z).sum()) for s in steps)


class Calls:
    """The update(sdf, 30 ms) calls of one phase, timed."""

    def __init__(self, what):
        self.what, self.times, self.counts = what, [], []

    def update(self, v, sdf):
        t0 = time.perf_counter()
        n = v.update(sdf, BUDGET)
        self.times.append(time.perf_counter() - t0)
        self.counts.append(n)
        return n

    def msg(self, extra=""):
        t = np.asarray(self.times)
        k = int(t.argmax())
        return (f"{self.what}: {len(t)} calls, max {t[k] * 1e3:.1f} ms (call {k}, {self.counts[k]} voxels), "
                f"mean {t.mean() * 1e3:.1f} ms {extra}")

    def check(self, slow, threads):
        t = np.asarray(self.times)
        assert t.max() < CALL_LIMIT, self.msg()
        allowed = 1.5 * slow * COST / threads + 0.5
        assert t.sum() <= allowed, self.msg(f"total {t.sum():.2f} s > {allowed:.2f} s for {slow} slow samples")
        print(self.msg(f"total {t.sum():.2f} s (at most {allowed:.2f} s)"))


def load(host, oracle, lib, passes, threads, rng, what):
    sdf, raw = host.SDF.provider(lib), C.CDLL(lib)
    bb = sdf.bounding_box()
    v = host.Viewer.new_voxels(DIMS, bb, passes)
    v.set_ingest(threads, 0)
    ref = RefViewer(oracle, DIMS, bb, passes, raw.gyroid_sample_raw)
    # the viewer's set-up (transfer buffers, host mirror, worker threads, the process's first launch) happens in its first
    # update(): a zero budget makes that call one voxel per worker, timed apart from the frame loop (as bench.py's ingest does)
    n = v.update(sdf, 0.0)
    assert n > 0 and v.last_error() == "" and ref.update(None, n) == n
    calls = Calls(what)
    while v.remaining():
        n = calls.update(v, sdf)
        assert n > 0 and v.last_error() == "", calls.msg()
        assert ref.update(None, n) == n, calls.msg()
        assert calls.times[-1] < CALL_LIMIT, calls.msg()
        if rng.integers(4) == 0:
            assert_viewer_equals(v, ref, calls.msg())
    assert_viewer_equals(v, ref, calls.msg("(loaded)"))
    calls.check(slow_samples_fresh(bb), threads)
    return sdf, bb, v, ref


@pytest.mark.parametrize("threads", [1, 4])
def test_a_cost_cliff_keeps_every_call_within_the_budget(host, oracle, slow_gyroid, threads):
    """Fresh loads (one pass, then three) and a box edit after the complete load, through update(sdf, 30 ms) with the default
    buffers: the cheap voxels -- the lower two thirds of every pass, or the skips before the changed box -- come first, the 10 us
    samples after them.  Every call returns some voxels and ends well within budget + one gather; the load keeps its pace;
    every state checked equals the oracle's loop advanced by the returned counts."""
    rng = np.random.default_rng(100 + threads)
    load(host, oracle, slow_gyroid, 1, threads, rng, f"one-pass load, {threads} thread(s)")
    sdf, bb, v, ref = load(host, oracle, slow_gyroid, 3, threads, rng, f"three-pass load, {threads} thread(s)")
    assert sdf.set_parameter(0, 0.3) is None
    box = np.float32([bb[0], bb[1], SLOW_Z, bb[3], bb[4], bb[5]])
    calls = Calls(f"box edit, {threads} thread(s)")
    first = True
    for _ in range(100000):
        n = calls.update(v, sdf)
        assert v.last_error() == "", calls.msg()
        assert ref.update(box if first else None, n) == n, calls.msg()
        assert calls.times[-1] < CALL_LIMIT, calls.msg()
        first = False
        if n == 0 and not v.has_changed_box():
            break
        assert n > 0, calls.msg()
        if rng.integers(4) == 0:
            assert_viewer_equals(v, ref, calls.msg())
    assert not v.has_changed_box() and ref.box is None, calls.msg()
    assert_viewer_equals(v, ref, calls.msg("(edit worked off)"))
    calls.check(slow_samples_box_edit(bb), threads)
    assert sdf.set_parameter(0, 0.15) is None and sdf.changed() is not None   # (the fixture's default)


@pytest.fixture(scope="module")
def ingest_throw(tmp_path_factory):
    """tests/c/ingest_throw.cpp linked against the product library the way sdf-viewer-host-bench is."""
    lib = os.path.join(ROOT, "sdf-viewer_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")   # (the host Makefile's ROCM)
    exe = tmp_path_factory.mktemp("ingest_throw") / "ingest_throw"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(rocm, "include"), "-I", os.path.join(lib, "host"),
                           os.path.join(ROOT, "tests", "c", "ingest_throw.cpp"), "-o", str(exe), "-L", lib, "-lsdfviewer_host",
                           "-lsdfgrid", "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib"),
                           "-Wl,-rpath," + lib, "-ldl", "-pthread"])
    return str(exe)


@pytest.mark.parametrize("threads", [1, 4])
def test_a_throwing_sample_leaves_the_load_intact(ingest_throw, threads):
    """An application's SDFSurface whose sample() throws once on the calling thread, during a fresh load and again during a box
    edit: update() hands the exception to the caller after its workers have stopped, and the viewer's later calls finish the
    load -- tex0, tex1 and the distance volume end byte-identical to a viewer that loaded the same SDF without the throw."""
    r = subprocess.run([ingest_throw, str(threads)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert f"ingest_throw ok threads={threads} exceptions=2" in r.stdout, (r.stdout, r.stderr)
