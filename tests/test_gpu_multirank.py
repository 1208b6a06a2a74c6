"""The N>1 bench path (z-slab fill + halo exchange + replica gather + per-rank cameras) end to end on the ONE GPU
of the test box: two ranks share the device and talk over gloo (host-staged slices).  On a real node the same
code runs one rank per GPU over RCCL; here only the logic is checked, not the speed."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config", "roofline")
CONTRACT_LIMIT = 4096  # the 22 KB line of round 4 outgrew the driver's capture (BENCH_r04.json parsed: null)


def _no_constants(name):
    raise ValueError(f"{name} in the contract line: not JSON")


def run_bench(cmd, env=None, tmp_path=None, timeout=900):
    """Runs bench.py; returns (contract line = the LAST line of stdout, parsed strictly; the full record it points at; the
    CompletedProcess).  The contract line is what the driver parses: short, one line, nothing after it."""
    env = dict(os.environ if env is None else env)
    full_path = os.path.join(str(tmp_path), "bench_full.json") if tmp_path is not None else None
    if full_path:
        env["SDFV_BENCH_FULL_JSON"] = full_path
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines and lines[-1].startswith("{"), out.stdout[-500:]
    assert len([l for l in lines if l.startswith("{")]) == 1, "exactly one JSON line on stdout"
    assert len(lines[-1].encode()) < CONTRACT_LIMIT, len(lines[-1])
    c = json.loads(lines[-1], parse_constant=_no_constants)
    for key in CONTRACT_KEYS:
        assert key in c, key
    path = c["full"] if os.path.isabs(c["full"]) else os.path.join(ROOT, c["full"])
    full = json.loads(open(path).read(), parse_constant=_no_constants)
    assert "[bench full record] {" in out.stderr
    for key in ("value", "value_rays", "ms_per_step", "n_gpus", "steps", "warmup", "pipeline"):
        assert c[key] == full[key], key  # the short line is an excerpt of the record, not a second measurement
    assert c["roofline"]["frac"] == full["roofline"]["frac"] and c["roofline"]["avg_launch_ms"] == full["roofline"]["avg_launch_ms"]
    return c, full, out


@pytest.mark.parametrize("world,geometry", [(2, "slab"), (4, "cube"), (8, "slab"), (8, "cube")])
def test_bench_weak_scaling_path_two_ranks_one_gpu(world, geometry, tmp_path):
    """2, 4 and 8 ranks (the driver's SCALE run uses 1, 2, 4, 8) sharing the box's one GPU over gloo, both weak geometries."""
    env = dict(os.environ, SDFV_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    port = 29600 + world + os.getpid() % 300
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--full",
           "--gpus", str(world), "--steps", "2", "--warmup", "1", "--workload", "64", "--no-cpu-baseline",
           "--config4-side", "32", "--prewarm-ms", "5", "--per-step-samples", "4",
           "--weak-geometry", geometry]
    c, d, out = run_bench(cmd, env, tmp_path)
    assert c["config4"]["value"] > 0 and c["sharded_fill_verified"] is True and c["sharded_march"]["verified"] is True
    assert c["batch_raymarch"]["gather_ms"] > 0 and c["batch_raymarch"]["camera_split"]["gather_ms"] > 0
    assert d["n_gpus"] == world and d["scaling"] == "weak" and d["steps"] == 2
    assert d["config"]["voxels_per_gpu"] == 64 ** 3
    gx, gy, gz = d["config"]["grid_global"]
    assert gx * gy * gz == world * 64 ** 3
    cube = {2: (64, 64, 128), 4: (64, 128, 128), 8: (128, 128, 128)}[world]
    assert (gx, gy, gz) == ((64, 64, 64 * world) if geometry == "slab" else cube)
    assert d["value"] > 0 and d["value_rays"] > 0
    # the N > 1 line = the N = 1 contract + config4 + what RCCL saw (None here: gloo carries the halo, not the library's RCCL)
    for key in CONTRACT_KEYS + ("config4", "rccl_ranks", "torch_world_size", "roofline_raymarch", "batch_raymarch",
                                "ms_per_step_median", "ms_per_step_p95"):
        assert key in d, key
    assert d["rccl_ranks"] is None and d["torch_world_size"] == world
    assert d["roofline"]["frac_8d"] > 0 and d["roofline"]["algorithmic_bytes_per_voxel"] == 32
    # config 5 as BASELINE names it (image-tile split, balanced: interleaved tile bands) is the batch's top level; the
    # contiguous-rows form of the same split and the camera split ride beside it
    b = d["batch_raymarch"]
    assert b["value"] > 0 and b["split"] == "tiles" and b["rows_per_gpu"] == 512 // world and b["cameras_per_gpu"] == 64
    assert b["camera_split"]["value"] > 0 and b["camera_split"]["cameras_per_gpu"] == 64 // world
    assert b["contiguous_rows_split"]["value"] > 0 and b["contiguous_rows_split"]["rows_per_gpu"] == 512 // world
    # SURVEY 8(e)'s collective of config 5 is in the line with its own number (torch.distributed here: gloo carries it)
    for rep in (b, b["camera_split"], b["contiguous_rows_split"]):
        assert rep["gather_ms"] > 0 and 0 < rep["value_incl_gather"] < rep["value"], rep
        assert rep["gather_bytes_to_rank0"] == 64 * 512 * 512 * 16 * (world - 1) // world
    assert "torch.distributed" in b["gather_transport"]
    assert d["sharded_fill_verified"] is True  # gathered slabs == dense fill, ghost slices == neighbour's slices
    c4 = d["config4"]  # the cube geometry next to the default one, in the same line
    assert c4["value"] > 0 and c4["voxels_per_gpu"] == 32 ** 3 and len(c4["grid_global"]) == 3, c4
    # the grid raymarched where it lies (rays handed between the ranks over gloo) == the march over the whole grid
    assert d["sharded_march"]["verified"] is True, d["sharded_march"]


def test_bench_line_carries_the_whole_contract(tmp_path):
    """Every key the driver's contract names is in bench.py's short JSON line (N = 1, tiny workload): under 4 KB, strict JSON,
    the last line of stdout; everything else the run measured is in the full record it names."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--workload", "64",
           "--cpu-baseline-seconds", "1", "--prewarm-ms", "5"]
    c, d, out = run_bench(cmd, None, tmp_path, timeout=600)
    for key in ("cpu_baseline", "ms_per_step_median", "ms_per_step_p95", "roofline_raymarch", "host_load", "progressive", "box"):
        assert key in c, key
    assert c["n_gpus"] == 1 and c["steps"] == 2 and c["warmup"] == 1 and c["higher_is_better"] is True
    assert c["scaling"] == "weak" and c["vs_baseline"] is None and c["dtype"] == "f32" and "workload" in c["config"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "algorithmic_bytes_per_launch", "avg_launch_ms"):
        assert key in c["roofline"], key
    for key in ("value", "unit", "cores", "kind", "sample", "all_cores", "value_rays"):
        assert key in c["cpu_baseline"], key
    assert c["roofline"]["bound"] == "hbm" and c["cpu_baseline"]["kind"] == "port" and c["incomplete"] is None
    assert c["roofline"]["target_512"]["plain"]["frac_8d"] > 0 and c["roofline"]["target_512"]["fused"]["frac_8d"] > 0
    assert c["roofline"]["target_512"]["fused_ilv"]["frac_8d"] > 0  # the fill SDFViewer runs at that size
    assert c["host_load"]["64"]["update_ms"] > 0 and c["progressive"]["64"]["virgin_load_2_passes"][0] > 0
    for key in CONTRACT_KEYS + ("cpu_baseline", "ms_per_step_median", "ms_per_step_p95", "per_step"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and "workload" in d["config"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in d["roofline"], key
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in d["cpu_baseline"], key
    assert d["roofline"]["bound"] == "hbm" and d["cpu_baseline"]["kind"] == "port"
    # one consistent pipeline: value / value_rays / ms_per_step / roofline all come from `pipeline`
    pipe = d["pipeline_" + d["pipeline"]]
    assert d["pipeline"] in ("plain", "fused", "fused_ilv") and abs(pipe["ms_per_step"] - d["ms_per_step"]) < 1e-3
    # the roofline is priced on 32 B/voxel whatever the launch stores; the bus figure rides beside it
    assert d["roofline"]["algorithmic_bytes_per_voxel"] == 32 and d["roofline"]["frac"] == d["roofline"]["frac_8d"]
    assert d["roofline"]["bus_bytes_per_voxel"] == (32 if d["pipeline"] == "plain" else 36)
    assert abs(d["roofline"]["frac_8d"] * 36 / 32 - d["roofline"]["frac_bus"]) < 2e-3 or d["pipeline"] == "plain"
    assert d["per_step"]["fill"]["median"] > 0 and d["per_step"]["raymarch"]["p95"] >= d["per_step"]["raymarch"]["median"]
    for name in ("plain", "fused", "fused_ilv"):  # the reported pipeline is the fastest of the three, end to end
        assert pipe["ms_per_step"] <= d["pipeline_" + name]["ms_per_step"], name
    assert d["target_512"]["frac"] > 0 and d["target_512"]["grid"] == [512, 512, 512]
    assert d["target_512"]["frac_8d"] == d["target_512"]["frac"] and 0 < d["target_512"]["fused_commit"]["frac_8d"] < d["target_512"]["fused_commit"]["frac"]
    rr = d["roofline_raymarch"]
    assert "note" in rr and rr["avg_launch_ms"] > 0
    # round 4: the target configuration's fractions inside the nested object the driver's record keeps whole; the drop-in
    # host's load through libsdfviewer_host.so; where the line was measured; no extra hung
    t = d["roofline"]["target_512"]
    assert t["plain"]["frac_8d"] == d["target_512"]["frac_8d"] and t["fused"]["frac_8d"] == d["target_512"]["fused_commit"]["frac_8d"]
    assert d["incomplete"] is None and d["box"]["arch"].startswith("gfx950")
    h = d["host_load"]["64"]
    assert h["dense"]["update_calls"] == 1 and h["progressive"]["update_calls"] == 2 and h["dense"]["load_ms"] > 0
    assert h["dense"]["iterations"] == 64 ** 3 + 32 ** 3 == h["progressive"]["iterations"]
    assert d["progressive"]["64"]["virgin_load_2_passes"]["ms"] > 0


def test_plain_bench_run_times_the_headline_alone_and_dumps_its_outputs(tmp_path, pkg, oracle):
    """A plain run (no --full): the probe's pick is the one pipeline timed, for exactly --steps steps, and nothing beside the
    headline is measured.  --dump-outputs writes the last timed step's textures and frame: the same words in two runs, the
    textures those of the oracle's 64^3 fill, the frame within the RGBA tolerance of the oracle's march."""
    import numpy as np
    dumps = []
    for k in range(2):
        where = tmp_path / f"dump{k}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--workload", "64",
               "--prewarm-ms", "5", "--dump-outputs", str(where)]
        c, d, out = run_bench(cmd, None, tmp_path, timeout=600)
        assert c["steps"] == 7 and c["warmup"] == 2 and c["full_run"] is False and c["dtype"] == "f32" and c["higher_is_better"] is True
        assert abs(c["ms_per_step"] - c["ms_per_step_fill"] - c["ms_per_step_raymarch"]) < 1e-3 and c["value"] > 0
        probe = d["pipeline_probe"]["ms_per_step"]
        # the pick is the fastest probe; the line carries the probe times rounded to 1e-4 ms, where two of them can tie
        assert sorted(probe) == ["fused", "fused_ilv", "plain"] and probe[d["pipeline"]] == min(probe.values())
        for name in ("plain", "fused", "fused_ilv"):  # only the picked pipeline was timed
            assert (d["pipeline_" + name] is not None) == (name == d["pipeline"]), name
        assert abs(d["pipeline_" + d["pipeline"]]["ms_per_step"] - d["ms_per_step"]) < 1e-3
        assert d["roofline"]["frac"] > 0 and d["roofline_raymarch"]["avg_launch_ms"] > 0
        assert "cpu_baseline" not in d and "per_step" not in d and d["pipeline_overlapped"] is None and d["box"] is None
        assert all(d[key] is None for key in ("target_512", "progressive", "host_load", "ingest", "batch_raymarch", "halo_loopback"))
        arrays = {name: np.load(where / f"{name}.npy") for name in ("tex0", "tex1", "rgba")}
        assert sorted(os.listdir(where)) == ["rgba.npy", "tex0.npy", "tex1.npy"]
        assert all(a.dtype == np.float32 for a in arrays.values())
        assert arrays["tex0"].shape == arrays["tex1"].shape == (64, 64, 64, 4) and arrays["rgba"].shape == (1, 512, 512, 4)
        dumps.append(arrays)
    for name in ("tex0", "tex1", "rgba"):
        assert np.array_equal(dumps[0][name].view(np.uint32), dumps[1][name].view(np.uint32)), name
    r0, r1 = oracle.fill_dense(oracle.default_params(), (64, 64, 64), threads=4)
    assert np.array_equal(dumps[0]["tex0"].view(np.uint32), r0.view(np.uint32))
    assert np.array_equal(dumps[0]["tex1"].view(np.uint32), r1.view(np.uint32))
    rp = oracle.copy_struct(oracle.RenderParams, pkg.default_render_params(pkg.make_grid((64, 64, 64))))
    cam = oracle.copy_struct(oracle.Camera, pkg.camera_look_at(aspect=1.0))
    want, _ = oracle.raymarch(rp, r0, r1, cam, 512, 512, threads=4, want_aux=False)
    assert float(np.abs(dumps[0]["rgba"][0] - want).max()) <= 1e-4


def test_bench_multi_gpu_path_over_rccl_in_loopback(tmp_path):
    """The N > 1 path under the backend the driver uses (nccl = RCCL), as far as one GPU can take it: world size 1 with
    SDFV_BENCH_FORCE_MULTI=1 -- torch's RCCL process group AND the library's own RCCL communicator in one process, the rank
    its own z-neighbour, the fused slab step, config 4's geometry on the same communicator, the collectives of the
    self-checks on device tensors.  (Two ranks on one device are refused by RCCL: test below.)"""
    env = dict(os.environ, SDFV_BENCH_FORCE_MULTI="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29700 + os.getpid() % 200),
               WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "64",
           "--no-cpu-baseline", "--config4-side", "32", "--prewarm-ms", "5"]
    c, d, out = run_bench(cmd, env, tmp_path, timeout=600)
    assert c["loopback"] is True and c["rccl_ranks"] == 1 and c["roofline"]["rccl_ranks"] == 1 and c["halo_transport"] == "sdfv_slab_fill_step"
    assert d["loopback"] is True and d["backend"] == "rccl" and d["n_gpus"] == 1
    assert d["halo_transport"].startswith("sdfv_slab_fill_step"), (d["halo_transport"], out.stderr[-1500:])
    assert d["sharded_fill_verified"] is True, (d["sharded_fill_verified"], out.stderr[-1500:])
    assert d["value"] > 0 and d["value_rays"] > 0 and d["pipeline"] == "fused"
    assert d["config4"]["value"] > 0, d["config4"]
    assert d["rccl_ranks"] == 1 and d["rccl_rank_of_rank0"] == 0 and d["torch_world_size"] == 1  # ncclCommCount of the library communicator
    assert d["roofline"]["rccl_ranks"] == 1  # ... also inside the nested object the driver's record keeps whole
    b = d["batch_raymarch"]  # the batch's gather ran over the library communicator (sdfv_comm_gather_bands)
    assert b["gather_ms"] > 0 and "library RCCL communicator" in b["gather_transport"], b
    assert "skipped" in str(d["sharded_march"]["verified"])  # a periodic slab; the gloo runs above cover the sharded march


def test_two_processes_on_one_gpu_over_the_library_rccl_communicator():
    """two ranks, one device, RCCL (no loopback wrap, no gloo).  RCCL either accepts two ranks on the
    same GPU -- then the fill step's ghosts must equal the neighbour's slices -- or refuses; the refusal is then a
    clean status code with RCCL's message on both ranks (and is what DESIGN.md 6 records)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rccl_two_ranks_one_gpu.py")], cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["backend"] == "rccl" and d["ranks"] == 2
    if d["same_device_accepted"]:
        for r in d["ranks_out"]:
            assert r["result"]["rc"] == 0 and r["result"]["ghosts_and_owned_equal_dense_fill"] is True, d
    else:
        for r in d["ranks_out"]:
            assert r["result"] is not None and r["result"]["stage"] in ("comm_create", "unique_id"), d
            assert r["result"]["rc"] == -5 and "RCCL" in r["result"]["error"], d


def _auto_transport_worker(rank, world, port, q):
    """SlabFiller(transport="auto") with CUDA tensors, a distance volume and world > 1: the constructor asks the process
    group for its backend (a parameter named `dist` once shadowed the torch.distributed alias right there)."""
    import importlib
    import torch
    import torch.distributed as c10d
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    c10d.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pkg = importlib.import_module("sdf-viewer_amd")
        par = importlib.import_module("sdf-viewer_amd.parallel")
        torch.cuda.set_device(0)
        dims = (64, 32, 24)
        prm = pkg.default_params()
        slab = par.alloc_slab(dims, rank, world, "cuda", fill_value=-7.0)
        vol = torch.full(tuple(slab.tex0.shape[:3]), -7.0, dtype=torch.float32, device="cuda")
        filler = par.SlabFiller(pkg, prm, dims, slab, rank, world, transport="auto", dist=vol)
        for _ in range(2):
            filler.step()
        torch.cuda.synchronize()
        full = pkg.make_grid(dims)
        f0, f1 = pkg.alloc_textures(full)
        pkg.fill_grid(prm, full, f0, f1)
        lo, hi = slab.z_begin - slab.ghost_lo, slab.z_end + slab.ghost_hi
        ok = filler.transport == "torch"  # gloo: the torch transport is what "auto" must resolve to
        ok &= torch.equal(slab.tex0.view(torch.int32), f0[lo:hi].view(torch.int32))
        ok &= torch.equal(slab.tex1.view(torch.int32), f1[lo:hi].view(torch.int32))
        ok &= torch.equal(vol.view(torch.int32), f0[lo:hi, ..., 0].contiguous().view(torch.int32))
        q.put((rank, bool(ok)))
    finally:
        c10d.destroy_process_group()


def test_slab_filler_auto_transport_with_distance_volume_two_ranks():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29900 + os.getpid() % 90
    procs = [ctx.Process(target=_auto_transport_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok in results), results


def test_watchdog_prints_the_measured_line_when_an_extra_hangs(tmp_path):
    """First-contact insurance: once the contract's two timed regions are in, a hang in any EXTRA (self-check, config-4 block,
    batch ...) must not lose them.  SDFV_BENCH_EXTRAS_S = 0.01 makes the watchdog fire inside the first extra: the process
    exits 0 and its one JSON line carries value / value_rays / ms_per_step / roofline plus a "watchdog" note naming the stage."""
    env = dict(os.environ, SDFV_BENCH_EXTRAS_S="0.01")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--workload", "64",
           "--no-cpu-baseline", "--prewarm-ms", "5", "--per-step-samples", "2"]
    c, d, out = run_bench(cmd, env, tmp_path, timeout=600)
    assert c["value"] > 0 and c["value_rays"] > 0 and c["incomplete"] is True and "watchdog" in c and "WATCHDOG" in out.stderr
    assert d["value"] > 0 and d["value_rays"] > 0 and "watchdog" in d


@pytest.mark.parametrize("world", [2, 3, 8])
def test_library_multi_rank_paths_over_a_mock_rccl_on_one_gpu(world, tmp_path):
    """The C++ library's multi-rank code between DIFFERENT ranks on one GPU: tests/c/mock_rccl.cpp stands in for librccl.so.1
    (in-process rendezvous, device-to-device copies, stream-ordered like NCCL), tests/c/multirank_mock.cpp runs `world` ranks as
    threads of one process -- a rank with an upper neighbour only, with both (world 3), with a lower one only: the fill step in
    both message forms, the halo exchange, one and two upper ghost slices, the all-gather of slabs, both gathers of config 5 to
    rank 0 and to the last rank, and sdfv_slab_march's rounds with the merge -- each compared bit for bit with the library's
    single-device result.  RCCL refuses two ranks on one device (test above) and no run here has had two devices: this is the
    only execution those branches get before real hardware."""
    mock_dir = tmp_path / "mock"
    mock_dir.mkdir()
    hip = ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall", *hip,
                        os.path.join(ROOT, "tests", "c", "mock_rccl.cpp"), "-o", str(mock_dir / "librccl.so.1"),
                        "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-soname,librccl.so.1", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = tmp_path / "multirank_mock"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", *hip, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c", "multirank_mock.cpp"), "-o", str(exe),
                        "-L", os.path.join(ROOT, "sdf-viewer_amd"), "-lsdfgrid", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread",
                        "-Wl,-rpath," + os.path.join(ROOT, "sdf-viewer_amd"), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, LD_LIBRARY_PATH=str(mock_dir) + ":" + os.environ.get("LD_LIBRARY_PATH", ""), GPU_MAX_HW_QUEUES="8")
    out = subprocess.run(["timeout", "-s", "KILL", "240", str(exe), str(world)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith(f"ok {world} ranks"), (out.returncode, out.stdout[-800:], out.stderr[-2500:])


@pytest.mark.parametrize("world", [2, 3])
def test_python_multi_rank_paths_over_a_mock_rccl_on_one_gpu(world, tmp_path):
    """... and the Python layer above it (tests/mock_ranks.py): parallel.SlabComm with a host-carried id, SlabFiller(transport=
    "rccl"), raymarch_sharded / SlabComm.march, gather_replica, gather_images, gather_bands over the library communicator, the
    ranks as THREADS of one process (the mock is loaded through SDFV_OPT_RCCL_LIBRARY; a process of its own because RCCL is
    loaded once per process).  Every rank's result against the single-device one, bit for bit."""
    mock = tmp_path / "libsdfv_mock_rccl.so"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", os.path.join(ROOT, "tests", "c", "mock_rccl.cpp"), "-o", str(mock),
                        "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    out = subprocess.run(["timeout", "-s", "KILL", "280", sys.executable, os.path.join(ROOT, "tests", "mock_ranks.py"), str(mock), str(world)],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=320)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith(f"ok {world} ranks as threads"), \
        (out.returncode, out.stdout[-2500:], out.stderr[-1500:])
