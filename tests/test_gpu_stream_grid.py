"""The grid entry points on the caller's stream (tests/stream_gate.py): grid_init, grid_init_unvisited[_ex], fill_grid,
fill_grid_commit, fill_grid_pass_ex, commit_distance, commit_pairs, commit_interleaved, pack_samples and emit_update_points, over
the grids (20, 6, 5) and (40, 12, 7) of tests/test_gpu_containment_pass.py.  Expected texels are the oracle's (fill_dense, the
viewer_update load states, pack) and numpy's; every host argument -- params, grid, the changed box -- is the test's own and is
overwritten the moment the call returns.

Passes: steps 4, 2 and 1 of a load, without a box, and as an edit of the loaded grid with a changed box; without a volume, with
the plain and with the interleaved one; and piecewise, SDFV_OPT_PASS_INDEX_LIMIT at two (three) slices and one voxel, so that
the pass is three launches.  grid_init and the fills have no device input: the late output poison carries their ordering check
alone.  emit_update_points is a select, a memset and a kernel over a run of 600 points; `count` is read by the snapshot on the
stream.  Capture's second replay: another source volume for the commits, other indices and samples for pack_samples."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import arena as A
import stream_gate as SG
import test_gpu_containment_pass as CP
from program_fill_check import interleave
from stream_gate import capture, gate  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
F = np.float32
GRIDS = [(20, 6, 5), (40, 12, 7)]
IDS = ["x".join(map(str, d)) for d in GRIDS]


def host_of(pkg, dims, z=None, box=None, **params):
    def host():
        h = {"params": pkg.default_params(**params), "grid": pkg.make_grid(dims) if z is None else pkg.make_grid(dims, z_begin=z[0], z_end=z[1])}
        if box is not None:
            h["box"] = (C.c_float * 6)(*[float(x) for x in box])
        return h
    return host


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def pairs_of(dist):
    below = np.concatenate([dist[:, 1:], dist[:, -1:]], axis=1)  # d[min(y + 1, H - 1)]
    return np.ascontiguousarray(np.stack([dist, below], axis=-1))


@functools.lru_cache(maxsize=None)
def other_volume(dims):
    W, H, D = dims
    r0 = np.random.default_rng(W * H * D).uniform(-1.0, 1.0, (D, H, W, 4)).astype(F)
    r0.setflags(write=False)
    return r0


# ---- cases --------------------------------------------------------------------------------------------------------------------
def init_case(pkg, dims):
    W, H, D = dims
    air = np.full((D, H, W, 4), F(pkg.AIR_DIST), F)
    return SG.Case(f"grid_init{dims}", lambda t, h: pkg.check(pkg.lib.sdfv_grid_init(C.byref(h["grid"]), ptr(t["tex0"]), ptr(t["tex1"]), stream_ptr())),
                   {"tex0": air, "tex1": air}, outputs={"tex0": (air.shape, F, 16), "tex1": (air.shape, F, 16)}, host=host_of(pkg, dims))


def init_unvisited_case(pkg, dims, step, volume, ex=True):
    """ex False: sdfv_grid_init_unvisited, the exported form without flags (the plain volume or none)."""
    W, H, D = dims
    r0, r1 = CP.dense(dims)
    air = F(pkg.AIR_DIST)
    y, z = np.arange(H)[None, :], np.arange(D)[:, None]
    visited = (y % step == 0) & (z % step == 0)
    want0, want1 = (np.where(visited[:, :, None, None], r, air) for r in (r0, r1))
    inouts = {"tex0": (r0, 16), "tex1": (r1, 16)}
    expected = {"tex0": want0, "tex1": want1}
    if volume is not None:
        inouts["vol"] = (CP.layout(r0[..., 0], volume), 8 if volume == "ilv" else 4)
        expected["vol"] = CP.layout(want0[..., 0], volume)
    flags = pkg._capi.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0
    if not ex:
        assert flags == 0
        return SG.Case(f"grid_init_unvisited{dims}-{step}-{volume}",
                       lambda t, h: pkg.check(pkg.lib.sdfv_grid_init_unvisited(C.byref(h["grid"]), step, ptr(t["tex0"]), ptr(t["tex1"]), ptr(t.get("vol")),
                                                                               stream_ptr())),
                       expected, inouts=inouts, host=host_of(pkg, dims))
    return SG.Case(f"grid_init_unvisited_ex{dims}-{step}-{volume}",
                   lambda t, h: pkg.check(pkg.lib.sdfv_grid_init_unvisited_ex(C.byref(h["grid"]), step, ptr(t["tex0"]), ptr(t["tex1"]), ptr(t.get("vol")),
                                                                              flags, stream_ptr())),
                   expected, inouts=inouts, host=host_of(pkg, dims))


def fill_case(pkg, dims, commit):
    r0, r1 = CP.dense(dims)
    outputs = {"tex0": (r0.shape, F, 16), "tex1": (r1.shape, F, 16)}
    expected = {"tex0": r0, "tex1": r1}
    if commit:
        outputs["dist"] = (r0.shape[:-1], F, 4)
        expected["dist"] = np.ascontiguousarray(r0[..., 0])

    def call(t, h):
        if commit:
            pkg.check(pkg.lib.sdfv_fill_grid_commit(C.byref(h["params"]), pkg.SDF_DEMO, C.byref(h["grid"]), ptr(t["tex0"]), ptr(t["tex1"]), ptr(t["dist"]),
                                                    stream_ptr()))
        else:
            pkg.check(pkg.lib.sdfv_fill_grid(C.byref(h["params"]), pkg.SDF_DEMO, C.byref(h["grid"]), ptr(t["tex0"]), ptr(t["tex1"]), stream_ptr()))
    return SG.Case(f"fill_grid{'_commit' if commit else ''}{dims}", call, expected, outputs=outputs, host=host_of(pkg, dims))


def pass_case(pkg, dims, step, volume, box, pieces=False):
    """One pass of a load (box None) or of an edit of the loaded grid with a changed box, as tests/test_gpu_containment_pass.py
    runs them; pieces: SDFV_OPT_PASS_INDEX_LIMIT so that the pass is three launches."""
    K = pkg._capi
    W, H, D = dims
    done = CP.STEPS[:CP.STEPS.index(step)]
    s = CP.load_states(dims) if box is None else CP.load_states(dims, True, box)
    before, after = s[done], s[done + (step,)]
    inouts = {"tex0": (before[0], 16), "tex1": (before[1], 16)}
    expected = {"tex0": after[0], "tex1": after[1]}
    if volume is not None:
        inouts["vol"] = (CP.layout(before[0][..., 0], volume), 16)
        expected["vol"] = CP.layout(after[0][..., 0], volume)
    flags = K.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0
    params = dict(sphere_radius=0.8, cube_material=1) if box is not None else {}
    per_piece = {5: 2, 7: 3}[D]  # slices per piece: three pieces
    options = {K.OPT_PASS_INDEX_LIMIT: per_piece * W * H + 1} if pieces else {}

    def call(t, h):
        pkg.check(pkg.lib.sdfv_fill_grid_pass_ex(C.byref(h["params"]), pkg.SDF_DEMO, C.byref(h["grid"]), step, h.get("box"), ptr(t["tex0"]), ptr(t["tex1"]),
                                                 ptr(t.get("vol")), flags, stream_ptr()))
    return SG.Case(f"fill_grid_pass_ex{dims}-{step}-{volume}-{'box' if box else 'load'}{'-pieces' if pieces else ''}", call, expected, inouts=inouts,
                   host=host_of(pkg, dims, box=box, **params), options=options)


def pass_cases(pkg, dims, step):
    box = CP.boxes_for(dims)[1]
    for volume in (None, "plain", "ilv"):
        for b in (None, box):
            yield pass_case(pkg, dims, step, volume, b)
    if step in (2, 1):
        yield pass_case(pkg, dims, step, "plain", None, pieces=True)
    if step == 1:
        yield pass_case(pkg, dims, 1, "ilv", box, pieces=True)


def commit_case(pkg, dims, what):
    r0 = CP.dense(dims)[0]
    o0 = other_volume(dims)
    dist, odist = np.ascontiguousarray(r0[..., 0]), np.ascontiguousarray(o0[..., 0])
    fn = {"distance": pkg.lib.sdfv_commit_distance, "pairs": pkg.lib.sdfv_commit_pairs, "interleaved": pkg.lib.sdfv_commit_interleaved}[what]
    src, osrc = (r0, o0) if what == "distance" else (dist, odist)
    make = {"distance": lambda a: np.ascontiguousarray(a[..., 0]), "pairs": pairs_of, "interleaved": lambda d: interleave(d).reshape(d.shape)}[what]
    want, owant = make(src), make(osrc)
    return SG.Case(f"commit_{what}{dims}", lambda t, h: pkg.check(fn(C.byref(h["grid"]), ptr(t["src"]), ptr(t["out"]), stream_ptr())),
                   {"out": want}, inputs={"src": (src, 16 if what == "distance" else 4)},
                   outputs={"out": (want.shape, F, {"distance": 4, "pairs": 8, "interleaved": 8}[what])}, host=host_of(pkg, dims),
                   second=({"src": osrc}, {"out": owant}))


def pack_data(pkg, oracle, dims, z, seed, volume):
    """Scattered indices over the slab (its last voxel among them) and their samples -> (indices, samples, tex0, tex1, vol)."""
    W, H, D = dims
    n_vox = W * H * (z[1] - z[0])
    rng = np.random.default_rng(seed)
    where = np.concatenate([np.sort(rng.choice(n_vox - 1, size=257, replace=False)), [n_vox - 1]])
    rng.shuffle(where)
    samples = rng.uniform(0.0, 1.0, size=(len(where), 7)).astype(F)
    samples[:, 0] = rng.uniform(-0.3, 1.0, size=len(where)).astype(F)
    air = F(pkg.AIR_DIST)
    want0 = np.full((z[1] - z[0], H, W, 4), air, F)
    want1 = want0.copy()
    f0, f1 = want0.reshape(-1, 4), want1.reshape(-1, 4)
    for k, v in enumerate(where):
        p0, p1 = oracle.pack(samples[k])
        f0[v], f1[v, :3] = p0, p1[:3]
    return where.astype(np.uint32), samples, want0, want1, (None if volume is None else CP.layout(want0[..., 0], volume))


def pack_case(pkg, oracle, dims, volume):
    z = (1, dims[2] - 1)
    idx, samples, want0, want1, want_vol = pack_data(pkg, oracle, dims, z, 17, volume)
    idx2, samples2, other0, other1, other_vol = pack_data(pkg, oracle, dims, z, 18, volume)
    before = np.full_like(want0, F(pkg.AIR_DIST))
    inouts = {"tex0": (before, 16), "tex1": (before, 16)}
    expected, second = {"tex0": want0, "tex1": want1}, {"tex0": other0, "tex1": other1}
    if volume is not None:
        inouts["vol"] = (before[..., 0], 8 if volume == "ilv" else 4)
        expected["vol"], second["vol"] = want_vol, other_vol
    flags = pkg._capi.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0
    return SG.Case(f"pack_samples{dims}-{volume}",
                   lambda t, h: pkg.check(pkg.lib.sdfv_pack_samples(C.byref(h["grid"]), 0, ptr(t["indices"]), ptr(t["samples"]), len(idx), ptr(t["tex0"]),
                                                                    ptr(t["tex1"]), ptr(t.get("vol")), flags, stream_ptr())),
                   expected, inputs={"samples": (samples, 4), "indices": (idx, 4)}, inouts=inouts, host=host_of(pkg, dims, z=z),
                   second=({"samples": samples2, "indices": idx2}, second))


def emit_case(pkg, dims, volume):
    from test_gpu_viewer_abi import emit_reference
    bmin, bmax, step, cursor, n = (-1.0, -0.5, -0.75), (1.0, 0.5, 0.75), 1, 65, 600
    W, H, D = dims
    air = F(pkg.AIR_DIST)

    def data(seed):
        rng = np.random.default_rng(seed)
        vol = rng.uniform(0.0, 1.0, (D, H, W)).astype(F)
        vol[rng.uniform(size=vol.shape) < 0.4] = air
        want_p, want_i = emit_reference(dims, bmin, bmax, step, cursor, n, box, vol, air)
        k = len(want_i)
        assert 256 < k < n
        full_p, full_i = np.zeros((n, 3), F), np.zeros(n, np.uint32)
        full_p[:k], full_i[:k] = want_p, want_i
        beyond = np.arange(n) >= k
        return CP.layout(vol, volume).reshape(-1), {"points": A.Untouched(full_p, undefined=beyond[:, None]), "indices": A.Untouched(full_i, undefined=beyond),
                                                    "count": np.array([k], np.uint32),
                                                    "scratch": A.Untouched(np.zeros(scratch_bytes, np.uint8), undefined=True)}
    box = np.array([-0.2, -0.1, -0.8, 0.6, 0.3, 0.9], F)
    scratch_bytes = pkg.lib.sdfv_emit_update_points_scratch_bytes(n)
    assert scratch_bytes > 0, pkg.lib.sdfv_last_error()
    vol, expected = data(7)
    vol2, expected2 = data(8)
    flags = pkg._capi.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0

    def host():
        return {"grid": pkg.make_grid(dims, bmin, bmax), "box": (C.c_float * 6)(*box)}

    def call(t, h):
        rc = pkg.lib.sdfv_emit_update_points(C.byref(h["grid"]), step, cursor, n, h["box"], t["dist"].data_ptr(), flags, t["points"].data_ptr(),
                                             t["indices"].data_ptr(), t["count"].data_ptr(), t["scratch"].data_ptr(), scratch_bytes,
                                             torch.cuda.current_stream().cuda_stream)
        assert rc == 0, pkg.lib.sdfv_last_error()
    return SG.Case(f"emit_update_points{dims}-{volume}", call, expected, inputs={"dist": (vol, 8 if volume == "ilv" else 4)},
                   outputs={"points": ((n, 3), F, 4), "indices": ((n,), np.uint32, 4), "count": ((1,), np.uint32, 4),
                            "scratch": ((scratch_bytes,), np.uint8, 16)}, host=host, second=({"dist": vol2}, expected2))


def cases_of(pkg, oracle, dims, group):
    if group == "init_fill":
        yield init_case(pkg, dims)
        for volume in (None, "plain", "ilv"):
            yield init_unvisited_case(pkg, dims, 2, volume)
        yield init_unvisited_case(pkg, dims, 2, "plain", ex=False)
        yield fill_case(pkg, dims, False)
        yield fill_case(pkg, dims, True)
    elif group == "commit":
        for what in ("distance", "pairs", "interleaved"):
            yield commit_case(pkg, dims, what)
    elif group == "pack_samples":
        for volume in (None, "plain", "ilv"):
            yield pack_case(pkg, oracle, dims, volume)
    elif group == "emit_update_points":
        if dims[0] * dims[1] * dims[2] >= 65 + 600:   # the run of 600 points from point 65 lies within the step-1 pass
            for volume in ("plain", "ilv"):
                yield emit_case(pkg, dims, volume)
    elif group in (4, 2, 1):
        yield from pass_cases(pkg, dims, group)
    else:
        raise KeyError(group)


GROUPS = ["init_fill", "commit", "pack_samples", "emit_update_points", 4, 2, 1]
RUNS = [(d, g) for d in GRIDS for g in GROUPS if not (g == "emit_update_points" and d == GRIDS[0])]
RUN_IDS = ["x".join(map(str, d)) + "-" + (f"pass{g}" if isinstance(g, int) else g) for d, g in RUNS]


# ---- tests --------------------------------------------------------------------------------------------------------------------
def run_all(cases, runner, pkg):
    failures, n = [], 0
    for case in cases:
        n += 1
        try:
            runner(pkg, case)
        except SG.GateError as e:
            failures.append(f"{type(e).__name__}: {e}")
        except Exception as e:  # noqa: BLE001 (a capture that torch refuses is a RuntimeError: name the case, go on with the others)
            failures.append(f"{case.name}: {type(e).__name__}: {e}")
    assert n > 0
    assert not failures, "\n\n".join(failures)


@pytest.mark.parametrize("dims,group", RUNS, ids=RUN_IDS)
def test_grid_calls_run_on_the_callers_stream(pkg, oracle, gate, dims, group):
    run_all(cases_of(pkg, oracle, dims, group), gate.run, pkg)


@pytest.mark.parametrize("dims,group", RUNS, ids=RUN_IDS)
def test_grid_calls_only_enqueue(pkg, oracle, capture, dims, group):
    run_all(cases_of(pkg, oracle, dims, group), capture.run, pkg)
