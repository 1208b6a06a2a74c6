"""GPU tests that hold sdfv_program_compile to include/sdfgrid.h's two promises on every route: "what a compiled route writes
equals what the interpreter writes, word for word" and "launches through a finished handle are as thread-safe as a plain one's".

Every comparison is the compiled handle against the INTERPRETED handle of the same program through the same call: every 32-bit
word equal (sample records: or both distances NaN), rgba within the march's 1e-4.  The programs are the ones the interpreter is
held on from three sides elsewhere and the compiler had not met: the march catalogue and the march's share of the fuzz corpus
through the march's own evaluator (Compiled<true> of csrc/program_compile.hip, the one text only a compiled march reaches), the
extreme corpus and four programs of foldable operands (tests/program_compile_cases.py) through the samplers and the fill, where
operands are immediates the optimiser may fold, the 256-instruction programs through every route, one handle with all three
routes next to another, and host threads.  One case is one compile of one route (compiling dominates: 0.5 s for a short program,
about 10 s for 256 instructions) and a few launches.  What makes the programs worth running is asserted on the restatement by
tests/test_program_compile_cases_cpu.py."""
import functools
import importlib
import threading

import numpy as np
import pytest
import torch

import program_compile_cases as CC
import program_fuzz as Z
import program_march_ref as M
import program_ref as R
from test_gpu_program_compile import assert_equal, assert_equal_nan_rule, expected_point_launches, launches
from test_gpu_program_fuzz import explained
from test_gpu_program_march import RGBA_TOL
from test_program_compile_cpu import deepest_of_corpus

# The longest case compiles one route of a 256-instruction program (up to 12 s on a slow host) or six routes of short ones.
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
CANARY = -7.0
FILL_DIMS = (70, 6, 4)                     # one full and one ragged wave per row, H even (the interleaved volume pairs rows)
CATALOGUE_SIZE = M.SIZES[1]                # 67 x 41: neither a multiple of 8
CATALOGUE = ("anchor", "no_material", "all_ops", "deep", "sixteen", "single", "envelope", "late_material", "ties", "ties_zero", M.GRAZE)
FOLDING = ("tiny_k", "pow2_k", "identities", "subnormal_sizes")
WORST = {"rgba": 0.0, "frames": 0}         # over the march cases of this run, printed by the last of them


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


@functools.lru_cache(maxsize=None)
def fuzz_corpus():
    return Z.corpus(Z.seed(), Z.size())


@functools.lru_cache(maxsize=None)
def fuzz_share():
    return tuple(CC.march_share(fuzz_corpus()))


@functools.lru_cache(maxsize=None)
def extreme_short():
    return tuple(CC.short_extreme(Z.seed()))


@functools.lru_cache(maxsize=None)
def extreme_fill():
    return tuple(CC.fill_extreme(Z.seed()))


def on_device(points):
    return torch.from_numpy(np.ascontiguousarray(points, np.float32)).cuda()


# ---- the march ----
def march_equal(plain, comp, cams, size, rp, what, **kw):
    """One render of all `cams` through both handles, aux and depth asked for: the 18 aux words and the depth equal as words,
    rgba within RGBA_TOL.  -> the interpreted aux as a structured array [n_cam, h, w]."""
    w, h = size
    a = plain.render(cams, w, h, rp=rp, want_aux=True, want_depth=True, **kw)
    b = comp.render(cams, w, h, rp=rp, want_aux=True, want_depth=True, **kw)
    assert_equal(a[1], b[1], what + " aux")
    assert_equal(a[2], b[2], what + " depth")
    delta = float((a[0] - b[0]).abs().max())
    print(f"{what}: max |d rgba| between the interpreted and the compiled march = {delta:.3e}")
    WORST["rgba"], WORST["frames"] = max(WORST["rgba"], delta), WORST["frames"] + len(cams)
    assert delta <= RGBA_TOL, (what, delta)
    return M.aux_view(a[1].cpu().numpy())


def rgba8_equal(plain, comp, cams, size, rp, what, **kw):
    w, h = size
    assert_equal(plain.render(cams, w, h, rp=rp, rgba8=True, **kw), comp.render(cams, w, h, rp=rp, rgba8=True, **kw), what + " rgba8")


INTERPRETED = {}                           # (kind, key) -> the interpreted aux of a march case's plain frames


def interpreted_catalogue_frames(pkg, PM, name):
    """The interpreted aux of `name`'s two 67 x 41 frames: what the catalogue cases compare against, kept for the conditions over
    the whole parametrisation (rendered here if the case did not run)."""
    if ("catalogue", name) not in INTERPRETED:
        w, h = CATALOGUE_SIZE
        aux = M.builders(PM)[name].build().render(list(M.cameras(pkg, name, w, h)), w, h, rp=M.render_params(pkg, name), want_aux=True)[1]
        INTERPRETED["catalogue", name] = M.aux_view(aux.cpu().numpy())
    return INTERPRETED["catalogue", name]


@pytest.mark.parametrize("name", CATALOGUE)
def test_the_compiled_march_equals_the_interpreted_one_on_the_catalogue(pkg, PM, name):
    """Every scene of tests/program_march_ref.py -- `envelope` (256 instructions, 85 materials), `ties`, `late_material` and
    `graze` (status -1) among them -- from its orbit camera and its camera inside the box."""
    K = pkg._capi
    assert set(CATALOGUE) == set(M.builders(PM))
    plain = M.builders(PM)[name].build()
    comp = plain.compile(PM.MARCH)
    rp, cams = M.render_params(pkg, name), list(M.cameras(pkg, name, *CATALOGUE_SIZE))
    INTERPRETED["catalogue", name] = march_equal(plain, comp, cams, CATALOGUE_SIZE, rp, name)
    count = 1
    if name in ("envelope", "deep"):
        march_equal(plain, comp, cams, CATALOGUE_SIZE, rp, name + " normal_h=0.01", normal_h=0.01)
        rgba8_equal(plain, comp, cams, CATALOGUE_SIZE, rp, name)
        rgba8_equal(plain, comp, cams, CATALOGUE_SIZE, rp, name + " normal_h=0.01", normal_h=0.01)
        count += 3
    if name in ("sixteen", "envelope"):
        before = pkg.get_option(K.OPT_EXT_SRGB_QUANT)
        try:
            pkg.set_option(K.OPT_EXT_SRGB_QUANT, 1)
            march_equal(plain, comp, cams, CATALOGUE_SIZE, rp, name + " srgb_quant=1")
            count += 1
        finally:
            pkg.set_option(K.OPT_EXT_SRGB_QUANT, before)
    assert launches(comp) == count and launches(plain) == 0


def materials_in_tiles(aux):
    """The largest number of distinct materials among the hits of one 8 x 8 tile (a wave of the march) of a frame."""
    h, w = aux.shape
    texels = np.concatenate([aux["raw0"][..., 1:], aux["raw1"][..., :3]], axis=-1).view(np.uint32)
    best = 0
    for y in range(0, h, 8):
        for x in range(0, w, 8):
            hit = aux["status"][y:y + 8, x:x + 8] == 1
            if hit.any():
                best = max(best, len(np.unique(texels[y:y + 8, x:x + 8][hit], axis=0)))
    return best


def test_the_catalogue_frames_hold_what_the_march_can_get_wrong(pkg, PM):
    """On the interpreted output of the cases above: more than 5 000 hits, a pixel that ran out of steps (status -1, what `graze`
    is built for), an 8 x 8 tile whose hits carry three materials."""
    frames = [f for name in CATALOGUE for f in interpreted_catalogue_frames(pkg, PM, name)]
    hits = sum(int((f["status"] == 1).sum()) for f in frames)
    grazed = sum(int((f["status"] == -1).sum()) for f in frames)
    tile = max(materials_in_tiles(f) for f in frames)
    print(f"{len(frames)} frames: {hits} hits, {grazed} pixels with status -1, up to {tile} materials in one 8 x 8 tile")
    assert len(frames) == 2 * len(CATALOGUE) and hits > 5000 and grazed >= 1 and tile >= 3


def interpreted_share_frames(pkg, PM, index):
    if ("share", index) not in INTERPRETED:
        ops, bb = fuzz_corpus()[index]
        w, h = Z.MARCH_SIZE
        aux = Z.builder(PM, ops, bb).build().render(list(Z.march_cameras(pkg, bb)), w, h, rp=Z.render_params(pkg, bb), want_aux=True)[1]
        INTERPRETED["share", index] = M.aux_view(aux.cpu().numpy())
    return INTERPRETED["share", index]


@pytest.mark.parametrize("k", range(13))
def test_the_compiled_march_equals_the_interpreted_one_on_the_fuzz_share(pkg, PM, k):
    """One program of every length of the corpus, 233 and 256 instructions included -- the lengths the march's evaluator states
    its operands anew per step for ("Operands in a loop")."""
    share = fuzz_share()
    assert len(share) >= 13
    for index in share[k:k + 1] + (share[13:] if k == 12 else ()):          # (a re-seeded corpus may share out more than 13)
        ops, bb = fuzz_corpus()[index]
        with explained(index, ops, bb):
            plain = Z.builder(PM, ops, bb).build()
            comp = plain.compile(PM.MARCH)
            INTERPRETED["share", index] = march_equal(plain, comp, list(Z.march_cameras(pkg, bb)), Z.MARCH_SIZE, Z.render_params(pkg, bb),
                                                      f"corpus[{index}] ({len(ops)} instructions)")
            assert launches(comp) == 1 and launches(plain) == 0


def test_the_fuzz_share_frames_hold_hits_and_rays_that_leave(pkg, PM):
    """The condition of test_the_direct_march_equals_its_restatement_on_the_corpus, on the interpreted output of the cases above,
    and the largest |d rgba| any march case of this run measured."""
    frames = [f for index in fuzz_share() for f in interpreted_share_frames(pkg, PM, index)]
    mixed = sum(bool((f["status"] == 1).any() and (f["status"] == -2).any()) for f in frames)
    print(f"{len(frames)} frames, {mixed} with hits and with rays that leave the box; over {WORST['frames']} compiled frames of this run "
          f"max |d rgba| = {WORST['rgba']:.3e}")
    assert len(frames) >= 26 and 4 * mixed >= 3 * len(frames)


# ---- the samplers on edge operands ----
def sampler_programs():
    return [f"extreme{k}" for k in range(CC.N_SHORT)] + list(FOLDING)


def edge_program(PM, case, share):
    """(builder, ops, a context that explains a failure) of a case of the samplers' or the fill's list: a folding program by
    name, or "extreme<k>", the k-th program of `share`."""
    if case in FOLDING:
        b = CC.folding_programs(PM)[case]
        return b, b.ops, explained(case, b.ops, b.bb, "folding_programs")
    i, ops, bb = share[int(case[len("extreme"):])]
    return Z.builder(PM, ops, bb), ops, explained(i, ops, bb, "extreme_corpus")


@pytest.mark.parametrize("case", sampler_programs())
def test_the_compiled_samplers_equal_the_interpreted_ones_on_edge_operands(pkg, PM, case):
    """program_ref.odd_batch() (inf, NaN, +-3e38 and subnormal coordinates among ordinary points; the staged kernel and its
    scalar tail) and 191 of its points in a buffer that is not 16-byte aligned (the scalar kernel alone), records and distances
    only.  The four folding programs are new to the interpreter too: both handles are also held to the restatement."""
    assert len(extreme_short()) == CC.N_SHORT
    builder, ops, context = edge_program(PM, case, extreme_short())
    odd, ordinary = R.odd_batch()
    dev = on_device(odd)
    flat = torch.empty(3 * 191 + 1, device="cuda")
    flat[1:] = dev[64:64 + 191].reshape(-1)
    unaligned = flat[1:].view(191, 3)
    assert dev.data_ptr() % 16 == 0 and unaligned.data_ptr() % 16 != 0 and len(odd) > 256 and len(odd) % 256
    assert not ordinary[64:64 + 191].all() and ordinary[64:64 + 191].any()
    with context:
        plain = builder.build()
        comp = plain.compile(PM.POINTS)
        count = 0
        for distance_only in (False, True):
            a, b = plain.sample_points(dev, distance_only), comp.sample_points(dev, distance_only)
            assert_equal_nan_rule(a, b, f"{case} odd batch d_only={distance_only}")
            assert_equal_nan_rule(plain.sample_points(unaligned, distance_only), comp.sample_points(unaligned, distance_only),
                                  f"{case} unaligned d_only={distance_only}")
            count += expected_point_launches(len(odd), True) + expected_point_launches(191, False)
            if case in FOLDING:
                want, decided = R.run(ops, odd, distance_only, want_decided=True)
                for got, who in ((b, "compiled"), (a, "interpreted")):
                    R.assert_records_under_the_nan_rule(got.cpu().numpy(), want, decided, ordinary, f"{case} {who} d_only={distance_only}")
        assert launches(comp) == count == 6 and launches(plain) == 0


# ---- the fill on edge operands ----
NAN_VOXELS = {}                            # case -> NaN voxels left out of the comparison


def fill_programs():
    return list(FOLDING) + [f"extreme{k}" for k in range(CC.N_FILL)]


@pytest.mark.parametrize("case", fill_programs())
def test_the_compiled_fill_equals_the_interpreted_one_on_edge_operands(pkg, PM, case):
    """(70, 6, 4) over the program's box, without a volume and with the interleaved one, OPT_FILL_NONTEMPORAL 0 and 1: tex0, tex1
    and the volume equal as words.  A voxel whose interpreted distance is NaN must be NaN in the compiled fill and is left out,
    at most 2 % of a program's voxels (grid positions are ordinary points: none is expected)."""
    K = pkg._capi
    assert len(extreme_fill()) == CC.N_FILL
    builder, ops, context = edge_program(PM, case, extreme_fill())
    with context:
        plain = builder.build()
        comp = plain.compile(PM.FILL)
        g = pkg.make_grid(FILL_DIMS, builder.bb[:3], builder.bb[3:])
        shape = FILL_DIMS[::-1]
        count = left_out = 0
        for volume in (None, "ilv"):
            for nt in (0, 1):
                got = []
                for p in (plain, comp):
                    t0, t1 = (torch.full(shape + (4,), CANARY, device="cuda") for _ in range(2))
                    dist = None if volume is None else torch.full(shape, CANARY, device="cuda")
                    with pkg.options({K.OPT_FILL_NONTEMPORAL: nt}):
                        p.fill_grid(g, t0, t1, dist=dist, flags=K.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0)
                    got.append((t0, t1, dist))
                count += 1
                what = f"{case} volume={volume} nt={nt}"
                nan = torch.isnan(got[0][0][..., 0])
                n_nan = int(nan.sum())
                left_out = max(left_out, n_nan)
                assert 50 * n_nan <= nan.numel(), (what, n_nan, "NaN voxels: more than 2 %")
                assert bool(torch.isnan(got[1][0][..., 0])[nan].all()), what + ": a NaN voxel of the interpreter is one of the compiled fill"
                keep = ~nan
                assert_equal(got[0][0][keep], got[1][0][keep], what + " tex0")
                assert_equal(got[0][1][keep], got[1][1][keep], what + " tex1")
                if volume is not None:
                    a, b = got[0][2].reshape(-1), got[1][2].reshape(-1)
                    assert int(torch.isnan(a).sum()) == n_nan and bool(torch.isnan(b)[torch.isnan(a)].all()), what + " dist NaN"
                    assert_equal(a[~torch.isnan(a)], b[~torch.isnan(a)], what + " dist")
                    assert not bool((b == CANARY).any())
                assert not bool((got[1][0] == CANARY).any()) and not bool((got[1][1] == CANARY).any())
                assert launches(comp) == count and launches(plain) == 0, what
        NAN_VOXELS[case] = left_out
        print(f"{case}: {left_out} NaN voxels left out of {nan.numel()}")


# ---- the longest programs ----
@pytest.mark.parametrize("route", ["fill", "points"])
def test_the_deepest_256_instruction_program(pkg, PM, route):
    """The program of the corpus with the deepest stacks (256 instructions), one route per case: the fill with the plain volume,
    the samplers on 257 points.  (Its kind through the march: the fuzz share above, and `envelope`.)"""
    ops, bb = deepest_of_corpus()
    assert len(ops) == R.MAX_OPS
    with explained("deepest", ops, bb):
        plain = Z.builder(PM, ops, bb).build()
        if route == "fill":
            comp = plain.compile(PM.FILL)
            g = pkg.make_grid(FILL_DIMS, bb[:3], bb[3:])
            got = []
            for p in (plain, comp):
                t0, t1 = (torch.full(FILL_DIMS[::-1] + (4,), CANARY, device="cuda") for _ in range(2))
                dist = torch.full(FILL_DIMS[::-1], CANARY, device="cuda")
                p.fill_grid(g, t0, t1, dist=dist)
                got.append((t0, t1, dist))
            for k, what in enumerate(("tex0", "tex1", "dist")):
                assert_equal(got[0][k], got[1][k], what)
                assert not bool((got[1][k] == CANARY).any())
            assert len(torch.unique(got[1][2])) > 100                       # a model, not a constant
            assert launches(comp) == 1 and launches(plain) == 0
        else:
            comp = plain.compile(PM.POINTS)
            pts = on_device(R.points()[:257])
            for distance_only in (False, True):
                assert_equal_nan_rule(plain.sample_points(pts, distance_only), comp.sample_points(pts, distance_only), f"d_only={distance_only}")
            assert launches(comp) == 2 * expected_point_launches(257, True) == 4 and launches(plain) == 0


# ---- one handle with every route, next to another ----
def route_calls(pkg, PM, name):
    """{route: call(handle) -> tuple of output tensors} for a catalogue program, and the specialised launches each makes."""
    builder = M.builders(PM)[name]
    g = pkg.make_grid(FILL_DIMS, builder.bb[:3], builder.bb[3:])
    pts = on_device(R.points()[:257])
    w, h = Z.MARCH_SIZE
    rp, cams = M.render_params(pkg, name), list(M.cameras(pkg, name, w, h))

    def fill(p):
        t0, t1 = (torch.full(FILL_DIMS[::-1] + (4,), CANARY, device="cuda") for _ in range(2))
        dist = torch.full(FILL_DIMS[::-1], CANARY, device="cuda")
        p.fill_grid(g, t0, t1, dist=dist)
        return t0, t1, dist

    def points(p):
        return (p.sample_points(pts),)

    def march(p):
        return p.render(cams, w, h, rp=rp, want_aux=True, want_depth=True)

    return {"fill": (fill, 1), "points": (points, expected_point_launches(257, True)), "march": (march, 1)}


def routes_equal(route, got, want, what):
    if route == "points":
        assert_equal_nan_rule(want[0], got[0], what)
    elif route == "march":
        assert float((got[0] - want[0]).abs().max()) <= RGBA_TOL, what + " rgba"
        assert bool((M.aux_view(want[1].cpu().numpy())["status"] == 1).any()), what + ": some pixels hit"
        assert_equal(want[1], got[1], what + " aux")
        assert_equal(want[2], got[2], what + " depth")
    else:
        for k, name in enumerate(("tex0", "tex1", "dist")):
            assert_equal(want[k], got[k], f"{what} {name}")


def test_two_handles_with_every_route_launch_in_turn(pkg, PM):
    """Every module exports the same ten kernel names: `all_ops` (A) and `late_material` (B), each compiled for all three
    routes, both alive, launched alternately -- each call writes what ITS program's interpreter writes and counts on its own
    handle."""
    plain = {n: M.builders(PM)[n].build() for n in ("all_ops", "late_material")}
    comp = {n: p.compile(PM.FILL | PM.POINTS | PM.MARCH) for n, p in plain.items()}
    calls = {n: route_calls(pkg, PM, n) for n in plain}
    want = {(n, r): calls[n][r][0](plain[n]) for n in plain for r in ("fill", "points", "march")}
    a, b = "all_ops", "late_material"
    assert not torch.equal(want[a, "fill"][0], want[b, "fill"][0])
    expected = {a: 0, b: 0}
    for n, r in ((a, "fill"), (b, "fill"), (a, "points"), (b, "march"), (a, "march"), (b, "points"), (a, "fill")):
        call, n_launches = calls[n][r]
        routes_equal(r, call(comp[n]), want[n, r], f"{n} {r}")
        expected[n] += n_launches
        assert {k: launches(comp[k]) for k in comp} == expected, (n, r)
    assert expected == {a: 5, b: 4} and all(launches(p) == 0 for p in plain.values())


# ---- host threads ----
THREAD_PROGRAMS = ("anchor", "all_ops", "late_material", "ties")
THREAD_DIMS = (70, 6, 5)
JOIN_SECONDS = 120.0                       # four compiles of short programs and a few launches: seconds; a thread still out is a failure


def run_threads(targets):
    """Starts one thread per target and joins each with a timeout; -> the names of those that had not come back."""
    threads = [threading.Thread(target=t, daemon=True) for t in targets]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_SECONDS)
    return [i for i, t in enumerate(threads) if t.is_alive()]


def fill_on(p, grid, stream=None):
    t0, t1 = (torch.full(THREAD_DIMS[::-1] + (4,), CANARY, device="cuda") for _ in range(2))
    p.fill_grid(grid, t0, t1, stream=stream)
    return t0, t1


def test_host_threads_compile_and_launch_on_their_own_streams(pkg, PM):
    """Four threads each compile a program of their own and fill with it three times; then four threads share one handle compiled
    for the fill and the march and each fills and renders three times into buffers of its own, every thread on its own stream.
    Everything written equals what the interpreted handles wrote serially, the shared handle counts 4 x (3 + 3) launches, and no
    thread is left with an error text."""
    builders = {n: R.catalogue(PM)[n] for n in THREAD_PROGRAMS}
    grids = {n: pkg.make_grid(THREAD_DIMS, b.bb[:3], b.bb[3:]) for n, b in builders.items()}
    want_fill = {n: fill_on(b.build(), grids[n]) for n, b in builders.items()}
    shared_name = "all_ops"
    w, h = Z.MARCH_SIZE
    rp = M.render_params(pkg, shared_name)
    orbit = M.SCENES[shared_name][2]
    cams = [pkg.camera_look_at(eye=(orbit[0] + 0.3 * k, orbit[1], orbit[2] + 0.2 * k), aspect=w / h) for k in range(4)]
    shared_plain = builders[shared_name].build()
    want_march = [shared_plain.render(cams[k], w, h, rp=rp, want_aux=True) for k in range(4)]
    torch.cuda.synchronize()
    assert all(bool((M.aux_view(a.cpu().numpy())["status"] == 1).any()) for _, a in want_march)
    assert not torch.equal(want_march[0][1], want_march[1][1])
    results, errors = {}, []

    def own(k):
        def work():
            try:
                name = THREAD_PROGRAMS[k]
                stream = torch.cuda.Stream()
                comp = builders[name].build().compile(PM.FILL)
                with torch.cuda.stream(stream):
                    fills = [fill_on(comp, grids[name], stream) for _ in range(3)]
                stream.synchronize()
                results["own", k] = (fills, launches(comp), pkg.lib.sdfv_last_error().decode())
            except Exception as e:  # noqa: BLE001
                errors.append(("own", k, repr(e)))
        return work

    assert run_threads([own(k) for k in range(4)]) == [], "threads that did not come back"
    assert not errors, errors
    for k, name in enumerate(THREAD_PROGRAMS):
        fills, n_launches, error_text = results["own", k]
        for t0, t1 in fills:
            assert_equal(want_fill[name][0], t0, f"thread {k} {name} tex0")
            assert_equal(want_fill[name][1], t1, f"thread {k} {name} tex1")
        assert n_launches == 3 and error_text == "", (k, n_launches, error_text)

    shared = shared_plain.compile(PM.FILL | PM.MARCH)

    def sharing(k):
        def work():
            try:
                stream = torch.cuda.Stream()
                with torch.cuda.stream(stream):
                    fills = [fill_on(shared, grids[shared_name], stream) for _ in range(3)]
                    frames = [shared.render(cams[k], w, h, rp=rp, want_aux=True, stream=stream) for _ in range(3)]
                stream.synchronize()
                results["shared", k] = (fills, frames, pkg.lib.sdfv_last_error().decode())
            except Exception as e:  # noqa: BLE001
                errors.append(("shared", k, repr(e)))
        return work

    assert run_threads([sharing(k) for k in range(4)]) == [], "threads that did not come back"
    assert not errors, errors
    for k in range(4):
        fills, frames, error_text = results["shared", k]
        for t0, t1 in fills:
            assert_equal(want_fill[shared_name][0], t0, f"shared, thread {k} tex0")
            assert_equal(want_fill[shared_name][1], t1, f"shared, thread {k} tex1")
        for rgba, aux in frames:
            assert_equal(want_march[k][1], aux, f"shared, thread {k} aux")
            assert float((want_march[k][0] - rgba).abs().max()) <= RGBA_TOL, k
        assert error_text == "", (k, error_text)
    assert launches(shared) == 4 * (3 + 3) and launches(shared_plain) == 0
