"""GPU tests of sdfv_program_raycast (include/sdfgrid.h): the kernel against the host mirror byte for byte -- the mirror itself is
held to the numpy restatement and to float64 geometry by tests/test_program_cast_cpu.py -- over the list lengths, wave shapes,
parameters and alignments at which the kernel takes another path; against the point-list routes of the same handle; through a
compiled handle; and WHERE and WHEN it touches memory (tests/arena.py, tests/stream_gate.py).  No list is longer than 4096 rays."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import arena as A
import program_cast_ref as CR
import program_march_ref as M
import stream_gate as SG
import test_program_cast_cpu as CPU
from stream_gate import capture, gate  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
F = np.float32
UNIT = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


@functools.lru_cache(maxsize=None)
def case(name):
    """(builder, handle, box, the CPU test's ray set for this program)."""
    PM = importlib.import_module("sdf-viewer_amd.program")  # noqa: N806
    b, box, seed = {n: (b, box, seed) for n, b, box, seed in CPU.compared_programs(PM)}[name]
    return b, b.build(), box, CR.rays(seed, box)


def device_cast(prog, rays, **kw):
    """[n, 8] float32 -> HIT_DTYPE records, through the device."""
    out = prog.cast(torch.from_numpy(np.ascontiguousarray(rays, F)).cuda(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(CR.HIT_DTYPE).reshape(-1)


@pytest.mark.parametrize("name", ["demo3", "spheres8", "example_sixteen", M.GRAZE])
def test_device_equals_the_host_mirror_on_every_byte(pkg, PM, name):
    b, prog, box, rays = case(name)
    want = prog.cast_host(rays, box=box)
    got = device_cast(prog, rays, box=box)
    CR.assert_hits_bitwise(got, want, name)
    st = want["status"]
    if name == "example_sixteen":
        assert (st != 1).all() and (st == -2).sum() >= 100                  # a list of misses
    elif name == M.GRAZE:
        assert (st == -1).sum() >= 50 and (want["steps"][st == -1] == 256).all()
    else:
        assert (st == 1).sum() >= 100 and (st == 0).sum() >= 100 and (st == -2).sum() >= 100


@functools.lru_cache(maxsize=None)
def long_list():
    """4096 rays against demo3 and the host mirror's records for them: shared by the tests that cut or permute it."""
    b, prog, box, _ = case("demo3")
    rays = CR.rays(4096, box, 4096)
    want = prog.cast_host(rays, box=box)
    rays.setflags(write=False), want.setflags(write=False)
    return rays, want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4096])
def test_list_lengths(pkg, PM, n):
    """Partial waves, a partial last workgroup, several workgroups; a ray's record does not depend on what follows it."""
    _, prog, box, _ = case("demo3")
    rays, want = long_list()
    got = device_cast(prog, rays[:n], box=box)
    assert len(got) == n
    CR.assert_hits_bitwise(got, want[:n], n)


def miss_rays(n):
    """n rays that pass the unit box by."""
    r = np.zeros((n, 8), F)
    r[:, 0], r[:, 1], r[:, 2] = 3.0, np.linspace(1.5, 2.5, n), 0.25
    r[:, 4], r[:, 7] = -1.0, 100.0
    return r


def graze_rays(n):
    """n rays inside the unit box, parallel to the grazed plane y = -0.95 a hair above it: they run out of steps."""
    r = np.zeros((n, 8), F)
    r[:, 0], r[:, 1], r[:, 2] = -0.9, -0.95 + np.linspace(5e-5, 4e-4, n), np.linspace(-0.5, 0.5, n)
    r[:, 4], r[:, 7] = 2.0, 100.0
    return r


def test_wave_shapes(pkg, PM):
    _, demo3, box, rays = case("demo3")
    # a wave of 64 rays that all miss the box (it leaves before it touches the program) beside a wave that hits
    hitting = rays[CR.cast(case("demo3")[0].ops, box, rays)["status"] == 1][:64]
    assert len(hitting) == 64
    both = np.concatenate([miss_rays(64), hitting])
    want = demo3.cast_host(both, box=box)
    assert (want["status"][:64] == 0).all() and (want["status"][64:] == 1).all()
    CR.assert_hits_bitwise(device_cast(demo3, both, box=box), want, "misses beside hits")
    # one long grazing ray among 63 misses
    _, graze, gbox, _ = case(M.GRAZE)
    one = miss_rays(64)
    one[37] = graze_rays(1)[0]
    want = graze.cast_host(one, box=gbox)
    assert want["status"][37] == -1 and want["steps"][37] == 256 and (np.delete(want["status"], 37) == 0).all()
    CR.assert_hits_bitwise(device_cast(graze, one, box=gbox), want, "one grazing ray")
    # one lane hitting at step 1, from inside the solid, among lanes that run to max_steps
    many = graze_rays(64)
    many[5, :3] = (0.1, -0.97, 0.2)
    want = graze.cast_host(many, box=gbox)
    assert want["status"][5] == 1 and want["steps"][5] == 1 and want["t"][5] == 0.0
    assert (np.delete(want["status"], 5) == -1).all() and (np.delete(want["steps"], 5) == 256).all()
    CR.assert_hits_bitwise(device_cast(graze, many, box=gbox), want, "one hit at step 1")


@pytest.mark.parametrize("kw", [dict(max_steps=1), dict(max_steps=4096), dict(hit_eps=3e-3, normal_eps=0.02), dict(box=(-0.85,) * 3 + (0.85,) * 3)],
                         ids=["max_steps1", "max_steps4096", "eps", "smaller_box"])
def test_parameters(pkg, PM, kw):
    name = M.GRAZE if "max_steps" in kw else "demo3"      # (the grazing rays are the ones that use 4096 steps)
    b, prog, box, rays = case(name)
    rays = rays[:600]
    args = dict(dict(box=box), **kw)
    want = prog.cast_host(rays, **args)
    CR.assert_hits_bitwise(device_cast(prog, rays, **args), want, kw)
    default = prog.cast_host(rays, box=box)
    assert (want.view(np.uint32) != default.view(np.uint32)).any()          # the parameter matters on this list
    if kw.get("max_steps") == 4096:
        assert want["steps"].max() > 256
    if "box" in kw:                                       # the smaller box cuts the surface: hits inside it, and rays that now leave early
        assert (want["status"] == 1).sum() >= 50 and ((default["status"] == 1) & (want["status"] != 1)).sum() >= 10
        assert (np.abs(want["pos"][want["status"] == 1]) <= 0.85 + 1e-6).all()


def test_cross_route_and_flags(pkg, PM):
    """For the hits, `sample` is sdfv_program_sample_points(pos) and `normal` is sdfv_program_normal_points(pos, normal_eps) of the
    same handle, bit for bit; with flags 0, 1 and 2 what was not asked for is 0 and everything else is unchanged."""
    for name, normal_eps in (("spheres8", 0.0), ("deep", 0.02)):        # (programs with materials)
        _, prog, box, rays = case(name)
        full = device_cast(prog, rays, box=box, normal_eps=normal_eps)
        h = full["status"] == 1
        assert h.sum() >= 100
        pos = torch.from_numpy(np.ascontiguousarray(full["pos"][h])).cuda()
        rec = prog.sample_points(pos).cpu().numpy()
        nrm = prog.normal_points(pos, eps=normal_eps).cpu().numpy()
        assert (full["sample"][h].view(np.uint32) == rec.view(np.uint32)).all()
        assert (full["normal"][h].view(np.uint32) == nrm.view(np.uint32)).all()
        assert (full["sample"][h][:, 1:] != 0).any() and (full["normal"][h] != 0).any()
        for flags in (0, 1, 2):
            got = device_cast(prog, rays, box=box, normal_eps=normal_eps, normals=bool(flags & 1), materials=bool(flags & 2))
            want = full.copy()
            if not flags & 1:
                want["normal"] = 0
            if not flags & 2:
                want["sample"][:, 1:] = 0
            CR.assert_hits_bitwise(got, want, (name, flags))
            assert (got["sample"][~h] == 0).all() and (got["normal"][~h] == 0).all()


def test_a_compiled_handle_is_interpreted(pkg, PM):
    b, prog, box, rays = case("demo3")
    compiled = prog.compile(routes=PM.MARCH | PM.POINTS | PM.MESH)
    before = compiled.compiled_info()["launches"]
    CR.assert_hits_bitwise(device_cast(compiled, rays, box=box), device_cast(prog, rays, box=box), "compiled handle")
    assert compiled.compiled_info()["launches"] == before and compiled.compiled_info()["routes"] == PM.MARCH | PM.POINTS | PM.MESH


N_ARENA = 300     # two workgroups, the second partial; the last wave partial


@functools.lru_cache(maxsize=None)
def arena_case():
    b, prog, box, rays = case("spheres8")
    rays = np.ascontiguousarray(rays[:N_ARENA])
    want = CR.cast(b.ops, box, rays)                      # the restatement: nothing here comes from the library
    assert {1, 0, -2} <= set(want["status"].tolist())
    return prog, box, rays, np.ascontiguousarray(want).view(F).reshape(N_ARENA, 16)


@pytest.mark.parametrize("hits_align", [16, 4])
@pytest.mark.parametrize("rays_align", [16, 4])
def test_containment_and_alignment(pkg, PM, rays_align, hits_align):
    """Guard words around rays and hits, rays unchanged, every byte of n records written and none beyond, whatever lies around the
    arrays; the arrays at 16-byte alignment and at 4-byte (not 8-byte) alignment in the four combinations: the same bytes."""
    prog, box, rays, want = arena_case()
    arrays = [rays, want]
    band = A.band_for(*arrays)
    ar = A.Arena(A.arena_bytes(band, *arrays), band=band)
    r = ar.input(rays, align=rays_align, name="rays")
    h = ar.output(want.shape, F, align=hits_align, name="hits")
    assert r.data_ptr() % rays_align == 0 and r.data_ptr() % (2 * rays_align) != 0 and h.data_ptr() % (2 * hits_align) != 0
    # (the records' zeros: a word of an output that is expected to be 0 can never be taken for the canary, which is never 0)
    ar.twin(lambda: prog.cast(r, box=box, out=h), {"hits": want}, kinds=("canary", "nan"))


def cast_case(pkg, name="cast"):
    prog, box, rays, want = arena_case()

    def host():
        return {"desc": pkg._capi.ProgramCastDesc(), "lo": (C.c_float * 3)(*box[:3]), "hi": (C.c_float * 3)(*box[3:])}

    def call(t, h):
        d = h["desc"]
        d.size, d.program = C.sizeof(d), prog.h
        d.bb_min, d.bb_max = h["lo"], h["hi"]
        d.rays, d.hits, d.n = t["rays"].data_ptr(), t["hits"].data_ptr(), N_ARENA
        d.flags = pkg._capi.CAST_NORMALS | pkg._capi.CAST_MATERIALS
        pkg.check(pkg.lib.sdfv_program_raycast(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    c = SG.Case(name, call, {"hits": want}, inputs={"rays": (rays, 16)}, outputs={"hits": (want.shape, F, 16)}, host=host)
    c.keep = prog
    return c


def test_the_cast_runs_on_the_callers_stream(pkg, PM, gate, capture):  # noqa: F811
    """Behind a sleep on the caller's stream, and captured into a graph and replayed; the descriptor and the host box are free
    once the call has returned (the harness scribbles over them)."""
    gate.run(pkg, cast_case(pkg))
    capture.run(pkg, cast_case(pkg))


def test_determinism_and_order_independence(pkg, PM):
    """Two calls write equal bytes; the same list shuffled gives the same records under the permutation: a ray's record depends
    on neither its lane nor its neighbours."""
    _, prog, box, _ = case("demo3")
    rays, want = long_list()
    first, second = device_cast(prog, rays, box=box), device_cast(prog, rays, box=box)
    CR.assert_hits_bitwise(first, second, "two calls")
    perm = np.random.default_rng(5).permutation(len(rays))
    CR.assert_hits_bitwise(device_cast(prog, rays[perm], box=box), first[perm], "shuffled")
    CR.assert_hits_bitwise(first, want, "host mirror")
