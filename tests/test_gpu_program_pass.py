"""GPU tests of sdfv_program_grid_pass (one LoadingManager pass with an SDF program as the SDF) on a 70 x 34 x 19 grid: every
texel and every entry of the distance volume after a pass, bit for bit, against
where(mask, sdfv_program_fill_grid_commit(new program), before) with the mask restated in numpy (tests/program_pass_ref.py)."""
import importlib

import numpy as np
import pytest
import torch

import program_pass_ref as P
import program_ref as R
from program_fill_check import interleave

pytestmark = pytest.mark.gpu
VOLUMES = ("plain", "ilv", None)


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    assert bad.size == 0, (what, bad.size, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


def edited(builder):
    """Program B: `all_ops` with one operand edited -- the cutting plane y + 0.55 moved to y + 0.45."""
    ops = list(builder.ops)
    assert ops[13][0] == R.PLANE and ops[13][1][3] == 0.55
    ops[13] = (R.PLANE, ops[13][1][:3] + (0.45,))
    return ops


def build(PM, ops, bb):
    b = PM.Program(bb)
    b.ops = list(ops)
    return b.build()


class Scene:
    """Programs A and B, the grid, and the dense fills of both (numpy), per Srgba::from policy."""

    def __init__(self, pkg, PM):
        self.pkg, self.K = pkg, pkg._capi
        builder = R.catalogue(PM)["all_ops"]
        self.A, self.B = builder.build(), build(PM, edited(builder), builder.bb)
        self.grid = pkg.make_grid(P.DIMS, P.BB_MIN, P.BB_MAX)
        self.air = np.float32(pkg.AIR_DIST)
        self.dense = {}
        for srgb in (0, 1):
            for name, prog in (("A", self.A), ("B", self.B)):
                t0, t1 = pkg.alloc_textures(self.grid)
                with pkg.options({self.K.OPT_EXT_SRGB_QUANT: srgb}):
                    prog.fill_grid(self.grid, t0, t1)
                torch.cuda.synchronize()
                self.dense[name, srgb] = (t0.cpu().numpy(), t1.cpu().numpy())
        a, b = self.dense["A", 0], self.dense["B", 0]
        self.differs = (a[0].view(np.uint32) != b[0].view(np.uint32)).any(-1) | (a[1].view(np.uint32) != b[1].view(np.uint32)).any(-1)
        # A has a surface on this grid, and no stored voxel passes for air
        assert (a[0][..., 0] < self.air).any() and (a[0][..., 0] > self.air).any()
        assert not (a[0][..., 0] == self.air).any() and not (b[0][..., 0] == self.air).any()

    def flags(self, volume, extra=0):
        return extra | (self.K.PASS_VOLUME_INTERLEAVED if volume == "ilv" else 0)

    def upload(self, state, volume):
        """(tex0, tex1, volume tensor or None) on the device from numpy textures; the volume is tex0.r in its layout."""
        t0, t1 = torch.from_numpy(state[0].copy()).cuda(), torch.from_numpy(state[1].copy()).cuda()
        vol = None
        if volume:
            plain = state[0][..., 0].copy()
            vol = torch.from_numpy(interleave(plain) if volume == "ilv" else plain.reshape(-1)).cuda()
        return t0, t1, vol

    def check(self, dev, want, volume, what):
        torch.cuda.synchronize()
        same_bits(dev[0].cpu().numpy(), want[0], what + " tex0")
        same_bits(dev[1].cpu().numpy(), want[1], what + " tex1")
        if volume:
            same_bits(dev[2].cpu().numpy(), interleave(want[2]) if volume == "ilv" else want[2].reshape(-1), what + " volume")

    def air_state(self):
        W, H, D = P.DIMS
        t = np.full((D, H, W, 4), self.air, np.float32)
        return t, t.copy()


@pytest.fixture(scope="module")
def scene(pkg, PM):
    return Scene(pkg, PM)


@pytest.mark.parametrize("volume", VOLUMES)
def test_a_pass_over_a_loaded_grid_updates_the_box_and_nothing_else(scene, volume):
    W, H, D = P.DIMS
    before = (scene.dense["A", 0][0].copy(), scene.dense["A", 0][1].copy())
    if volume is None:   # sentinels where update() never writes: they must survive
        before[1][..., 3] = np.arange(D * H * W, dtype=np.float32).reshape(D, H, W) + 2.0
    for step in P.STEPS:
        lat = P.lattice(P.DIMS, step)
        for name, (box, kind) in P.boxes(step).items():
            mask = P.update_mask(P.DIMS, P.BB_MIN, P.BB_MAX, step, before[0][..., 0], box, scene.air)
            # the case is what its name says, and a wrong mask would show: B differs from A inside it and outside it
            if kind == "some":
                assert mask.any() and (lat & ~mask).any() and (mask & scene.differs).any() and (lat & ~mask & scene.differs).any(), (step, name)
            else:
                assert (mask == lat).all() if kind == "all" else not mask.any(), (step, name)
            want = P.expected(before, scene.dense["B", 0], mask, scene.air, volume)
            dev = scene.upload(before, volume)
            scene.B.grid_pass(scene.grid, step, dev[0], dev[1], dist=dev[2], changed_box=box, flags=scene.flags(volume))
            scene.check(dev, want, volume, f"step {step} box {name} volume {volume}")
    # the three face boxes are three different index ranges at step 1: the ulp matters
    m = [P.inside(P.DIMS, P.BB_MIN, P.BB_MAX, P.boxes(1)[n][0]).sum() for n in ("faces_in", "faces", "faces_out")]
    assert m[0] < m[1] and m[1] <= m[2]


@pytest.mark.parametrize("volume", VOLUMES)
def test_an_edit_in_the_middle_of_a_load(scene, volume):
    """init, A at step 4 (fresh), then B at step 2 with a box and B at step 1 without: lattice voxels that still hold AIR get B
    wherever they are, stored ones keep A outside the box and get B inside it."""
    K = scene.K
    box = P.boxes(2)["generic"][0]
    state = scene.air_state()
    dev = scene.upload(state, volume)
    scene.pkg.grid_init(scene.grid, dev[0], dev[1])
    plan = ((scene.A, "A", 4, None, K.PASS_FRESH_GRID), (scene.B, "B", 2, box, 0), (scene.B, "B", 1, None, 0))
    for prog, name, step, bx, fl in plan:
        mask = P.update_mask(P.DIMS, P.BB_MIN, P.BB_MAX, step, state[0][..., 0], bx, scene.air)
        if step == 2:
            stored = state[0][..., 0] != scene.air
            inbox = P.inside(P.DIMS, P.BB_MIN, P.BB_MAX, bx)
            lat = P.lattice(P.DIMS, 2)
            assert (lat & stored & inbox & scene.differs).any()        # stored, inside the box: rewritten with B
            assert (lat & stored & ~inbox & scene.differs).any()       # stored, outside: keeps A
            assert (lat & ~stored & ~inbox).any()                      # AIR outside the box: gets B
            assert (mask & stored).any() and (mask & ~stored & ~inbox).any() and (lat & ~mask).any()
        state = P.expected(state, scene.dense[name, 0], mask, scene.air, volume)[:2]
        prog.grid_pass(scene.grid, step, dev[0], dev[1], dist=dev[2], changed_box=bx, flags=scene.flags(volume, fl))
        scene.check(dev, state + (state[0][..., 0],), volume, f"{name} step {step} volume {volume}")
    # a mix of both programs at the end: stored A outside the box on the step-4 lattice, B elsewhere
    assert (state[0].view(np.uint32) != scene.dense["B", 0][0].view(np.uint32)).any()


@pytest.mark.parametrize("volume", VOLUMES)
def test_flags_are_knowledge_and_the_hint_is_a_hint(scene, volume):
    """A legitimate load with FRESH_GRID / SAME_LOAD equals the unflagged one after every pass and the dense fill at the end."""
    K = scene.K
    runs = {}
    for label, flags in (("unflagged", (0, 0, 0)), ("flagged", (K.PASS_FRESH_GRID, K.PASS_SAME_LOAD, K.PASS_SAME_LOAD)),
                         ("hinted", (K.PASS_EXPECT_NOOP,) * 3)):
        dev = scene.upload(scene.air_state(), volume)
        scene.pkg.grid_init(scene.grid, dev[0], dev[1])
        runs[label] = []
        for step, fl in zip((4, 2, 1), flags):
            scene.B.grid_pass(scene.grid, step, dev[0], dev[1], dist=dev[2], flags=scene.flags(volume, fl))
            torch.cuda.synchronize()
            runs[label].append(tuple(None if t is None else t.cpu().numpy() for t in dev))
    state = scene.air_state()
    for k, step in enumerate((4, 2, 1)):
        mask = P.update_mask(P.DIMS, P.BB_MIN, P.BB_MAX, step, state[0][..., 0], None, scene.air)
        state = P.expected(state, scene.dense["B", 0], mask, scene.air, volume)[:2]
        for label in runs:
            got = runs[label][k]
            same_bits(got[0], state[0], f"{label} step {step} tex0")
            same_bits(got[1], state[1], f"{label} step {step} tex1")
            if volume:
                plain = state[0][..., 0]
                same_bits(got[2], interleave(plain) if volume == "ilv" else plain.reshape(-1), f"{label} step {step} volume")
    same_bits(state[0], scene.dense["B", 0][0], "the load ends in the dense fill: tex0")
    same_bits(state[1], scene.dense["B", 0][1], "the load ends in the dense fill: tex1")


@pytest.mark.parametrize("volume", VOLUMES)
def test_a_slab_is_those_slices_of_the_whole_grid_with_the_lattice_in_global_z(scene, volume):
    W, H, D = P.DIMS
    z0, z1 = 5, 14
    slab = scene.pkg.make_grid(P.DIMS, P.BB_MIN, P.BB_MAX, z_begin=z0, z_end=z1)
    before = scene.dense["A", 0]
    for step in P.STEPS:
        box = P.boxes(step)["generic"][0]
        mask = P.update_mask(P.DIMS, P.BB_MIN, P.BB_MAX, step, before[0][..., 0], box, scene.air)
        assert mask[z0:z1].any() and not mask[z0:z1].all() and (step == 1 or not mask[z0].any())   # z = 5 is off the coarse lattices
        want = P.expected(before, scene.dense["B", 0], mask, scene.air, volume)
        dev = scene.upload(before, volume)
        vol = None if dev[2] is None else dev[2].view(D, H * W)[z0:z1]
        scene.B.grid_pass(slab, step, dev[0][z0:z1], dev[1][z0:z1], dist=vol, changed_box=box, flags=scene.flags(volume))
        # the slices outside the slab keep what they held
        m = mask.copy()
        m[:z0], m[z1:] = False, False
        scene.check(dev, P.expected(before, scene.dense["B", 0], m, scene.air, volume), volume, f"slab step {step} volume {volume}")
        same_bits(dev[0].cpu().numpy()[z0:z1], want[0][z0:z1], "the slab's slices of the whole-grid result")


def test_the_srgb_rounding_option_is_honoured_and_restored(scene):
    K, pkg = scene.K, scene.pkg
    assert pkg.get_option(K.OPT_EXT_SRGB_QUANT) == 0
    assert (scene.dense["B", 0][0].view(np.uint32) != scene.dense["B", 1][0].view(np.uint32)).any()   # the policy shows on this scene
    before = scene.dense["A", 1]
    box = P.boxes(1)["generic"][0]
    mask = P.update_mask(P.DIMS, P.BB_MIN, P.BB_MAX, 1, before[0][..., 0], box, scene.air)
    assert (mask[..., None] & (scene.dense["B", 0][0].view(np.uint32) != scene.dense["B", 1][0].view(np.uint32))).any()
    dev = scene.upload(before, "plain")
    try:
        pkg.set_option(K.OPT_EXT_SRGB_QUANT, 1)
        scene.B.grid_pass(scene.grid, 1, dev[0], dev[1], dist=dev[2], changed_box=box)
    finally:
        pkg.set_option(K.OPT_EXT_SRGB_QUANT, 0)
    scene.check(dev, P.expected(before, scene.dense["B", 1], mask, scene.air, "plain"), "plain", "rounded sRGB")
    assert pkg.get_option(K.OPT_EXT_SRGB_QUANT) == 0


# ---- the viewer takes whole passes for an editor ----
def editable(PM):
    b = PM.Program(P.BB_MIN + P.BB_MAX)
    b.material(0.8, 0.2, 0.1, 0.1, 0.6, 0.9).push_affine(PM.translation(0.25, 0.0, 0.0))
    affine = len(b.ops) - 1
    b.box(0.5, 0.3, 0.2).pop()
    box = len(b.ops) - 2
    b.material(0.1, 0.9, 0.3, 0.0, 1.0, 0.5).torus(0.6, 0.15).smooth_union(0.15)
    b.param("tx", [(affine, 3, PM.PARAM_NEGATED)], -0.5, 0.5, 0.01, 0.25, box=(-1.0, -0.45, -0.35, 1.0, 0.45, 0.35))
    b.param("hz", [(box, 2, PM.PARAM_VALUE)], 0.05, 0.9, 0.05, 0.2, box=(-0.8, -0.45, -0.95, 0.8, 0.45, 0.95))
    return b


@pytest.mark.parametrize("layout", ("plain", "interleaved"))
def test_the_pass_route_of_the_viewer_equals_the_device_sampled_route_after_every_call(pkg, PM, layout):
    V = importlib.import_module("sdf-viewer_amd.viewer")
    lay = V.LAYOUT_INTERLEAVED if layout == "interleaved" else V.LAYOUT_PLAIN
    budget = 60.0                                                 # every pass of a manager fits one call
    routes = {}
    for name in ("passes", "sampled"):
        ed = editable(PM).build_editor()
        routes[name] = (ed, V.Viewer.new_voxels(P.DIMS, P.BB_MIN + P.BB_MAX, 3, layout=lay), ed.as_surface())

    def call(name):
        ed, viewer, surface = routes[name]
        n = ed.update_viewer(viewer, budget_s=budget) if name == "passes" else viewer.update(surface, budget_s=budget)
        return (n,) + viewer.download() + (viewer.state(),)

    def both(what):
        a, b = call("passes"), call("sampled")
        assert a[0] == b[0] and a[3] == b[3], (what, a[0], b[0], a[3], b[3])
        same_bits(a[1], b[1], what + " tex0")
        same_bits(a[2], b[2], what + " tex1")
        return a

    def until_idle(what):
        last = None
        for k in range(6):
            last = both(f"{what}, call {k}")
            if last[0] == 0:
                return last
        raise AssertionError((what, "never idle", last[3]))

    loaded = until_idle("load")
    grid = pkg.make_grid(P.DIMS, P.BB_MIN, P.BB_MAX)
    d0, d1 = pkg.alloc_textures(grid)
    routes["passes"][0].program.fill_grid(grid, d0, d1)
    torch.cuda.synchronize()
    same_bits(loaded[1], d0.cpu().numpy(), "a load ends in the dense fill: tex0")
    same_bits(loaded[2], d1.cpu().numpy(), "a load ends in the dense fill: tex1")
    state = loaded
    for name, value in (("tx", -0.2), ("hz", 0.6)):
        for ed, _, _ in routes.values():
            ed.set(name, value)
        first = both(f"set {name}: the call that finds the box")
        assert first[0] > 0 and (first[1].view(np.uint32) != state[1].view(np.uint32)).any()
        state = until_idle(f"set {name}")
        assert state[3]["remaining"] == 0 and not state[3]["has_changed_box"]
        # the edit reached its box and nothing else: outside it the grid holds what it held
        routes["passes"][0].program.fill_grid(grid, d0, d1)
        torch.cuda.synchronize()
        box = next(p["box"] for p in routes["passes"][0].parameters() if p["name"] == name)
        inside = P.inside(P.DIMS, P.BB_MIN, P.BB_MAX, box)
        assert inside.any() and not inside.all()
        same_bits(state[1], np.where(inside[..., None], d0.cpu().numpy(), loaded[1]), f"set {name}: tex0 is the new program inside the box")
        loaded = state
    for ed, viewer, _ in routes.values():
        viewer.close()
        ed.close()
