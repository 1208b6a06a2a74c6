"""CPU tests of sdfviewer::LoadState (host/load_state.hpp): what SDFViewer::update may tell a pass about the grid.

A flag too few costs only time (a load 1.5x slower with every bit right), so no test of the textures can see it.  Here the
module is driven with the events the three routes of update() report, and the decisions are compared with what the rules say:
the SDFV_PASS_* flags of every pass, whether the grid must be materialised first, the dense shortcut, box_covers_grid."""
import itertools

import numpy as np
import pytest

FRESH, SAME, VIRGIN, ILV, NOOP = 1, 2, 4, 8, 16  # SDFV_PASS_* (include/sdfgrid.h)
STEPS = (4, 2, 1)  # three passes
DEMO, DEMO_EDITED = 1, 2  # two parameter blocks of a device SDF
PROGRAM = 0x1000  # a snapshot of a whole-pass program


def whole_passes(ls, *, device_sdf=DEMO, program=0, box=False, report=False, steps=STEPS, between=None):
    """update() calls with a budget below 1 ms over one LoadingManager: a pass per call.  -> [(materialised first, flags)]"""
    out = []
    for i, step in enumerate(steps):
        ls.observe(device_sdf, program, change_reported=report and i == 0)
        ls.event("device_route_entered")
        first, flags = ls.next_pass(has_box=box, program=bool(program))
        if first:
            ls.event("materialized")
        out.append((first, flags))
        ls.event("pass_ran", step)
        if step == 1:
            ls.event("manager_finished")
        if between:
            between(i)
    return out


@pytest.mark.parametrize("ilv", [0, ILV], ids=["plain", "interleaved"])
def test_a_virgin_load_stays_virgin_until_its_last_pass(host, ilv):
    ls = host.LoadState(interleaved=bool(ilv))
    assert whole_passes(ls) == [(False, VIRGIN | SAME | ilv)] * 3
    assert ls.material() == {"pairs_valid": False, "undefined_rows": False, "defined_step": 1}
    assert not is_fresh(ls)


def test_a_virgin_load_records_the_rows_its_passes_defined(host):
    ls = host.LoadState()
    assert ls.material()["undefined_rows"] and ls.material()["defined_step"] == 0 and is_fresh(ls)
    whole_passes(ls, steps=(4,))
    assert ls.material()["undefined_rows"] and ls.material()["defined_step"] == 4 and not is_fresh(ls)
    whole_passes(ls, steps=(2,))
    assert ls.material()["undefined_rows"] and ls.material()["defined_step"] == 2


def test_b_a_frame_between_passes_materialises_the_grid(host):
    ls = host.LoadState()
    got = whole_passes(ls, between=lambda i: ls.event("materialized") if i == 0 else None)
    assert got == [(False, VIRGIN | SAME), (False, SAME), (False, SAME)]


def test_c_a_download_before_the_first_pass_leaves_a_fresh_grid(host):
    ls = host.LoadState()
    ls.event("materialized")
    assert whole_passes(ls) == [(False, FRESH | SAME), (False, SAME), (False, SAME)]


def test_d_a_program_pass_never_takes_a_virgin_grid(host):
    ls = host.LoadState()
    assert whole_passes(ls, device_sdf=None, program=PROGRAM) == [(True, FRESH | SAME), (False, SAME), (False, SAME)]


@pytest.mark.parametrize("ilv", [0, ILV], ids=["plain", "interleaved"])
def test_e_f_a_changed_box_and_the_manager_after_it(host, ilv):
    ls = host.LoadState(interleaved=bool(ilv))
    whole_passes(ls)
    # (e) a reported box, a renewed manager: the passes read the grid; materialising is a no-op
    assert whole_passes(ls, box=True, report=True) == [(False, ilv)] * 3
    # (f) the box is worked off, the manager renewed without one: nothing to do, and the load never becomes "the same" again
    assert whole_passes(ls) == [(False, ilv | NOOP)] * 3
    assert ls.observe(DEMO) is False


def test_g_a_box_before_the_first_pass(host):
    ls = host.LoadState()
    assert whole_passes(ls, box=True, report=True, steps=(4,)) == [(True, 0)]


def test_h_another_parameter_block_mid_load(host):
    ls = host.LoadState()
    assert whole_passes(ls, steps=(4,)) == [(False, VIRGIN | SAME)]
    assert ls.observe(DEMO_EDITED) is False
    assert whole_passes(ls, device_sdf=DEMO_EDITED, steps=(2,)) == [(True, 0)]  # no NOOP: nothing has run to the end


def test_another_parameter_block_over_a_fresh_grid_is_still_the_same_load(host):
    ls = host.LoadState()
    assert ls.observe(DEMO) and ls.observe(DEMO_EDITED)  # nothing an earlier pass could have written
    assert whole_passes(ls, device_sdf=DEMO_EDITED, steps=(4,)) == [(False, VIRGIN | SAME)]


def test_another_program_snapshot_ends_the_load(host):
    ls = host.LoadState()
    whole_passes(ls, device_sdf=None, program=PROGRAM, steps=(4,))
    assert ls.observe(None, PROGRAM) is True
    assert ls.observe(None, PROGRAM + 64) is False
    assert whole_passes(ls, device_sdf=None, program=PROGRAM + 64, steps=(2, 1)) == [(False, 0), (False, 0)]


@pytest.mark.parametrize("route", ["device_sampled", "host_sampled"])
def test_i_a_record_route_leaves_the_single_load_regime(host, route):
    ls = host.LoadState()
    whole_passes(ls)
    ls.event("pairs_built")  # commit() of the loaded grid
    assert ls.material()["pairs_valid"] and not ls.commit_derives_pairs(loaded=True)
    # the record route over a renewed manager
    ls.observe(None, 0)
    if route == "device_sampled":
        ls.event("device_route_entered")
    else:
        assert ls.mirror() == "read_back"  # the whole passes wrote the grid
        ls.event("mirror_rebuilt")
    ls.event("records_packed")
    # what the routes' four lines left: no single load, nothing fresh, no pair volume; the mirror as the route had it
    assert ls.observe(None, 0) is False and not is_fresh(ls)
    assert not ls.material()["pairs_valid"] and ls.commit_derives_pairs(loaded=True)
    assert ls.mirror() == ("valid" if route == "host_sampled" else "read_back")
    ls.event("manager_finished")
    # the demo again, a renewed manager, no box
    assert whole_passes(ls) == [(False, NOOP)] * 3
    assert ls.mirror() == "read_back"  # (cleared at the entry of the whole-pass route)


def test_a_record_route_over_a_fresh_grid(host):
    ls = host.LoadState()
    assert ls.mirror() == "all_air"
    ls.event("materialized")
    ls.event("mirror_rebuilt")
    ls.event("records_packed")
    assert ls.mirror() == "valid"
    ls.event("mirror_lost")
    assert ls.mirror() == "read_back"
    # the demo takes over mid-load: it reads the grid
    assert whole_passes(ls, steps=(4,)) == [(False, 0)]


def test_without_a_volume_there_is_no_layout_and_no_pair_volume(host):
    ls = host.LoadState(volume=False, interleaved=True)
    assert whole_passes(ls) == [(False, VIRGIN | SAME)] * 3
    assert not ls.commit_derives_pairs(loaded=True)
    assert host.LoadState().commit_derives_pairs(loaded=True) and not host.LoadState().commit_derives_pairs(loaded=False)
    assert not host.LoadState(interleaved=True).commit_derives_pairs(loaded=True)


# ---- the dense shortcut ----
DIMS, BB = (24, 20, 16), (-1.0, -2.0, -0.5, 1.0, 2.0, 1.5)  # (sizes 2, 4, 2: the last voxel's coordinate is the bound itself)


def is_fresh(ls):
    """Fresh: the dense shortcut applies without a box."""
    return ls.dense_shortcut(0, 1, 1.0, DIMS, BB)


def inside(face):
    """BB with one face one ulp inside."""
    box = np.array(BB, np.float32)
    box[face] = np.nextafter(box[face], np.float32(np.inf if face < 3 else -np.inf))
    return box


@pytest.mark.parametrize("iterations,step,budget", itertools.product([0, 5], [0, 1, 4], [0.0005, 0.001, 0.03]))
def test_dense_shortcut_truth_table(host, iterations, step, budget):
    fits = iterations == 0 and step != 0 and budget >= 0.001
    fresh, loaded = host.LoadState(), host.LoadState()
    whole_passes(loaded)
    assert fresh.dense_shortcut(iterations, step, budget, DIMS, BB) == fits  # fresh, no box
    assert loaded.dense_shortcut(iterations, step, budget, DIMS, BB) is False  # written, no box
    for ls in (fresh, loaded):
        assert ls.dense_shortcut(iterations, step, budget, DIMS, BB, box=BB) == fits  # a box that covers the grid
        assert ls.dense_shortcut(iterations, step, budget, DIMS, BB, box=inside(4)) is False  # ... and one that does not


def test_box_covers_grid(host):
    assert host.box_covers_grid(DIMS, BB, BB)
    assert host.box_covers_grid(DIMS, BB, (-9, -9, -9, 9, 9, 9))
    for face in range(6):
        assert not host.box_covers_grid(DIMS, BB, inside(face))
        nan = np.array(BB, np.float32)
        nan[face] = np.nan
        assert not host.box_covers_grid(DIMS, BB, nan)
    assert not host.box_covers_grid((1, 5, 7), BB, (-9, -9, -9, 9, 9, 9))  # 0/0 on the axis with one voxel
    assert host.box_covers_grid((2, 2, 2), BB, BB)


def test_voxel_coordinate_rounds_three_separate_steps(host):
    lo, hi = np.float32(-0.7), np.float32(0.9)
    for dim in (2, 17, 24, 255):
        for i in (0, 1, dim // 3, dim - 1):
            want = np.float32(np.float32(np.float32(i) / np.float32(dim - 1)) * np.float32(hi - lo)) + lo
            assert host.voxel_coordinate(float(i), dim, lo, hi) == want
    assert np.isnan(host.voxel_coordinate(0.0, 1, lo, hi))


def test_next_run_length(host):
    assert host.next_run_length(0.5, 2.0 ** -20, 16 * 65536, 1 << 23) == 1 << 18  # half of what is left over the cost per voxel
    assert host.next_run_length(0.5, 2.0 ** -30, 16 * 4096, 1 << 23) == 16 * 4096  # capped by growth
    assert host.next_run_length(10.0, 1e-9, 8.0 * (1 << 22), 1 << 16) == 1 << 16  # ... and by capacity
    assert host.next_run_length(0.010, 0.0, 8 * 16, 1 << 16) == 8 * 16  # no cost known: capacity, capped by growth
    assert host.next_run_length(-0.001, 1e-6, 8 * 16, 1 << 16) == 1  # the budget is spent: at least one voxel
