"""Seeded random SDF programs (tests/program_fuzz.py) through the compiled fill and samplers, against the interpreted handle of
the same program: every word equal (a NaN distance: NaN on both sides).  Two of the programs are then given new operands on the
same structure and compiled again: a compile that reused a module made for other constants would show here."""
import importlib

import numpy as np
import pytest
import torch

import program_fuzz as Z
import program_ref as R
from test_gpu_program_compile import assert_equal, assert_equal_nan_rule, launches

pytestmark = pytest.mark.gpu
SEED = 20261020
N_PROGRAMS = 8
DIMS = (17, 6, 5)


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


def corpus():
    return Z.corpus(SEED, Z.CORPUS_SIZE)[5:5 + 3 * N_PROGRAMS:3]    # eight programs of eight different lengths


def compare(pkg, PM, ops, bb, what):
    plain = Z.builder(PM, ops, bb).build()
    comp = plain.compile(PM.FILL | PM.POINTS)
    g = pkg.make_grid(DIMS, bb[:3], bb[3:])
    got = []
    for p in (plain, comp):
        t0, t1 = pkg.alloc_textures(g)
        dist = torch.empty(DIMS[::-1], device="cuda")
        p.fill_grid(g, t0, t1, dist=dist)
        got.append((t0, t1, dist))
    for k, name in enumerate(("tex0", "tex1", "dist")):
        assert_equal(got[0][k], got[1][k], f"{what} {name}")
    pts = torch.from_numpy(np.ascontiguousarray(R.points()[:257])).cuda()
    for distance_only in (False, True):
        assert_equal_nan_rule(plain.sample_points(pts, distance_only), comp.sample_points(pts, distance_only), f"{what} points")
    assert launches(comp) == 1 + 2 * 2 and launches(plain) == 0    # one fill; a staged and a tail launch per sampler call
    return got[1][0]


@pytest.mark.parametrize("index", range(N_PROGRAMS))
def test_compiled_equals_interpreted(pkg, PM, index):
    ops, bb = corpus()[index]
    what = Z.label(SEED, index, ops, bb)
    first = compare(pkg, PM, ops, bb, what)
    if index in (2, 5):
        # the same structure, every non-zero operand of a primitive moved a little: new constants, a new module
        rng = np.random.default_rng([SEED, index])
        mutated = [(op, tuple(float(np.float32(v) * np.float32(rng.uniform(0.9, 1.1))) if op in Z.PRIMITIVES else v for v in a))
                   for op, a in ops]
        assert mutated != list(ops) and [op for op, _ in mutated] == [op for op, _ in ops]
        second = compare(pkg, PM, mutated, bb, what + " (mutated operands)")
        assert not torch.equal(first, second), "the mutated program fills the grid differently"
