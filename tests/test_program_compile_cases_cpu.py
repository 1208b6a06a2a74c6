"""CPU tests of tests/program_compile_cases.py: what each program handed to tests/test_gpu_program_compile_corpus.py is for,
asserted on the numpy restatement (tests/program_ref.py) and the header's validity rule (tests/program_fuzz.first_error) alone,
so that the device comparison of compiled against interpreted handles cannot become one of constants, of NaNs, or of programs
that no longer hold the operand they were built around."""
import importlib

import numpy as np
import pytest

import program_compile_cases as CC
import program_fuzz as Z
import program_ref as R

F = np.float32
TINY = np.finfo(F).tiny


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


def operands(ops, *opcodes):
    return [a for op, a in ops if op in opcodes]


def test_the_quarter_of_each_tiny_k_is_what_the_program_was_built_for():
    assert 0 < F(CC.TINY_K) * F(0.25) < TINY <= F(CC.TINY_K)         # a normal k whose quarter is subnormal
    assert F(CC.LEAST_K) > 0 and F(CC.LEAST_K) * F(0.25) == 0        # the least subnormal: its quarter is zero
    assert 0 < F(1e-41) < TINY and F(1e-41) * F(0.25) > 0
    assert F(2.0 ** -100) * F(0.25) == F(2.0 ** -102) >= TINY         # a power of two: the quarter is exact and normal


@pytest.mark.parametrize("name", ["tiny_k", "pow2_k", "identities", "subnormal_sizes"])
def test_the_folding_programs_are_valid_numeric_and_not_constant(PM, name):
    """sdfv_program_create's rule accepts the program; on the moderate points of program_ref.points() the restatement gives no
    NaN, no undecided material and more than 3 800 distinct distances."""
    b = CC.folding_programs(PM)[name]
    assert b.bb == CC.UNIT and Z.first_error(b.ops, b.bb) is None
    pts = R.points()
    pts = pts[Z.moderate(pts)]
    rec, decided = R.run(b.ops, pts, want_decided=True)
    assert not np.isnan(rec).any() and decided.all()
    distinct = len(np.unique(rec[:, 0].view(np.uint32)))
    print(f"{name}: {len(b.ops)} instructions, {distinct} distinct distances on {len(pts)} moderate points")
    assert distinct > 3800
    b.build()                                                        # ... and the library's validator agrees


def test_each_folding_program_keeps_the_fold_it_was_built_for(PM):
    progs = {k: b.ops for k, b in CC.folding_programs(PM).items()}
    smooth = lambda ops: [F(a[0]) for a in operands(ops, R.SMOOTH_UNION, R.SMOOTH_SUBTRACT)]    # noqa: E731
    k = smooth(progs["tiny_k"])
    assert F(CC.TINY_K) in k and F(CC.LEAST_K) in k and F(1e-41) in k
    assert all(v * F(0.25) < TINY for v in k)                        # every quarter subnormal or zero
    k = smooth(progs["pow2_k"])
    assert len(k) == 4 and all(np.frexp(v)[0] == 0.5 for v in k)     # powers of two: x / k is a multiply, k / 4 exact
    assert min(k) == F(2.0 ** -100) and max(k) == F(8.0) and max(k) < F(2.0 ** 100)
    ident = progs["identities"]
    zeros = [F(a[0]) for a in operands(ident, R.ROUND, R.SHELL)]
    assert [bool(np.signbit(v)) for v in zeros] == [False, True, False] and all(v == 0 for v in zeros)   # x - 0, x - (-0), |x| - 0
    affines = operands(ident, R.PUSH_AFFINE)
    assert affines[0] == CC.IDENTITY and affines[1] == CC.NEGATING
    assert sum(np.signbit(F(v)) and v == 0 for v in CC.NEGATING) == 2                           # ... zeros of both signs
    assert [a[:2] for a in operands(ident, R.PUSH_SCALE)] == [(1.0, 1.0), (2.0, 0.5)]           # 1.0f * x; a power of two
    assert any(a == (1.0, 0.0, 0.0, -0.0) and np.signbit(F(a[3])) for a in operands(ident, R.PLANE))
    sub = progs["subnormal_sizes"]
    flat = np.array([v for op, a in sub for v in a], F)
    assert ((flat != 0) & (np.abs(flat) < TINY)).sum() >= 8 and (flat == 0).any() and (flat < 0).any()
    assert Z.has_edge_operands(sub) and Z.has_edge_operands(progs["tiny_k"])


def test_the_short_extreme_programs_hold_edge_operands_and_both_kinds_of_result():
    short = CC.short_extreme(Z.DEFAULT_SEED)
    assert all(len(ops) <= CC.SHORT for _, ops, _ in short)
    assert {len(ops) for _, ops, _ in short} == {n for n in Z.LENGTHS if n <= CC.SHORT}
    edged = sum(Z.has_edge_operands(ops) for _, ops, _ in short)
    odd, ordinary = R.odd_batch()
    nans = numbers = 0
    for _, ops, _ in short:
        d = R.run(ops, odd, distance_only=True)[:, 0]
        assert not np.isnan(d[ordinary]).any()
        nans += int(np.isnan(d).sum())
        numbers += int((~np.isnan(d[~ordinary])).sum())
    print(f"{len(short)} programs, {edged} with edge operands; {nans} NaN and {numbers} numeric results at odd points")
    assert len(short) >= 20 and edged >= 20 and nans > 0 and numbers > 0
    fill = CC.fill_extreme(Z.DEFAULT_SEED)
    assert len(fill) == CC.N_FILL == 7 and len(short) == CC.N_SHORT == 27 and all(len(ops) <= CC.FILL_SHORT for _, ops, _ in fill) and any(Z.has_edge_operands(ops) for _, ops, _ in fill)


def test_the_march_share_is_one_program_of_every_length():
    corpus = Z.corpus(Z.DEFAULT_SEED, Z.CORPUS_SIZE)
    share = CC.march_share(corpus)
    lengths = [len(corpus[i][0]) for i in share]
    print(f"{len(share)} programs of lengths {sorted(lengths)}")
    assert len(share) >= 13 and R.MAX_OPS in lengths and 233 in lengths
