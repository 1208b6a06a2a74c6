"""CPU tests over seeded random SDF programs (tests/program_fuzz.py): the corpus reaches what it claims, on the generator and the
numpy restatement alone; the host mirror -- the interpreter source the kernels compile -- equals the restatement bit for bit on
every program, through the surface callbacks and the direct march; sdfv_program_create accepts exactly what the header's rule,
restated, accepts.  No device needed.  Every failure message carries the seed, the program's index and the program as builder
calls."""
import importlib
import re

import numpy as np
import pytest

import program_fuzz as Z
import program_march_ref as M
import program_ref as R
from test_program_cpu import INVALID, create_rc, surface_records


@pytest.fixture(scope="module")
def PM(pkg):
    return importlib.import_module("sdf-viewer_amd.program")


@pytest.fixture(scope="module")
def V(pkg):
    return importlib.import_module("sdf-viewer_amd.viewer")


@pytest.fixture(scope="module")
def corpus():
    return Z.corpus(Z.seed(), Z.size())


@pytest.fixture(scope="module")
def extreme():
    return Z.extreme_corpus(Z.seed(), Z.size())


def corpus_conditions(programs):
    """The conditions of "the corpus is what it claims" -> (list of what is missed, text of the tables and counts)."""
    only_ops = [ops for ops, _ in programs]
    values_t, frames_t = Z.depth_table(only_ops)
    need_v, need_f = Z.required_cells()
    missed = [("value cell", Z.NAMES[op], d) for op, d in need_v if (op, d) not in values_t]
    missed += [("frame cell", Z.NAMES[op], d) for op, d in need_f if (op, d) not in frames_t]
    crossing = sum(bool(Z.crossing_combinators(ops)) for ops in only_ops)
    framed_materials = sum(bool(Z.materials_inside_frames(ops)) for ops in only_ops)
    lengths = {len(ops) for ops in only_ops}
    if crossing == 0:
        missed.append("no combinator consumes a value pushed before the innermost open frame")
    if framed_materials == 0:
        missed.append("no MATERIAL between a push and its pop")
    tied = {}
    for ops in only_ops:
        for op, count in Z.ties(ops).items():
            tied[op] = tied.get(op, 0) + count
    missed += [("no exact tie under", Z.NAMES[op]) for op in Z.COMBINATORS if op not in tied]
    if not {1, R.MAX_OPS} <= lengths:
        missed.append(("lengths", sorted(lengths)))
    missed += [("invalid", i, Z.first_error(ops, bb)) for i, (ops, bb) in enumerate(programs) if Z.first_error(ops, bb) is not None]
    pts = R.points()
    pts = pts[Z.moderate(pts)]
    assert len(pts) >= 4096
    for i, (ops, bb) in enumerate(programs):
        rec, decided = R.run(ops, pts, want_decided=True)
        if np.isnan(rec[:, 0]).any() or not decided.all():
            missed.append(("a NaN distance or an undecided material", i))
    signed = sum(Z.changes_sign(ops, bb) for ops, bb in programs)
    if 4 * signed < 3 * len(programs):
        missed.append(("both signs on the 13^3 lattice", signed, len(programs)))
    text = (f"{Z.format_tables(values_t, frames_t)}\n{len(programs)} programs, lengths {sorted(lengths)}; {crossing} hold a combinator "
            f"that reaches across a frame, {framed_materials} a MATERIAL inside a frame; exact ties per combinator {[tied.get(op, 0) for op in Z.COMBINATORS]}; {signed} change sign on their 13^3 lattice; "
            f"{len(pts)} points without a NaN or an undecided material")
    return missed, text


def test_the_corpus_is_what_it_claims():
    """A property of the generator and the restatement alone, for the default seed and three others.  CORPUS_CYCLES is the
    smallest number of whole cycles of the length list at which all four seeds meet it: one cycle fewer misses a cell for each."""
    assert Z.CORPUS_SIZE == Z.CORPUS_CYCLES * len(Z.LENGTHS) and Z.LENGTHS[0] == 1 and Z.LENGTHS[-1] == R.MAX_OPS
    fewer = 0
    for s in (Z.DEFAULT_SEED,) + Z.OTHER_SEEDS:
        missed, text = corpus_conditions(Z.corpus(s, Z.CORPUS_SIZE))
        print(f"seed {s}:\n{text}")
        assert not missed, (s, missed)
        fewer += bool(corpus_conditions(Z.corpus(s, Z.CORPUS_SIZE - len(Z.LENGTHS)))[0])
    assert fewer >= 1, "a smaller corpus meets the conditions for every seed: CORPUS_CYCLES is not the smallest"
    # the extreme corpus has the same shapes, and its operands are at the edges
    ordinary, edges = Z.corpus(Z.DEFAULT_SEED, Z.CORPUS_SIZE), Z.extreme_corpus(Z.DEFAULT_SEED, Z.CORPUS_SIZE)
    assert [[op for op, _ in a] for a, _ in ordinary] == [[op for op, _ in a] for a, _ in edges]
    assert all(Z.first_error(ops, bb) is None for ops, bb in edges)
    with_edges = sum(Z.has_edge_operands(ops) for ops, _ in edges)
    print(f"extreme corpus: {with_edges} of {len(edges)} programs hold an operand at an edge")
    assert 4 * with_edges >= 3 * len(edges) and not any(Z.has_edge_operands(ops) for ops, _ in ordinary)
    flat = [(op, a) for ops, _ in edges for op, a in ops]
    sub = lambda v: 0 < abs(v) < float(np.finfo(np.float32).tiny)                 # noqa: E731
    smooth = [a[0] for op, a in flat if op in (R.SMOOTH_UNION, R.SMOOTH_SUBTRACT)]
    radii = [a[0] for op, a in flat if op in (R.SPHERE, R.CUBE)]
    scales = [a for op, a in flat if op == R.PUSH_SCALE]
    assert any(sub(k) for k in smooth) and any(not sub(k) and sub(float(np.float32(k) * np.float32(0.25))) for k in smooth)
    assert any(sub(r) for r in radii) and any(r == 0 for r in radii) and any(r < 0 for r in radii)
    assert any(a[:3] == (0.0, 0.0, 0.0) for op, a in flat if op == R.PLANE)
    assert any(abs(np.linalg.det(np.array(a).reshape(3, 4)[:, :3])) < 1e-12 for op, a in flat if op == R.PUSH_AFFINE)
    assert any(s < 1e-18 for s, _ in scales) and any(s > 1e18 for s, _ in scales) and all(s > 0 and i > 0 for s, i in scales)
    assert any(abs(v) == float(np.float32(3e38)) for _, a in flat for v in a)


def test_the_failure_text_rebuilds_the_program(pkg, PM, corpus, extreme):
    """describe() is what a failure prints: executed as builder calls it gives the program back bit for bit."""
    for ops, bb in corpus[:13] + extreme[:13]:
        text = Z.describe(ops, bb)
        assert len(text.split("\n")) == len(ops) + 1
        rebuilt = eval("PM." + text.replace("\n", ""), {"PM": PM, "nan": float("nan"), "inf": float("inf")})   # noqa: S307
        assert rebuilt.bb == tuple(bb)
        assert [(op, np.array(a, np.float32).tobytes()) for op, a in rebuilt.ops] == [(op, np.array(a, np.float32).tobytes()) for op, a in ops]


def test_host_mirror_equals_the_numpy_restatement_bitwise_on_the_corpus(pkg, PM, V, corpus):
    """Every program of the corpus through the surface's batched host callback on program_ref.points(), with and without the
    material."""
    pts = R.points()
    for i, (ops, bb) in enumerate(corpus):
        surf = Z.builder(PM, ops, bb).build().as_surface()
        for distance_only in (False, True):
            want = R.run(ops, pts, distance_only)
            got = surface_records(V, surf, pts, distance_only, True)
            number = ~np.isnan(want[:, 0])                # (a NaN -- the huge points make some -- has no specified payload)
            bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1) & number)
            assert bad.size == 0, (Z.label(Z.seed(), i, ops, bb), distance_only, pts[bad[:4]], got[bad[:4]], want[bad[:4]])
            assert np.isnan(got[~number, 0]).all(), Z.label(Z.seed(), i, ops, bb)


def test_host_mirror_of_the_direct_march_equals_its_restatement_on_the_corpus(pkg, PM, corpus):
    """sdfv_program_raymarch_host against tests/program_march_ref.py on a share of the corpus (one program of every length): one
    43 x 27 frame from an orbit camera; every field of the march record and the depth bit for bit, rgba within the march's
    tolerance (pow is the one inexact step)."""
    from test_program_march_cpu import RGBA_TOL
    w, h = Z.MARCH_SIZE
    assert w % 8 and h % 8
    picked = Z.share(corpus)
    assert len(picked) >= 13
    air = pkg.lib.sdfv_air_dist()
    with_hits = 0
    for i in picked:
        ops, bb = corpus[i]
        rp, cam = Z.render_params(pkg, bb), Z.march_cameras(pkg, bb)[0]
        want_aux, want_rgba = M.march(ops, rp, cam, w, h, air_dist=air)
        rgba, aux, depth = Z.builder(PM, ops, bb).build().render_host(cam, w, h, rp=rp, want_aux=True, want_depth=True, threads=4)
        what = Z.label(Z.seed(), i, ops, bb)
        M.assert_aux_bitwise(M.aux_view(aux[0]), want_aux, what)
        assert (depth[0].view(np.uint32) == want_aux["depth"].view(np.uint32)).all(), what
        err = float(np.abs(rgba[0] - want_rgba).max())
        assert err <= RGBA_TOL, (what, err)
        with_hits += bool((want_aux["status"] == 1).any() and (want_aux["status"] == -2).any())
    print(f"direct march on the host: {len(picked)} programs, {with_hits} frames with hits and with rays that leave the box")
    assert 4 * with_hits >= 3 * len(picked)


def test_extreme_operands_through_the_host_callbacks(pkg, PM, V, extreme):
    """The extreme corpus on program_ref.odd_batch() -- +-inf, NaN, +-3e38 and subnormal coordinates among ordinary points --
    under the header's rule for NaN; that the batches hold both NaN and numeric results at odd points is asserted over the
    corpus as a whole."""
    pts, ordinary = R.odd_batch()
    nans = numbers = 0
    for i, (ops, bb) in enumerate(extreme):
        surf = Z.builder(PM, ops, bb).build().as_surface()
        for distance_only in (False, True):
            want, decided = R.run(ops, pts, distance_only, want_decided=True)
            got = surface_records(V, surf, pts, distance_only, True)
            R.assert_records_under_the_nan_rule(got, want, decided, ordinary, (Z.label(Z.seed(), i, ops, bb, "extreme_corpus"), distance_only),
                                                both_kinds=False)
        nans += int(np.isnan(want[:, 0]).sum())
        numbers += int((~np.isnan(want[~ordinary, 0])).sum())
    print(f"extreme corpus on the odd batch: {nans} NaN results, {numbers} numeric results at odd points")
    assert nans > 0 and numbers > 0


MESSAGES = {"unknown opcode": "unknown opcode", "reserved": "reserved words must be 0", "not finite": "is not finite", "k <= 0": "must be > 0",
            "s <= 0": "must be > 0", "value underflow": "value stack underflow", "value overflow": "value stack overflow",
            "frame underflow": "frame stack underflow", "frame overflow": "frame stack overflow",
            "POP closes a PUSH_SCALE": "closes a PUSH_SCALE", "POP_SCALE closes a PUSH_AFFINE": "closes a PUSH_AFFINE",
            "count": "instructions, not", "open frames": "open frame", "values": "values, not 1", "box": "bounding box"}


def test_create_agrees_with_the_restated_validity_rule(pkg, corpus, extreme):
    """sdfv_program_create on every program of both corpora and on 24 one-instruction edits of each: it succeeds exactly when
    first_error() finds nothing; otherwise it returns SDFV_ERR_INVALID_ARGUMENT with the kind of fault in its message, which
    starts with "op <index>" and, after the opcode's name if it gives one, a colon when the fault is an instruction's."""
    assert set(MESSAGES) == set(Z.ERROR_KINDS)
    rng = np.random.default_rng([Z.seed(), 7])
    valid = invalid = 0
    kinds = {}

    def check(ops, bb, what):
        reserved = [(i, k) for i, ins in enumerate(ops) if len(ins) > 2 for k in range(3) if ins[2][k]]
        want = Z.first_error(ops, bb)
        rc, msg = create_rc(pkg, [ins[:2] for ins in ops], bb=bb, reserved=reserved[0] if reserved else None)
        if want is None:
            assert rc == 0, (what, msg, Z.describe(ops, bb))
            return None
        index, kind = want
        assert rc == INVALID and MESSAGES[kind] in msg, (what, want, rc, msg, Z.describe(ops, bb))
        if index is not None:
            assert re.match(rf"op {index}( \([A-Z_]+\))?:", msg), (what, want, msg, Z.describe(ops, bb))
        kinds[kind] = kinds.get(kind, 0) + 1
        return kind

    for name, programs in (("corpus", corpus), ("extreme_corpus", extreme)):
        for i, (ops, bb) in enumerate(programs):
            assert check(ops, bb, (name, Z.seed(), i)) is None
            for what, edited in Z.mutations(rng, ops, 24):
                if check(edited, bb, (name, Z.seed(), i, what)) is None:
                    valid += 1
                else:
                    invalid += 1
    nan, inf = float("nan"), float("inf")
    for bb in ((-1, -1, -1, 1, -1, 1), (-1, -1, -1, 1, 1, -2), (-1, nan, -1, 1, 1, 1), (-1, -1, -1, inf, 1, 1), (0, 0, 0, 0, 0, 0)):
        for ops, _ in corpus[:5]:
            assert check(ops, bb, ("box", bb)) == "box"
    print(f"{valid} edits stay valid, {invalid} do not; refusals by kind: {dict(sorted(kinds.items()))}")
    assert 3 * valid >= valid + invalid and 3 * invalid >= valid + invalid, (valid, invalid)
    assert set(kinds) == set(Z.ERROR_KINDS), set(Z.ERROR_KINDS) - set(kinds)
