"""The point-list entry points on the caller's stream (tests/stream_gate.py): sample_points (+ distance only), normal_points,
source_sample_scalar, source_sample_normal, mesh_postproc, the three program forms, lattice_points, lattice_from_samples and
lattice_normals.  Values and launches are tests/test_gpu_containment_points.py's tables (oracle and numpy restatements).

Shapes: n = 257 with every array 16-byte aligned is one staged workgroup plus a scalar tail of one point -- the two launches of
launch_staged_then_tail (csrc/kernel_common.h), both of which must be on the caller's stream; n = 255 with every array off a
16-byte boundary by 4 is the scalar kernel alone.  lattice_points has no device input: the late output poison carries its
ordering check alone.  Capture's second replay: the inputs reversed give the outputs reversed."""
import numpy as np
import pytest

import stream_gate as SG
import test_gpu_containment_points as CP
from stream_gate import capture, gate  # noqa: F401 (fixtures)
from test_gpu_containment_points import PM  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
SHAPES = [(257, 0), (255, 4)]   # n, bytes off a 16-byte boundary


def case_of(pkg, PM, entry, n, off):  # noqa: N803
    inputs, inplace, outputs = CP.reference(entry)
    cut = lambda name, a: a if name in CP.WHOLE_INPUTS else np.ascontiguousarray(a[:n])  # noqa: E731
    rev = lambda name, a: a if name in CP.WHOLE_INPUTS else np.ascontiguousarray(a[:n][::-1])  # noqa: E731
    expected = {name: np.ascontiguousarray(a[:n]) for name, a in outputs.items()}
    over = {name: rev(name, a) for name, a in (*inputs.items(), *inplace.items())}
    second = (over, {name: np.ascontiguousarray(a[:n][::-1]) for name, a in outputs.items()}) if over else None
    return SG.Case(f"{entry}[{n}+{off}]", lambda t, h: CP.launch(pkg, PM, entry, t, n, prm=h["params"]), expected,
                   inputs={name: (cut(name, a), 16, off) for name, a in inputs.items()},
                   inouts={name: (cut(name, a), 16, off) for name, a in inplace.items()},
                   outputs={name: (a[:n].shape, a.dtype, 16, off) for name, a in outputs.items() if name not in inplace},
                   host=lambda: {"params": pkg.default_params()}, second=second)


@pytest.mark.parametrize("n,off", SHAPES)
@pytest.mark.parametrize("entry", CP.ENTRIES)
def test_point_lists_run_on_the_callers_stream(pkg, PM, gate, entry, n, off):  # noqa: N803
    gate.run(pkg, case_of(pkg, PM, entry, n, off))


@pytest.mark.parametrize("n,off", SHAPES)
@pytest.mark.parametrize("entry", CP.ENTRIES)
def test_point_lists_only_enqueue(pkg, PM, capture, entry, n, off):  # noqa: N803
    capture.run(pkg, case_of(pkg, PM, entry, n, off))
