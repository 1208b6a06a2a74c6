"""The point-list calls of the compiled mesh route on the caller's stream (tests/stream_gate.py): sdfv_program_normal_points and
sdfv_program_mesh_postproc through a handle compiled with SDFV_COMPILE_MESH wait behind a sleep on the caller's stream, and
normal_points is captured into a graph and replays to the same bits.  The cases -- shapes, expected values -- are the plain
handle's (tests/test_gpu_stream_points.py); sdfv_program_compile is synchronous host work (it also loads the module and makes
the device copy), done before the gate closes or the capture begins."""
import pytest

import test_gpu_containment_points as CPP
import test_gpu_stream_points as SPT
from stream_gate import capture, gate  # noqa: F401 (fixtures)
from test_gpu_containment_points import PM  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
N, OFF = SPT.SHAPES[0]   # 257 points, every array 16-byte aligned: a staged launch and a tail launch


@pytest.fixture
def compiled(monkeypatch, PM):  # noqa: N803
    """The program of the borrowed cases compiled with MESH, before the case runs."""
    handle = CPP.R.catalogue(PM)["all_ops"].build().compile(PM.MESH)
    monkeypatch.setattr(CPP, "built_program", lambda: handle)
    return handle


@pytest.mark.parametrize("entry", ["program_normal_points", "program_mesh_postproc"])
def test_compiled_mesh_calls_run_on_the_callers_stream(pkg, PM, gate, compiled, entry):  # noqa: N803
    gate.run(pkg, SPT.case_of(pkg, PM, entry, N, OFF))
    assert compiled.compiled_info()["launches"] > 0


def test_compiled_normal_points_only_enqueues(pkg, PM, capture, compiled):  # noqa: N803
    capture.run(pkg, SPT.case_of(pkg, PM, "program_normal_points", N, OFF))
    assert compiled.compiled_info()["launches"] > 0
