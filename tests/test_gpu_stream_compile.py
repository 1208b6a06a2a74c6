"""The three compiled routes on the caller's stream (tests/stream_gate.py): the specialised launches of a compiled handle wait
behind a sleep on the caller's stream, are captured into a graph and replay to the same bits.  The cases -- shapes, expected
values, host arguments -- are the plain handle's (tests/test_gpu_stream_program.py, tests/test_gpu_stream_points.py) with every
handle they build compiled first: sdfv_program_compile is synchronous host work (it also loads the module and makes the device
copy), done before the gate closes or the capture begins."""
import pytest

import test_gpu_containment_points as CPP
import test_gpu_stream_points as SPT
import test_gpu_stream_program as SP
from stream_gate import capture, gate  # noqa: F401 (fixtures)
from test_gpu_containment_program import PM  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture
def compiled(monkeypatch, PM):  # noqa: N803
    """Every Program.build() of the borrowed cases returns a handle compiled for all three routes; -> the handles made."""
    made = []
    plain_build = PM.Program.build

    def build(self):
        made.append(plain_build(self).compile(PM.FILL | PM.POINTS | PM.MARCH))
        return made[-1]
    monkeypatch.setattr(PM.Program, "build", build)
    SP.program.cache_clear()
    sampled = CPP.R.catalogue(PM)["all_ops"].build()   # (compiled here: the sampler's cases build their program inside the call)
    monkeypatch.setattr(CPP, "built_program", lambda: sampled)
    yield made
    SP.program.cache_clear()


def specialised_launches(made):
    return sum(p.compiled_info()["launches"] for p in made)


@pytest.mark.parametrize("volume", SP.VOLUMES)
def test_compiled_fill_runs_on_the_callers_stream(pkg, PM, gate, capture, compiled, volume):  # noqa: N803
    gate.run(pkg, SP.fill_case(pkg, volume))
    capture.run(pkg, SP.fill_case(pkg, volume))
    assert specialised_launches(compiled) > 0


@pytest.mark.parametrize("n_cam", [1, 20])
def test_compiled_march_runs_on_the_callers_stream(pkg, PM, gate, capture, compiled, n_cam):  # noqa: N803
    gate.run(pkg, SP.march_case(pkg, PM, n_cam))
    capture.run(pkg, SP.march_case(pkg, PM, n_cam))
    assert specialised_launches(compiled) > 0


@pytest.mark.parametrize("n,off", SPT.SHAPES)
def test_compiled_sampler_runs_on_the_callers_stream(pkg, PM, gate, capture, compiled, n, off):  # noqa: N803
    gate.run(pkg, SPT.case_of(pkg, PM, "program_sample_points", n, off))
    capture.run(pkg, SPT.case_of(pkg, PM, "program_sample_points", n, off))
    assert specialised_launches(compiled) > 0
