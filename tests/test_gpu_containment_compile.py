"""Containment of the three compiled routes (tests/arena.py): the specialised kernels write only their declared outputs and read
only their declared inputs.  The cases are the plain handle's -- tests/test_gpu_containment_program.py's fill over one width of
each launcher class and its march, tests/test_gpu_containment_points.py's sampler -- with every handle they build compiled
first; their expected values are the numpy restatements', so this also holds the compiled kernels to those."""
import pytest

import test_gpu_containment_points as CPP
import test_gpu_containment_program as CP
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
    sampled = CPP.R.catalogue(PM)["all_ops"].build()   # (compiled here: the sampler's cases build their program inside the call)
    monkeypatch.setattr(CPP, "built_program", lambda: sampled)
    return made


def specialised_launches(made):
    return sum(p.compiled_info()["launches"] for p in made)


@pytest.mark.parametrize("slab", ["whole", "middle"])
@pytest.mark.parametrize("dims", [(40, 6, 3), (100, 6, 3), (257, 3, 5)], ids=["tx64", "tx128", "tx256"])
def test_compiled_fill(pkg, PM, compiled, dims, slab):  # noqa: N803
    CP.test_program_fill(pkg, PM, dims, "all_ops", slab)
    assert specialised_launches(compiled) > 0


@pytest.mark.parametrize("n_cam", [1, 17])
def test_compiled_march(pkg, PM, compiled, n_cam):  # noqa: N803
    CP.test_program_raymarch(pkg, PM, n_cam)
    assert specialised_launches(compiled) > 0


@pytest.mark.parametrize("in_off,out_off", [(0, 0), (4, 0), (0, 4)])
def test_compiled_sampler(pkg, PM, compiled, in_off, out_off):  # noqa: N803
    CPP.test_point_lists_stay_inside_their_buffers(pkg, PM, "program_sample_points", in_off, out_off)
    assert specialised_launches(compiled) > 0
