"""Containment of the point-list calls of the compiled mesh route (tests/arena.py): the specialised kernels of
sdfv_program_normal_points and sdfv_program_mesh_postproc write only their declared outputs and read only their declared
inputs.  The cases are the plain handle's (tests/test_gpu_containment_points.py) with the handle compiled with
SDFV_COMPILE_MESH first; their expected values are the numpy restatements', so this also holds the compiled kernels to those."""
import pytest

import test_gpu_containment_points as CPP
from test_gpu_containment_points import PM  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture
def compiled(monkeypatch, PM):  # noqa: N803
    handle = CPP.R.catalogue(PM)["all_ops"].build().compile(PM.MESH)
    monkeypatch.setattr(CPP, "built_program", lambda: handle)
    return handle


@pytest.mark.parametrize("entry", ["program_normal_points", "program_mesh_postproc"])
def test_compiled_mesh_calls_stay_inside_their_buffers(pkg, PM, compiled, entry):  # noqa: N803
    """16-byte aligned arrays: n = 256, 257 and 513 reach the staged kernel and the tail, postproc its 16-byte form."""
    CPP.test_point_lists_stay_inside_their_buffers(pkg, PM, entry, 0, 0)
    assert compiled.compiled_info()["launches"] > 0
