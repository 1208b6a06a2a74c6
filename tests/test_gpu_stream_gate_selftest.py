"""The stream harness catches what it claims (tests/stream_gate.py): four fake entry points written in torch, each wrong in one
way and harmless, must each be reported by exactly the assertion that names the fault; the same entry written correctly passes
the gate and the capture.  The entry: y = x * k, x and y device arrays of 1000 floats, k a HOST array of one float."""
import ctypes as C

import numpy as np
import pytest
import torch

import stream_gate as SG
from stream_gate import capture, gate  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
N = 1000
_PINNED = {}   # address of a host argument -> the pinned tensor behind it (what lets a fake read it LATE, from a stream)


def host_k():
    """A fresh host argument: a ctypes array of one float (3.0) over pinned memory."""
    pin = torch.empty(4, dtype=torch.float32).pin_memory()
    pin[:] = 3.0
    k = (C.c_float * 4).from_address(pin.data_ptr())
    _PINNED.clear()
    _PINNED[C.addressof(k)] = pin
    return {"k": k}


def correct(t, h):
    torch.mul(t["x"], float(h["k"][0]), out=t["y"])


def on_the_default_stream(t, h):
    with torch.cuda.stream(torch.cuda.default_stream()):
        torch.mul(t["x"], float(h["k"][0]), out=t["y"])


def synchronises(t, h):
    torch.mul(t["x"], float(h["k"][0]), out=t["y"])
    torch.cuda.current_stream().synchronize()


def reads_its_host_argument_late(t, h):
    """Keeps the array and uploads it from a second stream, ordered behind the caller's stream and joined back into it: in the
    right order on the device, but the host memory is read when the copy runs, after the call has returned."""
    s, side = torch.cuda.current_stream(), torch.cuda.Stream()
    kdev = t["k_scratch"]
    side.wait_stream(s)
    with torch.cuda.stream(side):
        kdev.copy_(_PINNED[C.addressof(h["k"])], non_blocking=True)
    s.wait_stream(side)
    torch.mul(t["x"], kdev[0], out=t["y"])


def writes_from_an_unjoined_stream(t, h):
    """Ordered behind the caller's earlier work, but the caller's stream never waits for it."""
    s, side = torch.cuda.current_stream(), torch.cuda.Stream()
    k = float(h["k"][0])
    side.wait_stream(s)
    with torch.cuda.stream(side):
        SG.sleep_ms(2.0)
        torch.mul(t["x"], k, out=t["y"])


def case_of(call):
    x = np.random.default_rng(3).uniform(1.0, 2.0, N).astype(np.float32)
    outputs = {"y": ((N,), np.float32, 4)}
    expected = {"y": x * np.float32(3.0)}
    if call is reads_its_host_argument_late:   # its device scratch: inside the arena, content open
        outputs["k_scratch"] = ((4,), np.float32, 4)
        expected["k_scratch"] = SG.A.Untouched(np.zeros(4, np.float32), undefined=True)
    return SG.Case(call.__name__, call, expected, inputs={"x": (x, 4)}, outputs=outputs, host=host_k,
                   second=({"x": x[::-1]}, {**expected, "y": x[::-1] * np.float32(3.0)}))


def test_a_correct_entry_passes(pkg, gate, capture):
    gate.run(pkg, case_of(correct))
    capture.run(pkg, case_of(correct))


@pytest.mark.parametrize("fake,assertion", [(on_the_default_stream, SG.NotOrdered), (synchronises, SG.Waited),
                                            (reads_its_host_argument_late, SG.HostArgsLate), (writes_from_an_unjoined_stream, SG.NotVisible)],
                         ids=["default-stream", "synchronises", "late-host-read", "unjoined-stream"])
def test_each_fault_is_reported_by_the_assertion_that_names_it(pkg, gate, fake, assertion):
    with pytest.raises(SG.GateError) as e:
        gate.run(pkg, case_of(fake))
    print(e.value)
    assert e.type is assertion, f"{fake.__name__} was reported as {e.type.__name__}: {e.value}"
    torch.cuda.synchronize()
