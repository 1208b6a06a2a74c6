"""tests/mesh_ref.py is the one restatement that every device extraction route is held to, bit for bit; this holds it, through
every SDF kind's adapter, to tests/golden/mesh_ref_pins.json: sha256 digests of the vertices, the indices and the cube cases
(marching cubes) or the Hermite records, cells, mass points and edge counts (dual contouring), recorded from the per-kind
restatements that mesh_ref.py replaced.  The cases and the digest are tests/golden/make_golden.py's (mesh_ref_pin_cases), which
also regenerates the file.  No device needed."""
import importlib.util
import json
import os

import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
make_golden = importlib.util.module_from_spec(spec)
spec.loader.exec_module(make_golden)
CASES = make_golden.mesh_ref_pin_cases()
PINS = json.load(open(os.path.join(GOLD, "mesh_ref_pins.json")))


@pytest.mark.parametrize("name", sorted(set(CASES) | set(PINS)))
def test_the_restatement_returns_what_is_pinned(name):
    assert name in CASES and name in PINS, "every case is pinned and every pin is a case"
    assert CASES[name]() == PINS[name]
