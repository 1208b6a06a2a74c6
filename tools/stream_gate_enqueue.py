#!/usr/bin/env python3
"""The figures behind tests/stream_gate.py's T: runs tests/test_gpu_stream_*.py in this process (one MI355X) and prints the host
time of every gated sequence -- the sleep's enqueue to the return of the call under test -- slowest first, with the T that
follows from the slowest: max(50 ms, 100 x slowest).  The self-test's fakes are left out (one of them waits on purpose).

    python tools/stream_gate_enqueue.py [--top 10] [--out profiles/stream_gate_enqueue.json]

stream_gate.ENQUEUE_MS_SLOWEST and T_MS are written by hand from this output; a slowest time that has grown past
ENQUEUE_MS_SLOWEST means they are due again."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["test_gpu_stream_points.py", "test_gpu_stream_grid.py", "test_gpu_stream_program.py", "test_gpu_stream_march.py"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pytest
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider"] + [os.path.join(ROOT, "tests", f) for f in FILES])
    import stream_gate  # (tests/conftest.py has put tests/ on the path; the module the tests filled)
    times = dict(sorted(stream_gate.ENQUEUE_LOG.items(), key=lambda kv: -kv[1]))
    if not times:
        print("no gate ran", file=sys.stderr)
        return int(rc) or 1
    slowest = next(iter(times.values()))
    for name, ms in list(times.items())[:args.top]:
        print(f"{ms:8.3f} ms  {name}")
    record = {"cases": len(times), "slowest_ms": slowest, "t_ms": max(50.0, 100.0 * slowest),
              "in_use": {"ENQUEUE_MS_SLOWEST": stream_gate.ENQUEUE_MS_SLOWEST, "T_MS": stream_gate.T_MS}, "enqueue_ms": times}
    print(json.dumps({k: v for k, v in record.items() if k != "enqueue_ms"}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
    return int(rc)


if __name__ == "__main__":   # (tests that spawn workers re-import the main module)
    sys.exit(main())
