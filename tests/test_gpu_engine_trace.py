"""The engine's sequencing on the device provider, call by call, against tests/golden/engine_trace_gpu.json (recorded by
tools/engine_trace.py --record-gpu at the commit before the engine's decisions moved into one plan per pass): what the CPU mock cannot
reach -- the second stream and the `other` closure, a ragged batch with flip TTA -- with the same `hip_ops` calls in the same order on
the same buffers and on the same stream (launch stream or not).  Equality only: no arithmetic is compared here."""
import hashlib
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('engine_trace', os.path.join(ROOT, 'tools', 'engine_trace.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_engine_issues_the_recorded_device_calls():
    tool = _tool()
    with open(os.path.join(ROOT, 'tests', 'golden', 'engine_trace_gpu.json')) as f:
        golden = json.load(f)['cases']
    cases = tool.gpu_cases()
    assert [name for name, _ in cases] == list(golden)
    bad = []
    for name, spec in cases:
        calls = tool.run_gpu_case(spec)
        digests = [tool.call_digest(c) for c in calls]
        if hashlib.sha256(''.join(digests).encode()).hexdigest() == golden[name]['sha256']:
            continue
        bad.append(name)
        want = golden[name]['calls']
        i = next((i for i, d in enumerate(digests) if d[:4] != want[4 * i:4 * i + 4]), len(digests))
        print(f'{name}: {len(digests)} calls, recorded {len(want) // 4}; first difference at call {i}:',
              json.dumps(calls[i]) if i < len(calls) else '(the recorded sequence goes on)')
    assert not bad, bad
