"""The engine's sequencing, call by call, against tests/golden/engine_trace.json (recorded by tools/engine_trace.py at the commit before
the sub-layer helpers of engine.py replaced the per-sub-layer copies): in every mode the same `ops` calls in the same order on the same
buffers.  What a call records, and the matrix of cases, are described in the tool."""
import hashlib
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('engine_trace', os.path.join(ROOT, 'tools', 'engine_trace.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'engine_trace.json')) as f:
        return json.load(f)


def test_engine_issues_the_recorded_calls():
    tool, golden = _tool(), _golden()['cases']
    cases = tool.cases()
    assert [name for name, _ in cases] == list(golden)
    bad = []
    for name, spec in cases:
        calls, _ = tool.run_case(spec)
        digests = [tool.call_digest(c) for c in calls]
        if hashlib.sha256(''.join(digests).encode()).hexdigest() == golden[name]['sha256']:
            continue
        bad.append(name)
        want = golden[name]['calls']
        i = next((i for i, d in enumerate(digests) if d[:4] != want[4 * i:4 * i + 4]), len(digests))
        print(f'{name}: {len(digests)} calls, recorded {len(want) // 4}; first difference at call {i}:',
              json.dumps(calls[i]) if i < len(calls) else '(the recorded sequence goes on)')
    assert not bad, bad


def test_linear_names_and_folded_pairs_keep_their_order():
    """The flat gradient layout and the descriptor tables of the packers follow these lists."""
    assert _tool().layouts() == _golden()['layouts']
