"""The decode of csrc/jpeg_sync.hip run on the HOST: tools/jpeg_sync_host.cpp includes the kernels' own reader, lookup and sync_decode (they are
__host__ __device__) and walks the stages over them lane by lane.  Built here with AddressSanitizer and UBSan as a stand-alone program, so
that the code which reads bytes it did not write is checked against the numpy model (tests/jpegsyncerr.py) and for reads outside the
interval before it ever runs on a GPU: coefficients, route and the rounds of the speculation."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import jpegdecerr as D
from tests import jpegerr as J
from tests import jpegsyncerr as Y
from tests.helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    hipcc = next((c for c in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc') if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip('hipcc not available')
    out = str(tmp_path_factory.mktemp('jpeg_sync_host') / 'jpeg_sync_host')
    subprocess.run([hipcc, '-x', 'hip', '--offload-arch=gfx950', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                    '-fno-sanitize-recover=undefined', os.path.join(ROOT, 'tools', 'jpeg_sync_host.cpp'), '-o', out], check=True)
    return out


@pytest.fixture(scope='module')
def lib():
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    return hip_ops.load_library()


def _intervals(name, f=None):
    """(raw bytes, dht, bpm, MCUs, reference coef, model route) of every interval of an input whose markers are right"""
    (coef, _), (_, _, route) = Y.reference(name) if f is None else (D.entropy(f)[:2], Y.entropy_sync(f))
    f = Y.inputs()[name] if f is None else f
    p = D.parse(f)
    mx, my, bpm = D.geometry(p['H'], p['W'], p['sub'])
    n_int, per = D.n_intervals(p['H'], p['W'], p['sub'], p['restart']), p['restart'] or mx * my
    pos, ok = D.positions(f, p['scan'], n_int)
    for k in range(n_int if ok else 0):
        a, b = k * per, min(k * per + per, mx * my)
        yield f[pos[k]:max(pos[k + 1] - 2, pos[k])], p['dht'], bpm, b - a, coef[a:b], int(route[k])


def test_the_kernels_decode_on_the_host_equals_the_model(program, lib, tmp_path):
    names = [k for k in sorted(Y.inputs()) if not k.startswith('sweep') or int(k[6:]) % 4 == 0]
    items = [(name,) + it for name in names for it in _intervals(name)]
    cases, _ = D.load_fixture(os.path.join(GOLDEN, 'jpeg_dec_pil.npz'))    # the files Pillow wrote: 4:2:2, optimised tables, every restart
    items += [(D.case_name(c),) + it for c in cases for it in list(_intervals(None, c['file']))[:3]]
    with open(tmp_path / 'in.bin', 'wb') as f:
        f.write(struct.pack('<i', len(items)))
        for _, raw, dht, bpm, n_mcu, _, _ in items:
            tables = np.zeros((6, 228), np.uint32)
            dht = None if dht is None else np.ascontiguousarray(dht, np.uint8)
            assert lib.mbx_jpeg_dec_tables(None if dht is None else dht.ctypes.data, tables.ctypes.data) == 0
            f.write(struct.pack('<qii', len(raw), bpm, n_mcu) + tables.tobytes() + raw)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')
    subprocess.run([program, str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')], check=True, env=env)
    out, at, failed = open(tmp_path / 'out.bin', 'rb').read(), 0, []
    for name, raw, dht, bpm, n_mcu, ref, route in items:
        got_route, got_rounds = struct.unpack_from('<ii', out, at)
        coef = np.frombuffer(out, np.int16, n_mcu * bpm * 64, at + 8).reshape(n_mcu, bpm, 64)
        at += 8 + coef.nbytes
        if route != 3 and got_route != route:
            failed.append(f'{name}: route {got_route} against {route}')
        if got_route == 0:
            failed += J.gate_equal(name, coef, ref)
        if name.startswith('white.') and route == 0 and got_rounds != Y.rounds(raw, dht, bpm):
            failed.append(f'{name}: {got_rounds} rounds against {Y.rounds(raw, dht, bpm)}')
    assert at == len(out) and len(items) > 60
    assert not failed, failed
