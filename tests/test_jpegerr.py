"""The numpy JPEG reference (tests/jpegerr.py) against libjpeg-turbo's own files (tests/golden/jpeg_pil.npz, tools/mint_jpeg.py), its entropy
coder against its decoder on crafted blocks, and ten seeded corruptions that the gates must catch."""
import io
import os

import numpy as np
import pytest

from tests import jpegerr as J
from tests.helpers import GOLDEN

CASES, VERSIONS = J.load_fixture(os.path.join(GOLDEN, 'jpeg_pil.npz'))
BY_NAME = {J.case_name(c): c for c in CASES}


def test_fixture_covers_what_it_should():
    assert any('libjpeg-turbo' in v for v in VERSIONS) and any('Pillow' in v for v in VERSIONS)
    assert {(c['H'], c['W']) for c in CASES} == {(1, 1), (16, 16), (33, 17), (40, 56), (72, 72), (250, 250), (16, 2048)}
    assert {c['kind'] for c in CASES} == {'noise', 'ramp', 'render', 'white', 'black'}
    assert {c['quality'] for c in CASES} == {25, 75, 90, 100} and {c['sub'] for c in CASES} == {'420', '444'}
    for size in {(c['H'], c['W']) for c in CASES}:
        assert any(c['kind'] == 'noise' and c['quality'] == 100 for c in CASES if (c['H'], c['W']) == size), size
    kinds = set()
    for c in CASES:
        mx, my, _ = J.geometry(c['H'], c['W'], c['sub'])
        kinds.add('row' if c['restart'] == mx and my > 1 else 'all' if c['restart'] > mx * my else c['restart'])
    assert {1, 3, 'row', 'all'} <= kinds
    assert os.path.getsize(os.path.join(GOLDEN, 'jpeg_pil.npz')) < 1 << 20


@pytest.mark.parametrize('c', CASES, ids=J.case_name)
def test_reference_equals_libjpeg(c):
    """every byte of the file, and every coefficient of the front stage"""
    ours = J.encode(c['rgb'], c['quality'], c['sub'], c['restart'])
    assert not J.gate_file('file', ours, c['file'])
    assert not J.gate_equal('coef', J.front(c['rgb'], c['quality'], c['sub']), c['coef'])
    p = J.parse(c['file'], decode=c['H'] * c['W'] <= 72 * 72)
    assert (p['H'], p['W'], p['sub'], p['restart'], p['header_len']) == (c['H'], c['W'], c['sub'], c['restart'], 629)
    assert np.array_equal(p['q'], J.quant_tables(c['quality'])[:, J.ZIGZAG])
    assert [(tc, bits, vals) for tc, bits, vals in p['huff']] == [(tc, b, v) for tc, (b, v) in zip((0x00, 0x10, 0x01, 0x11), J.HUFF)]
    assert p['rst'] == [i % 8 for i in range(len(p['intervals']) - 1)]
    if 'coef' in p:
        assert np.array_equal(p['coef'], c['coef'])
        assert J.scan(p['coef'], c['restart']) == p['scan']             # libjpeg's coefficients through our coder: its scan bytes


def test_fresh_cases_against_pillow():
    """where Pillow imports: sizes and contents that the fixture does not hold, and Pillow opens the reference's files"""
    Image = pytest.importorskip('PIL.Image')
    n = 0
    for (H, W) in ((7, 9), (8, 8), (17, 33), (24, 40), (31, 48), (50, 16)):
        for kind in ('noise', 'ramp', 'render'):
            for q, sub in ((25, '444'), (75, '420'), (90, '444'), (100, '420')):
                mx = J.geometry(H, W, sub)[0]
                for rs in (1, 3, mx, 5000):
                    rgb = J.content(kind, H, W, seed=1000 + n)
                    b = io.BytesIO()
                    Image.fromarray(rgb).save(b, 'JPEG', quality=q, subsampling={'420': 2, '444': 0}[sub], optimize=False, restart_marker_blocks=rs)
                    ours = J.encode(rgb, q, sub, rs)
                    assert not J.gate_file(f'{H}x{W} {kind} q{q} {sub} r{rs}', ours, b.getvalue())
                    n += 1
            im = Image.open(io.BytesIO(ours))
            im.load()
            assert im.size == (W, H) and im.mode == 'RGB'
    assert n == 288


@pytest.mark.parametrize('name', sorted(J.crafted_blocks()))
def test_crafted_blocks_round_trip(name):
    coef, rs = J.crafted_blocks()[name]
    n = coef.shape[0]
    my = 1 if n <= 256 else 2
    H, W = 8 * my, 8 * (n // my)
    parts = J.intervals(coef, rs)
    assert len(parts) == -(-n // rs) and all(b'\xff' not in p.replace(b'\xff\x00', b'') for p in parts)
    data = J.header(H, W, 90, '444', rs) + J.join(parts) + b'\xff\xd9'
    p = J.parse(data)
    assert np.array_equal(p['coef'], coef) and p['rst'] == [i % 8 for i in range(len(parts) - 1)]
    if name == 'only_63':                                                # DC 0 (2 bits), 3 ZRL (11 bits each), one symbol: no EOB
        bw = J._Bits()
        J.encode_block(bw, coef[0, 0], 0, J.DERIVED[0], J.DERIVED[1])
        assert 8 * len(bw.out) + bw.n == 2 + 3 * 11 + int(J.DERIVED[1][1][0xf3]) + 3
    if name == 'many_intervals':
        assert len(parts) == 11 and p['rst'][8:] == [0, 1]
    if name == 'ff_bytes':
        assert sum(x.count(b'\xff\x00') for x in parts) > 0
    if name == 'longest_block':          # the longest block there is: 11 + 11 bits of DC, 63 times (0, 10) at 12 + 10 bits; the bound of mbx.h is 22 + 63 * 26
        bw = J._Bits()
        J.encode_block(bw, coef[1, 1], int(coef[0, 1, 0]), J.DERIVED[2], J.DERIVED[3])
        assert 8 * len(bw.out) + bw.n == 22 + 63 * 22 <= 22 + 63 * 26
        assert max(int(t[1].max()) for t in J.DERIVED) == 16


# corruption -> the fixture case that shows it
SHOWS = dict(bias_swapped='33x17.noise.q100.420.r3', replicate_first='40x56.ramp.q25.420.r3', dummy_transformed='72x72.noise.q100.420.r1',
             half_even='72x72.noise.q90.420.r32', no_stuffing='72x72.noise.q100.420.r1', rst_not_mod8='72x72.noise.q100.420.r1',
             pred_not_reset='33x17.noise.q25.420.r1', pad_zero='40x56.noise.q75.444.r3', eob_after_63='16x16.noise.q100.420.r1',
             zrl_trailing='72x72.render.q90.444.r9')


@pytest.mark.parametrize('corrupt', J.CORRUPTIONS)
def test_seeded_corruptions_fail_a_gate(corrupt):
    assert set(SHOWS) == set(J.CORRUPTIONS) and len(J.CORRUPTIONS) >= 10
    c = BY_NAME[SHOWS[corrupt]]
    bad = J.encode(c['rgb'], c['quality'], c['sub'], c['restart'], corrupt=(corrupt,))
    msgs = J.gate_file(corrupt, bad, c['file'])
    assert msgs and 'differs at byte' in msgs[0] and 'restart interval' in msgs[0], msgs
    assert J.gate_files(corrupt, np.frombuffer(bad, np.uint8), np.array([0, len(bad)]), [c['file']])
    if corrupt in ('bias_swapped', 'replicate_first', 'dummy_transformed', 'half_even'):
        assert J.gate_equal('coef', J.front(c['rgb'], c['quality'], c['sub'], (corrupt,)), c['coef'])
    else:
        assert not J.gate_equal('coef', J.front(c['rgb'], c['quality'], c['sub'], (corrupt,)), c['coef'])


def test_gates_name_the_place():
    c = BY_NAME['72x72.noise.q100.420.r1']
    data = bytearray(c['file'])
    p = J.parse(c['file'], decode=False)
    at = p['header_len'] + sum(len(x) + 2 for x in p['intervals'][:7]) + 3
    data[at] ^= 0x10
    assert J.gate_file('x', data, c['file']) == [f'x: differs at byte {at} (lengths {len(data)} against {len(data)}), restart interval 7 of 25, byte 3 of its '
                                                 f'{len(p["intervals"][7])}']
    data = bytearray(c['file'])
    data[30] ^= 1
    assert 'in the header' in J.gate_file('x', data, c['file'])[0]
    assert J.gate_files('x', np.frombuffer(c['file'], np.uint8), np.array([0, 5]), [c['file']])      # offsets that do not frame the data
    assert not J.gate_files('x', np.frombuffer(c['file'] * 2, np.uint8), np.array([0, len(data), 2 * len(data)]), [c['file']] * 2)
