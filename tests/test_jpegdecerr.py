"""The numpy restatement of libjpeg's default decode path (tests/jpegdecerr.py) against libjpeg-turbo itself: the fixture minted from Pillow
(tests/golden/jpeg_dec_pil.npz), freshly drawn files where Pillow imports, the files of the encoder's reference; seeded corruptions that must
each fail a gate; malformed scans with their status codes; the refusals of the host parser (motionbert_amd.video.parse_jpeg)."""
import io
import os

import numpy as np
import pytest

from motionbert_amd import video as V
from tests import jpegdecerr as D
from tests import jpegerr as J
from tests.helpers import GOLDEN

CASES, VERSIONS = D.load_fixture(os.path.join(GOLDEN, 'jpeg_dec_pil.npz'))
ENC_CASES, _ = J.load_fixture(os.path.join(GOLDEN, 'jpeg_pil.npz'))


@pytest.mark.parametrize('i', range(len(CASES)), ids=[D.case_name(c) for c in CASES])
def test_reference_equals_the_fixture(i):
    c = CASES[i]
    p = D.parse(c['file'])
    assert (p['H'], p['W'], p['sub'], p['restart']) == (c['H'], c['W'], c['sub'], c['restart'])
    assert (p['dht'] is not None) and (not c['optimize'] or not np.array_equal(p['dht'], D.annex_k()))
    assert not J.gate_equal(D.case_name(c), D.decode(c['file']), c['rgb'])
    v = V.parse_jpeg(c['file'])                                          # the package's parser gives the same facts
    assert (v['H'], v['W'], v['subsampling'], v['restart'], v['scan']) == (p['H'], p['W'], p['sub'], p['restart'], p['scan'])
    assert np.array_equal(v['q'], p['q']) and np.array_equal(v['dht'], p['dht'])


def test_the_fixture_reaches_every_branch():
    subs = {c['sub'] for c in CASES}
    assert subs == {'444', '420', '422'} and {c['quality'] for c in CASES} == {25, 90, 100} and {c['optimize'] for c in CASES} == {False, True}
    assert any(c['restart'] == 0 for c in CASES) and any(c['restart'] == 1 for c in CASES)
    for sub in ('420', '422'):
        dws = {-(-c['W'] // 2) for c in CASES if c['sub'] == sub}
        assert dws & {1, 2} and 4 in dws and 1024 in dws, (sub, dws)
    assert any(len(v) for v in VERSIONS)


def test_fresh_files_against_pillow():
    """a few hundred small files drawn now, where Pillow is installed"""
    Image = pytest.importorskip('PIL.Image')
    g = np.random.default_rng(77)
    for n in range(300):
        H, W = int(g.integers(1, 41)), int(g.integers(1, 41))
        sub = ('444', '420', '422')[n % 3]
        rgb = J.content(('noise', 'ramp', 'render')[int(g.integers(0, 3))], H, W, seed=n)
        b = io.BytesIO()
        Image.fromarray(rgb).save(b, 'JPEG', quality=int(g.choice([25, 60, 90, 100])), subsampling={'444': 0, '422': 1, '420': 2}[sub],
                                  optimize=bool(n & 1), restart_marker_blocks=int(g.integers(0, 4)))
        ref = np.asarray(Image.open(io.BytesIO(b.getvalue())).convert('RGB'))
        assert not J.gate_equal(f'fresh {n} {H}x{W} {sub}', D.decode(b.getvalue()), ref)


@pytest.mark.parametrize('i', [i for i, c in enumerate(ENC_CASES) if c['H'] * c['W'] <= 72 * 72], ids=lambda i: J.case_name(ENC_CASES[i]))
def test_the_encoders_files_come_back(i):
    """jpegerr.encode writes libjpeg's file (tests/test_jpegerr.py); decoding it gives libjpeg's coefficients unchanged, and libjpeg's pixels"""
    c = ENC_CASES[i]
    data = J.encode(c['rgb'], c['quality'], c['sub'], c['restart'])
    assert data == c['file']
    coef, status, _ = D.entropy(data)
    assert not status.any() and not J.gate_equal('coef', coef, c['coef']) and not J.gate_equal('front', coef, J.front(c['rgb'], c['quality'], c['sub']))
    assert np.array_equal(coef, J.parse(data)['coef'])
    try:
        from PIL import Image
    except ImportError:
        return
    assert not J.gate_equal('pixels', D.decode(data), np.asarray(Image.open(io.BytesIO(data)).convert('RGB')))


@pytest.mark.parametrize('name', D.CORRUPTIONS)
def test_every_seeded_corruption_fails_a_gate(name):
    failed = 0
    for c in CASES:
        if c['H'] * c['W'] > 64 * 48:
            continue
        try:
            failed += bool(J.gate_equal(name, D.decode(c['file'], corrupt=(name,)), c['rgb']))
        except ValueError:                                                # the corrupted decoder runs out of bits or codes
            failed += 1
    if name == 'clamp_not_table':                                         # no picture leaves the clamp-like part of the table: jpegdecerr.crafted_range
        assert not failed
        failed = bool(J.gate_equal(name, D.decode(D.crafted_range(), corrupt=(name,)), D.decode(D.crafted_range())))
    assert failed, f'{name} passes every case'


def test_extend_and_range_table():
    """the two places the spelled-out definition is easiest to get wrong"""
    assert [D._Reader(bytes([v << 5])).receive(3) for v in range(8)] == [-7, -6, -5, -4, 4, 5, 6, 7]
    assert D.LIMIT.shape == (1024,) and D.LIMIT[[0, 127, 128, 511, 512, 895, 896, 1023]].tolist() == [128, 255, 255, 255, 0, 0, 0, 127]
    assert (D._fix(1.402), D._fix(1.772), D._fix(0.34414), D._fix(0.71414)) == (91881, 116130, 22554, 46802)


@pytest.mark.parametrize('name', sorted(D.malformed()))
def test_malformed_scans_have_a_defined_result(name):
    data, k, st = D.malformed()[name]
    coef, status, pos = D.entropy(data)
    good, _, _ = D.entropy(J.encode(J.content('noise', 16, 24, seed=11), 90, '444', 2))
    assert status[k] == st
    if st == D.MARKERS:
        assert (status == st).all() and not coef.any()
    else:
        others = [j for j in range(3) if j != k]
        assert not status[others].any() and all(np.array_equal(coef[2 * j:2 * j + 2], good[2 * j:2 * j + 2]) for j in others if name != 'run_past_63' or j)
        blocks = coef[2 * k:2 * k + 2].reshape(6, 64)
        if st != D.LEFTOVER:
            first_zero = next(i for i in range(6) if not blocks[i].any())
            assert not blocks[first_zero:].any() and first_zero < 6
    with pytest.raises(ValueError, match='interval'):
        D.decode(data)
    with pytest.raises(ValueError, match=f'frame 0, restart interval {0 if st == D.MARKERS else k} of 3: status {st}'):
        V.decode_jpeg([data], ops=D.RefOps())


def _good():
    return J.encode(J.content('render', 16, 24, seed=2), 90, '420', 1)


def _patch(data, at, new):
    return data[:at] + bytes(new) + data[at + len(bytes(new)):]


def test_parser_refuses_by_name():
    good = _good()
    sof, dqt, sos = good.index(b'\xff\xc0'), good.index(b'\xff\xdb'), good.index(b'\xff\xda')
    assert V.parse_jpeg(good)['subsampling'] == '420'
    bad = [(_patch(good, sof + 1, [0xc1]), 'SOF1'), (_patch(good, sof + 1, [0xc2]), 'SOF2'), (_patch(good, sof + 1, [0xc9]), 'SOF9'),
           (_patch(good, sof + 1, [0xcf]), 'SOF15'), (good[:sof] + b'\xff\xcc\x00\x04\x00\x10' + good[sof:], 'DAC'),
           (_patch(good, sof + 4, [12]), 'SOF0: 12 bit'), (_patch(good, dqt + 4, [0x10]), 'DQT: table 0 has 16-bit'),
           (_patch(good, sof + 9, [1]), 'SOF0: 1 components'), (_patch(good, sof + 9, [4]), 'SOF0: 4 components'),
           (_patch(good, sof + 11, [0x12]), 'SOF0: sampling factors'), (_patch(good, sof + 14, [0x22]), 'SOF0: sampling factors'),
           (good[:-2] + b'\xff\xda' + good[sos + 2:], 'SOS after the scan'), (good[:-2] + b'\xff\xdc\x00\x04\x00\x10\xff\xd9', 'DNL after the scan'),
           (good[:-2] + b'\xff\xc4\x00\x02\xff\xd9', 'DHT after the scan'), (good[2:], 'SOI'), (good[:-2], 'EOI'), (good[:sos], 'SOS'),
           (_patch(good, sos + 4, [1]), 'SOS: a scan of 1 components'), (_patch(good, sos + 11, [1]), 'SOS: spectral selection'),
           (good[:sof] + b'\xff\xdc\x00\x04\x00\x10' + good[sof:], 'DNL'), (_patch(good, sof + 5, [0x10, 0]), 'SOF0: a frame of 4096')]
    for data, match in bad:
        with pytest.raises(ValueError, match=match):
            V.parse_jpeg(data)
        with pytest.raises(ValueError, match=match):                     # and nothing is launched
            ops = D.RefOps()
            try:
                V.decode_jpeg([good, data], ops=ops)
            finally:
                assert not ops.calls
    # what is skipped: APPn, COM, fill bytes; a frame without DHT takes Annex K; any table ids
    dht = good.index(b'\xff\xc4')
    bare = good[:dht] + good[good.index(b'\xff\xdd'):]
    assert V.parse_jpeg(bare)['dht'] is None and np.array_equal(D.decode(bare), D.decode(good))
    extra = good[:2] + b'\xff\xfe\x00\x05abc' + b'\xff\xff\xff\xe1\x00\x04xy' + good[2:]
    assert np.array_equal(V.decode_jpeg([extra, bare], ops=D.RefOps())[1].numpy(), D.decode(good))
    with pytest.raises(ValueError, match='DHT'):
        V.parse_jpeg(_patch(good, dht + 2, [0x00, 0x05]))                # a table shorter than its sixteen counts
