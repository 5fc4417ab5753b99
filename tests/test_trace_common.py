"""tools/trace_common.py on the CPU: synthetic stamp buffers with planted phase lengths, two hardware ids and unwritten records."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location('trace_common', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'trace_common.py'))
tc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tc)

WIDTH, PHASES_US = 6, (3.0, 10.0, 1.5, 4.0)       # a record: five stamps (four phases) and the hardware id
TOTAL_US, GAP_US = sum(PHASES_US), 2.5


def make(n, unwritten=(), scale=None):
    """n records on two CUs (hardware ids 7 and 9, alternating): on each CU a record enters GAP_US after its predecessor's last stamp.
    scale[k] stretches every phase of record k (default 1).  The records in `unwritten` stay zero."""
    scale = np.ones(n) if scale is None else np.asarray(scale, dtype=np.float64)
    buf = np.zeros((n + 3, WIDTH), dtype=np.int64)          # three records behind the n of the launch: never looked at
    clock = {7: 1000.0, 9: 1003.0}                          # us; the stamps are 100 MHz ticks
    for k in range(n):
        hw = 7 if k % 2 == 0 else 9
        t = clock[hw] + np.concatenate([[0.0], np.cumsum(np.array(PHASES_US) * scale[k])])
        clock[hw] = t[-1] + GAP_US
        if k not in unwritten:
            buf[k, :5], buf[k, 5] = np.round(t * tc.TICKS_PER_US).astype(np.int64), hw
    buf[n:] = -1
    return buf.reshape(-1)


def medians(lines):
    return [float(ln.split(' us (')[0].split()[-1]) for ln in lines]


def test_records_drops_exactly_the_unwritten_rows():
    raw = tc.records(make(40, unwritten=(0, 17, 39)), 40, WIDTH)
    assert raw.shape == (37, WIDTH) and (raw[:, 0] > 0).all() and (raw != -1).all()
    assert (raw[:, 5] == 7).sum() == 19 and (raw[:, 5] == 9).sum() == 18       # record 0 ran on CU 7, records 17 and 39 on CU 9
    assert len(tc.records(make(40), 40, WIDTH)) == 40


def test_phase_table_reports_the_planted_medians():
    raw = tc.records(make(41, unwritten=(5,)), 41, WIDTH)
    lines = tc.phase_table(tc.to_us(raw[:, :5]), ['a', 'b', 'c', 'd'], 0, 12, whole='whole thing')
    assert [ln.split()[0] for ln in lines] == ['a', 'b', 'c', 'd', 'whole']
    assert medians(lines) == [3.0, 10.0, 1.5, 4.0, TOTAL_US]
    assert all('(10th / 90th percentile ' in ln for ln in lines) and lines[0].startswith('a' + ' ' * 12)


def test_cut_rule():
    cut = 4
    for n in (4 * cut - 1, 4 * cut, 4 * cut + 1, 40):
        scale = np.ones(n)
        scale[:2 * cut:2], scale[1:2 * cut:2] = 3.0, 3.0        # the first `cut` records of each CU = the first 2 cut in order of entry ...
        us = tc.to_us(tc.records(make(n, scale=scale), n, WIDTH)[:, :5])
        st = tc.steady(us, cut)
        assert (np.diff(st[:, 0]) >= 0).all()                   # in order of entry
        if n <= 4 * cut:
            assert len(st) == n                                 # everything is kept at or below 4 cut records
        else:
            assert len(st) == n - 2 * cut                       # `cut` records leave at each end
            order = np.argsort(us[:, 0], kind='stable')
            assert np.array_equal(st, us[order][cut:n - cut])
        assert len(tc.steady(us, 0)) == n
    # ... so at 40 records the cut of 4 removes half of the stretched ones and the median phase is still the planted one
    assert medians(tc.phase_table(us, ['a', 'b', 'c', 'd'], cut, 4))[:4] == [3.0, 10.0, 1.5, 4.0]


def test_same_cu_gaps_returns_the_planted_gaps():
    raw = tc.records(make(30), 30, WIDTH)
    gaps = tc.same_cu_gaps(tc.to_us(raw[:, :5]), raw[:, 5], 4)
    assert len(gaps) == 28 and np.allclose(gaps, GAP_US, atol=0.011)      # 15 records per CU: 14 gaps each; stamps are rounded to 10 ns ticks
    assert len(tc.same_cu_gaps(tc.to_us(raw[:1, :5]), raw[:1, 5], 4)) == 0
