"""What the kernel trace tools (tools/*_trace.py) share: arming a diagnostic build of the library with a sized stamp buffer, one timed
launch, and the arithmetic on the stamps (plain numpy: tests/test_trace_common.py runs it without a GPU or a library).
A diagnostic build exports mbx_diag_set_trace(buf, bytes) and mbx_diag_last_need(): every traced launch computes the bytes its grid can
write and stamps only if the armed buffer holds them (csrc/mbx_diag.h)."""
import atexit
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # the tools import motionbert_amd from the tree

TICKS_PER_US = 100.0      # s_memrealtime: 100 MHz


def arm(ops, n_int64):
    """A zeroed int64 device buffer of n_int64 elements, handed to the library behind `ops`; withdrawn again at exit."""
    import torch
    if not hasattr(ops.lib, 'mbx_diag_set_trace'):
        raise SystemExit('the loaded library has no mbx_diag_set_trace: it is not a diagnostic build.  Build one with the flag in this tool\'s '
                         'docstring and load it:\n    python tools/build_variants.py NAME -DMBX_..._TRACE\n    MBX_LIB=tools/variants/libmbx_NAME.so python tools/..._trace.py')
    set_trace = ops.lib.mbx_diag_set_trace
    set_trace.argtypes, set_trace.restype = [ctypes.c_void_p, ctypes.c_size_t], None
    ops.lib.mbx_diag_last_need.restype = ctypes.c_size_t
    buf = torch.zeros(n_int64, dtype=torch.int64, device='cuda')
    set_trace(buf.data_ptr(), buf.numel() * 8)
    atexit.register(lambda: (set_trace(None, 0), buf))     # (the closure keeps the buffer alive until it is withdrawn)
    return buf


def timed_launch(fn, buf, warm=3):
    """Milliseconds of one fn() after `warm` warm-up calls; the buffer is zeroed in between, so it holds the timed launch only."""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    buf.zero_()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def check_need(ops, buf, n_int64):
    """The last traced launch must have asked for exactly the tool's layout of n_int64 stamps: a tool and a kernel that drifted apart fail
    here instead of mis-reading.  A smaller buffer than that is refused by the library: say so and stop."""
    need = int(ops.lib.mbx_diag_last_need())
    assert need == n_int64 * 8, f'the traced launch writes {need} bytes, this tool reads {n_int64 * 8}: the record layouts differ, or another kernel ran'
    if buf.numel() < n_int64:
        raise SystemExit(f'# no trace: the launch needs {need} bytes (last_need), the armed buffer has {buf.numel() * 8}: the library armed nothing, '
                         f'{int((buf != 0).sum())} int64 written, 0 written records')


def records(buf, n, width):
    """The first n records of `width` int64 as a numpy array, without those that were never written (first stamp 0)."""
    raw = np.asarray(buf.cpu() if hasattr(buf, 'cpu') else buf)[:n * width].reshape(-1, width)
    return raw[raw[:, 0] > 0]


def to_us(stamps):
    """Wall-clock stamps -> microseconds since the earliest entry (column 0)."""
    st = np.asarray(stamps, dtype=np.float64)
    return (st - st[:, 0].min()) / TICKS_PER_US


def steady(us, cut):
    """The records in order of entry, without the first and the last `cut` (a launch's first and last round) if more than 4 cut exist."""
    us = us[np.argsort(us[:, 0], kind='stable')]
    return us[cut:len(us) - cut] if cut and len(us) > 4 * cut else us


def phase_table(us, names, cut, label_width, whole='whole tile', num_width=8):
    """The printed lines: median and 10th / 90th percentile over the steady-state records, per phase (consecutive stamps) and for the whole."""
    st = steady(us, cut)
    cols = list(np.diff(st, axis=1).T[:len(names)]) + [st[:, len(names)] - st[:, 0]]
    return [f'{nm:{label_width}s} {np.median(d):{num_width}.2f} us (10th / 90th percentile {np.percentile(d, 10):.2f} / {np.percentile(d, 90):.2f})'
            for nm, d in zip(list(names) + [whole], cols)]


def same_cu_gaps(us, hw, last_col):
    """Gaps between a record's stamp `last_col` and the entry of the next record with the same hardware id (the next workgroup on the CU)."""
    gaps = []
    for h in np.unique(hw):
        rows = us[hw == h][np.argsort(us[hw == h][:, 0])]
        gaps += list(rows[1:, 0] - rows[:-1, last_col])
    return np.array(gaps)
