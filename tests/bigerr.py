"""Checks for kernels at row counts where BYTE OFFSETS pass 2^31 and 2^32 (tests/test_gpu_big_rows.py; this module's own tests:
tests/test_bigerr.py).

The benchmark's headline runs 256 clips x 243 frames x 17 joints = 1,057,536 token rows.  At that size almost every activation is
larger than 2^31 bytes and the fp32 ones of 1024 and 1536 columns are larger than 2^32, but a kernel that wraps an offset there is
still right on most of its rows: for 2048-byte rows only the last 8,960 of them (0.85 %) lie past 2^31.  Two checks see such a defect:

  quarters_equal      one launch on all rows against one launch per QUARTER (64 clips: the row count every other kernel test uses, less
                      than 2^31 bytes at every row width) on row slices of the same operands: bit-identical over the WHOLE tensor.  A
                      sub-launch has the same row arithmetic with small offsets.  Exhaustive, and it needs no reference.
  slabs_of_interest   where a float64 reference is worth its cost: the first and last rows, 512 rows on either side of every crossing
                      (of every tensor the kernel addresses), the ragged last tiles, and a seeded sample of the rest.

Plain module: no fixtures; runs on whatever device its tensors live on."""
import numpy as np
import torch

MARK31, MARK32 = 1 << 31, 1 << 32
MARKS = (MARK31, MARK32)
CLIP = 243 * 17                  # rows of one clip
QUARTER_CLIPS = 64
M_STEP = QUARTER_CLIPS * CLIP    # 264,384: a quarter
M256 = 256 * CLIP                # 1,057,536
# M256 is a multiple of 256 rows: two more row counts whose last 128- and 256-row tile is ragged and lies past the crossings
M_RAGGED = (M256 - CLIP + 5, M256 + 37)
HALO = 512
SAMPLE = 4096


def mark_name(mark):
    return f'2^{mark.bit_length() - 1}' if mark & (mark - 1) == 0 else str(mark)


def crossings(M, row_bytes, marks=MARKS):
    """{mark: the first row whose byte offset row * row_bytes is >= mark}; a mark the tensor does not reach (no such row below M) is
    left out.  The row in front of it may straddle the mark."""
    out = {}
    for mark in marks:
        row = -(-mark // row_bytes)
        if row < M:
            out[mark] = row
    return out


def side(row, row_bytes, marks=MARKS):
    """which side of each mark the START of `row` lies on, as words for a report or a failure message"""
    return ', '.join(('past ' if row * row_bytes >= mark else 'before ') + mark_name(mark) for mark in marks)


class Slabs:
    """ranges: sorted, disjoint (r0, r1) row ranges; sample: sorted further rows outside them; rows(): all of them, ascending"""

    def __init__(self, M, ranges, sample):
        self.M, self.ranges, self.sample = M, ranges, sample

    def rows(self):
        parts = [np.arange(r0, r1, dtype=np.int64) for r0, r1 in self.ranges] + [np.asarray(self.sample, dtype=np.int64)]
        return np.unique(np.concatenate(parts))

    def index(self, device):
        return torch.from_numpy(self.rows()).to(device)

    def covers(self, row):
        return any(r0 <= row < r1 for r0, r1 in self.ranges) or row in set(int(r) for r in self.sample)


def slabs_of_interest(M, row_bytes, unit=1, tiles=(128, 256), sample=SAMPLE, seed=0, halo=HALO, marks=MARKS):
    """Row ranges for a float64 reference of a kernel over M rows.  row_bytes: the bytes per row of EVERY tensor the kernel addresses by
    row (an int or several).  The first `halo` rows, the last `halo` rows, `halo` rows on either side of every crossing of every one of
    those tensors, the ragged last tile of every tile height in `tiles`, all widened to whole units of `unit` rows (a clip, where the
    kernel works per clip; M is then a multiple of it), and `sample` further rows (whole units, at least one) drawn with `seed`."""
    widths = (row_bytes,) if isinstance(row_bytes, int) else tuple(row_bytes)
    want = [(0, halo), (M - halo, M)]
    for rb in widths:
        for row in crossings(M, rb, marks).values():
            want.append((row - halo, row + halo))
    for t in tiles:
        if M % t:
            want.append((M - M % t, M))
    want = sorted((max(0, r0) // unit * unit, min(M, -(-min(M, r1) // unit) * unit)) for r0, r1 in want)
    ranges = []
    for r0, r1 in want:
        if ranges and r0 <= ranges[-1][1]:
            ranges[-1] = (ranges[-1][0], max(ranges[-1][1], r1))
        else:
            ranges.append((r0, r1))
    covered = np.zeros(-(-M // unit), dtype=bool)
    for r0, r1 in ranges:
        covered[r0 // unit:-(-r1 // unit)] = True
    free = np.nonzero(~covered)[0]
    n = min(len(free), max(1, sample // unit)) if sample else 0
    picked = np.sort(np.random.default_rng(seed).choice(free, size=n, replace=False)) if n else np.zeros(0, dtype=np.int64)
    rows = (picked[:, None] * unit + np.arange(unit)[None, :]).reshape(-1)
    return Slabs(M, ranges, rows[rows < M])


def quarters(M, quarter=M_STEP):
    return [(r0, min(M, r0 + quarter)) for r0 in range(0, M, quarter)]


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def first_difference(a, b, chunk=1 << 16):
    """first row (index along dim 0) at which two tensors of one shape and type differ in a bit, or None"""
    if torch.equal(_bits(a), _bits(b)):
        return None
    for r0 in range(0, a.shape[0], chunk):
        ne = (_bits(a[r0:r0 + chunk]) != _bits(b[r0:r0 + chunk])).reshape(min(chunk, a.shape[0] - r0), -1).any(1)
        if bool(ne.any()):
            return r0 + int(torch.nonzero(ne)[0])
    raise AssertionError('torch.equal and the row-wise comparison disagree')


def quarters_equal(launch, M, outs, quarter=M_STEP, marks=MARKS, name='', sync=None):
    """launch(r0, r1) runs the kernel on rows r0:r1: on row slices of the same operands, writing rows r0:r1 of every tensor of `outs`
    ({name: tensor whose dim 0 is the row}).  Once on all rows, then once per quarter, into outputs pre-filled with NaN (integer
    outputs: with -1).  Asserts that every output of the full launch is finite and that the two agree in every bit, over the whole
    tensor; a mismatch is reported with its first row, that row's byte offset and the side of each mark it lies on.
    Returns {name: row_bytes} of what was compared (for the report)."""
    sync = sync or (lambda: torch.cuda.synchronize() if any(o.is_cuda for o in outs.values()) else None)

    def fill():
        for o in outs.values():
            o.fill_(float('nan') if o.is_floating_point() else -1)
    fill()
    launch(0, M)
    sync()
    full = {k: o.clone() for k, o in outs.items()}
    for k, o in full.items():
        assert o.shape[0] == M, f'{name}{k}: dim 0 is {o.shape[0]}, not the {M} rows'
        if o.is_floating_point():
            for r0 in range(0, M, 1 << 18):
                bad = ~torch.isfinite(o[r0:r0 + (1 << 18)]).reshape(min(1 << 18, M - r0), -1).all(1)
                if bool(bad.any()):
                    row = r0 + int(torch.nonzero(bad)[0])
                    rb = o[0].numel() * o.element_size()
                    raise AssertionError(f'{name}{k}: the launch on all {M} rows left a non-finite value in row {row} (byte offset '
                                         f'{row * rb:,}: {side(row, rb, marks)})')
    fill()
    for r0, r1 in quarters(M, quarter):
        launch(r0, r1)
    sync()
    widths = {}
    for k, o in outs.items():
        rb = widths[k] = o[0].numel() * o.element_size()
        row = first_difference(full[k], o)
        if row is not None:
            q = row // quarter
            raise AssertionError(f'{name}{k}: the launch on all {M} rows and the launch on rows {q * quarter}:{min(M, (q + 1) * quarter)} differ '
                                 f'first in row {row} (byte offset {row * rb:,} of {rb}-byte rows: {side(row, rb, marks)}; crossings at rows '
                                 f'{ {mark_name(m): r for m, r in crossings(M, rb, marks).items()} })')
    del full
    return widths


def attn_mask_elements(B, T, J, H, temporal):
    """elements of the reference's attention tensor, over which the dropout mask's index runs (dropmask.py)"""
    return B * H * J * T * T if temporal else B * T * H * J * J


def slab_gate(name, got_rows, rows, x64, bound64, row_bytes, marks=MARKS, check=True):
    """The elementwise bound (localerr.bound_check: |got - x| <= bound for EVERY element, no margin) on the rows `rows` of an output:
    got_rows = output[rows], x64 / bound64 the float64 reference and bound of those rows.  Returns dict(ratio, row, col, violations,
    side, rows_judged) with `row` the worst element's row in the whole tensor."""
    from tests import localerr as LE
    b = LE.bound_check(got_rows, x64, bound64)
    row = int(rows[b['row']])
    res = dict(ratio=b['ratio'], row=row, col=b['col'], violations=b['violations'], side=side(row, row_bytes, marks), rows_judged=int(len(rows)))
    if check:
        assert b['violations'] == 0, (f'{name}: {b["violations"]} elements of the {len(rows)} judged rows outside the elementwise bound, the worst at '
                                      f'{b["ratio"]:.3g} x in row {row}, col {b["col"]} (byte offset {row * row_bytes:,}: {res["side"]})')
    return res
