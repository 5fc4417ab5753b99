"""tests/bigerr.py catches what it is for: numpy stand-ins for a row-wise kernel whose byte offset wraps, over a small logical tensor
with the marks scaled down (2^23 and 2^24 instead of 2^31 and 2^32; 12-byte rows, so that -- as with the 3072- and 6144-byte rows of the
real tensors -- a row straddles each mark).  Every wrapped stand-in fails quarters_equal AND the float64 gate on slabs_of_interest,
while the whole-tensor relative L2 of tests/test_gpu_kernels.py stays under that file's tolerance: the gap the big-row tests close."""
import numpy as np
import pytest
import torch

from tests import bigerr as BE
from tests import localerr as LE

TOL_KERNELS_BF16 = 4e-3      # TOL_T[bfloat16] of tests/test_gpu_kernels.py, the looser of its two


# ------------------------------------------------------------------------------------------------ the table of the 256-clip tensors
def test_crossings_reproduce_the_table():
    assert BE.M256 == 1057536 and BE.CLIP == 4131 and BE.M_STEP == 264384 and BE.M256 == 4 * BE.M_STEP
    table = {2048: (2165833728, 1048576, None), 3072: (3248750592, 699051, None), 4096: (4331667456, 524288, 1048576), 6144: (6497501184, 349526, 699051)}
    for rb, (total, r31, r32) in table.items():
        assert BE.M256 * rb == total
        c = BE.crossings(BE.M256, rb)
        assert c.get(BE.MARK31) == r31 and c.get(BE.MARK32) == r32, (rb, c)
        for mark, row in c.items():
            assert (row - 1) * rb < mark <= row * rb
    assert BE.M256 - 1048576 == 8960                                # the rows of a 2048-byte-row tensor past 2^31: 0.85 %
    assert BE.crossings(BE.M_STEP, 6144) == {}                      # a quarter reaches no mark at any width of the table
    assert BE.M_STEP * 6144 < BE.MARK31
    assert BE.crossings(1048576, 2048) == {}                        # the mark is reached by the first row PAST such a tensor
    assert BE.crossings(1048577, 2048) == {BE.MARK31: 1048576}
    assert BE.side(699050, 3072) == 'before 2^31, before 2^32' and BE.side(699051, 3072) == 'past 2^31, before 2^32'
    assert BE.side(1048576, 4096) == 'past 2^31, past 2^32'


def test_ragged_row_counts_put_a_ragged_tile_past_the_crossings():
    assert BE.M256 % 256 == 0
    for M in BE.M_RAGGED:
        assert M % 128 and M % 256
        for rb in (2048, 3072, 4096, 6144):
            assert (M - M % 256) * rb >= max(BE.crossings(M, rb))      # the ragged tile starts past the last mark the tensor reaches


def test_attention_dropout_mask_index_stays_below_2_31():
    """the index of the probability-dropout mask runs over the reference's attention tensor: at 256 clips 2,055,849,984 elements in the
    temporal case -- 96 % of 2^31, not past it -- and 143,824,896 in the spatial one"""
    assert BE.attn_mask_elements(256, 243, 17, 8, True) == 2055849984 < BE.MARK31
    assert BE.attn_mask_elements(256, 243, 17, 8, False) == 143824896
    assert BE.attn_mask_elements(268, 243, 17, 8, True) >= BE.MARK31 > BE.attn_mask_elements(267, 243, 17, 8, True)


# ------------------------------------------------------------------------------------------------ slabs_of_interest
def test_slabs_cover_edges_crossings_tails_and_a_sample():
    for M in (BE.M256,) + BE.M_RAGGED:
        s = BE.slabs_of_interest(M, (3072, 2048, 6144))
        rows = s.rows()
        assert np.all(np.diff(rows) > 0) and rows[0] == 0 and rows[-1] == M - 1
        have = set(rows.tolist())
        want = list(range(512)) + list(range(M - 512, M)) + list(range(M - M % 128, M)) + list(range(M - M % 256, M))
        for rb in (3072, 2048, 6144):
            for row in BE.crossings(M, rb).values():
                want += list(range(row - 512, min(M, row + 512)))
        assert have.issuperset(want)
        assert len(s.sample) == BE.SAMPLE and not any(r0 <= r < r1 for r in s.sample[::97] for r0, r1 in s.ranges)
        assert len(rows) < 16384                                      # a float64 reference of these rows stays small
        assert np.array_equal(rows, BE.slabs_of_interest(M, (3072, 2048, 6144)).rows())      # seeded
        assert not np.array_equal(s.sample, BE.slabs_of_interest(M, (3072, 2048, 6144), seed=1).sample)


def test_slabs_widen_to_whole_clips():
    s = BE.slabs_of_interest(BE.M256, 3072, unit=BE.CLIP)
    assert all(r0 % BE.CLIP == 0 and r1 % BE.CLIP == 0 for r0, r1 in s.ranges)
    clips = sorted(set((s.rows() // BE.CLIP).tolist()))
    c = 699051 // BE.CLIP                                             # the clip that holds the crossing of qkv (bf16 [M, 1536])
    assert {0, 255, c}.issubset(clips) and (699051 - 512) // BE.CLIP in clips and (699051 + 511) // BE.CLIP in clips
    assert len(s.sample) == BE.CLIP and len(clips) <= 6
    assert len(s.rows()) == len(clips) * BE.CLIP


# ------------------------------------------------------------------------------------------------ the stand-ins
RB, NCOL = 12, 3                              # three fp32 columns: 12-byte rows
MARKS = (1 << 23, 1 << 24)                    # the scaled marks: rows 699,051 and 1,398,102 are the first past them
QUARTER = 264384                              # a quarter stays below the first mark: 264,384 x 12 = 3,172,608 < 2^23
GUARD = MARKS[0] // 4                         # floats in front of the tensor: what a negative offset reads


def _wrap_signed(off, mark):
    return (off + mark) % (2 * mark) - mark


def standin(variant):
    """y[r, c] = 2 x[r, c] + 1 in fp32, x read at byte offset off = r RB + 4 c from the base of the slice it is launched on:
      exact     off
      signed    the whole offset as a signed value of the first mark's width (a 32-bit int): past the mark it is negative
      unsigned  the whole offset modulo the second mark (a 32-bit unsigned)
      lane      base + lane offset: the column part sits in the exact 64-bit base, the row part r RB alone is the signed narrow value"""
    def kernel(arena, x_first, y, r0, r1):
        r = np.arange(r1 - r0, dtype=np.int64)[:, None]
        c = np.arange(NCOL, dtype=np.int64)[None, :]
        off = r * RB + 4 * c
        if variant == 'signed':
            off = _wrap_signed(off, MARKS[0])
        elif variant == 'unsigned':
            off = off % MARKS[1]
        elif variant == 'lane':
            off = _wrap_signed(r * RB, MARKS[0]) + 4 * c
        y[r0:r1] = np.float32(2.0) * arena[x_first + r0 * NCOL + off // 4] + np.float32(1.0)
    return kernel


@pytest.fixture(scope='module')
def arena():
    """GUARD floats of other data, then x [M_max, NCOL] with a scale and an offset per row"""
    m_max = 1398102 + 8
    g = np.random.default_rng(0)
    x = g.standard_normal((m_max, NCOL), dtype=np.float32) * (0.5 + np.abs(g.standard_normal((m_max, 1), dtype=np.float32))) \
        + 0.3 * g.standard_normal((m_max, 1), dtype=np.float32)
    return np.concatenate([g.standard_normal(GUARD, dtype=np.float32), x.reshape(-1)])


def _run(arena, variant, M):
    """(quarters_equal's verdict, the slab gate's verdict, the whole-tensor relative L2) of a stand-in on M rows"""
    kernel = standin(variant)
    y = torch.empty(M, NCOL)
    try:
        BE.quarters_equal(lambda r0, r1: kernel(arena, GUARD, y.numpy(), r0, r1), M, {'y': y}, quarter=QUARTER, marks=MARKS, name=variant + '.')
        q_msg = None
    except AssertionError as e:
        q_msg = str(e)
    kernel(arena, GUARD, y.numpy(), 0, M)
    x64 = torch.from_numpy(arena[GUARD:GUARD + M * NCOL].reshape(M, NCOL)).double()
    ref = 2.0 * x64 + 1.0
    # y = 2 x + 1: an exact doubling, one fp32 addition, rounded once to fp32
    rows = BE.slabs_of_interest(M, RB, marks=MARKS).rows()
    idx = torch.from_numpy(rows)
    s = BE.slab_gate(variant, y[idx], rows, ref[idx], LE.elementwise_bound(ref[idx], 2.0 * x64[idx].abs(), 0, LE.R_F32, ops=1, mag64=2.0 * x64[idx].abs() + 1.0),
                     RB, marks=MARKS, check=False)
    return q_msg, s, LE.rel(y, ref)


M31 = 699051 + 2       # two rows start past the first mark (and the row in front of them straddles it)
M32 = 1398102 + 2      # ... past the second


@pytest.mark.parametrize('M', [QUARTER, M31, M32])
def test_exact_standin_passes(arena, M):
    q, s, rel = _run(arena, 'exact', M)
    assert q is None and s['violations'] == 0 and s['ratio'] <= 1.0 and rel < 1e-7


@pytest.mark.parametrize('variant', ['signed', 'unsigned', 'lane'])
def test_wrapped_standins_are_right_at_the_row_count_the_suite_had(arena, variant):
    """a quarter (the largest row count of the kernel tests before these) reaches no mark: every check passes there"""
    q, s, rel = _run(arena, variant, QUARTER)
    assert q is None and s['violations'] == 0 and rel < 1e-7


@pytest.mark.parametrize('variant,M,first_row', [('signed', M31, 699050), ('lane', M31, 699051), ('unsigned', M32, 1398101)])
def test_wrapped_standins_fail_both_checks_and_pass_the_norm(arena, variant, M, first_row):
    q, s, rel = _run(arena, variant, M)
    # quarters_equal: the first differing row, its offset and its side.  `signed` and `unsigned` wrap the column part too: they already
    # break the row that straddles the mark (its last columns); `lane` breaks whole rows from the crossing on
    assert q is not None and f'first in row {first_row} ' in q and f'byte offset {first_row * RB:,}' in q, q
    want_side = BE.side(first_row, RB, MARKS)
    assert want_side in q, q
    # the float64 gate on the slabs: violations, the worst one within the rows that went wrong
    assert s['violations'] >= 2 * NCOL and s['ratio'] > 1e3 and first_row <= s['row'] < M
    # ... and the whole-tensor norm of tests/test_gpu_kernels.py does not notice
    assert 1e-4 < rel < TOL_KERNELS_BF16, rel


def test_quarters_equal_reports_an_output_the_launch_did_not_write():
    y = torch.empty(1000, 2)

    def launch(r0, r1):
        y[r0:r1] = 1.0
        if r1 - r0 == 1000:
            y[700:] = float('nan')      # the launch on all rows leaves its tail unwritten
    with pytest.raises(AssertionError, match='non-finite value in row 700'):
        BE.quarters_equal(launch, 1000, {'y': y}, quarter=250, marks=(4096, 8192))

    def launch2(r0, r1):
        y[r0:r1] = 1.0
        if r1 - r0 != 1000 and r0 == 750:
            y[r1 - 1, 1] = float('nan')      # a quarter's launch does
    with pytest.raises(AssertionError, match='first in row 999 .byte offset 7,992 of 8-byte rows: past 2\\^12, before 2\\^13'):
        BE.quarters_equal(launch2, 1000, {'y': y}, quarter=250, marks=(4096, 8192))


def test_quarters_split_the_ragged_row_counts():
    assert BE.quarters(BE.M256) == [(i * BE.M_STEP, (i + 1) * BE.M_STEP) for i in range(4)]
    assert BE.quarters(BE.M256 + 37)[-1] == (BE.M256, BE.M256 + 37) and len(BE.quarters(BE.M256 + 37)) == 5
    assert BE.quarters(BE.M_RAGGED[0])[-1] == (3 * BE.M_STEP, BE.M_RAGGED[0])
    assert all((r1 - r0) * 6144 < BE.MARK31 for M in (BE.M256,) + BE.M_RAGGED for r0, r1 in BE.quarters(M))


@pytest.mark.parametrize('temporal', [False, True])
def test_attention_mask_of_chosen_clips_is_the_full_batch_mask(temporal):
    """localerr.attn_mask with clip numbers: the masks of clips 1 and 4 of a batch of five, built from their own indices, are those
    clips of the mask built over the whole batch"""
    B, T, J, H, drop = 5, 7, 3, 2, (0.3, 0x1234567890ABCDEF)
    full = LE.attn_mask(B, T, J, H, temporal, drop, 'cpu')
    part = LE.attn_mask(2, T, J, H, temporal, drop + ([1, 4],), 'cpu')
    assert torch.equal(part, full[[1, 4]]) and 0.2 < float((full == 0).double().mean()) < 0.4
