"""Sequences longer than 256 frames: what is decided before any launch (no GPU needed)."""
import os
from functools import partial

import pytest
import torch
import torch.nn as nn

from motionbert_amd.engine import MODE_TEMPORAL


@pytest.fixture(scope='module')
def lib():
    from motionbert_amd import build, hip_ops
    if not os.path.exists(hip_ops.LIB_PATH):
        build.build(verbose=False)
    return hip_ops.load_library()


def test_long_sequence_argument_checks(lib):
    """T > 256 is no longer refused; a shape whose launch grid would overflow int is, before any launch; the head-dim check holds."""
    B = 1 << 24      # 2^24 clips x 17 joints x 8 heads = 2.3e9 temporal problems
    rc = lib.mbx_attn_fwd(1, 1, 1, B, 300, 17, 8, 64, 0.125, MODE_TEMPORAL, 0, None)
    assert rc != 0 and b'launch grid' in lib.mbx_last_error()
    rc = lib.mbx_attn_bwd(1, 1, 1, 1, 1, B, 300, 17, 8, 64, 0.125, MODE_TEMPORAL, 0, None)
    assert rc != 0 and b'launch grid' in lib.mbx_last_error()
    rc = lib.mbx_attn_fwd(1, 1, 1, 1, 300, 17, 8, 48, 0.125, MODE_TEMPORAL, 0, None)
    assert rc != 0 and b'head dim' in lib.mbx_last_error()


def test_maxlen_bounds_the_sequence_length():
    from motionbert_amd import DSTformer
    model = DSTformer(dim_feat=64, dim_rep=64, depth=1, num_heads=2, mlp_ratio=2, maxlen=300, norm_layer=partial(nn.LayerNorm, eps=1e-6))
    assert model.temp_embed.shape[1] == 300
    with pytest.raises(ValueError, match='maxlen=300'):
        model(torch.zeros(1, 301, 17, 3))
