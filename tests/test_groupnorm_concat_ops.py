"""The concatenations the GroupNorm statistics tests cover (tests/test_groupnorm_stats_gpu.py SD2_CONCATS) are the ones the
SD2-depth engine builds: read from the engine's op list through dh_dbg_unet_concat_ops, which builds the op list on the host
only (no GPU)."""
import ctypes

from diffusionhandles_amd import _lib
from oracle import unet_torch as U
from test_groupnorm_stats_gpu import SD2_CONCATS


def concat_ops(cfg):
    c = _lib.UNetConfig()
    c.in_channels, c.out_channels, c.n_levels = cfg["in_channels"], cfg["out_channels"], 4
    for i in range(4):
        c.block_out_channels[i] = cfg["block_out_channels"][i]
        c.heads[i] = cfg["heads"][i]
    c.layers_per_block, c.cross_attention_dim, c.norm_groups = cfg["layers_per_block"], cfg["cross_attention_dim"], cfg["norm_groups"]
    c.sample_size, c.text_len, c.max_batch, c.max_diff_batch, c.dtype = cfg["sample_size"], 77, 1, 1, 0
    out = (ctypes.c_int * (5 * 64))()
    n = ctypes.c_int(0)
    _lib.check(_lib.lib().dh_dbg_unet_concat_ops(ctypes.byref(c), out, 64, ctypes.byref(n)), "dh_dbg_unet_concat_ops")
    return [tuple(out[5 * i:5 * i + 5]) for i in range(n.value)]


def test_sd2_concats_match_the_engine_op_list():
    ops = concat_ops(U.SD2_DEPTH)
    assert len(ops) == 4 * (U.SD2_DEPTH["layers_per_block"] + 1), ops
    assert all(o[4] == 1 for o in ops), "every up-path concatenation fuses the GroupNorm statistics"
    assert sorted({o[:4] for o in ops}) == sorted(SD2_CONCATS)
    # groups across the a | b boundary are in the list
    assert any(ca % ((ca + cb) // g) for ca, cb, _, g in SD2_CONCATS)
