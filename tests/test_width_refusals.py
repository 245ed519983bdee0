"""CPU: the LayerNorm kernels hold a row as at most eight sixteen-byte chunks per lane of one wave (C % 8 == 0, C <= 4096) and the GEGLU
kernels work on whole 16-column halves of the paired layout (F % 16 == 0).  Wider or ragged rows used to run and give a wrong answer
(k_ln_* read the first 4096 channels and divided by C).  Every engine refuses them when it is created and every debug entry per call:
the return code and the dh_last_error text, with nothing launched (the pointers are NULL or host memory, and no GPU is needed)."""
import ctypes

import pytest

from diffusionhandles_amd import _lib

DH_ERR_ARG = -1
LIMIT = b"4096"


def unet_config(channels, heads):
    c = _lib.UNetConfig()
    c.in_channels, c.out_channels, c.n_levels = 4, 4, 4
    for i in range(4):
        c.block_out_channels[i], c.heads[i] = channels[i], heads[i]
    c.layers_per_block, c.cross_attention_dim, c.norm_groups, c.sample_size = 1, 64, 32, 8
    c.text_len, c.max_batch, c.max_diff_batch, c.dtype = 77, 1, 1, 0
    return c


@pytest.mark.parametrize("level", [1, 3])
def test_unet_create_refuses_a_level_wider_than_a_layernorm_row(level):
    L = _lib.lib()
    ch = [64, 128, 256, 512]
    ch[level] = 8192                             # (level 0 is held to 2048 by the few-channel convolutions)
    c, h = unet_config(ch, [v // 64 for v in ch]), ctypes.c_void_p()
    rc = L.dh_unet_create(ctypes.byref(c), ctypes.byref(h))
    err = L.dh_last_error()
    assert rc == DH_ERR_ARG and not h.value, (rc, err)
    assert err == b"dh_unet_create: block_out_channels must be <= " + LIMIT + b" (LayerNorm row width)", err


def test_text_encoder_create_refuses_hidden_wider_than_a_layernorm_row():
    L = _lib.lib()
    c, h = _lib.TextConfig(), ctypes.c_void_p()
    c.hidden, c.heads, c.layers, c.intermediate, c.max_tokens, c.max_batch, c.eps, c.dtype = 8192, 128, 1, 64, 77, 1, 1e-5, 0
    rc = L.dh_text_encoder_create(ctypes.byref(c), ctypes.byref(h))
    err = L.dh_last_error()
    assert rc == DH_ERR_ARG and not h.value, (rc, err)
    assert err == b"dh_text_encoder_create: hidden must be <= " + LIMIT + b" (LayerNorm row width)", err
    # the limit itself is not refused for its width (without a GPU the creation then fails at its first allocation)
    c.hidden, c.heads = 4096, 64
    rc = L.dh_text_encoder_create(ctypes.byref(c), ctypes.byref(h))
    if rc == 0:
        L.dh_text_encoder_destroy(h)
    else:
        assert b"LayerNorm" not in L.dh_last_error(), L.dh_last_error()


@pytest.mark.parametrize("C", [4, 12, 1028, 4104, 8192])
def test_layernorm_debug_entries_refuse_unsupported_widths(C):
    L = _lib.lib()
    want = b": C must be a multiple of 8 and <= " + LIMIT + b" (LayerNorm row width)"
    rc = L.dh_dbg_layernorm(0, None, None, None, None, None, None, None, None, 4, C, 1e-5, None)
    assert rc == DH_ERR_ARG and L.dh_last_error() == b"dh_dbg_layernorm" + want, (rc, L.dh_last_error())
    rc = L.dh_dbg_layernorm_ld(0, None, C, None, None, None, None, None, None, None, 4, C, 1e-5, None)
    assert rc == DH_ERR_ARG and L.dh_last_error() == b"dh_dbg_layernorm_ld" + want, (rc, L.dh_last_error())


def test_layernorm_ld_refuses_a_backward_without_statistics_and_a_short_pitch():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = L.dh_dbg_layernorm_ld(0, p, 8, p, p, p, None, p, None, p, 1, 8, 1e-5, None)
    assert rc == DH_ERR_ARG and b"stats must not be NULL" in L.dh_last_error(), (rc, L.dh_last_error())
    for ldx in (0, 4, 12):
        rc = L.dh_dbg_layernorm_ld(0, p, ldx, p, p, p, None, None, None, None, 1, 8, 1e-5, None)
        assert rc == DH_ERR_ARG and b"ldx >= C" in L.dh_last_error(), (ldx, rc, L.dh_last_error())


@pytest.mark.parametrize("Fd", [0, 8, 24, 1288])
def test_geglu_debug_entry_refuses_ragged_widths(Fd):
    L = _lib.lib()
    rc = L.dh_dbg_geglu(0, None, None, None, None, 4, Fd, None)
    assert rc == DH_ERR_ARG, rc
    assert L.dh_last_error() == b"dh_dbg_geglu: F must be a positive multiple of 16 (paired column layout)", L.dh_last_error()


def test_gemm_layernorm_bwd_debug_entry_refuses_wide_rows():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = L.dh_dbg_gemm_layernorm_bwd(0, p, 64, p, 4, 4160, 64, p, 4160, p, p, None, p, p, None, 0, None, None)
    assert rc == DH_ERR_ARG and b"N must be <= " + LIMIT in L.dh_last_error(), (rc, L.dh_last_error())
