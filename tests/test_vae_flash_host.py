"""Host side of the VAE's flash attention route (no GPU): `vae.mid_attention_route` and the switch of `AutoencoderKL`."""
import types

import pytest

from imagdressing_amd import vae as V


@pytest.mark.parametrize("tokens,channels,flash,want", [
    (1, 512, False, "gemm"), (4096, 512, False, "gemm"), (5120, 512, False, "gemm"), (16384, 512, False, "gemm"),       # today's sizes: today's launches
    (16385, 512, False, "flash"), (16448, 512, False, "flash"), (20480, 512, False, "flash"),                           # sizes that raise today
    (1, 512, True, "flash"), (63, 512, True, "flash"), (4096, 512, True, "flash"), (16384, 512, True, "flash"), (20480, 512, True, "flash"),
])
def test_route_table_at_512_channels(tokens, channels, flash, want):
    assert V.mid_attention_route(tokens, channels, flash) == want


@pytest.mark.parametrize("channels", [128, 256, 320, 511, 513, 1024])
@pytest.mark.parametrize("tokens", [64, 16384, 16385, 20480])
@pytest.mark.parametrize("flash", [False, True])
def test_other_widths_keep_the_three_launches(tokens, channels, flash):
    """(and with them the 16384-token limit: there is no flash kernel for their head dim)"""
    assert V.mid_attention_route(tokens, channels, flash) == "gemm"


def test_the_limit_is_softmax_rows_limit():
    assert V.SOFTMAX_ROWS_MAX_TOKENS == 256 * 64 and V.FLASH_CHANNELS == 512


def test_switch_defaults_to_off_and_round_trips():
    assert V.AutoencoderKL.use_flash_attention is False and V._MidAttention.flash is False
    vae = V.AutoencoderKL.__new__(V.AutoencoderKL)          # (the constructor needs a GPU; the switch does not)
    vae.e_mid = types.SimpleNamespace(attn=V._MidAttention.__new__(V._MidAttention))
    vae.d_mid = types.SimpleNamespace(attn=V._MidAttention.__new__(V._MidAttention))
    mids = (vae.e_mid.attn, vae.d_mid.attn)
    assert not vae.use_flash_attention and not any(m.flash for m in mids)
    vae.enable_flash_attention()
    assert vae.use_flash_attention is True and all(m.flash is True for m in mids)
    vae.disable_flash_attention()
    assert vae.use_flash_attention is False and not any(m.flash for m in mids)
    vae.enable_flash_attention(True); vae.enable_flash_attention(False)
    assert vae.use_flash_attention is False and not any(m.flash for m in mids)
    assert V._MidAttention.flash is False, "the switch is per VAE, not per process"
