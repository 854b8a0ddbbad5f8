"""Host side of ``enable_request_adapter_scales`` (no GPU): the switch on the pipelines' base, the folded / row decision per argument,
the row layout, and the augmented weights of the unfolded route against the folded ones in float64."""
import pytest
import torch

from imagdressing_amd.dressing_sd.pipelines import _base as B


def _pipeline_classes():
    from imagdressing_amd.dressing_sd.pipelines import (IMAGDressing_v1_pipeline, IMAGDressing_v1_pipeline_controlnet,
                                                        IMAGDressing_v1_pipeline_controlnet_inpainting, IMAGDressing_v1_pipeline_ipa_controlnet)
    return [m.IMAGDressing_v1 for m in (IMAGDressing_v1_pipeline, IMAGDressing_v1_pipeline_controlnet,
                                        IMAGDressing_v1_pipeline_controlnet_inpainting, IMAGDressing_v1_pipeline_ipa_controlnet)]


def test_switch_exists_on_all_four_pipelines_and_is_off_by_default():
    for cls in _pipeline_classes():
        assert issubclass(cls, B.PipelineBase)
        pipe = cls.__new__(cls)
        assert not getattr(pipe, "_request_adapter_scales", False)
        assert pipe.enable_request_adapter_scales() is pipe and pipe._request_adapter_scales is True
        assert pipe.disable_request_adapter_scales() is pipe and pipe._request_adapter_scales is False
        assert pipe.enable_request_adapter_scales(False) is pipe and pipe._request_adapter_scales is False
    doc = B.PipelineBase.enable_request_adapter_scales.__doc__
    assert "no-op" in doc and "Off by default" in doc and "no-face" in doc


def test_only_the_ipa_pipeline_reads_the_switch():
    """the other three have none of the three arguments: the switch is a documented no-op there"""
    import inspect
    for cls in _pipeline_classes():
        params = inspect.signature(cls.__call__).parameters
        has = [n in params for n in ("ipa_scale", "s_lora_scale", "c_lora_scale")]
        assert all(has) or not any(has)
        src = inspect.getsource(cls.__call__)
        assert ("_request_adapter_scales" in src) == all(has)


def test_equal_values_stay_folded_and_differing_ones_ride_in_rows():
    f = B.PipelineBase._adapter_scales
    assert f("ipa_scale", 0.9, 3, 1.0) == (0.9, None)
    assert f("ipa_scale", [0.9], 3, 1.0) == (0.9, None)
    assert f("s_lora_scale", [0.2, 0.2, 0.2], 3, 0.0) == (0.2, None)
    assert f("s_lora_scale", (0.2, 0.8, 0.0), 3, 0.0) == (0.0, [0.2, 0.8, 0.0])
    assert f("ipa_scale", [0.9, 0.3], 2, 1.0) == (1.0, [0.9, 0.3])
    for name in ("ipa_scale", "s_lora_scale", "c_lora_scale"):
        with pytest.raises(ValueError, match=f"{name} has 3 entries for 2 requests"):
            f(name, [0.1, 0.2, 0.3], 2, 0.0)


def test_switch_off_still_refuses_differing_sequences():
    for name in ("ipa_scale", "s_lora_scale", "c_lora_scale"):
        assert name in B.PER_CALL_KEYS
        with pytest.raises(ValueError, match=name):
            B.request_count(dict(prompt=["a", "b"]), {name: [0.1, 0.2]})
        assert B.request_count(dict(prompt=["a", "b"]), {name: [0.2, 0.2]}) == 2


def test_rows_are_request_major_for_n_images():
    lay = B.RequestLayout(3, 2)
    rows = lay.per_row(B.per_request_floats("s_lora_scale", [0.2, 0.8, 0.0], 3))
    assert rows.dtype == torch.float32 and rows.tolist() == pytest.approx([0.2, 0.2, 0.8, 0.8, 0.0, 0.0])
    full = rows.repeat(2)          # what _denoise puts into the cross-attention kwargs: cond rows, then uncond rows, the same values
    assert full.shape == (12,) and torch.equal(full[:6], full[6:])
    for b in range(12):
        assert full[b].item() == pytest.approx([0.2, 0.8, 0.0][lay.request_of_row(b)])


class _Attn:
    """the attribute surface of an attention layer the processors read"""

    def __init__(self, C, Kd, seed):
        g = torch.Generator().manual_seed(seed)
        self.heads = 2
        self.to_q, self.to_k, self.to_v = (torch.nn.Linear(k, C, bias=False) for k in (C, Kd, Kd))
        self.to_out = torch.nn.ModuleList([torch.nn.Linear(C, C)])
        with torch.no_grad():
            for m in (self.to_q, self.to_k, self.to_v, self.to_out[0]):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * m.weight.shape[1] ** -0.5)


@pytest.mark.parametrize("rank,alpha", [(16, None), (4, 8.0)], ids=["rank16", "rank4_alpha8"])
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
def test_augmented_weights_state_the_folded_layer(cross, rank, alpha):
    """[x | s (x D^T)] [W | U]^T == x (W + s alpha/rank U D)^T for every projection launch, the block structure of the stacked ones
    included (q's tail columns do not reach k or v); the tail is padded to a multiple of 16 with zeros"""
    from imagdressing_amd.adapter import attention_processor as AP
    C, Kd = 80, (64 if cross else 80)
    attn = _Attn(C, Kd, 5)
    proc = AP.LoRAIPAttnProcessor2_0(C, Kd, rank=rank, network_alpha=alpha) if cross else AP.LoraRefSAttnProcessor2_0("n", C, rank=rank, network_alpha=alpha)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for nm in ("q", "k", "v", "out"):
            lo = getattr(proc, f"to_{nm}_lora")
            lo.down.weight.copy_(torch.randn(lo.down.weight.shape, generator=g) * 0.1)
            lo.up.weight.copy_(torch.randn(lo.up.weight.shape, generator=g) * 0.1)
    u = proc._unfolded(attn, torch.device("cpu"), torch.float32)
    assert proc._unfolded(attn, torch.device("cpu"), torch.float32) is u          # cached: no scale in the key
    s = 0.7
    proc.lora_scale = s
    w = proc._fold(attn, torch.device("cpu"), torch.float32)
    launches = [("q", "d_q", C, 1), ("kv", "d_kv", Kd, 2), ("o", "d_o", C, 1)] + ([] if cross else [("qkv", "d_qkv", C, 3)])
    for wk, dk, cin, G in launches:
        W, D = u[wk].double(), u[dk].double()
        T = D.shape[0]
        assert T % 16 == 0 and T >= G * rank and W.shape == (w[wk].shape[0], cin + T) and D.shape[1] == cin
        assert not D[G * rank:].any() and not W[:, cin + G * rank:].any()
        x = torch.randn(7, cin, generator=g).double()
        aug = torch.cat([x, s * (x @ D.T)], 1)
        assert torch.allclose(aug @ W.T, x @ w[wk].double().T, atol=1e-6, rtol=1e-6)
    if cross:
        assert u["qkv"] is None and w["qkv"] is None
    else:          # the q rows see U_q in their own r columns and zeros in the others
        Wq = u["qkv"][:C, C:]
        assert Wq[:, :rank].any() and not Wq[:, rank:].any()
        Wv = u["qkv"][2 * C:, C:]
        assert Wv[:, 2 * rank:3 * rank].any() and not Wv[:, :2 * rank].any()
    # a new scale re-folds the folded weights and leaves the augmented ones alone
    proc.lora_scale = 0.1
    assert proc._fold(attn, torch.device("cpu"), torch.float32) is not w
    assert proc._unfolded(attn, torch.device("cpu"), torch.float32) is u


def test_row_tensors_are_checked():
    from imagdressing_amd.adapter.attention_processor import _check_rows
    dev = torch.device("cpu")
    ok = torch.ones(4)
    assert _check_rows(ok, 4, "lora_rows", dev) is ok
    for bad in (torch.ones(3), torch.ones(4, dtype=torch.float64), torch.ones(2, 2), torch.ones(8)[::2], [1.0] * 4):
        with pytest.raises(ValueError, match="lora_rows"):
            _check_rows(bad, 4, "lora_rows", dev)
