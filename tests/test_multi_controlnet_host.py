"""Several ControlNets on the host, without a GPU: the three arguments per net (and per request under the switch), the table of a
hand-written case against literals, which nets every call of the loop runs and which slice of the table the mix launch is handed, every
refusal by name, the list -> ``MultiControlNetModel`` wrapping, the delegation of a wrapper of one net, and the compat import paths."""
import importlib
import os
import sys

import pytest
import torch

from imagdressing_amd import ops
from imagdressing_amd.dressing_sd.pipelines._base import (PipelineBase, RequestLayout, control_scale_table, multi_control_images,
                                                          multi_control_plan, multi_control_scale_table, multi_control_values)
from imagdressing_amd.unet import SD15_CONFIG, ControlNetModel, DeepCache, MultiControlNetModel
from tests import multi_controlnet_cases as M
from tests.test_control_rows_host import _RecordingControlNet, no_launches  # noqa: F401  (the fixture)
from tests.test_deepcache_host import _RecordingUNet, _pipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (16, 32)


class _Net(ControlNetModel):
    """stand-in for an engine ControlNet inside a MultiControlNetModel: records every forward, returns residuals filled with ``tag``"""

    def __init__(self, tag, dtype=torch.float16, widths=WIDTHS, layers=1):
        self.tag, self.dtype, self.device = float(tag), dtype, torch.device("cpu")
        self.cfg = dict(SD15_CONFIG, block_out_channels=widths, layers_per_block=layers)
        self.config = None
        self.calls = []

    def precompute_time_embeddings(self, timesteps, device):          # (the loop's per-schedule table: nothing to embed here)
        self.tables = getattr(self, "tables", 0) + 1
        return torch.zeros(len(timesteps), 1)

    def clear_time_embeddings(self):
        self.cleared = getattr(self, "cleared", 0) + 1

    def forward_nhwc(self, x, t, ehs, cond, conditioning_scale=1.0, deepcache=None, scale_rows=None):
        self.calls.append(dict(scale=conditioning_scale, rows=scale_rows, cond=cond, cache=deepcache, batch=x.shape[0]))
        shallow = deepcache is not None and not deepcache.full
        down, mid = MultiControlNetModel.residual_shapes(self, x.shape[0], x.shape[1], x.shape[2], deepcache.depth if shallow else None)
        mk = lambda s: torch.full(s, self.tag, dtype=self.dtype)          # noqa: E731
        return [mk(s) for s in down], None if mid is None else mk(mid)


@pytest.fixture
def mixes(monkeypatch):
    """``ops.residual_mix_rows`` as a recorder: (sources, scales, out) of every launch the loop would make"""
    seen = []

    def record(sources, scales, out=None):
        seen.append(dict(sources=[list(s) for s in sources], scales=scales.clone(), scales_id=id(scales), out=out))
        return list(out)
    monkeypatch.setattr(ops, "residual_mix_rows", record)
    return seen


# ---- the arguments ----
def test_scalars_hold_for_all_nets_and_flat_lists_are_per_net():
    assert multi_control_values(0.5, 0.0, 1.0, 2, 3) == [[(0.5, 0.0, 1.0)] * 3] * 2
    assert multi_control_values([0.5, 0.25], 0.1, [1.0, 0.5], 2, 1) == [[(0.5, 0.1, 1.0)], [(0.25, 0.1, 0.5)]]
    assert multi_control_values((0.5, 0.25, 1.0), 0.0, 1.0, 3, 2) == [[(0.5, 0.0, 1.0)] * 2, [(0.25, 0.0, 1.0)] * 2, [(1.0, 0.0, 1.0)] * 2]
    assert multi_control_values([0.0, -1.5], 0.0, 1.0, 2, 1) == [[(0.0, 0.0, 1.0)], [(-1.5, 0.0, 1.0)]]          # 0 and negative are scales


@pytest.mark.parametrize("name", ["controlnet_conditioning_scale", "control_guidance_start", "control_guidance_end"])
def test_a_wrong_length_names_the_argument_and_both_counts(name):
    base = dict(controlnet_conditioning_scale=1.0, control_guidance_start=0.0, control_guidance_end=1.0)
    order = list(base)
    for bad, K in (([0.5, 0.5, 0.5], 2), ([0.5], 2), ([0.5, 0.5], 3), ([], 2)):
        args = dict(base, **{name: bad})
        with pytest.raises(ValueError, match=rf"{name} has {len(bad)} entries for {K} ControlNets"):
            multi_control_values(*(args[k] for k in order), K, 2)
    # a list per request inside a net's entry: only under the switch, and then 1 or R long
    args = dict(base, **{name: [0.5, [0.25, 0.75]]})
    with pytest.raises(ValueError, match=rf"{name}\[1\] is a list: a value per request needs enable_request_control_scales"):
        multi_control_values(*(args[k] for k in order), 2, 2)
    multi_control_values(*(args[k] for k in order), 2, 2, per_request=True)
    with pytest.raises(ValueError, match=rf"{name}\[1\] has 2 entries for 3 requests"):
        multi_control_values(*(args[k] for k in order), 2, 3, per_request=True)


def test_the_limits_hold_per_value():
    for a, b in ((0.5, 0.5), (0.6, 0.4), (-0.1, 1.0), (0.0, 1.5), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="of net 1, request 0: need 0 <= start < end <= 1"):
            multi_control_values(1.0, [0.0, a], [1.0, b], 2, 1)
    with pytest.raises(ValueError, match="of net 0, request 1: need 0 <= start < end <= 1"):
        multi_control_values(1.0, [[0.0, 0.9], 0.0], [[1.0, 0.8], 1.0], 2, 2, per_request=True)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="controlnet_conditioning_scale of net 1, request 0 must be finite"):
            multi_control_values([1.0, bad], 0.0, 1.0, 2, 1)


def test_control_images_one_entry_per_net():
    a, b = torch.zeros(1, 3, 32, 32), torch.zeros(3, 3, 32, 32)
    assert multi_control_images("pose_image", [a, b], 2, 3) == [a, b]
    assert multi_control_images("pose_image", (a, [a, a, a]), 2, 3)[1] == [a, a, a]
    for bad, n in ((a, 1), ([a], 1), ([a, a, a], 3), (None, 0)):
        with pytest.raises(ValueError, match=rf"pose_image has {n} entries for 2 ControlNets"):
            multi_control_images("pose_image", bad, 2, 1)
    with pytest.raises(ValueError, match=r"pose_image\[1\] has 3 entries for 2 requests"):
        multi_control_images("pose_image", [a, b], 2, 2)
    with pytest.raises(ValueError, match="pose_image: 1 of the 2 entries are None"):
        multi_control_images("pose_image", [a, None], 2, 1)
    assert multi_control_images("control_image", [None, a], 2, 1, allow_none=1) == [None, a]
    with pytest.raises(ValueError, match="control_image: 2 of the 2 entries are None"):
        multi_control_images("control_image", [None, None], 2, 1, allow_none=1)


# ---- the table ----
def test_the_hand_written_table():
    """K = 2, R = 3, 10 steps: net 0 opens at step 3 for everyone; net 1 has a scale and a window per request"""
    rows = multi_control_plan(*(M.TABLE_ARGS[k] for k in ("controlnet_conditioning_scale", "control_guidance_start", "control_guidance_end")),
                              2, 3, M.TABLE_STEPS, per_request=True)
    assert len(rows) == 2 and all(len(net) == 3 for net in rows)
    for k in range(2):
        for r in range(3):
            assert rows[k][r] == [pytest.approx(v) for v in M.TABLE_ROWS[k][r]], (k, r)
    lay = RequestLayout(3, 1)
    tab = multi_control_scale_table(rows, 10, lay, clamp=False)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (10, 2, 6) and tab.is_contiguous()
    assert tab[0].tolist() == [[0.0] * 6, [1.0, 0.0, 2.0] * 2]
    assert tab[2].tolist() == [[0.0] * 6, [1.0, 0.25, 2.0] * 2]
    assert tab[3].tolist() == [[0.5] * 6, [1.0, 0.25, 2.0] * 2]
    assert tab[5].tolist() == [[0.5] * 6, [1.0, 0.25, 0.0] * 2]
    assert tab[9].tolist() == [[0.5] * 6, [1.0, 0.25, 0.0] * 2]
    assert torch.equal(tab[:, :, :3], tab[:, :, 3:])                             # the uncond half repeats the cond half
    for k in range(2):
        assert torch.equal(tab[:, k], control_scale_table(rows[k], 10, lay, clamp=False))
    # two images per request: request-major
    tab2 = multi_control_scale_table(rows, 10, RequestLayout(3, 2), clamp=False)
    assert tuple(tab2.shape) == (10, 2, 12) and torch.equal(tab2[:, :, :6], tab[:, :, :3].repeat_interleave(2, dim=2))
    assert torch.equal(tab2[:, :, 6:], tab2[:, :, :6])
    # PNDM: one UNet call more than steps reads the last gate; without clamp a missing entry is an error
    tab3 = multi_control_scale_table(rows, 11, lay, clamp=True)
    assert tuple(tab3.shape) == (11, 2, 6) and torch.equal(tab3[:10], tab) and torch.equal(tab3[10], tab[9])
    with pytest.raises(ValueError, match="10 entries for 11 UNet calls"):
        multi_control_scale_table(rows, 11, lay, clamp=False)


# ---- the model ----
def test_multi_controlnet_checks_its_nets():
    a, b = _Net(1), _Net(2)
    m = MultiControlNetModel([a, b])
    assert m.nets == [a, b] and len(m) == 2 and m.dtype == torch.float16 and MultiControlNetModel.MAX_NETS == 4
    assert MultiControlNetModel((a, b)).nets == [a, b] and MultiControlNetModel(m).nets == [a, b] and MultiControlNetModel(a).nets == [a]
    with pytest.raises(ValueError, match="expected 1 to 4 ControlNets, got 0"):
        MultiControlNetModel([])
    with pytest.raises(ValueError, match="expected 1 to 4 ControlNets, got 5"):
        MultiControlNetModel([a] * 5)
    with pytest.raises(TypeError, match="net 1 is a _RecordingControlNet, expected a ControlNetModel"):
        MultiControlNetModel([a, _RecordingControlNet()])
    with pytest.raises(ValueError, match="net 1 is torch.bfloat16 on cpu, net 0 is torch.float16 on cpu"):
        MultiControlNetModel([a, _Net(2, dtype=torch.bfloat16)])
    with pytest.raises(ValueError, match="net 1 has block_out_channels"):
        MultiControlNetModel([a, _Net(2, widths=(16, 64))])
    with pytest.raises(ValueError, match="net 1 has layers_per_block"):
        MultiControlNetModel([a, _Net(2, layers=2)])


def test_residual_shapes_are_those_of_the_engine():
    from tests.control_rows_cases import residual_row_elems
    m = MultiControlNetModel([_Net(1, widths=(320, 640, 1280, 1280), layers=2)] * 2)
    for h, w in ((8, 8), (5, 7), (64, 80)):
        down, mid = m.residual_shapes(2, h, w)
        got = [s[1] * s[2] * s[3] for s in down + [mid]]
        assert tuple(got) == residual_row_elems(h, w) and all(s[0] == 2 for s in down)
    assert m.residual_shapes(4, 8, 8, depth=2) == ([(4, 8, 8, 320)] * 2, None)


def test_forward_runs_the_nets_in_order_then_one_mix(mixes):
    a, b, c = _Net(1), _Net(2), _Net(3)
    m = MultiControlNetModel([a, b, c])
    x = torch.zeros(4, 2, 2, 8, dtype=torch.float16)
    conds = [torch.zeros(1), torch.ones(1), torch.ones(2)]
    sc = torch.arange(12, dtype=torch.float32).view(3, 4)
    down, mid = m.forward_nhwc(x, 5, "ehs", conds, sc)
    assert [len(n.calls) for n in (a, b, c)] == [1, 1, 1]
    for n, cond in zip((a, b, c), conds):
        assert n.calls[0]["scale"] == 1.0 and n.calls[0]["rows"] is None and n.calls[0]["cond"] is cond          # out_scale 1, its own cond
    assert len(mixes) == 1 and mixes[0]["scales"] is not sc and torch.equal(mixes[0]["scales"], sc)
    srcs = mixes[0]["sources"]
    assert len(srcs) == 3 and [len(s) for s in srcs] == [5] * 3          # widths (16, 32), 1 layer: conv_in, layer, downsample, layer + mid
    assert [float(s[0].flatten()[0]) for s in srcs] == [1.0, 2.0, 3.0]
    assert all(o is s for o, s in zip(mixes[0]["out"], srcs[0]))          # mixed in place on the first net's fresh tensors
    assert len(down) == 4 and mid is mixes[0]["out"][-1]
    # a gated net is not run; its slot in the launch holds the destination (never read at scale 0)
    mixes.clear()
    down, mid = m.forward_nhwc(x, 5, "ehs", conds, sc, run=[False, True, False])
    assert [len(n.calls) for n in (a, b, c)] == [1, 2, 1] and len(mixes) == 1
    srcs = mixes[0]["sources"]
    assert float(srcs[1][0].flatten()[0]) == 2.0 and all(o is s for o, s in zip(mixes[0]["out"], srcs[1]))
    assert all(p is q for k in (0, 2) for p, q in zip(srcs[k], mixes[0]["out"]))
    # every net gated: fresh tensors of the engine's shapes, still one launch (which writes +0)
    mixes.clear()
    down, mid = m.forward_nhwc(x, 5, "ehs", conds, sc, run=[False] * 3)
    assert [len(n.calls) for n in (a, b, c)] == [1, 2, 1] and len(mixes) == 1
    assert [tuple(t.shape) for t in down] == [(4, 2, 2, 16), (4, 2, 2, 16), (4, 1, 1, 16), (4, 1, 1, 32)] and tuple(mid.shape) == (4, 1, 1, 32)
    assert all(t.dtype == torch.float16 for t in down)
    with pytest.raises(ValueError, match="2 conditioning images for 3 nets"):
        m.forward_nhwc(x, 5, "ehs", conds[:2], sc)
    with pytest.raises(ValueError, match=r"scale_table_row must be a device fp32 tensor \[3, 4\]"):
        m.forward_nhwc(x, 5, "ehs", conds, sc.t())
    with pytest.raises(ValueError, match="run has 2 flags for 3 nets"):
        m.forward_nhwc(x, 5, "ehs", conds, sc, run=[True, False])


def test_forward_in_a_shallow_deepcache_call_mixes_depth_residuals(mixes):
    a, b = _Net(1), _Net(2)
    m = MultiControlNetModel([a, b])
    x = torch.zeros(2, 2, 2, 8, dtype=torch.float16)
    dc = DeepCache(1)
    dc.full = True
    down, mid = m.forward_nhwc(x, 5, "ehs", [None, None], torch.ones(2, 2), deepcache=dc, run=[False, False])
    assert len(down) == 4 and mid is not None and a.calls == []
    dc.full = False          # (the full call noted the ControlNet's geometry although no net ran)
    down, mid = m.forward_nhwc(x, 5, "ehs", [None, None], torch.ones(2, 2), deepcache=dc)
    assert len(down) == 1 and mid is None and len(mixes[-1]["out"]) == 1 and a.calls[0]["cache"] is dc and b.calls[0]["cache"] is dc
    down, mid = m.forward_nhwc(x, 5, "ehs", [None, None], torch.ones(2, 2), deepcache=dc, run=[False, False])
    assert [tuple(t.shape) for t in down] == [(2, 2, 2, 16)] and mid is None


def test_a_wrapper_of_one_net_is_that_net(mixes):
    a = _Net(1)
    m = MultiControlNetModel([a])
    sc = torch.ones(1, 4)
    m.forward_nhwc(torch.zeros(4, 2, 2, 8, dtype=torch.float16), 5, "ehs", ["cond"], sc)
    assert mixes == [] and a.calls[0]["scale"] == 1.0 and a.calls[0]["cond"] == "cond" and torch.equal(a.calls[0]["rows"], sc[0])


# ---- the pipeline ----
def test_a_list_is_wrapped_and_one_net_delegates(no_launches):  # noqa: F811
    a, b = _Net(1), _Net(2)
    pipe = PipelineBase()
    kw = dict(vae=None, reference_unet=None, unet=_RecordingUNet(), tokenizer=None, text_encoder=None, image_encoder=None, ImgProj=None,
              scheduler=_pipe(_RecordingUNet()).scheduler)
    pipe._init_common(controlnet=[a, b], **kw)
    assert isinstance(pipe.controlnet, MultiControlNetModel) and pipe.controlnet.nets == [a, b] and pipe._control_nets() == [a, b]
    pipe._init_common(controlnet=(a, b), **kw)
    assert isinstance(pipe.controlnet, MultiControlNetModel) and pipe._single_controlnet() is pipe.controlnet
    pipe._init_common(controlnet=a, **kw)
    assert pipe.controlnet is a and pipe._control_nets() == [a] and pipe._single_controlnet() is a
    pipe._init_common(controlnet=None, **kw)
    assert pipe._control_nets() == [] and pipe._single_controlnet() is None
    # MultiControlNetModel([a]) and [a]: the call the pipeline makes for ``a`` itself, folded and rows route alike
    for given in (MultiControlNetModel([a]), [a]):
        pipe._init_common(controlnet=given, **kw)
        assert isinstance(pipe.controlnet, MultiControlNetModel) and pipe._single_controlnet() is a
        for control in (dict(scale=0.8, keep=[0.0, 1.0, 1.0, 1.0]), dict(scale=1.0, keep=[1.0] * 4, rows=[[1.0] * 4, [0.5, 0.5, 0.0, 0.0]])):
            a.calls.clear()
            _denoise(pipe, 2, control, steps=4, image=torch.zeros(1, 32, 32, 8, dtype=torch.float16))
            ref = _RecordingControlNet()
            pipe.controlnet, keep = ref, pipe.controlnet
            _denoise(pipe, 2, control, steps=4, image=torch.zeros(1, 32, 32, 8, dtype=torch.float16))
            pipe.controlnet = keep
            assert [c["scale"] for c in a.calls] == [c["scale"] for c in ref.calls]
            assert [None if c["rows"] is None else c["rows"].tolist() for c in a.calls] == \
                   [None if c["rows"] is None else c["rows"].tolist() for c in ref.calls]


def _denoise(pipe, R, control, steps=10, n=1, **kw):
    ctl = dict(dict(prompt_embeds=torch.zeros(R, 3, 8), negative_prompt_embeds=torch.zeros(R, 3, 8)), **control, **kw)
    return pipe._denoise(latents=torch.zeros(R * n, 4, 4, 4), prompt_embeds=torch.zeros(R, 3, 8), negative_prompt_embeds=torch.zeros(R, 3, 8),
                         sa_hidden_states={}, num_inference_steps=steps, guidance_scale=7.5, requests=R, control=ctl)


def _multi_pipe(sched="ddim", K=2):
    pipe = _pipe(_RecordingUNet(), sched)
    nets = [_Net(k + 1) for k in range(K)]
    pipe.controlnet = MultiControlNetModel(nets)
    return pipe, nets


@pytest.mark.parametrize("sched", ["ddim", "dpm", "pndm"])
def test_the_loop_hands_every_call_its_slice_and_skips_gated_nets(no_launches, mixes, sched):  # noqa: F811
    pipe, (a, b) = _multi_pipe(sched)
    rows = multi_control_plan(*(M.TABLE_ARGS[k] for k in ("controlnet_conditioning_scale", "control_guidance_start", "control_guidance_end")),
                              2, 3, 10, per_request=True)
    imgs = [torch.zeros(1, 32, 32, 8, dtype=torch.float16), torch.ones(3, 32, 32, 8, dtype=torch.float16)]
    _denoise(pipe, 3, dict(image=imgs, scale=1.0, multi_rows=rows))
    calls = 11 if sched == "pndm" else 10
    assert len(mixes) == calls                                               # exactly one mix launch per UNet call
    assert len(a.calls) == calls - 3 and len(b.calls) == calls               # net 0 is closed for the first three calls: not run
    want = multi_control_scale_table(rows, calls, RequestLayout(3, 1), clamp=True)
    for i, mx in enumerate(mixes):
        assert torch.equal(mx["scales"], want[i]) and tuple(mx["scales"].shape) == (2, 6)
    assert all(c["scale"] == 1.0 and c["rows"] is None and c["batch"] == 6 for c in a.calls + b.calls)
    assert tuple(a.calls[0]["cond"].shape) == (1, 32, 32, 8) and tuple(b.calls[0]["cond"].shape) == (6, 32, 32, 8)          # per request: 2B rows
    assert len(pipe.unet.calls) == calls
    # every net gated at some calls: the launch is still made (it writes +0), no net runs
    mixes.clear(), a.calls.clear(), b.calls.clear()
    _denoise(pipe, 1, dict(image=imgs[:1] * 2, scale=1.0, multi_rows=multi_control_plan(1.0, 0.5, 1.0, 2, 1, 10)))
    assert len(mixes) == calls and len(a.calls) == len(b.calls) == calls - 5
    with pytest.raises(ValueError, match="1 nets' scales and 2 images for 2 ControlNets"):
        _denoise(pipe, 3, dict(image=imgs, scale=1.0, multi_rows=rows[:1]))
    with pytest.raises(ValueError, match="every net needs the scales of 3 requests"):
        _denoise(pipe, 3, dict(image=imgs, scale=1.0, multi_rows=[rows[0], rows[1][:2]]))


def test_the_mix_route_composes_with_deepcache(no_launches, mixes):  # noqa: F811
    pipe, (a, b) = _multi_pipe()
    pipe.enable_deepcache(cache_interval=2, depth=1)
    img = torch.zeros(1, 32, 32, 8, dtype=torch.float16)
    _denoise(pipe, 1, dict(image=[img, img], scale=1.0, multi_rows=multi_control_plan([1.0, 0.5], 0.0, [1.0, 0.5], 2, 1, 4)), steps=4)
    assert len(mixes) == 4 and [len(m["out"]) for m in mixes] == [5, 1, 5, 1]          # full, shallow (depth 1), full, shallow
    assert len(a.calls) == 4 and len(b.calls) == 2 and all(c["cache"] is not None for c in a.calls + b.calls)
    assert len({id(c["cache"]) for c in a.calls + b.calls}) == 1 and a.calls[0]["cache"] is pipe.unet.calls[0]["cache"]


MODULES = ("IMAGDressing_v1_pipeline_controlnet", "IMAGDressing_v1_pipeline_ipa_controlnet", "IMAGDressing_v1_pipeline_controlnet_inpainting")


def _real_pipe(mod, controlnet):
    cls = importlib.import_module("imagdressing_amd.dressing_sd.pipelines." + mod).IMAGDressing_v1
    pipe = object.__new__(cls)
    pipe._init_common(vae=None, reference_unet=None, unet=_RecordingUNet(), tokenizer=None, text_encoder=None, image_encoder=None, ImgProj=None,
                      scheduler=_pipe(_RecordingUNet()).scheduler, controlnet=controlnet)
    return pipe


@pytest.mark.parametrize("mod", MODULES)
def test_refusals_by_name(mod):
    a, b = _Net(1), _Net(2)
    pipe = _real_pipe(mod, [a, b])
    img = torch.zeros(1, 3, 32, 32)
    image_kw = dict(control_image=[img, img]) if mod.endswith("inpainting") else dict(pose_image=[img, img])
    call = dict(prompt=None, null_prompt="", negative_prompt=None, ref_image=None, width=32, height=32, num_inference_steps=4, guidance_scale=7.5,
                prompt_embeds=torch.zeros(1, 3, 8), negative_prompt_embeds=torch.zeros(1, 3, 8))
    with pytest.raises(NotImplementedError, match="open_session"):
        pipe.open_session(2, 32, 32)
    with pytest.raises(NotImplementedError, match="shard_over_ranks=True on a pipeline with 2 ControlNets"):
        pipe(**call, **image_kw, shard_over_ranks=True)
    with pytest.raises(NotImplementedError, match="guess_mode"):
        pipe(**call, **image_kw, guess_mode=True)
    if mod.endswith("inpainting"):
        with pytest.raises(ValueError, match="control_image has 0 entries for 2 ControlNets"):
            pipe(**call)
        with pytest.raises(ValueError, match="control_image has 1 entries for 2 ControlNets"):
            pipe(**call, control_image=img)
        with pytest.raises(ValueError, match="control_image: 2 of the 2 entries are None"):
            pipe(**call, control_image=[None, None])


def test_open_session_is_refused_with_several_nets_only():
    a, b = _Net(1), _Net(2)
    pipe = _real_pipe(MODULES[0], [a, b])
    with pytest.raises(NotImplementedError, match="open_session on a pipeline with 2 ControlNets"):
        pipe.open_session(2, 32, 32)
    with pytest.raises(NotImplementedError, match="open_session on a pipeline with 2 ControlNets"):
        pipe._open_session(2, 32, 32, with_controlnet=True)
    assert pipe._multi_control("pose_image", None, False) == 0 and pipe._multi_control("pose_image", [1, 2], False) == 2
    one = _real_pipe(MODULES[0], [a])
    assert one._multi_control("pose_image", [1], True) == 0                  # one net: today's routes, today's refusals
    one._refuse_multi("open_session")


# ---- the compat import paths ----
def test_the_three_compat_import_paths(monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "compat"))
    saved = {k: v for k, v in sys.modules.items() if k == "diffusers" or k.startswith("diffusers.")}
    for k in saved:
        monkeypatch.delitem(sys.modules, k)
    try:
        import diffusers
        assert diffusers.__file__.startswith(os.path.join(ROOT, "compat"))
        from diffusers import MultiControlNetModel as A
        from diffusers.pipelines.controlnet import MultiControlNetModel as B
        from diffusers.pipelines.controlnet.multicontrolnet import MultiControlNetModel as C
        assert A is B is C is MultiControlNetModel and "MultiControlNetModel" in diffusers.__all__
    finally:
        for k in [k for k in sys.modules if k == "diffusers" or k.startswith("diffusers.")]:
            del sys.modules[k]
        sys.modules.update(saved)
