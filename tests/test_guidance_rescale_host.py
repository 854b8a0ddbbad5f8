"""guidance_rescale on the host, without a GPU: where the keyword sits in the four ``__call__`` signatures, the validation of its
values, per-request expansion, and when ``_denoise`` and ``DenoiseSession.step`` issue the launch -- never with every value 0, once
per UNet call otherwise (a recorder in place of ``ops.guidance_rescale``) -- the refusal of the host-stepped UniPC, ``check_request``."""
import importlib
import inspect
import types

import pytest
import torch

from imagdressing_amd import ops
from imagdressing_amd.dressing_sd.pipelines._base import PipelineBase, guidance_rescale_values, request_count
from imagdressing_amd.session import check_request
from tests.test_deepcache_host import _RecordingUNet, _pipe, _run

MODULES = ("IMAGDressing_v1_pipeline", "IMAGDressing_v1_pipeline_controlnet", "IMAGDressing_v1_pipeline_controlnet_inpainting",
           "IMAGDressing_v1_pipeline_ipa_controlnet")
LEADING = ["self", "prompt", "null_prompt", "negative_prompt", "ref_image", "width", "height", "num_inference_steps", "guidance_scale"]


@pytest.mark.parametrize("mod", MODULES)
def test_keyword_position_and_default(mod):
    cls = importlib.import_module("imagdressing_amd.dressing_sd.pipelines." + mod).IMAGDressing_v1
    params = list(inspect.signature(cls.__call__).parameters.values())
    names = [p.name for p in params]
    assert names[:len(LEADING)] == LEADING                                  # the reference's leading parameters stay in place
    assert params[-1].kind is inspect.Parameter.VAR_KEYWORD
    p = params[names.index("guidance_rescale")]
    assert p.default == 0.0 and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    if mod.endswith("inpainting"):
        assert names[-3:] == ["guidance_rescale", "overlay", "kwargs"]
    else:
        assert names[-2:] == ["guidance_rescale", "kwargs"]
    assert names.index("guidance_rescale") > names.index("trace")            # appended to the extension keywords


def test_values_are_validated_and_expanded():
    assert guidance_rescale_values(0.7, 3) == [0.7] * 3
    assert guidance_rescale_values([0.0, 0.7, 1.0], 3) == [0.0, 0.7, 1.0]
    assert guidance_rescale_values([0.5], 2) == [0.5, 0.5]
    assert guidance_rescale_values(0, 1) == [0.0] and guidance_rescale_values(1, 1) == [1.0]
    for bad in (-0.1, 1.0001, float("nan"), float("inf"), -float("inf"), [0.0, 2.0]):
        with pytest.raises(ValueError, match=r"guidance_rescale must be finite and in \[0, 1\]"):
            guidance_rescale_values(bad, 2)
    with pytest.raises(ValueError, match="guidance_rescale has 3 entries for 2 requests"):
        guidance_rescale_values([0.1, 0.2, 0.3], 2)
    # a request-batched call: one value per request (or one shared), checked with the other per-request arguments
    args = dict(prompt=["a", "b", "c"], guidance_scale=[5.0, 7.5, 9.0])
    assert request_count(dict(args, guidance_rescale=[0.0, 0.7, 0.0])) == 3 and request_count(dict(args, guidance_rescale=0.7)) == 3
    with pytest.raises(ValueError, match="guidance_rescale has 2 entries for 3 requests"):
        request_count(dict(args, guidance_rescale=[0.0, 0.7]))
    with pytest.raises(ValueError, match=r"in \[0, 1\]"):
        request_count(dict(args, guidance_rescale=[0.0, 0.7, 1.5]))


@pytest.fixture
def recorder(monkeypatch):
    """the step launches leave the latent alone; ``ops.guidance_rescale`` records its arguments"""
    calls = []
    for name in ("ddim_cfg_step", "sampler_step", "unipc_step", "sampler_step_rows", "sampler_step_rows_at", "session_input_rows"):
        monkeypatch.setattr(ops, name, lambda *a, **k: None)
    monkeypatch.setattr(ops, "lincomb", lambda terms, out=None: out if out is not None else terms[0][1].clone())
    monkeypatch.setattr(ops, "workspace", lambda tag, shape, dtype, device, init=None: torch.zeros(tuple(shape), dtype=dtype))
    monkeypatch.setattr(ops, "ensure_device", lambda device: None)
    monkeypatch.setattr(ops, "guidance_rescale", lambda eps, *, guidance, rescale: calls.append(
        dict(eps=tuple(eps.shape), guidance=guidance, rescale=rescale.clone() if isinstance(rescale, torch.Tensor) else rescale)))
    return calls


def _run_requests(pipe, R, steps=5, **kw):
    return pipe._denoise(latents=torch.zeros(R, 4, 4, 4), prompt_embeds=torch.zeros(R, 3, 8), negative_prompt_embeds=torch.zeros(R, 3, 8),
                         sa_hidden_states={}, num_inference_steps=steps, requests=R, **kw)


@pytest.mark.parametrize("sched", ["ddim", "dpm", "pndm"])
def test_denoise_launches_once_per_unet_call_or_never(recorder, sched):
    unet = _RecordingUNet()
    pipe = _pipe(unet, sched)
    _run(pipe)
    _run(pipe, guidance_rescale=0.0)
    _run(pipe, guidance_rescale=[0.0])
    _run_requests(pipe, 2, guidance_scale=[5.0, 7.5], guidance_rescale=[0.0, 0.0])
    assert recorder == [] and len(unet.calls) > 0                            # every value 0: nothing new
    unet.calls.clear()
    _run(pipe, guidance_rescale=0.7)
    assert len(recorder) == len(unet.calls) > 0                              # (PNDM: one UNet call more than it has steps)
    assert all(c == dict(eps=(2, 16, 4), guidance=7.5, rescale=0.7) for c in recorder)
    recorder.clear(), unet.calls.clear()
    _run_requests(pipe, 3, guidance_scale=[5.0, 7.5, 9.0], guidance_rescale=[0.0, 0.7, 0.0])
    assert len(recorder) == len(unet.calls) > 0
    for c in recorder:
        assert c["eps"] == (6, 16, 4) and torch.equal(c["guidance"], torch.tensor([5.0, 7.5, 9.0]))
        assert c["rescale"].dtype == torch.float32 and torch.equal(c["rescale"], torch.tensor([0.0, 0.7, 0.0]))
    assert len({id(c["guidance"]) for c in recorder}) == 1                   # one tensor for the whole call, like g_arg
    recorder.clear()
    # two images per request: a request's value on each of its rows; equal values stay a scalar
    pipe._denoise(latents=torch.zeros(4, 4, 4, 4), prompt_embeds=torch.zeros(2, 3, 8), negative_prompt_embeds=torch.zeros(2, 3, 8),
                  sa_hidden_states={}, num_inference_steps=3, requests=2, guidance_scale=7.5, guidance_rescale=[0.25, 0.5])
    assert torch.equal(recorder[0]["rescale"], torch.tensor([0.25, 0.25, 0.5, 0.5])) and recorder[0]["guidance"] == 7.5
    recorder.clear()
    _run_requests(pipe, 2, guidance_scale=7.5, guidance_rescale=[0.5, 0.5])
    assert recorder[0]["rescale"] == 0.5
    with pytest.raises(ValueError, match=r"in \[0, 1\]"):
        _run(pipe, guidance_rescale=1.5)


def test_host_stepped_unipc_is_refused_by_name(recorder):
    unet = _RecordingUNet()
    pipe = _pipe(unet, "unipc")
    _run(pipe, guidance_rescale=0.0)                                         # 0 runs as before
    assert recorder == [] and len(unet.calls) == 7
    with pytest.raises(NotImplementedError, match=r"enable_fused_step\(\)"):
        _run(pipe, guidance_rescale=0.7)
    assert len(unet.calls) == 7                                              # refused before the first forward
    pipe.scheduler.enable_fused_step()
    unet.calls.clear()
    _run(pipe, guidance_rescale=0.7)
    assert len(recorder) == len(unet.calls) == 7


def test_check_request_refuses_bad_values():
    ok = dict(size=(128, 128), num_inference_steps=4, guidance_scale=7.5)
    check_request(**ok)
    check_request(guidance_rescale=0.7, **ok), check_request(guidance_rescale=0, **ok), check_request(guidance_rescale=1.0, **ok)
    for bad in (-0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"guidance_rescale must be finite and in \[0, 1\]"):
            check_request(guidance_rescale=bad, **ok)
    with pytest.raises(ValueError, match="guidance_rescale is per request in a session"):
        check_request(guidance_rescale=[0.0, 0.7], **ok)


# ---- DenoiseSession.step on stand-ins ----
class _SessionUNet(_RecordingUNet):
    temb_proj = types.SimpleNamespace(weight=torch.zeros(8, 2))
    attn_processors = {}

    def use_time_embedding(self, buf):
        pass

    def clear_time_embeddings(self):
        pass

    def _time_embed_rows(self, ts):
        return torch.zeros(len(ts), 8)


class _SessionPipe(PipelineBase):
    def set_scale(self, scale):
        pass

    def _request_garments(self, *a, **k):
        return None, None, 1

    def _garment_features(self, ref_lat, cloth_tokens, garments=1):
        return {"layer": torch.zeros(1, 2, 8)}


def _session_pipe():
    from imagdressing_amd import scheduler as S
    pipe = _SessionPipe()
    pipe._init_common(vae=None, reference_unet=None, unet=_SessionUNet(), tokenizer=None, text_encoder=None, image_encoder=None, ImgProj=None,
                      scheduler=S.DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                                              beta_schedule="scaled_linear"))
    return pipe


def _submit(ses, steps, phi=None):
    kw = {} if phi is None else dict(guidance_rescale=phi)
    return ses.submit(num_inference_steps=steps, guidance_scale=7.5, prompt_embeds=torch.zeros(1, 3, 8),
                      negative_prompt_embeds=torch.zeros(1, 3, 8), latents=torch.zeros(1, 4, 4, 4), output_type="latent", **kw)


@pytest.mark.parametrize("compact", [False, True], ids=["slots", "compact"])
def test_session_launches_only_while_a_running_request_asks(recorder, compact):
    pipe = _session_pipe()
    with pipe._open_session(3, 32, 32, compact=compact) as ses:
        _submit(ses, 3), _submit(ses, 4, 0.0)
        ses.drain()
        assert recorder == [] and ses.steps_run == 4                         # every value 0: the launch is never issued
        assert not ses.rescale.any() and (ses.rescale_rows is None) == (not compact)
    with pipe._open_session(3, 32, 32, compact=compact) as ses:
        a, b = _submit(ses, 2, 0.7), _submit(ses, 5)
        ses.step()
        assert len(recorder) == 1 and a.slot == 0 and b.slot == 1
        call = recorder[0]
        assert call["eps"] == (2 * ses.width, 16, 4)
        assert call["rescale"].tolist()[:2] == [pytest.approx(0.7), 0.0] and not call["rescale"][2:].any()
        assert isinstance(call["guidance"], torch.Tensor) and call["guidance"].numel() == call["rescale"].numel()
        ses.step()                                                           # a's last step
        assert len(recorder) == 2 and a.done
        assert not ses.rescale.any() and (not compact or not ses.rescale_rows.any())          # released: back to 0
        c = _submit(ses, 2)                                                  # the next occupant of a's slot does not ask
        ses.drain()
        assert c.slot == 0 and len(recorder) == 2 and ses.steps_run == 5     # nobody asks any more: no launch
        d = _submit(ses, 1, 1.0)
        ses.drain()
        assert len(recorder) == 3 and recorder[2]["rescale"][d.slot if not compact else 0] == 1.0
        assert not ses.rescale.any()
