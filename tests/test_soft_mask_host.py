"""soft_mask on the host, without a GPU: the keyword of the inpainting ``__call__`` and its refusals, the step table of the samplers
(PNDM's doubled first call, ``strength`` < 1), when ``_denoise`` issues ``ops.soft_mask_rows`` and with which rows, and that
``soft_mask=False`` builds the ``inpaint`` dict of a call without the keyword."""
import inspect

import numpy as np
import pytest
import torch

from imagdressing_amd import ops
from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline_controlnet_inpainting as inp
from imagdressing_amd.dressing_sd.pipelines._base import soft_step_table
from tests.soft_mask_cases import three_level_mask
from tests.test_deepcache_host import _RecordingUNet, _pipe
from tests.test_multi_request import _Stub, _sched


# ---- the keyword ----
def test_keyword_position_and_default():
    params = list(inspect.signature(inp.IMAGDressing_v1.__call__).parameters.values())
    names = [p.name for p in params]
    p = params[names.index("soft_mask")]
    assert p.default is False and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert names.index("mask_blur") < names.index("soft_mask") < names.index("guidance_rescale")          # beside the mask keywords
    assert names[-3:] == ["guidance_rescale", "overlay", "kwargs"]                                        # (what was last stays last)


def test_values_are_checked():
    f = inp._soft_mask_requests
    assert f(False, 3) is None and f([False, False], 2) is None and f(0, 1) is None
    assert f(True, 2) == [True, True] and f([False, True], 2) == [False, True] and f((True,), 1) == [True]
    for bad, R in (([True], 2), ([True, False, True], 2), ([], 1)):
        with pytest.raises(ValueError, match=f"entries for {R} requests"):
            f(bad, R)
    for bad in (0.5, "yes", None, 2, [True, 0.3]):
        with pytest.raises(ValueError, match="soft_mask takes True or False"):
            f(bad, 2)


def _bare_call(**kw):
    pipe = inp.IMAGDressing_v1.__new__(inp.IMAGDressing_v1)
    pipe.scheduler = None
    base = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=128, height=128, num_inference_steps=3,
                guidance_scale=5.0)
    base.update(kw)
    return pipe(**base)


def test_call_errors_precede_any_work():
    """a pipeline without engines raises them: the checks come before the first engine is touched"""
    from PIL import Image
    m = Image.fromarray(three_level_mask((64, 96), (8, 12), 128)[0])
    with pytest.raises(ValueError, match="soft_mask has 2 entries for 1 requests"):
        _bare_call(mask_image=m, soft_mask=[True, False])
    with pytest.raises(ValueError, match="soft_mask reads the gray levels of mask_image"):
        _bare_call(soft_mask=True)
    with pytest.raises(NotImplementedError, match="soft_mask with shard_over_ranks"):
        _bare_call(mask_image=m, soft_mask=True, shard_over_ranks=True)
    for bad in (float("nan"), float("inf"), -0.25, 1.5):
        levels = torch.full((1, 1, 16, 16), 0.5)
        levels[0, 0, 3, 4] = bad
        with pytest.raises(ValueError, match=r"mask_latents must be finite and in \[0, 1\]"):
            _bare_call(mask_latents=levels, soft_mask=True)
    with pytest.raises(ValueError, match="soft_mask with mask_latents: a float"):
        _bare_call(mask_latents=torch.ones(1, 1, 16, 16, dtype=torch.int32), soft_mask=True)
    # soft_mask=False does not look: the call goes on to the next check, as without the keyword
    with pytest.raises(NotImplementedError, match="guess_mode"):
        _bare_call(mask_latents=torch.full((1, 1, 16, 16), float("nan")), soft_mask=False, guess_mode=True)


# ---- the step table ----
def _timesteps(name, steps, t_start=0):
    from imagdressing_amd import scheduler as S
    kw = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    sch = {"ddim": lambda: S.DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **kw),
           "dpm": lambda: S.DPMSolverMultistepScheduler(**kw), "pndm": lambda: S.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **kw)}[name]()
    sch.set_timesteps(steps)
    return [float(t) for t in sch.timesteps][t_start:]


def test_step_table_of_the_samplers():
    for name in ("ddim", "dpm"):
        ts = _timesteps(name, 6)
        assert soft_step_table(ts, 6, [True]) == [[k] for k in range(6)]
        assert soft_step_table(ts, 6, [False, True, True]) == [[-1, k, k] for k in range(6)]
        # strength 0.5: the last three positions run, and only they count
        assert soft_step_table(_timesteps(name, 6, 3), 3, [True, False]) == [[0, -1], [1, -1], [2, -1]]
    ts = _timesteps("pndm", 6)
    assert len(ts) == 7 and ts[1] == ts[2]                                     # N + 1 UNet calls, the second position twice
    assert soft_step_table(ts, 6, [True]) == [[0], [0], [1], [2], [3], [4], [5]]          # both first calls aim at position 1
    assert soft_step_table([5.0], 1, [True]) == [[0]]
    assert soft_step_table(_timesteps("ddim", 4), 4, [False]) == [[-1]] * 4
    # the last blend -- towards the clean image latents -- is never past n - 1: a pixel with release n stays the original
    for ts, n in ((_timesteps("pndm", 6), 6), (_timesteps("pndm", 6, 3), 3), (_timesteps("dpm", 5), 5)):
        table = soft_step_table(ts, n, [True])
        assert table[-1] == [n - 1] and all(0 <= a[0] <= b[0] for a, b in zip(table, table[1:]))


@pytest.fixture
def recorder(monkeypatch):
    """the step launches leave the latent alone; ``ops.soft_mask_rows`` records its arguments"""
    calls = []
    for name in ("ddim_cfg_step", "sampler_step", "unipc_step"):
        monkeypatch.setattr(ops, name, lambda *a, **k: calls.append("step"))
    monkeypatch.setattr(ops, "ensure_device", lambda device: None)
    monkeypatch.setattr(ops, "soft_mask_rows", lambda mask, release, step_rows: calls.append(
        dict(mask=mask, release=release.clone(), step_rows=step_rows.clone())))
    return calls


def _denoise(pipe, B=1, R=1, steps=5, t_start=0, **inpaint):
    base = dict(mask=torch.zeros(1, 1, 4, 4), image_latents=torch.zeros(1, 4, 4, 4), noise=torch.zeros(B, 4, 4, 4))
    base.update(inpaint)
    return pipe._denoise(latents=torch.zeros(B, 4, 4, 4), prompt_embeds=torch.zeros(R, 3, 8), negative_prompt_embeds=torch.zeros(R, 3, 8),
                         sa_hidden_states={}, num_inference_steps=steps, guidance_scale=7.5, requests=R, t_start=t_start, inpaint=base)


@pytest.mark.parametrize("sched", ["ddim", "dpm", "pndm"])
def test_denoise_launches_in_front_of_every_step_or_never(recorder, sched):
    unet = _RecordingUNet()
    pipe = _pipe(unet, sched)
    release = torch.arange(16, dtype=torch.int32).reshape(1, 4, 4) % 6
    _denoise(pipe)
    _denoise(pipe, release=release, soft_rows=[False])
    assert all(c == "step" for c in recorder) and len(recorder) == 2 * len(unet.calls) // 2 > 0          # no soft row: nothing new
    recorder.clear(), unet.calls.clear()
    _denoise(pipe, release=release)                                            # soft_rows None: every request
    calls = 6 if sched == "pndm" else 5
    assert len(unet.calls) == calls and len(recorder) == 2 * calls
    assert [type(c) for c in recorder] == [dict, str] * calls                  # right in front of each step launch
    want = [0, 0, 1, 2, 3, 4] if sched == "pndm" else [0, 1, 2, 3, 4]
    launches = recorder[0::2]
    assert [c["step_rows"].tolist() for c in launches] == [[k] for k in want]
    for c in launches:
        assert c["release"].dtype == torch.uint16 and tuple(c["release"].shape) == (1, 16)
        assert c["release"].to(torch.int32).tolist() == [release.reshape(-1).tolist()]
        assert c["step_rows"].dtype == torch.int32
    assert len({c["mask"].data_ptr() for c in launches}) == 1                  # the one mask buffer of the call
    # strength < 1: t_start = 2 of 5 -> n = 3 positions.  PNDM's run from a later position holds no doubled entry: its four calls aim
    # at four different levels (scheduler.PNDMScheduler.plan), the table follows them and stops at n - 1
    recorder.clear()
    _denoise(pipe, t_start=2, release=release)
    got = [c["step_rows"].tolist() for c in recorder if isinstance(c, dict)]
    assert got == ([[0], [1], [2], [2]] if sched == "pndm" else [[0], [1], [2]])


def test_denoise_rows_of_a_request_batch(recorder):
    pipe = _pipe(_RecordingUNet(), "dpm")
    release = torch.stack([torch.full((4, 4), 3, dtype=torch.int32), torch.full((4, 4), 65535, dtype=torch.int32)])
    _denoise(pipe, B=4, R=2, steps=3, release=release, soft_rows=[False, True])           # two images per request
    launches = [c for c in recorder if isinstance(c, dict)]
    assert [c["step_rows"].tolist() for c in launches] == [[-1, -1, k, k] for k in range(3)]
    assert launches[0]["release"].to(torch.int32)[:, 0].tolist() == [3, 3, 65535, 65535]          # request-major rows; 65535 survives the uint16
    recorder.clear()
    _denoise(pipe, B=2, R=2, steps=3, release=torch.from_numpy(np.full((1, 4, 4), 2, np.uint16)), soft_rows=[True, False])        # one shared map
    launches = [c for c in recorder if isinstance(c, dict)]
    assert launches[1]["step_rows"].tolist() == [1, -1] and launches[1]["release"].to(torch.int32).unique().tolist() == [2]
    with pytest.raises(ValueError, match="soft_rows has 3 entries for 2 requests"):
        _denoise(pipe, B=2, R=2, release=release, soft_rows=[True, False, True])
    with pytest.raises(ValueError, match="inpaint release: expected an integer"):
        _denoise(pipe, release=torch.zeros(1, 4, 4))
    with pytest.raises(ValueError, match="inpaint release: expected an integer"):
        _denoise(pipe, release=torch.zeros(1, 4, 5, dtype=torch.int32))


# ---- the inpaint dict of the pipeline ----
class _HostPipe(inp.IMAGDressing_v1):
    """the inpainting pipeline up to ``denoise``, which records its keywords; nothing touches an engine"""

    def set_scale(self, scale):
        pass

    def _request_garments(self, *a, **k):
        return None, None, 1

    def _sa_states(self, *a, **k):
        return {}

    def denoise(self, **kw):
        self.seen.append(kw)
        return kw["latents"]


def _host_pipe():
    pipe = _HostPipe(vae=None, reference_unet=_Stub(), unet=_Stub(), tokenizer=None, text_encoder=None, controlnet=_Stub(),
                     image_encoder=None, ImgProj=lambda h: h, scheduler=_sched())
    pipe.seen = []
    return pipe


def _host_call(pipe, **kw):
    base = dict(prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, width=96, height=64, num_inference_steps=6,
                guidance_scale=5.0, prompt_embeds=torch.zeros(1, 77, 64), negative_prompt_embeds=torch.zeros(1, 77, 64),
                control_image=torch.zeros(1, 3, 64, 96), image_latents=torch.zeros(1, 4, 8, 12), latents=torch.zeros(1, 4, 8, 12),
                output_type="latent")
    base.update(kw)
    pipe(**base)
    return pipe.seen[-1]["inpaint"]


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert (torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k]), k


def test_false_and_absent_build_the_same_inpaint_dict():
    from PIL import Image
    from imagdressing_amd.image import mask_release_reference
    m, level = three_level_mask((64, 96), (8, 12), 128)
    pil = Image.fromarray(m)
    pipe = _host_pipe()
    absent = _host_call(pipe, mask_image=pil)
    assert sorted(absent) == ["image_latents", "mask", "noise"]
    _same(_host_call(pipe, mask_image=pil, soft_mask=False), absent)
    _same(_host_call(pipe, mask_image=pil, soft_mask=[False]), absent)
    on = _host_call(pipe, mask_image=pil, soft_mask=True)
    assert sorted(on) == ["image_latents", "mask", "noise", "release", "soft_rows"] and on["soft_rows"] == [True]
    _same({k: on[k] for k in absent}, absent)                                  # the hard mask is still what it was
    assert on["release"].dtype == torch.uint16 and tuple(on["release"].shape) == (1, 8, 12)
    assert np.array_equal(on["release"].numpy(), mask_release_reference(m, 8, 12, 6)[None])
    # strength 0.5: n = init_steps = 3
    half = _host_call(pipe, mask_image=pil, soft_mask=True, strength=0.5)
    assert np.array_equal(half["release"].numpy(), mask_release_reference(m, 8, 12, 3)[None])
    # mask_blur: the filtered mask is what is read (padding_mask_crop encodes with the VAE: tests/test_soft_mask_pipeline_gpu.py)
    from imagdressing_amd.image import mask_filter_host
    blurred = _host_call(pipe, mask_image=pil, soft_mask=True, mask_blur=4)
    want = np.asarray(mask_filter_host(pil, 0, 4.0))
    assert np.array_equal(blurred["release"].numpy(), mask_release_reference(want, 8, 12, 6)[None]) and not np.array_equal(want, m)
    # float mask_latents: the levels themselves
    levels = torch.tensor([0.0, 0.5, 1.0])[torch.from_numpy(level)][None, None]
    lat = _host_call(pipe, mask_latents=levels, soft_mask=True)
    assert lat["release"].to(torch.int32)[0].tolist() == (6 - torch.tensor([0, 3, 6])[torch.from_numpy(level)]).tolist()
    # a request batch: one shared mask, the second request soft
    two = _host_call(pipe, mask_image=pil, soft_mask=[False, True], prompt_embeds=torch.zeros(2, 77, 64),
                     negative_prompt_embeds=torch.zeros(2, 77, 64), latents=torch.zeros(2, 4, 8, 12))
    assert two["soft_rows"] == [False, True] and tuple(two["release"].shape) == (1, 8, 12)


def test_the_loop_writes_a_mask_buffer_of_its_own(recorder):
    """an fp32 mask of B rows passes into the loop without a copy; with a soft row the launches get a clone, without one the tensor itself"""
    pipe = _pipe(_RecordingUNet(), "ddim")
    mask = torch.rand(1, 1, 4, 4)
    seen = []
    ops.ddim_cfg_step = lambda *a, **k: seen.append(k["mask"])            # (monkeypatched by the fixture: restored after the test)
    _denoise(pipe, mask=mask)
    assert seen and all(m.data_ptr() == mask.data_ptr() for m in seen)    # no soft row: nothing is allocated
    seen.clear()
    _denoise(pipe, mask=mask, release=torch.zeros(1, 4, 4, dtype=torch.int32))
    launches = [c for c in recorder if isinstance(c, dict)]
    assert len(launches) == 5 and all(c["mask"].data_ptr() != mask.data_ptr() for c in launches)
    assert all(m.data_ptr() == launches[0]["mask"].data_ptr() for m in seen)          # the step reads the buffer the launch wrote


def test_release_values_outside_the_uint16_are_refused(recorder):
    pipe = _pipe(_RecordingUNet(), "dpm")
    for bad in (-1, 65536, 2 ** 31):
        rel = torch.zeros(1, 4, 4, dtype=torch.int64)
        rel[0, 1, 2] = bad
        with pytest.raises(ValueError, match=r"a release step is in \[0, 65535\]"):
            _denoise(pipe, release=rel)
    ok = torch.zeros(1, 4, 4, dtype=torch.int64)
    ok[0, 0, 0] = 65535
    _denoise(pipe, release=ok)
    assert [c for c in recorder if isinstance(c, dict)][0]["release"].to(torch.int32)[0, 0] == 65535


def test_numpy_bools_are_taken():
    f = inp._soft_mask_requests
    assert f(list(np.array([0.2, 0.7]) > 0.5), 2) == [False, True] and f(np.True_, 2) == [True, True] and f(np.False_, 1) is None
