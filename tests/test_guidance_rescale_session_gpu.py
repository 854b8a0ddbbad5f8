"""guidance_rescale in denoising sessions (SMALL config, DPM-Solver++): a request's bits do not depend on what the other slots ask
for -- the reduction order of imd_guidance_rescale is a function of HW alone, and a row with 0 is neither read nor written -- in a
default and in a compacting session; a slot released by a rescaled request serves its next occupant as if it had never been."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.harness import SMALL, build_pair  # noqa: E402
from tests.test_multi_request_gpu import R3_GUIDANCE, _Requests  # noqa: E402
from tests.unipc_cases import KW  # noqa: E402


@pytest.fixture(scope="module")
def pipe():
    from imagdressing_amd.dressing_sd.pipelines.IMAGDressing_v1_pipeline import IMAGDressing_v1
    from imagdressing_amd.scheduler import DPMSolverMultistepScheduler
    torch.manual_seed(0)
    p = build_pair(SMALL, seed=5, dtype=torch.float16)
    return IMAGDressing_v1(vae=None, reference_unet=p["e_ref"], unet=p["e_unet"], tokenizer=None, text_encoder=None, image_encoder=None,
                           ImgProj=lambda h: h, scheduler=DPMSolverMultistepScheduler(**KW), safety_checker=None, feature_extractor=None)


def _submit(ses, reqs, r, steps, phi=None):
    kw = {} if phi is None else dict(guidance_rescale=phi)
    return ses.submit(num_inference_steps=steps, guidance_scale=R3_GUIDANCE[r], image_scale=1.0, prompt_embeds=reqs.pe[r].cuda(),
                      negative_prompt_embeds=reqs.ne[r].cuda(), ref_clip_hidden_states=reqs.cloth[r][1:2].cuda(),
                      ref_image_latents=reqs.refl[r].cuda(), latents=reqs.latent(r).cuda(), output_type="latent", **kw)


def _open(pipe, compact):
    # (compacting: the ladder pinned to (3,), so a request runs at the same widths alone and in company)
    return pipe.open_session(slots=3, width=128, height=128, compact=compact, **(dict(widths=(3,)) if compact else {}))


@pytest.mark.parametrize("compact", [False, True], ids=["slots", "compact"])
@torch.no_grad()
def test_a_request_keeps_its_bits_whatever_the_others_ask(pipe, compact):
    reqs = _Requests()
    with _open(pipe, compact) as ses:
        a = _submit(ses, reqs, 0, 8, 0.7)
        ses.drain()
        alone = a.result().images
    with _open(pipe, compact) as ses:
        a = _submit(ses, reqs, 0, 8)
        ses.drain()
        plain = a.result().images
    with _open(pipe, compact) as ses:
        a = _submit(ses, reqs, 0, 8, 0.7)
        ses.step(), ses.step()
        b, c = _submit(ses, reqs, 1, 9, 0.25), _submit(ses, reqs, 2, 4)
        ses.drain()
        assert (a.slot, b.slot, c.slot) == (0, 1, 2)
        crowded, b_mixed, c_mixed = a.result().images, b.result().images, c.result().images
    assert torch.isfinite(alone).all() and not torch.equal(alone, plain)
    assert torch.equal(alone, crowded), (alone - crowded).abs().max().item()
    # a request with 0 beside rescaled ones == the same request in a session in which nobody asks
    with _open(pipe, compact) as ses:
        a = _submit(ses, reqs, 0, 8)
        ses.step(), ses.step()
        b, c = _submit(ses, reqs, 1, 9), _submit(ses, reqs, 2, 4)
        ses.drain()
        b_off, c_off = b.result().images, c.result().images
    assert torch.equal(c_mixed, c_off) and not torch.equal(b_mixed, b_off)


@pytest.mark.parametrize("compact", [False, True], ids=["slots", "compact"])
@torch.no_grad()
def test_the_next_occupant_of_a_released_slot_is_unaffected(pipe, compact):
    reqs = _Requests()
    with _open(pipe, compact) as ses:
        first = _submit(ses, reqs, 1, 3, 0.7)
        ses.drain()
        second = _submit(ses, reqs, 0, 6)
        ses.drain()
        assert first.slot == second.slot == 0
        got = second.result().images
        assert not ses.rescale.any() and (not compact or not ses.rescale_rows.any())
    with _open(pipe, compact) as ses:
        first = _submit(ses, reqs, 1, 3)
        ses.drain()
        second = _submit(ses, reqs, 0, 6)
        ses.drain()
        want = second.result().images
    assert torch.isfinite(got).all() and torch.equal(got, want)
