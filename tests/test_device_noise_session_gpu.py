"""Device noise in denoising sessions (``open_session(device_noise=...)``, ``submit(seed=, eta=)``), plain and compacting, with
Euler-ancestral and with DDIM at eta = 0.3: a request's final latents do not depend on its batch company (other seeds, step counts and
eta, arriving mid-flight) nor, in the plain session, on the slot it lands in; they equal the solo pipeline call with the same seed
within the bars tests/test_session_gpu.py uses; a deterministic session keeps its launches and bits; and with nothing switched on the
refusals are the old ones."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.harness import SMALL, build_pair  # noqa: E402
from tests.test_multi_request_gpu import _bar_small, _check, _Requests, _sched, _traj_bar  # noqa: E402
from tests.test_session_gpu import KW, _pipe, _submit_kw  # noqa: E402

SEEDS = (0x0123456789ABCDEF, 2 ** 64 - 1, 20261020)
ETA = {"euler_a": (0.0, 0.0, 0.0), "ddim": (0.3, 0.7, 0.0)}          # request 0 is the one under test; the others bring other values


def _scheduler(name):
    from imagdressing_amd import scheduler as S
    return {"ddim": _sched, "euler_a": lambda: S.EulerAncestralDiscreteScheduler(**KW), "dpm": lambda: S.DPMSolverMultistepScheduler(**KW)}[name]()


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def pair(request):
    torch.manual_seed(0)
    p = build_pair(SMALL, seed=0, dtype=request.param)
    p["dtype"] = request.param
    return p


def _req(reqs, name, r, steps, **over):
    kw = _submit_kw(reqs, r, steps, seed=SEEDS[r], eta=ETA[name][r])
    kw.pop("latents")
    kw.update(over)
    return kw


def _alone(pipe, reqs, name, **open_kw):
    with pipe.open_session(slots=3, width=128, height=128, device_noise=True, **open_kw) as ses:
        a = ses.submit(**_req(reqs, name, 0, 6))
        assert a.seed == SEEDS[0]
        ses.drain()
        assert a.slot == 0 and ses.steps_run == 6
        if name == "euler_a" or ETA[name][0] > 0:
            assert ses.noise is not None and tuple(ses.noise.shape) == (3, 256, 4) and tuple(ses.key_rows.shape) == (3, 8)
            assert not ses.noise[1:].any()                  # zero-filled at allocation, and the idle slots were never written
            assert ses.key_rows[1:, 4].tolist() == [0, 0]
        return a.result().images


@pytest.mark.parametrize("compact", [False, True], ids=["plain", "compact"])
@pytest.mark.parametrize("name", ["euler_a", "ddim"])
@torch.no_grad()
def test_a_request_does_not_see_its_batch_company(pair, name, compact):
    """compact: the ladder (3,) keeps the batch width, and with it the tile configurations, the same in both runs -- the rows still go
    through the row -> slot map (imd_sampler_step_rows_at), noise and keys by SLOT"""
    reqs = _Requests()
    pipe = _pipe(pair, _scheduler(name))
    open_kw = dict(compact=True, widths=(3,)) if compact else {}
    alone = _alone(pipe, reqs, name, **open_kw)
    with pipe.open_session(slots=3, width=128, height=128, device_noise=True, **open_kw) as ses:
        a = ses.submit(**_req(reqs, name, 0, 6))
        ses.step(), ses.step()
        b = ses.submit(**_req(reqs, name, 1, 8))
        ses.step(), ses.step()
        c = ses.submit(**_req(reqs, name, 2, 3))
        ses.drain()
        assert (a.slot, b.slot, c.slot) == (0, 1, 2) and ses.steps_run == 10
        crowded = a.result().images
        assert torch.isfinite(b.result().images).all() and torch.isfinite(c.result().images).all()
        assert not torch.equal(b.result().images, crowded)
    assert torch.isfinite(alone).all()
    assert torch.equal(alone, crowded), (alone - crowded).abs().max().item()


@pytest.mark.parametrize("name", ["euler_a", "ddim"])
@torch.no_grad()
def test_the_slot_does_not_matter_in_the_plain_session(pair, name):
    reqs = _Requests()
    pipe = _pipe(pair, _scheduler(name))
    alone = _alone(pipe, reqs, name)
    with pipe.open_session(slots=3, width=128, height=128, device_noise=True) as ses:
        f = ses.submit(**_req(reqs, name, 1, 2))
        g = ses.submit(**_req(reqs, name, 2, 9))
        a = ses.submit(**_req(reqs, name, 0, 6))
        ses.drain()
        assert (f.slot, g.slot, a.slot) == (0, 1, 2)
        assert torch.equal(a.result().images, alone)
    with pipe.open_session(slots=3, width=128, height=128, device_noise=True) as ses:          # a used slot: stale noise, stale latent
        f = ses.submit(**_req(reqs, name, 1, 3))
        g = ses.submit(**_req(reqs, name, 2, 2))
        ses.drain()
        a = ses.submit(**_req(reqs, name, 0, 6))
        h = ses.submit(**_req(reqs, name, 1, 4, eta=0.0))
        ses.drain()
        assert (a.slot, h.slot) == (0, 1) and torch.equal(a.result().images, alone)


@pytest.mark.parametrize("compact", [False, True], ids=["plain", "compact"])
@pytest.mark.parametrize("name", ["euler_a", "ddim"])
@torch.no_grad()
def test_equals_the_solo_pipeline_call_with_the_same_seed(pair, name, compact):
    """the pipeline switch on, device_noise left at None: the session follows it.  Two images of one request ride in two slots with
    counter word image = 0, 1, as the solo call's rows do."""
    reqs = _Requests()
    pipe = _pipe(pair, _scheduler(name)).enable_device_noise()
    solo_kw = reqs.solo_kwargs(0, n=2)
    solo_kw.pop("latents")
    solo = pipe(num_inference_steps=6, seed=SEEDS[0], eta=ETA[name][0], **solo_kw).images
    assert pipe.last_seeds == [SEEDS[0]] and solo.shape[0] == 2
    with pipe.open_session(slots=3, width=128, height=128, compact=compact) as ses:
        assert ses.device_noise
        t = ses.submit(**_req(reqs, name, 0, 6, num_images_per_prompt=2))
        ses.step()
        b = ses.submit(**_req(reqs, name, 1, 4))
        ses.drain()
        got = t.result().images
    assert got.shape == (2, 4, 16, 16) and not torch.equal(got[0], got[1])
    bar = _bar_small(pair["dtype"]) if name == "ddim" else _traj_bar(pair["dtype"])
    st = _check(got, solo, bar, floor=0.0 if name == "ddim" else 1.0)
    print(f"device-noise session vs the solo call, {name}, compact={compact} [{pair['dtype']}]: {st}")


@torch.no_grad()
def test_a_deterministic_session_keeps_its_launches_and_bits(pair):
    from imagdressing_amd import ops
    reqs = _Requests()
    pipe = _pipe(pair, _scheduler("dpm"))
    outs = []
    for dn in (False, True):
        before = ops.NOISE_COUNTER["launches"]
        with pipe.open_session(slots=2, width=128, height=128, device_noise=dn) as ses:
            assert ses.noise is None and ses.key_rows is None
            t = ses.submit(**_submit_kw(reqs, 0, 5, **(dict(seed=7) if dn else {})))          # latents= given: nothing is drawn
            ses.drain()
            outs.append(t.result().images)
        assert ops.NOISE_COUNTER["launches"] == before
    assert torch.equal(outs[0], outs[1])
    # DDIM with device noise and every eta 0: no noise launch either, the bits of the session without it
    pipe = _pipe(pair, _scheduler("ddim"))
    outs = []
    for dn in (False, True):
        before = ops.NOISE_COUNTER["launches"]
        with pipe.open_session(slots=2, width=128, height=128, device_noise=dn) as ses:
            t = ses.submit(**_submit_kw(reqs, 0, 5))
            ses.drain()
            outs.append(t.result().images)
        assert ops.NOISE_COUNTER["launches"] == before
    assert torch.equal(outs[0], outs[1])


@torch.no_grad()
def test_refusals(pair):
    reqs = _Requests()
    # nothing switched on: the old refusals
    with pytest.raises(NotImplementedError, match="Euler-ancestral"):
        _pipe(pair, _scheduler("euler_a")).open_session(slots=2, width=128, height=128)
    pipe = _pipe(pair, _scheduler("ddim"))
    with pipe.open_session(slots=2, width=128, height=128) as ses:
        assert not ses.device_noise
        with pytest.raises(NotImplementedError, match="eta > 0"):
            ses.submit(**_submit_kw(reqs, 0, 6, eta=0.3))
        with pytest.raises(ValueError, match="device_noise"):
            ses.submit(**_submit_kw(reqs, 0, 6, seed=1))
    # the pipeline switch on, the session told not to follow it
    pipe.enable_device_noise()
    with pipe.open_session(slots=2, width=128, height=128, device_noise=False) as ses:
        with pytest.raises(NotImplementedError, match="eta > 0"):
            ses.submit(**_submit_kw(reqs, 0, 6, eta=0.3))
    with pytest.raises(NotImplementedError, match="Euler-ancestral"):
        _pipe(pair, _scheduler("euler_a")).enable_device_noise().open_session(slots=2, width=128, height=128, device_noise=False)
    # device noise on: eta > 0 is DDIM's alone, seeds are checked at submit
    with _pipe(pair, _scheduler("dpm")).open_session(slots=2, width=128, height=128, device_noise=True) as ses:
        with pytest.raises(ValueError, match="stochastic DDIM step"):
            ses.submit(**_submit_kw(reqs, 0, 6, eta=0.3))
    with _pipe(pair, _scheduler("euler_a")).open_session(slots=2, width=128, height=128, device_noise=True) as ses:
        with pytest.raises(ValueError, match="stochastic DDIM step"):
            ses.submit(**_submit_kw(reqs, 0, 6, eta=0.3, seed=1))
        with pytest.raises(ValueError, match="seed must be an int"):
            ses.submit(**_submit_kw(reqs, 0, 6, seed=-5))
        t = ses.submit(**_submit_kw(reqs, 0, 2))                     # no seed, no generator: os.urandom, kept on the ticket
        u = ses.submit(**_submit_kw(reqs, 0, 2, generator=torch.Generator().manual_seed(99)))
        assert isinstance(t.seed, int) and 0 <= t.seed < 2 ** 64 and u.seed == 99
        ses.drain()
        assert torch.isfinite(t.result().images).all()
