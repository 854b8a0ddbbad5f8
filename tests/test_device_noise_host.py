"""The host side of the device noise source without a GPU: seed resolution and validation, key rows and draw numbering (strength < 1
included), ``ddim_row(eta)`` against the float64 DDIM step with ``variance_noise``, the session plan with ``device_noise`` -- and the
defaults, which refuse what they refused before."""
import inspect

import pytest
import torch

from imagdressing_amd import noise as N
from imagdressing_amd import ops
from imagdressing_amd import scheduler as S
from imagdressing_amd.session import SessionPlan, check_request, check_scheduler
from tests.test_session_host import KW, _mk


# ---- seeds ----
def test_seed_resolution_order():
    g = [torch.Generator().manual_seed(11), torch.Generator().manual_seed(2 ** 40 + 3)]
    assert N.resolve_seeds(5, g, 2) == [5, 5]                                   # 1. seed=
    assert N.resolve_seeds([7, 2 ** 64 - 1], g, 2) == [7, 2 ** 64 - 1]
    assert N.resolve_seeds((0, 1), None, 2) == [0, 1]
    assert N.resolve_seeds(None, g, 2) == [11, 2 ** 40 + 3]                     # 2. generator[r].initial_seed()
    assert N.resolve_seeds(None, g[1], 3) == [2 ** 40 + 3] * 3
    a, b = N.resolve_seeds(None, None, 4), N.resolve_seeds(None, None, 4)       # 3. os.urandom
    assert len(set(a + b)) == 8 and all(isinstance(s, int) and 0 <= s < 2 ** 64 for s in a + b)


@pytest.mark.parametrize("bad", [-1, 2 ** 64, 1.0, "7", True, None, [1, 2, 3], [1, -2], [1, 2.0], [[1], [2]]])
def test_seed_validation(bad):
    if bad is None:
        with pytest.raises(ValueError, match="seed must be an int"):
            N.check_seed(None)
        return
    with pytest.raises(ValueError, match="seed"):
        N.resolve_seeds(bad, None, 2)


def test_generator_list_must_match_the_requests():
    with pytest.raises(ValueError, match="generator has 3 entries for 2 requests"):
        N.resolve_seeds(None, [torch.Generator() for _ in range(3)], 2)


def test_key_rows():
    assert ops.noise_key_row(0x0123456789ABCDEF, 3, 52) == [0x89ABCDEF, 0x01234567, 3, 52, 1, 0, 0, 0]
    assert ops.noise_key_row(1, 0, 0, active=False) == [1, 0, 0, 0, 0, 0, 0, 0]
    assert ops.noise_key_row(2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1)[:4] == [0xFFFFFFFF] * 4
    for kw in (dict(seed=-1), dict(seed=2 ** 64), dict(image=-1), dict(image=2 ** 32), dict(draw=2 ** 32), dict(draw=1.0), dict(seed=True)):
        with pytest.raises(ValueError, match="noise_key_row"):
            ops.noise_key_row(**dict(dict(seed=1, image=0, draw=0), **kw))
    t = ops.noise_key_rows([ops.noise_key_row(2 ** 64 - 1, 1, 2), ops.noise_key_row(5, 0, 0, active=False)])
    assert t.dtype == torch.int32 and t.tolist() == [[-1, -1, 1, 2, 1, 0, 0, 0], [5, 0, 0, 0, 0, 0, 0, 0]]          # the words, as int32


def test_request_noise_rows_are_request_major():
    plan = N.RequestNoise([10, 20], 3)
    assert plan.rows == 6 and plan.pairs == [(10, 0), (10, 1), (10, 2), (20, 0), (20, 1), (20, 2)]
    assert plan.key_rows(4)[4] == ops.noise_key_row(20, 1, 4)
    part = plan.shard((2, 5))
    assert part.rows == 3 and part.pairs == [(10, 2), (20, 0), (20, 1)]
    with pytest.raises(ValueError):
        N.RequestNoise([], 1)


def test_draw_numbering():
    """draw 0: the initial noise; draw 1 + i: step index i of the FULL schedule, so strength < 1 starts at 1 + t_start"""
    assert N.INITIAL_DRAW == 0 and N.step_draw(0) == 1 and N.step_draw(50) == 51
    assert N.step_draws(0, 4) == [1, 2, 3, 4]
    steps, strength = 10, 0.6                       # the inpainting pipeline: init_steps = int(10 * 0.6) = 6, t_start = 4
    init_steps = min(int(steps * strength), steps)
    t_start = max(steps - init_steps, 0)
    assert N.step_draws(t_start, init_steps) == [5, 6, 7, 8, 9, 10]
    assert N.step_draws(t_start, init_steps) == N.step_draws(0, steps)[t_start:]          # the same draws at the same timesteps
    with pytest.raises(ValueError):
        N.step_draw(-1)


# ---- the DDIM row with eta ----
def test_ddim_row_eta_zero_is_todays_row():
    sch = _mk("ddim")
    sch.set_timesteps(20)
    sig = inspect.signature(S.ddim_row)
    assert list(sig.parameters) == ["scheduler", "t", "eta"] and sig.parameters["eta"].default == 0.0
    for t in sch.timesteps:
        a, b, c = S.ddim_row(sch, int(t)), S.ddim_row(sch, int(t), 0.0), S.ddim_row(sch, int(t), eta=0)
        for r in (b, c):
            assert all(getattr(a, k) == getattr(r, k) for k in S.SamplerRow.__slots__)
        assert a.z_n == 0.0
    with pytest.raises(ValueError, match="eta"):
        S.ddim_row(sch, int(sch.timesteps[0]), -0.1)


@pytest.mark.parametrize("eta", [0.3, 0.5, 1.0])
def test_ddim_row_eta_equals_the_oracle_step_in_float64(eta):
    """as tests/test_session_host.py::test_ddim_row_equals_the_oracle_step_in_float64, with ``variance_noise``: 1e-12 relative"""
    from oracle.ddim import DDIMOracle
    from tests.sampler_oracle import apply_row
    sch = _mk("ddim")
    sch.set_timesteps(20)
    orc = DDIMOracle()
    orc.alphas_cumprod = orc.alphas_cumprod.double()
    orc.final_alpha_cumprod = orc.final_alpha_cumprod.double()
    ts = orc.set_timesteps(20)
    gen = torch.Generator().manual_seed(3)
    z_row = z_orc = torch.randn(2, 64, 4, generator=gen, dtype=torch.float64)
    for t in ts:
        e = torch.randn(2, 64, 4, generator=gen, dtype=torch.float64)
        n = torch.randn(2, 64, 4, generator=gen, dtype=torch.float64)
        row = S.ddim_row(sch, int(t), eta)
        assert (row.m_x, row.m_e, row.keep, row.z_h, row.in_scale) == (0.0, 1.0, False, (), 1.0)
        assert abs(row.z_n - sch.sigma(int(t), eta)) <= 1e-15 and row.z_n > 0.0
        one = apply_row(row, z_orc, e, [], noise=n)
        z_orc = orc.step(e, t, z_orc, eta=eta, variance_noise=n)
        z_row = apply_row(row, z_row, e, [], noise=n)
        scale = z_orc.abs().max().item()
        assert (one - z_orc).abs().max().item() <= 1e-12 * scale, int(t)
        assert (z_row - z_orc).abs().max().item() <= 1e-12 * scale, int(t)


# ---- the session plan ----
def test_defaults_refuse_as_before():
    for fn, name in ((SessionPlan.__init__, "device_noise"), (check_scheduler, "device_noise"), (check_request, "device_noise")):
        p = inspect.signature(fn).parameters[name]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, fn
    with pytest.raises(NotImplementedError, match="Euler-ancestral"):
        SessionPlan(2, _mk("euler_a"))
    with pytest.raises(NotImplementedError, match="Euler-ancestral"):
        SessionPlan(2, _mk("euler_a"), device_noise=False)
    with pytest.raises(NotImplementedError, match="draws noise at every step"):
        check_scheduler(_mk("euler_a"))
    ok = dict(size=(128, 128), num_inference_steps=10, guidance_scale=7.5, slots=2)
    with pytest.raises(NotImplementedError, match="eta > 0: the stochastic DDIM step draws noise per step"):
        check_request(eta=0.5, **ok)
    with pytest.raises(ValueError, match="device_noise"):
        check_request(seed=3, **ok)
    with pytest.raises(NotImplementedError, match="eta > 0"):
        SessionPlan(2, _mk("ddim")).submit(10, eta=0.5)
    plain = SessionPlan(2, _mk("dpm"))
    plain.submit(3)
    plain.admit()
    st = plain.next_rows()
    assert st.noise is None and st.key_rows is None and not plain.noisy


def test_device_noise_accepts_what_it_should():
    check_scheduler(_mk("euler_a"), device_noise=True)
    with pytest.raises(NotImplementedError, match="UniPC"):          # the other refusals stay
        check_scheduler(_mk("unipc"), device_noise=True)
    ok = dict(size=(128, 128), num_inference_steps=10, guidance_scale=7.5, slots=2, device_noise=True)
    check_request(eta=0.5, scheduler=_mk("ddim"), seed=2 ** 64 - 1, **ok)
    check_request(eta=0.0, scheduler=_mk("dpm"), **ok)
    for name in ("dpm", "euler", "euler_a", "pndm"):
        with pytest.raises(ValueError, match="eta > 0 is the stochastic DDIM step"):
            check_request(eta=0.5, scheduler=_mk(name), **ok)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eta must be"):
            check_request(eta=bad, scheduler=_mk("ddim"), **ok)
    for bad in (-1, 2 ** 64, 1.5, "3"):
        with pytest.raises(ValueError, match="seed must be an int"):
            check_request(seed=bad, scheduler=_mk("ddim"), **ok)
    with pytest.raises(ValueError, match="eta > 0 is the stochastic DDIM step"):
        SessionPlan(2, _mk("dpm"), device_noise=True).submit(10, seed=1, eta=0.5)
    with pytest.raises(ValueError, match="seed"):
        SessionPlan(2, _mk("euler_a"), device_noise=True).submit(10)
    assert SessionPlan(2, _mk("euler_a"), device_noise=True).noisy and SessionPlan(2, _mk("ddim"), device_noise=True).noisy
    assert not SessionPlan(2, _mk("dpm"), device_noise=True).noisy


def _drive(plan, arrivals):
    """step the plan until it is empty -> the PlanStep of every step; ``arrivals`` = {step: [submit kwargs]}"""
    steps, k = [], 0
    while plan.running or plan.pending or any(s >= k for s in arrivals):
        for kw in arrivals.get(k, []):
            plan.submit(**kw)
        plan.admit()
        if plan.running:
            steps.append(plan.next_rows())
        k += 1
        assert k < 100
    return steps


@pytest.mark.parametrize("compact", [False, True])
def test_plan_keys_euler_ancestral(compact):
    """per step: (slot, seed, image, draw) of every running row, draw = 1 + the run's OWN step index, and the key row of every slot
    (inactive for a free one) -- by slot, compacting or not"""
    plan = SessionPlan(3, _mk("euler_a"), compact=compact, device_noise=True)
    steps = _drive(plan, {0: [dict(num_inference_steps=4, payload="a0", seed=100, image=0), dict(num_inference_steps=4, payload="a1", seed=100, image=1)],
                          2: [dict(num_inference_steps=3, payload="b", seed=2 ** 64 - 1, image=0)]})
    assert len(steps) == 5
    want = [[(0, 100, 0, 1), (1, 100, 1, 1)], [(0, 100, 0, 2), (1, 100, 1, 2)], [(0, 100, 0, 3), (1, 100, 1, 3), (2, 2 ** 64 - 1, 0, 1)],
            [(0, 100, 0, 4), (1, 100, 1, 4), (2, 2 ** 64 - 1, 0, 2)], [(2, 2 ** 64 - 1, 0, 3)]]
    assert [st.noise for st in steps] == want
    for st, keyed in zip(steps, want):
        assert len(st.key_rows) == 3
        by_slot = {s: ops.noise_key_row(seed, image, draw) for s, seed, image, draw in keyed}
        for s in range(3):
            assert st.key_rows[s] == by_slot.get(s, ops.noise_key_row(0, 0, 0, active=False))
    # the coefficient rows carry the sampler's z_n: the launch reads noise where the plan keyed it
    sch = _mk("euler_a")
    sch.set_timesteps(4)
    assert [steps[i].rows[0][8] for i in range(4)] == [sch.plan(i).z_n for i in range(4)]


def test_plan_keys_ddim_only_rows_with_eta():
    plan = SessionPlan(2, _mk("ddim"), device_noise=True)
    steps = _drive(plan, {0: [dict(num_inference_steps=3, payload="det"), dict(num_inference_steps=2, payload="sto", seed=9, eta=0.3)]})
    assert [st.noise for st in steps] == [[(1, 9, 0, 1)], [(1, 9, 0, 2)], []]
    assert steps[2].key_rows == [ops.noise_key_row(0, 0, 0, active=False)] * 2
    solo = _mk("ddim")
    solo.set_timesteps(2)
    for i, t in enumerate(int(t) for t in solo.timesteps):
        row = S.ddim_row(solo, t, 0.3)
        assert steps[i].rows[1][:13] == ops.sampler_coefs(0.0, 1.0, row.z_x, row.z_m, (), row.z_n, 1.0, 0.0, 1.0, -1)
        assert steps[i].rows[0][8] == 0.0 and steps[i].rows[1][8] > 0.0


# ---- the pipelines' switch, as far as the host goes ----
def test_pipeline_switch_and_seed_keyword():
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline as base
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline_controlnet as ctrl
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline_controlnet_inpainting as inp
    from imagdressing_amd.dressing_sd.pipelines import IMAGDressing_v1_pipeline_ipa_controlnet as ipa
    for mod in (base, ctrl, inp, ipa):
        pipe = object.__new__(mod.IMAGDressing_v1)
        assert not getattr(pipe, "_device_noise", False)                         # off by default
        with pytest.raises(ValueError, match=r"enable_device_noise\(\)"):
            pipe._request_noise({"seed": 3}, None, 1, 1)
        assert pipe._request_noise({}, torch.Generator().manual_seed(1), 1, 1) is None
        assert pipe.enable_device_noise() is pipe and pipe._device_noise is True
        assert pipe.disable_device_noise() is pipe and pipe._device_noise is False
        assert "seed" not in inspect.signature(mod.IMAGDressing_v1.__call__).parameters          # read from **kwargs, like variance_noise
    kw = dict(vae=None, reference_unet=None, unet=None, tokenizer=None, text_encoder=None, image_encoder=None, ImgProj=None)
    pipe = base.IMAGDressing_v1(scheduler=_mk("dpm"), **kw)
    pipe.unet = type("U", (), {"device": "cpu"})()
    pipe.enable_device_noise()
    plan = pipe._request_noise({"seed": [4, 5]}, None, 2, 2)
    assert pipe.last_seeds == [4, 5] and plan.pairs == [(4, 0), (4, 1), (5, 0), (5, 1)]
    assert pipe._request_noise({}, [torch.Generator().manual_seed(8), torch.Generator().manual_seed(9)], 2, 1).seeds == [8, 9]
    assert pipe.last_seeds == [8, 9]
    pipe._request_noise({}, None, 2, 1)
    assert len(pipe.last_seeds) == 2 and pipe.last_seeds[0] != pipe.last_seeds[1]
    with pytest.raises(ValueError, match="seed"):
        pipe._request_noise({"seed": 1.5}, None, 1, 1)
    for mod in (base, ctrl):
        assert inspect.signature(mod.IMAGDressing_v1.open_session).parameters["device_noise"].default is None
    # the session refusals with the switch off and device_noise unset are the pinned ones
    for name in ("euler_a",):
        with pytest.raises(NotImplementedError, match="open_session: scheduler"):
            base.IMAGDressing_v1(scheduler=_mk(name), **kw).open_session(slots=2, width=128, height=128)
        with pytest.raises(NotImplementedError, match="open_session: scheduler"):
            base.IMAGDressing_v1(scheduler=_mk(name), **kw).open_session(slots=2, width=128, height=128, device_noise=False)
