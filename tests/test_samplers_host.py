"""Host side of the samplers on the fused affine step (imagdressing_amd/scheduler.py: DPM-Solver++, Euler, Euler-ancestral, PNDM):
the float64 coefficient rows against the library-form restatements of tests/sampler_oracle.py, the anchors that tie each class to
known results (DDIM, exact integration of a constant data prediction, convergence orders on the Gaussian case, the Adams-Bashforth
weights), the history-slot bookkeeping, and the request-batched validation.  No GPU."""
import numpy as np
import pytest
import torch

from tests.sampler_oracle import DPMSolverOracle, EulerAncestralOracle, EulerOracle, PNDMOracle, apply_row

KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def _S():
    from imagdressing_amd import scheduler
    return scheduler


CASES = {
    "dpm2": (lambda S: S.DPMSolverMultistepScheduler(**KW), lambda: DPMSolverOracle()),
    "dpm1": (lambda S: S.DPMSolverMultistepScheduler(solver_order=1, **KW), lambda: DPMSolverOracle(solver_order=1)),
    "dpm2-karras": (lambda S: S.DPMSolverMultistepScheduler(use_karras_sigmas=True, **KW), lambda: DPMSolverOracle(use_karras_sigmas=True)),
    "dpm2-leading": (lambda S: S.DPMSolverMultistepScheduler(timestep_spacing="leading", steps_offset=1, **KW),
                     lambda: DPMSolverOracle(timestep_spacing="leading", steps_offset=1)),
    "euler": (lambda S: S.EulerDiscreteScheduler(**KW), lambda: EulerOracle()),
    "euler-leading": (lambda S: S.EulerDiscreteScheduler(timestep_spacing="leading", steps_offset=1, **KW),
                      lambda: EulerOracle(timestep_spacing="leading", steps_offset=1)),
    "euler-karras": (lambda S: S.EulerDiscreteScheduler(use_karras_sigmas=True, timestep_spacing="trailing", **KW),
                     lambda: EulerOracle(use_karras_sigmas=True, timestep_spacing="trailing")),
    "euler-ancestral": (lambda S: S.EulerAncestralDiscreteScheduler(**KW), lambda: EulerAncestralOracle()),
    "pndm": (lambda S: S.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **KW), lambda: PNDMOracle()),
    "pndm-alpha-one": (lambda S: S.PNDMScheduler(skip_prk_steps=True, set_alpha_to_one=True, timestep_spacing="trailing", **KW),
                       lambda: PNDMOracle(set_alpha_to_one=True, timestep_spacing="trailing")),
}


def _kernel_on_numpy(c, z, e, H, noise):
    """``imd_sampler_step`` for one block of ``ops.sampler_coefs`` values on numpy arrays: H = [K, ...] PHYSICAL slots, in place"""
    m = c[0] * z + c[1] * e
    zn = c[2] * z + c[3] * m + sum(c[4 + k] * H[k] for k in range(len(H))) + (c[8] * noise if noise is not None else 0.0)
    if int(c[12]) >= 0:
        H[int(c[12])] = m
    return zn


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("N", [10, 25])
def test_coefficient_rows_equal_the_library_form_restatement(name, N):
    """Whole runs with a nonlinear, state-dependent epsilon model that differs at every step (a history mistake shows): the rows of
    ``plan`` applied by hand (history by age) AND through ``SamplerHistory`` on physical slots, as the kernel does, against the
    tensor-form restatement, step for step, to rtol 1e-9."""
    S = _S()
    rng = np.random.default_rng(3)
    W = rng.standard_normal((6, 6)) * 0.4

    def eps_model(x, pos):
        return np.tanh(x @ W + 0.1 * pos) + 0.05 * x
    sch, orc = CASES[name][0](S), CASES[name][1]()
    assert not hasattr(sch, "step_guided") and sch.order == 1
    sch.set_timesteps(N)
    ts = orc.set_timesteps(N)
    assert sch.timesteps.dtype == ts.dtype and np.allclose(sch.timesteps.double().numpy(), ts.double().numpy(), rtol=0, atol=1e-9)
    assert sch.steps() == len(ts) == (N + 1 if name.startswith("pndm") else N)
    assert abs(sch.init_noise_sigma - orc.init_noise_sigma) <= 1e-12 * orc.init_noise_sigma
    if hasattr(orc, "sigmas"):
        assert np.allclose(sch.sigmas.double().numpy(), orc.sigmas, rtol=1e-6) and len(sch.sigmas) == N + 1
    x = rng.standard_normal((2, 6)) * sch.init_noise_sigma
    xo, xk = torch.from_numpy(x.copy()), x.copy()
    hist, ring, H = [], S.SamplerHistory(sch.history), np.zeros((sch.history, 2, 6))
    for i in range(sch.steps()):
        row = sch.plan(i)
        assert len(row.z_h) <= sch.history
        nz = rng.standard_normal((2, 6)) if sch.stochastic else None
        x_new = apply_row(row, x, eps_model(x * sch.input_scale(i), i), hist, noise=nz)
        xk = _kernel_on_numpy(ring.coefs(row), xk, eps_model(xk * sch.input_scale(i), i), H, nz)
        xo = orc.step(torch.from_numpy(eps_model(orc.scale_model_input(xo, ts[i]).numpy(), i)), ts[i], xo,
                      variance_noise=None if nz is None else torch.from_numpy(nz))
        assert abs(row.in_scale - sch.input_scale(i + 1)) < 1e-15 if i + 1 < sch.steps() else row.in_scale == 1.0
        x = x_new
        assert np.allclose(x, xo.numpy(), rtol=1e-9, atol=1e-10), (name, N, i, np.abs(x - xo.numpy()).max())
        assert np.allclose(xk, xo.numpy(), rtol=1e-9, atol=1e-10), (name, N, i, "physical slots")


def test_history_slots_never_move_data():
    """a new entry takes a free slot, then the oldest entry's; reading an entry that was never stored is an error"""
    S = _S()
    ring = S.SamplerHistory(3)
    stores = [int(ring.coefs(S.SamplerRow(keep=True))[12]) for _ in range(5)]
    assert stores == [0, 1, 2, 0, 1] and ring.slots == [1, 0, 2]
    c = ring.coefs(S.SamplerRow(z_h=(10.0, 20.0, 30.0), keep=False))
    assert c[4:8] == [20.0, 10.0, 30.0, 0.0] and c[12] == -1.0 and ring.slots == [1, 0, 2]
    c = ring.coefs(S.SamplerRow(z_h=(1.0,), keep=True))            # the slot that is overwritten may also be read, not here: oldest = 2
    assert c[4:8] == [0.0, 1.0, 0.0, 0.0] and c[12] == 2.0
    one = S.SamplerHistory(1)
    assert one.coefs(S.SamplerRow(keep=True))[12] == 0.0
    c = one.coefs(S.SamplerRow(z_h=(5.0,), keep=True))               # DPM-Solver++ 2M: slot 0 read and overwritten by one launch
    assert c[4] == 5.0 and c[12] == 0.0
    with pytest.raises(ValueError, match="history entry"):
        S.SamplerHistory(2).coefs(S.SamplerRow(z_h=(1.0,)))
    assert S.SamplerHistory(0).coefs(S.SamplerRow(keep=True))[12] == -1.0
    from imagdressing_amd import ops
    assert len(ops.sampler_coefs()) == ops.SAMPLER_COEFS == 13
    with pytest.raises(Exception, match="history coefficients"):
        ops.sampler_coefs(z_h=[1.0] * 5)


def _alpha_sigma(sig):
    a = 1.0 / np.sqrt(sig * sig + 1.0)
    return a, sig * a


def test_dpm_order1_is_ddim_and_euler_is_ddim_in_sigma_space():
    """On one sigma grid: DPM-Solver++ of order 1 takes DDIM's (eta = 0) step, z' = a' x0 + s' e, at every step, and the Euler
    trajectory divided by sqrt(sigma^2 + 1) is the DDIM trajectory."""
    S = _S()
    rng = np.random.default_rng(0)
    W = rng.standard_normal((5, 5)) * 0.3
    N = 12
    dpm = S.DPMSolverMultistepScheduler(solver_order=1, **KW); dpm.set_timesteps(N)
    sig = dpm._sig
    x = rng.standard_normal(5)
    xd = x.copy()
    hist = []
    for i in range(N):
        a, s = _alpha_sigma(sig[i]); a2, s2 = _alpha_sigma(sig[i + 1])
        e = np.tanh(xd @ W + i)
        x = apply_row(dpm.plan(i), x, np.tanh(x @ W + i), hist)
        xd = a2 * (xd - s * e) / a + s2 * e
        assert np.allclose(x, xd, rtol=1e-12, atol=1e-12), i
    # Euler on the grid of its own schedule (fractional timesteps): sigma-space sample / sqrt(sigma^2 + 1) == DDIM sample
    eu = S.EulerDiscreteScheduler(**KW); eu.set_timesteps(N)
    sig = eu._sig
    z = rng.standard_normal(5) * eu.init_noise_sigma
    xd = z * _alpha_sigma(sig[0])[0]
    for i in range(N):
        a, s = _alpha_sigma(sig[i]); a2, s2 = _alpha_sigma(sig[i + 1])
        assert abs(eu.input_scale(i) - a) < 1e-15
        z = apply_row(eu.plan(i), z, np.tanh((z * eu.input_scale(i)) @ W + i), [])
        e = np.tanh(xd @ W + i)
        xd = a2 * (xd - s * e) / a + s2 * e
        assert np.allclose(z * a2, xd, rtol=1e-12, atol=1e-13), (i, np.abs(z * a2 - xd).max())
    assert eu.plan(N - 1).in_scale == 1.0 and eu.plan(N - 1, blend=True).b_noise == 0.0        # the run ends at sigma = 0


@pytest.mark.parametrize("order", [1, 2])
def test_dpm_integrates_a_constant_data_prediction_exactly(order):
    """a model whose data prediction is the constant c: every difference in the second-order term vanishes, each step lands on
    (s_t / s_0)(x_0 - a_0 c) + a_t c, and the last step (sigma = 0) returns c itself"""
    S = _S()
    rng = np.random.default_rng(1)
    c, x0 = rng.standard_normal(5), rng.standard_normal(5)
    sch = S.DPMSolverMultistepScheduler(solver_order=order, **KW); sch.set_timesteps(12)
    a0, s0 = _alpha_sigma(sch._sig[0])
    x, hist = x0.copy(), []
    for i in range(12):
        a, s = _alpha_sigma(sch._sig[i])
        x = apply_row(sch.plan(i), x, (x - a * c) / s, hist)
        at, st = _alpha_sigma(sch._sig[i + 1])
        assert np.allclose(x, st / s0 * (x0 - a0 * c) + at * c, rtol=1e-9, atol=1e-9), i
    assert np.allclose(x, c, rtol=1e-9, atol=1e-9)


def test_convergence_orders_on_the_gaussian_case():
    """The case of test_unipc_convergence_orders_on_the_gaussian_case (data ~ N(0, 0.7^2), closed-form probability-flow solution, the
    smooth first half of a 40- against an 80-step schedule): the global error halves for Euler and DPM-Solver++ 1 and quarters for
    DPM-Solver++ 2M."""
    S = _S()
    sd = 0.7

    def model(x, a, s):                       # x in alpha space
        return (x - a * (a * sd * sd / (a * a * sd * sd + s * s)) * x) / s

    def err(mk, N, euler):
        sch = mk(); sch.set_timesteps(N)
        x0 = np.array([1.3, -0.4, 2.0])
        a0, s0 = _alpha_sigma(sch._sig[0])
        z = x0 / a0 if euler else x0.copy()
        hist = []
        for i in range(N // 2):
            a, s = _alpha_sigma(sch._sig[i])
            z = apply_row(sch.plan(i), z, model(z * sch.input_scale(i), a, s), hist)
        a1, s1 = _alpha_sigma(sch._sig[N // 2])
        exact = x0 * np.sqrt(a1 * a1 * sd * sd + s1 * s1) / np.sqrt(a0 * a0 * sd * sd + s0 * s0)
        got = z * a1 if euler else z
        return np.abs(got - exact).max() / np.abs(exact).max()
    for mk, euler, rate in ((lambda: S.EulerDiscreteScheduler(**KW), True, 1),
                            (lambda: S.DPMSolverMultistepScheduler(solver_order=1, **KW), False, 1),
                            (lambda: S.DPMSolverMultistepScheduler(solver_order=2, **KW), False, 2)):
        e40, e80 = err(mk, 40, euler), err(mk, 80, euler)
        print(f"gaussian case: rate {rate}: e40 / e80 = {e40 / e80:.3f}")
        assert 2 ** rate * 0.6 < e40 / e80 < 2 ** rate * 1.6, (rate, e40, e80)


def test_pndm_timesteps_repeat_the_second_entry_and_weights_are_adams_bashforth():
    S = _S()
    sch = S.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **KW)      # SD1.5's scheduler_config.json
    sch.set_timesteps(10)
    ts = [int(t) for t in sch.timesteps]
    assert ts == [901, 801, 801, 701, 601, 501, 401, 301, 201, 101, 1] and sch.steps() == 11
    want = {0: [1.0], 1: [0.5, 0.5], 2: [3 / 2, -1 / 2], 3: [23 / 12, -16 / 12, 5 / 12], 4: [55 / 24, -59 / 24, 37 / 24, -9 / 24]}
    for i in range(11):
        w = want[min(i, 4)]
        assert np.allclose(S.PNDMScheduler.plms_weights(i), w, rtol=1e-15) and abs(sum(w) - 1.0) < 1e-15
        row = sch.plan(i)
        assert (row.m_x, row.m_e) == (0.0, 1.0)
        c_s, c_e = sch._transfer(*sch._levels(i, 0))
        if i == 1:
            # the repeated timestep: the step from 901 to 801 again, from the SAVED sample z_0 = (z_1 + c_e e_0) / c_s with the mean of
            # the two epsilons: z' = z_1 - (c_e / 2) e_1 + (c_e / 2) e_0, and e_1 is not kept
            assert sch._levels(1, 0) == sch._levels(0, 0) == (901, 801) and not row.keep
            assert np.allclose([row.z_x, row.z_m, row.z_h[0]], [1.0, -c_e / 2, c_e / 2], rtol=1e-12)
        else:
            assert row.keep and row.z_x == c_s
            assert np.allclose([row.z_m] + list(row.z_h), [-c_e * x for x in w], rtol=1e-15)
    a, ap = float(sch._ac[901]), float(sch._ac[801])
    assert np.allclose(sch._transfer(901, 801), ((ap / a) ** 0.5, (ap - a) / (a * (1 - ap) ** 0.5 + (a * (1 - a) * ap) ** 0.5)), rtol=1e-15)
    assert sch._levels(10, 0) == (1, -99)                                # below 0: the final alpha, alphas_cumprod[0] unless set_alpha_to_one
    assert np.isclose(sch._transfer(1, -99)[0], (float(sch._ac[0]) / float(sch._ac[1])) ** 0.5, rtol=1e-15)


def test_blend_coefficients_are_the_schedulers_own_add_noise():
    """``plan(..., blend=True)``: b_img z_img + b_noise n is ``add_noise`` at the level the step lands on; the last step's target is the
    clean image latent"""
    S = _S()
    x0, n = torch.tensor([0.3, -1.2]), torch.tensor([0.7, 0.1])
    for name in ("dpm2", "dpm2-karras", "euler", "euler-ancestral", "pndm"):
        sch = CASES[name][0](S)
        sch.set_timesteps(8)
        steps = sch.steps()
        for start in (0, 3):
            for i in range(steps - start):
                row = sch.plan(i, start, blend=True)
                if start + i == steps - 1:
                    assert (row.b_img, row.b_noise) == (1.0, 0.0)
                else:
                    want = sch.add_noise(x0, n, sch.timesteps[start + i + 1])
                    assert torch.allclose(row.b_img * x0.double() + row.b_noise * n.double(), want.double(), rtol=1e-6), (name, start, i)
            assert (sch.plan(0, start).b_img, sch.plan(0, start).b_noise) == (1.0, 0.0)


def test_euler_surface():
    S = _S()
    sch = S.EulerDiscreteScheduler(**KW)
    sch.set_timesteps(6)
    assert sch.timesteps.dtype == torch.float64 and [round(float(t), 1) for t in sch.timesteps] == [999.0, 799.2, 599.4, 399.6, 199.8, 0.0]
    sig999 = ((1 - float(sch._ac[999])) / float(sch._ac[999])) ** 0.5
    assert abs(sch.init_noise_sigma - sig999) < 1e-12 and float(sch.sigmas[-1]) == 0.0
    x = torch.ones(1, 4, 2, 2)
    assert torch.allclose(sch.scale_model_input(x, sch.timesteps[2]), x / (float(sch.sigmas[2]) ** 2 + 1) ** 0.5, rtol=1e-6)
    assert torch.allclose(sch.add_noise(x, 2 * x, sch.timesteps[1]), x + float(sch.sigmas[1]) * 2 * x, rtol=1e-6)
    lead = S.EulerDiscreteScheduler(timestep_spacing="leading", steps_offset=1, **KW)
    lead.set_timesteps(10)
    assert [float(t) for t in lead.timesteps] == [901.0, 801.0, 701.0, 601.0, 501.0, 401.0, 301.0, 201.0, 101.0, 1.0]
    assert abs(lead.init_noise_sigma - (float(lead._sig[0]) ** 2 + 1) ** 0.5) < 1e-12
    anc = S.EulerAncestralDiscreteScheduler(**KW)
    anc.set_timesteps(6)
    row = anc.plan(2)
    s, t = anc._sig[2], anc._sig[3]
    up = (t * t * (s * s - t * t) / (s * s)) ** 0.5
    assert anc.stochastic and np.allclose([row.z_n, row.z_m], [up, (t * t - up * up) ** 0.5 - s], rtol=1e-12)
    assert anc.plan(5).z_n == 0.0 and not sch.stochastic


@pytest.mark.parametrize("cls,kw,word", [
    ("DPMSolverMultistepScheduler", dict(algorithm_type="sde-dpmsolver++"), "algorithm_type"),
    ("DPMSolverMultistepScheduler", dict(solver_type="heun"), "solver_type"),
    ("DPMSolverMultistepScheduler", dict(solver_order=3), "solver_order"),
    ("DPMSolverMultistepScheduler", dict(thresholding=True), "thresholding"),
    ("DPMSolverMultistepScheduler", dict(prediction_type="v_prediction"), "prediction_type"),
    ("EulerDiscreteScheduler", dict(interpolation_type="log_linear"), "interpolation_type"),
    ("EulerDiscreteScheduler", dict(prediction_type="sample"), "prediction_type"),
    ("EulerAncestralDiscreteScheduler", dict(use_karras_sigmas=True), "use_karras_sigmas"),
    ("PNDMScheduler", dict(skip_prk_steps=False), "skip_prk_steps"),
    ("PNDMScheduler", dict(skip_prk_steps=True, beta_schedule="squaredcos_cap_v2"), "beta_schedule"),
    ("PNDMScheduler", dict(skip_prk_steps=True, timestep_spacing="karras"), "timestep_spacing"),
])
def test_unsupported_options_name_themselves(cls, kw, word):
    with pytest.raises(NotImplementedError, match=word):
        getattr(_S(), cls)(**kw)


def test_compat_package_exports_the_classes():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_compat_diffusers_for_test", os.path.join(root, "compat", "diffusers", "__init__.py"))
    src = open(spec.origin).read()
    S = _S()
    for name in ("DPMSolverMultistepScheduler", "EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler", "PNDMScheduler"):
        assert name in src.split("__all__")[1] and f"{name}" in src.split("__all__")[0]
        cls = getattr(S, name)
        for attr in ("set_timesteps", "scale_model_input", "step", "add_noise", "plan"):
            assert callable(getattr(cls, attr)), (name, attr)
        sch = cls(**dict(KW, skip_prk_steps=True) if name == "PNDMScheduler" else KW)
        assert sch.order == 1 and isinstance(sch.config, dict) and sch.config["num_train_timesteps"] == 1000
        assert len(sch.timesteps) == 1000 and float(sch.init_noise_sigma) >= 1.0


# ---- request-batched calls: differing guidance is accepted (the per-row array feeds imd_sampler_step) ----
NEW = ["DPMSolverMultistepScheduler", "EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler", "PNDMScheduler"]


def _new_sched(name):
    return getattr(_S(), name)(**dict(KW, skip_prk_steps=True) if name == "PNDMScheduler" else KW)


@pytest.mark.parametrize("name", NEW)
def test_request_count_and_denoise_accept_differing_guidance(name):
    from imagdressing_amd.dressing_sd.pipelines._base import request_count
    from tests.test_multi_request import _kw, _pipe
    sch = _new_sched(name)
    assert request_count(dict(prompt_embeds=torch.zeros(3, 77, 64), guidance_scale=[5.0, 7.5, 9.0]), scheduler=sch) == 3
    pipe = _pipe("base")
    pipe.scheduler = sch
    # validation passes and the call goes on to the (stand-in) garment UNet ...
    with pytest.raises(AssertionError, match="reached the model"):
        pipe(**_kw(guidance_scale=[5.0, 7.5, 9.0]))
    # ... and ``denoise`` itself gets as far as the first UNet forward: no refusal of the guidance, of the blend or of anything else
    lat = torch.zeros(3, 4, 16, 16)
    for inpaint in (None, dict(mask=torch.ones(1, 1, 16, 16), image_latents=lat[:1], noise=lat)):
        with pytest.raises(AssertionError, match="reached the model"):
            pipe.denoise(latents=lat, prompt_embeds=torch.zeros(3, 77, 64), negative_prompt_embeds=torch.zeros(3, 77, 64),
                         sa_hidden_states={}, num_inference_steps=4, guidance_scale=[5.0, 7.5, 9.0], requests=3, inpaint=inpaint)
    # UniPC's refusal stands
    with pytest.raises(ValueError, match="UniPC"):
        _pipe("base", unipc=True)(**_kw(guidance_scale=[5.0, 7.5, 9.0]))
