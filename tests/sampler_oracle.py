"""Restatements of diffusers==0.24.0 ``DPMSolverMultistepScheduler`` (dpmsolver++, midpoint, orders 1 / 2), ``EulerDiscreteScheduler``,
``EulerAncestralDiscreteScheduler`` and ``PNDMScheduler`` (``skip_prk_steps``) -- TEST INFRASTRUCTURE; **parity unpinned**: third-party
arithmetic, un-vendored, no vectors in the reference (tools/check_against_diffusers.py compares them where the library exists).

Written in the LIBRARY'S OWN FORM -- ``convert_model_output`` / ``dpm_solver_first_order_update`` /
``multistep_dpm_solver_second_order_update``, ``step_plms`` / ``_get_prev_sample`` with its ``ets`` list and saved ``cur_sample``,
the sigma-space ``step`` of the Euler classes -- operating on tensors in float64, with their own schedule code, so that they are an
independent code path from ``imagdressing_amd/scheduler.py``, which reduces every step to one row of coefficients for the fused
kernel.  Two deliberate choices shared with that module (the issue that introduced the samplers sets them): the DPM-Solver++ schedule
ends at sigma = 0 (so its last step is first order), and timesteps are kept in float64.

Duck-compatible with the ``scheduler`` argument of ``oracle.pipeline.denoise``: ``set_timesteps(n)`` returns the timesteps,
``scale_model_input``, ``step(eps, t, sample, **kw)`` returns the next sample in ``sample``'s dtype, ``add_noise``.

``apply_row`` is the by-hand application of one ``scheduler.SamplerRow`` that the tests compare the device against."""
from __future__ import annotations

import numpy as np
import torch


def apply_row(row, z, e, hist, noise=None, blend=None):
    """One ``SamplerRow`` applied to arrays / float64 tensors: ``hist`` = list of earlier m, NEWEST FIRST (updated in place when the
    row keeps its m); ``blend`` = (mask, z_img, blend_noise).  -> z'"""
    m = row.m_x * z + row.m_e * e
    zn = row.z_x * z + row.z_m * m
    for c, h in zip(row.z_h, hist):
        zn = zn + c * h
    assert len(row.z_h) <= len(hist) or all(c == 0.0 for c in row.z_h[len(hist):])
    if noise is not None:
        zn = zn + row.z_n * noise
    if blend is not None:
        mask, z_img, bn = blend
        zn = (1 - mask) * (row.b_img * z_img + row.b_noise * bn) + mask * zn
    if row.keep:
        hist.insert(0, m)
    return zn


def _alphas_cumprod(T, beta_start, beta_end):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float64) ** 2        # scaled_linear
    return torch.cumprod(1.0 - betas, dim=0).numpy()


def _convert_to_karras(in_sigmas, n, rho=7.0):
    sigma_min, sigma_max = in_sigmas[-1], in_sigmas[0]
    ramp = np.linspace(0, 1, n)
    min_inv_rho, max_inv_rho = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
    return (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** rho


def _sigma_to_t(sigma, log_sigmas):
    log_sigma = np.log(sigma)
    dists = log_sigma - log_sigmas[:, np.newaxis]
    low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
    high_idx = low_idx + 1
    low, high = log_sigmas[low_idx], log_sigmas[high_idx]
    w = np.clip((low - log_sigma) / (low - high), 0, 1)
    return ((1 - w) * low_idx + w * high_idx).reshape(sigma.shape)


class _Base:
    init_noise_sigma = 1.0
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012):
        self.T = num_train_timesteps
        self.alphas_cumprod = _alphas_cumprod(num_train_timesteps, beta_start, beta_end)
        self.step_index = None

    def _index(self, t):
        if self.step_index is None:                      # the library's _init_step_index: first call of a run
            self.step_index = int(np.argmin(np.abs(self.timesteps.double().numpy() - float(t))))
        return self.step_index

    def scale_model_input(self, x, t=None):
        return x

    def add_noise(self, x0, noise, t):
        a = self.alphas_cumprod[int(t)]
        return a ** 0.5 * x0 + (1 - a) ** 0.5 * noise


class DPMSolverOracle(_Base):
    def __init__(self, solver_order=2, lower_order_final=True, use_karras_sigmas=False, timestep_spacing="linspace", steps_offset=0, **kw):
        super().__init__(**kw)
        self.solver_order, self.lower_order_final, self.use_karras_sigmas = solver_order, lower_order_final, use_karras_sigmas
        self.timestep_spacing, self.steps_offset = timestep_spacing, steps_offset

    def set_timesteps(self, n):
        T = self.T
        if self.timestep_spacing == "linspace":
            timesteps = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif self.timestep_spacing == "leading":
            timesteps = (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + self.steps_offset
        else:
            timesteps = (np.arange(T, 0, -T / n).round() - 1).astype(np.int64)
        sigmas = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5
        if self.use_karras_sigmas:
            log_sigmas = np.log(sigmas)
            sigmas = _convert_to_karras(np.flip(sigmas).copy(), n)
            timesteps = np.array([_sigma_to_t(s, log_sigmas) for s in sigmas]).round().astype(np.int64)
        else:
            sigmas = np.interp(timesteps, np.arange(0, len(sigmas)), sigmas)
        self.sigmas = np.concatenate([sigmas, [0.0]])                       # final sigma 0
        self.timesteps = torch.from_numpy(timesteps)
        self.num_inference_steps = n
        self.model_outputs = [None] * self.solver_order
        self.lower_order_nums = 0
        self.step_index = None
        return self.timesteps

    @staticmethod
    def _sigma_to_alpha_sigma_t(sigma):
        alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
        return alpha_t, sigma * alpha_t

    def convert_model_output(self, eps, sample):
        alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(self.sigmas[self.step_index])
        return (sample - sigma_t * eps) / alpha_t

    def _lambdas(self, *idx):
        out = []
        with np.errstate(divide="ignore"):
            for i in idx:
                a, s = self._sigma_to_alpha_sigma_t(self.sigmas[i])
                out.append((a, s, np.log(a) - np.log(s)))
        return out

    def dpm_solver_first_order_update(self, model_output, sample):
        (alpha_t, sigma_t, lambda_t), (alpha_s, sigma_s, lambda_s) = self._lambdas(self.step_index + 1, self.step_index)
        h = lambda_t - lambda_s
        return (sigma_t / sigma_s) * sample - (alpha_t * (np.exp(-h) - 1.0)) * model_output

    def multistep_dpm_solver_second_order_update(self, model_output_list, sample):
        (alpha_t, sigma_t, lambda_t), (alpha_s0, sigma_s0, lambda_s0), (_, _, lambda_s1) = self._lambdas(
            self.step_index + 1, self.step_index, self.step_index - 1)
        m0, m1 = model_output_list[-1], model_output_list[-2]
        h, h_0 = lambda_t - lambda_s0, lambda_s0 - lambda_s1
        r0 = h_0 / h
        D0, D1 = m0, (1.0 / r0) * (m0 - m1)
        return (sigma_t / sigma_s0) * sample - (alpha_t * (np.exp(-h) - 1.0)) * D0 - 0.5 * (alpha_t * (np.exp(-h) - 1.0)) * D1

    def step(self, eps, t, sample, **unused):
        out_dtype = sample.dtype
        eps, sample = eps.double(), sample.double()
        self._index(t)
        # the library: lower_order_final and fewer than 15 steps -- or a schedule that ends at sigma = 0
        lower_order_final = self.step_index == len(self.timesteps) - 1
        m = self.convert_model_output(eps, sample)
        self.model_outputs = self.model_outputs[1:] + [m]
        if self.solver_order == 1 or self.lower_order_nums < 1 or lower_order_final:
            prev = self.dpm_solver_first_order_update(m, sample)
        else:
            prev = self.multistep_dpm_solver_second_order_update(self.model_outputs, sample)
        if self.lower_order_nums < self.solver_order:
            self.lower_order_nums += 1
        self.step_index += 1
        return prev.to(out_dtype)


class EulerOracle(_Base):
    def __init__(self, use_karras_sigmas=False, timestep_spacing="linspace", steps_offset=0, **kw):
        super().__init__(**kw)
        self.use_karras_sigmas, self.timestep_spacing, self.steps_offset = use_karras_sigmas, timestep_spacing, steps_offset

    def set_timesteps(self, n):
        T = self.T
        if self.timestep_spacing == "linspace":
            timesteps = np.linspace(0, T - 1, n, dtype=np.float64)[::-1].copy()
        elif self.timestep_spacing == "leading":
            timesteps = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float64) + self.steps_offset
        else:
            timesteps = (np.arange(T, 0, -T / n)).round().astype(np.float64) - 1
        sigmas = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5
        log_sigmas = np.log(sigmas)
        sigmas = np.interp(timesteps, np.arange(0, len(sigmas)), sigmas)
        if self.use_karras_sigmas:
            sigmas = _convert_to_karras(sigmas, n)
            timesteps = np.array([_sigma_to_t(s, log_sigmas) for s in sigmas])
        self.sigmas = np.concatenate([sigmas, [0.0]])
        self.timesteps = torch.from_numpy(timesteps)
        smax = self.sigmas.max()
        self.init_noise_sigma = float(smax if self.timestep_spacing in ("linspace", "trailing") else (smax ** 2 + 1) ** 0.5)
        self.num_inference_steps = n
        self.step_index = None
        return self.timesteps

    def scale_model_input(self, x, t=None):
        sigma = self.sigmas[self._index(t)]
        return x / ((sigma ** 2 + 1) ** 0.5)

    def step(self, eps, t, sample, **unused):
        out_dtype = sample.dtype
        eps, sample = eps.double(), sample.double()
        sigma = self.sigmas[self._index(t)]
        pred_original_sample = sample - sigma * eps                    # (s_churn = 0: gamma = 0, sigma_hat = sigma)
        derivative = (sample - pred_original_sample) / sigma
        dt = self.sigmas[self.step_index + 1] - sigma
        self.step_index += 1
        return (sample + derivative * dt).to(out_dtype)

    def add_noise(self, x0, noise, t):
        i = int(np.argmin(np.abs(self.timesteps.double().numpy() - float(t))))
        return x0 + self.sigmas[i] * noise


class EulerAncestralOracle(EulerOracle):
    def step(self, eps, t, sample, variance_noise=None, **unused):
        out_dtype = sample.dtype
        eps, sample = eps.double(), sample.double()
        sigma = self.sigmas[self._index(t)]
        pred_original_sample = sample - sigma * eps
        sigma_from, sigma_to = sigma, self.sigmas[self.step_index + 1]
        sigma_up = (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5
        sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
        derivative = (sample - pred_original_sample) / sigma
        dt = sigma_down - sigma
        self.step_index += 1
        return (sample + derivative * dt + variance_noise.double() * sigma_up).to(out_dtype)


class PNDMOracle(_Base):
    def __init__(self, set_alpha_to_one=False, timestep_spacing="leading", steps_offset=1, **kw):
        super().__init__(**kw)
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else self.alphas_cumprod[0]
        self.timestep_spacing, self.steps_offset = timestep_spacing, steps_offset

    def set_timesteps(self, n):
        T = self.T
        if self.timestep_spacing == "linspace":
            _timesteps = np.linspace(0, T - 1, n).round().astype(np.int64)
        elif self.timestep_spacing == "leading":
            _timesteps = (np.arange(0, n) * (T // n)).round().astype(np.int64) + self.steps_offset
        else:
            _timesteps = np.round(np.arange(T, 0, -T / n))[::-1].astype(np.int64) - 1
        # skip_prk_steps: no Runge-Kutta timesteps; the PLMS list repeats the second entry
        self.timesteps = torch.from_numpy(np.concatenate([_timesteps[:-1], _timesteps[-2:-1], _timesteps[-1:]])[::-1].copy())
        self.num_inference_steps = n
        self.ets, self.counter, self.cur_sample = [], 0, None
        return self.timesteps

    def _get_prev_sample(self, sample, timestep, prev_timestep, model_output):
        alpha_prod_t = self.alphas_cumprod[timestep]
        alpha_prod_t_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        beta_prod_t, beta_prod_t_prev = 1 - alpha_prod_t, 1 - alpha_prod_t_prev
        sample_coeff = (alpha_prod_t_prev / alpha_prod_t) ** 0.5
        model_output_denom_coeff = alpha_prod_t * beta_prod_t_prev ** 0.5 + (alpha_prod_t * beta_prod_t * alpha_prod_t_prev) ** 0.5
        return sample_coeff * sample - (alpha_prod_t_prev - alpha_prod_t) * model_output / model_output_denom_coeff

    def step(self, eps, t, sample, **unused):                    # step_plms
        out_dtype = sample.dtype
        model_output, sample = eps.double(), sample.double()
        timestep = int(t)
        prev_timestep = timestep - self.T // self.num_inference_steps
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(model_output)
        else:
            prev_timestep = timestep
            timestep = timestep + self.T // self.num_inference_steps
        if len(self.ets) == 1 and self.counter == 0:
            self.cur_sample = sample
        elif len(self.ets) == 1 and self.counter == 1:
            model_output = (model_output + self.ets[-1]) / 2
            sample = self.cur_sample
            self.cur_sample = None
        elif len(self.ets) == 2:
            model_output = (3 * self.ets[-1] - self.ets[-2]) / 2
        elif len(self.ets) == 3:
            model_output = (23 * self.ets[-1] - 16 * self.ets[-2] + 5 * self.ets[-3]) / 12
        else:
            model_output = (1 / 24) * (55 * self.ets[-1] - 59 * self.ets[-2] + 37 * self.ets[-3] - 9 * self.ets[-4])
        prev_sample = self._get_prev_sample(sample, timestep, prev_timestep, model_output)
        self.counter += 1
        return prev_sample.to(out_dtype)
