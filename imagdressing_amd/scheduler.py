"""DDIM scheduler with the surface of diffusers==0.24.0 ``DDIMScheduler`` that the reference uses
(constructed at /root/reference/inference_IMAGdressing.py:119-127; ``set_timesteps``
IMAGDressing_v1_pipeline.py:386, ``scale_model_input`` :486, ``step`` :530, ``add_noise``
..._pipeline_controlnet_inpainting.py:496).  The per-step arithmetic runs in the fused HIP
``ddim_cfg_step`` kernel; this class owns the schedule (host-side scalars, fp32 like diffusers)."""
from __future__ import annotations

import numpy as np
import torch

from . import ops


class DDIMScheduler:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 clip_sample=True, set_alpha_to_one=True, steps_offset=0, prediction_type="epsilon",
                 timestep_spacing="leading", **unused):
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise NotImplementedError(f"beta_schedule {beta_schedule!r}")
        if clip_sample:
            raise NotImplementedError("clip_sample=True is not used by IMAGDressing (inference_IMAGdressing.py:124)")
        if prediction_type != "epsilon" or timestep_spacing != "leading":
            raise NotImplementedError("only epsilon prediction with leading spacing (the reference's inference config)")
        self.num_train_timesteps = num_train_timesteps
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.steps_offset = steps_offset
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self.config = dict(num_train_timesteps=num_train_timesteps, steps_offset=steps_offset)

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.steps_offset
        self.timesteps = torch.from_numpy(ts)        # kept on the host: the loop reads them as Python ints

    def scale_model_input(self, sample, timestep=None):
        return sample

    # ---- host-side coefficients for the fused kernel ----
    def alpha(self, t: int) -> float:
        return float(self.alphas_cumprod[int(t)])

    def alpha_prev(self, t: int) -> float:
        prev = int(t) - self.num_train_timesteps // self.num_inference_steps
        return float(self.alphas_cumprod[prev]) if prev >= 0 else float(self.final_alpha_cumprod)

    def sigma(self, t: int, eta: float) -> float:
        """std_dev_t of diffusers' ``DDIMScheduler.step``: eta * sqrt(_get_variance(t, prev_t))."""
        a_t, a_prev = self.alpha(t), self.alpha_prev(t)
        return float(eta) * ((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)) ** 0.5

    # ---- diffusers-compatible tensor API (NCHW in / out), thin over the same kernel ----
    def step(self, model_output, timestep, sample, eta: float = 0.0, use_clipped_model_output: bool = False, generator=None,
             variance_noise=None, return_dict: bool = False, **unused):
        """``eta`` > 0: the stochastic step; the noise is ``variance_noise`` or, like diffusers, a standard-normal draw of
        ``model_output``'s shape and dtype from ``generator`` (the reference forwards both through ``prepare_extra_step_kwargs``,
        IMAGDressing_v1_pipeline.py:102-119)."""
        if use_clipped_model_output:
            raise NotImplementedError("use_clipped_model_output (only meaningful with clip_sample=True, which the reference turns off)")
        B, Cc, H, W = sample.shape
        z = sample.float().permute(0, 2, 3, 1).reshape(B, H * W, Cc).contiguous()
        e = model_output.float().permute(0, 2, 3, 1).reshape(B, H * W, Cc).contiguous()
        kw = {}
        if eta > 0:
            if variance_noise is None:
                from .dressing_sd.pipelines._base import randn_tensor
                variance_noise = randn_tensor(tuple(model_output.shape), generator=generator, device=model_output.device, dtype=model_output.dtype)
            kw = dict(var_noise=variance_noise.to(sample.device).float().permute(0, 2, 3, 1).reshape(B, H * W, Cc).contiguous(),
                      sigma=self.sigma(timestep, eta))
        ops.ddim_cfg_step(z, torch.cat([e, e]), None, guidance=1.0, a_t=self.alpha(timestep), a_prev=self.alpha_prev(timestep), **kw)
        out = z.view(B, H, W, Cc).permute(0, 3, 1, 2).to(sample.dtype)
        return (out,)

    def add_noise(self, original_samples, noise, timesteps):
        a = self.alpha(int(torch.as_tensor(timesteps).reshape(-1)[0]))
        return a ** 0.5 * original_samples + (1 - a) ** 0.5 * noise


class UniPCMultistepScheduler:
    """UniPC (unified predictor-corrector, Zhao et al. 2023) multistep sampler with the surface of diffusers==0.24.0
    ``UniPCMultistepScheduler`` -- the sampler the IMAGDressing paper reports (supplementary p.1) and that
    /root/reference/app.py:28 imports; the inference scripts themselves construct DDIM.  SURVEY.md section 8f rank 4.

    diffusers is un-vendored and not installable here, and the reference holds no vectors for it: **parity unpinned**.  The
    restatement follows the paper's B(h) = e^h - 1 ("bh2") variant in data-prediction form with the library's defaults
    (solver_order 2, lower_order_final, corrector on every step after the first, "linspace" timestep spacing, final step to
    the sigma of training timestep 0) and is anchored by properties tested in tests/: order 1 without corrector == DDIM
    (eta = 0); a constant data prediction is integrated exactly; on the analytically solvable Gaussian case the error falls
    with the solver order.

    The coefficients of every update depend only on the timestep history, so they are computed on the host in float64
    (`x0_terms`, `corrector_terms`, `predictor_terms` return (coefficient, tensor-name) lists) and applied to the fp32
    latents by ONE `imd_lincomb` launch each: x0 prediction + classifier-free guidance, corrector, predictor.

    `fused_step=True` / `enable_fused_step()` (off by default; off, nothing above changes): the same three updates as ONE
    `imd_unipc_step` launch per step -- `plan_fused` states a step as a :class:`UniPCRow` from the same term lists and the
    same order bookkeeping, :class:`UniPCHistory` lays the x0 predictions and `last_sample` into `solver_order + 1` planes
    of a device buffer -- which gives the pipelines per-request guidance, the inpainting blend, step-graph replay and
    denoising sessions for this class.  The bits then differ from the three-launch route at fp32-rounding level."""

    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", solver_order=2,
                 prediction_type="epsilon", predict_x0=True, solver_type="bh2", lower_order_final=True, disable_corrector=(),
                 timestep_spacing="linspace", steps_offset=0, thresholding=False, fused_step=False, **unused):
        if beta_schedule == "scaled_linear":
            betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=np.float64) ** 2
        elif beta_schedule == "linear":
            betas = np.linspace(beta_start, beta_end, num_train_timesteps, dtype=np.float64)
        else:
            raise NotImplementedError(f"beta_schedule {beta_schedule!r}")
        if prediction_type != "epsilon" or not predict_x0 or thresholding:
            raise NotImplementedError("UniPC: epsilon prediction in data-prediction (predict_x0) form without thresholding only")
        if solver_type not in ("bh1", "bh2") or solver_order not in (1, 2, 3):
            raise NotImplementedError(f"UniPC: solver_type {solver_type!r} / order {solver_order}")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise NotImplementedError(f"timestep_spacing {timestep_spacing!r}")
        self.num_train_timesteps = num_train_timesteps
        ac = np.cumprod(1.0 - betas)
        self.alphas_cumprod = torch.from_numpy(ac.astype(np.float32))
        self._ac = ac
        self.order = solver_order
        self.solver_order, self.solver_type = solver_order, solver_type
        self.lower_order_final, self.disable_corrector = lower_order_final, tuple(disable_corrector)
        self.timestep_spacing, self.steps_offset = timestep_spacing, steps_offset
        self.config = dict(num_train_timesteps=num_train_timesteps, solver_order=solver_order, solver_type=solver_type)
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self.fused_step = bool(fused_step)
        self._reset()

    # ---- the fused-step switch (off by default: nothing about the class changes while it is off) ------------------------
    def enable_fused_step(self, flag: bool = True):
        """Opt in to ONE ``imd_unipc_step`` launch per step (:meth:`plan_fused`): the pipelines then give UniPC what the other
        samplers have -- per-request guidance, the inpainting blend and ``strength`` < 1, step-graph replay, denoising sessions.
        The bits change at fp32-rounding level against the three ``imd_lincomb`` launches (no intermediate tensor is rounded
        through memory); ``step`` / ``step_guided`` themselves are untouched."""
        self.fused_step = bool(flag)
        return self

    def disable_fused_step(self):
        return self.enable_fused_step(False)

    # ---- schedule --------------------------------------------------------------------------------------------------
    def _reset(self):
        self.model_outputs = []          # x0 predictions of the last `solver_order` steps, oldest first
        self.ts_hist = []                # schedule positions (indices into self._sig) they were made at
        self.last_sample = None
        self.lower_order_nums = 0
        self.step_index = 0

    def set_timesteps(self, num_inference_steps: int, device=None):
        T, N = self.num_train_timesteps, num_inference_steps
        if self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, N + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif self.timestep_spacing == "leading":
            ts = (np.arange(0, N + 1) * (T // (N + 1))).round()[::-1][:-1].copy().astype(np.int64) + self.steps_offset
        else:
            ts = (np.arange(T, 0, -T / N).round() - 1).astype(np.int64)
        self.num_inference_steps = N
        self.timesteps = torch.from_numpy(ts)
        sig_all = np.sqrt((1.0 - self._ac) / self._ac)
        # sigma at each sampled timestep, then the final target: the sigma of training timestep 0 (not exactly zero)
        self._sig = np.concatenate([sig_all[ts], sig_all[:1]])
        self._reset()

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _alpha_sigma(self, pos):
        s = self._sig[pos]
        a = 1.0 / np.sqrt(s * s + 1.0)
        return a, s * a

    def _lambda(self, pos):
        a, s = self._alpha_sigma(pos)
        return np.log(a) - np.log(s)

    # ---- host-side coefficient lists (float64) -----------------------------------------------------------------
    def x0_terms(self, pos, guidance=None):
        """x0 = (x - sigma_t eps) / alpha_t, with eps = g eps_c + (1 - g) eps_u when `guidance` is given."""
        a, s = self._alpha_sigma(pos)
        if guidance is None:
            return [(1.0 / a, "x"), (-s / a, "eps")]
        return [(1.0 / a, "x"), (-s / a * guidance, "eps_c"), (-s / a * (1.0 - guidance), "eps_u")]

    def _bh(self, pos_s0, pos_t, hist_pos, order):
        """shared pieces of UniP / UniC: (alpha_t, sigma_t / sigma_s0, h_phi_1, B_h, r_k list, R, b)"""
        lam_t, lam_s0 = self._lambda(pos_t), self._lambda(pos_s0)
        a_t, sg_t = self._alpha_sigma(pos_t)
        _, sg_s0 = self._alpha_sigma(pos_s0)
        h = lam_t - lam_s0
        rks = [(self._lambda(hist_pos[-(i + 1)]) - lam_s0) / h for i in range(1, order)]
        rks.append(1.0)
        hh = -h
        h_phi_1 = np.expm1(hh)
        h_phi_k = h_phi_1 / hh - 1.0
        B_h = hh if self.solver_type == "bh1" else np.expm1(hh)
        R, b, fact = [], [], 1
        for i in range(1, order + 1):
            R.append([rk ** (i - 1) for rk in rks])
            b.append(h_phi_k * fact / B_h)
            fact *= i + 1
            h_phi_k = h_phi_k / hh - 1.0 / fact
        return a_t, sg_t / sg_s0, h_phi_1, B_h, rks, np.array(R), np.array(b)

    @staticmethod
    def _expand(base_x, base_m0, d_coefs, rks, extra=None):
        """x_t = base_x * x + base_m0 * m0 + sum_k d_k * (m_k - m0) / r_k [+ extra_c * (m_t - m0)] as a flat term list over
        names "x", "m0", "m1", ... ("m_k" = k steps before the newest) and "mt"."""
        c_m0 = base_m0
        terms = [(base_x, "x")]
        for k, dk in enumerate(d_coefs):
            terms.append((dk / rks[k], f"m{k + 1}"))
            c_m0 -= dk / rks[k]
        if extra is not None:
            terms.append((extra, "mt"))
            c_m0 -= extra
        terms.insert(1, (c_m0, "m0"))
        return terms

    def predictor_terms(self, pos_s0, order, hist_pos=None):
        """UniP-p: sample at schedule position pos_s0 + 1 from `x` (at pos_s0) and the x0 history (m0 newest).  `hist_pos`: the
        positions the history was made at, oldest first (None: this instance's running `ts_hist`)."""
        a_t, ratio, h_phi_1, B_h, rks, R, b = self._bh(pos_s0, pos_s0 + 1, self.ts_hist if hist_pos is None else hist_pos, order)
        rhos = [] if order == 1 else ([0.5] if order == 2 else list(np.linalg.solve(R[:-1, :-1], b[:-1])))
        return self._expand(ratio, -a_t * h_phi_1, [-a_t * B_h * r for r in rhos], rks)

    def corrector_terms(self, pos_t, order, hist_pos=None):
        """UniC-p: re-estimate the sample at pos_t from `x` = the sample at pos_t - 1, the history (m0 = x0 at pos_t - 1) and
        `mt` = the x0 prediction just made at pos_t.  `hist_pos` as for `predictor_terms`."""
        a_t, ratio, h_phi_1, B_h, rks, R, b = self._bh(pos_t - 1, pos_t, self.ts_hist if hist_pos is None else hist_pos, order)
        rhos = [0.5] if order == 1 else list(np.linalg.solve(R, b))
        return self._expand(ratio, -a_t * h_phi_1, [-a_t * B_h * r for r in rhos[:-1]], rks, extra=-a_t * B_h * rhos[-1])

    def _order_now(self):
        return self._order_at(self.step_index, self.lower_order_nums)

    def _order_at(self, pos, lower_order_nums):
        """order of the predictor at schedule position `pos` when `lower_order_nums` steps of the ramp-up are behind it"""
        o = self.solver_order
        if self.lower_order_final:
            o = min(o, self.num_inference_steps - pos)
        return min(o, lower_order_nums + 1)

    # ---- the fused step: the same bookkeeping as `_advance`, as one coefficient row per step ------------------------------
    @property
    def history(self) -> int:
        """planes of the device history buffer of the fused step: `solver_order` x0 predictions and `last_sample`"""
        return self.solver_order + 1

    stochastic = False

    def steps(self, start: int = 0) -> int:
        return len(self.timesteps) - int(start)

    def input_scale(self, pos: int) -> float:
        return 1.0

    def plan_fused(self, i: int, t_start: int = 0, blend: bool = False) -> "UniPCRow":
        """The i-th step of a run that begins at schedule position `t_start`, as ONE :class:`UniPCRow` in float64 -- what
        `step_guided` + `_advance` apply with three launches, from the same `x0_terms` / `corrector_terms` / `predictor_terms` and
        the same order bookkeeping (ramp-up from order 1, `lower_order_final`, `disable_corrector`).  A pure function of the
        positions: the rows of a whole run are known before its first launch and the instance's running state is not touched.
        `blend`: the coefficients of the inpainting blend toward the NEXT position (the image latents re-noised to the next
        timestep; the clean image after the last step), as `plan` of the other samplers computes them."""
        i, start, so = int(i), int(t_start), self.solver_order
        pos = start + i
        N = len(self.timesteps)
        if not 0 <= pos < N:
            raise ValueError(f"plan_fused: step {i} of a run from position {start} is outside the {N} steps of the schedule")
        made = list(range(start, pos))                         # positions of the x0 predictions made before this step
        (m_x, _), (m_e, _) = self.x0_terms(pos)
        row = dict(m_x=m_x, m_e=m_e, s_h=(0.0,) * so)
        if i > 0 and (pos - 1) not in self.disable_corrector:
            order_prev = self._order_at(pos - 1, min(i - 1, so))     # `this_order` as the previous step left it
            named = {n: c for c, n in self.corrector_terms(pos, order_prev, made[-so:])}
            row.update(s_x=0.0, s_l=named.pop("x"), s_m=named.pop("mt"))
            row["s_h"] = tuple(named.get(f"m{k}", 0.0) for k in range(so))
        order = self._order_at(pos, min(i, so))
        named = {n: c for c, n in self.predictor_terms(pos, order, (made + [pos])[-so:])}
        row.update(z_s=named.pop("x"), z_m=named.pop("m0"))
        row["z_h"] = tuple(named.get(f"m{k + 1}", 0.0) for k in range(so))          # age k = the k-th newest BEFORE this step
        if blend:
            last = pos == N - 1
            a = 1.0 if last else float(self._ac[int(self.timesteps[pos + 1])])
            row.update(b_img=a ** 0.5, b_noise=(1.0 - a) ** 0.5)
        return UniPCRow(**row)

    # ---- device-side application -------------------------------------------------------------------------------
    def _apply(self, terms, named, out=None):
        return ops.lincomb([(c, named[n]) for c, n in terms if c != 0.0 or n == "x"], out=out)

    def step_guided(self, eps2: torch.Tensor, sample: torch.Tensor, guidance: float) -> torch.Tensor:
        """One sampler step on the CFG batch: eps2 [2B, ...] fp32 (rows [0,B) cond, [B,2B) uncond), sample [B, ...] fp32 ->
        next sample (a new tensor).  Call once per entry of `timesteps`, in order."""
        B = sample.shape[0]
        pos = self.step_index
        named = {"x": sample, "eps_c": eps2[:B], "eps_u": eps2[B:]}
        mt = self._apply(self.x0_terms(pos, guidance), named)
        return self._advance(mt, sample)

    def _advance(self, mt, sample):
        pos = self.step_index
        hist = {f"m{k}": m for k, m in enumerate(reversed(self.model_outputs))}
        if pos > 0 and (pos - 1) not in self.disable_corrector and self.last_sample is not None:
            sample = self._apply(self.corrector_terms(pos, self.this_order), dict(hist, x=self.last_sample, mt=mt))
        self.model_outputs = (self.model_outputs + [mt])[-self.solver_order:]
        self.ts_hist = (self.ts_hist + [pos])[-self.solver_order:]
        self.this_order = self._order_now()
        self.last_sample = sample
        hist = {f"m{k}": m for k, m in enumerate(reversed(self.model_outputs))}
        nxt = self._apply(self.predictor_terms(pos, self.this_order), dict(hist, x=sample))
        if self.lower_order_nums < self.solver_order:
            self.lower_order_nums += 1
        self.step_index += 1
        return nxt

    # diffusers-compatible tensor API (NCHW in / out)
    def step(self, model_output, timestep, sample, return_dict: bool = False, **unused):
        x = sample.float().contiguous()
        mt = self._apply(self.x0_terms(self.step_index), {"x": x, "eps": model_output.float().contiguous()})
        return (self._advance(mt, x).to(sample.dtype),)

    def add_noise(self, original_samples, noise, timesteps):
        a = float(self._ac[int(torch.as_tensor(timesteps).reshape(-1)[0])])
        return a ** 0.5 * original_samples + (1 - a) ** 0.5 * noise


def unipc_fused(scheduler) -> bool:
    """a UniPC whose fused-step switch is on: the pipelines' loop, the request checks and the sessions treat it like the samplers of
    ``imd_sampler_step`` (one launch per step, ``imd_unipc_step``); off, it is the three-launch class with its refusals"""
    return hasattr(scheduler, "plan_fused") and bool(getattr(scheduler, "fused_step", False))


class UniPCRow:
    """The float64 coefficients of ONE UniPC step, as ``imd_unipc_step`` applies them to the guided epsilon e:

        m  = m_x z + m_e e                                            the x0 prediction made at this position
        s' = s_x z + s_m m + s_l L + sum_j s_h[j] M_j                  UniC (no corrector: s_x = 1, the rest 0, s' = z)
        z' = z_s s' + z_m m + sum_j z_h[j] M_j                         UniP from s'
        z' = (1 - mask) (b_img z_img + b_noise blend_noise) + mask z'
        x_next = 16-bit(in_scale z');  the history gains m, and s' replaces L

    L = ``last_sample`` (the s' of the previous step), M_j = the j-th NEWEST x0 prediction stored BEFORE this step.  ``s_h`` /
    ``z_h`` are ordered by AGE; :class:`UniPCHistory` maps ages (and L) to the physical slots of the device buffer."""
    __slots__ = ("m_x", "m_e", "s_x", "s_m", "s_l", "s_h", "z_s", "z_m", "z_h", "b_img", "b_noise", "in_scale")

    def __init__(self, m_x=0.0, m_e=1.0, s_x=1.0, s_m=0.0, s_l=0.0, s_h=(), z_s=1.0, z_m=0.0, z_h=(), b_img=1.0, b_noise=0.0, in_scale=1.0):
        self.m_x, self.m_e, self.s_x, self.s_m, self.s_l = float(m_x), float(m_e), float(s_x), float(s_m), float(s_l)
        self.s_h, self.z_h = tuple(float(c) for c in s_h), tuple(float(c) for c in z_h)
        self.z_s, self.z_m = float(z_s), float(z_m)
        self.b_img, self.b_noise, self.in_scale = float(b_img), float(b_noise), float(in_scale)

    def __repr__(self):
        return "UniPCRow(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"


class UniPCHistory:
    """Host-side bookkeeping of the device history buffer [K][B HW 4] of the fused UniPC step, like :class:`SamplerHistory`: ONE slot
    is ``last_sample`` and is overwritten in place at every step; the new x0 prediction takes a free slot while there is one, then
    the slot of the oldest prediction (which the same launch may still read: every thread reads before it stores).  Data never
    moves; the slot indices travel in the coefficient block.  K = solver_order + 1 suffices: a step reads at most ``solver_order``
    stored predictions and ``last_sample``."""

    def __init__(self, K: int):
        self.K = int(K)
        if self.K < 2:
            raise ValueError(f"UniPCHistory: K = {K}; the fused step keeps last_sample and at least one x0 prediction")
        self.last = 0                     # the slot of last_sample
        self.slots = []                   # physical slots of the x0 predictions, newest first

    def coefs(self, row: UniPCRow):
        """-> the 19 values of ``ops.unipc_coefs`` for ``row`` (``s_h`` / ``z_h`` permuted to physical slots) -- and the history
        advances."""
        sh, zh = [0.0] * ops.SAMPLER_MAX_HISTORY, [0.0] * ops.SAMPLER_MAX_HISTORY
        for name, src, dst in (("s_h", row.s_h, sh), ("z_h", row.z_h, zh)):
            for age, c in enumerate(src):
                if c != 0.0:
                    if age >= len(self.slots):
                        raise ValueError(f"the step reads x0 prediction {age} ({name}) but only {len(self.slots)} are stored")
                    dst[self.slots[age]] = c
        sh[self.last] = row.s_l
        free = [s for s in range(self.K) if s != self.last and s not in self.slots]
        store_m = free[0] if free else self.slots[-1]
        self.slots = [store_m] + [s for s in self.slots if s != store_m]
        return ops.unipc_coefs(row.m_x, row.m_e, row.s_x, row.s_m, sh, row.z_s, row.z_m, zh, row.b_img, row.b_noise, row.in_scale,
                               store_m, self.last)


# ---------------------------------------------------------------------------------------------------------------------
# Samplers on the fused affine step (imd_sampler_step): DPM-Solver++, Euler, Euler-ancestral, PNDM/PLMS
# ---------------------------------------------------------------------------------------------------------------------
class SamplerRow:
    """The float64 coefficients of ONE step of an affine sampler, as ``imd_sampler_step`` applies them to the guided epsilon e:

        m  = m_x z + m_e e
        z' = z_x z + z_m m + sum_j z_h[j] H_j + z_n noise          H_j = the j-th NEWEST entry of the history before this step
        z' = (1 - mask) (b_img z_img + b_noise blend_noise) + mask z'
        x_next = 16-bit(in_scale z');  the history gains m when ``keep``

    ``z_h`` is ordered by AGE; :class:`SamplerHistory` maps ages to the physical slots of the device buffer."""
    __slots__ = ("m_x", "m_e", "z_x", "z_m", "z_h", "z_n", "b_img", "b_noise", "in_scale", "keep")

    def __init__(self, m_x=0.0, m_e=1.0, z_x=1.0, z_m=0.0, z_h=(), z_n=0.0, b_img=1.0, b_noise=0.0, in_scale=1.0, keep=False):
        self.m_x, self.m_e, self.z_x, self.z_m = float(m_x), float(m_e), float(z_x), float(z_m)
        self.z_h = tuple(float(c) for c in z_h)
        self.z_n, self.b_img, self.b_noise, self.in_scale, self.keep = float(z_n), float(b_img), float(b_noise), float(in_scale), bool(keep)

    def __repr__(self):
        return "SamplerRow(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"


class SamplerHistory:
    """Host-side bookkeeping of the device history buffer [K][B HW 4]: which physical slot holds the j-th newest entry.  A new entry
    takes a free slot while there is one, then the slot of the oldest entry -- data never moves, and the slot index travels in the
    coefficient block, so a captured step writes another slot at every replay."""

    def __init__(self, K: int):
        self.K = int(K)
        self.slots = []                   # physical slots, newest entry first

    def coefs(self, row: SamplerRow):
        """-> the 13 values of ``ops.sampler_coefs`` for ``row`` (``z_h`` permuted to physical slots) -- and the history advances."""
        zh = [0.0] * ops.SAMPLER_MAX_HISTORY
        for age, c in enumerate(row.z_h):
            if c != 0.0:
                if age >= len(self.slots):
                    raise ValueError(f"the step reads history entry {age} but only {len(self.slots)} are stored")
                zh[self.slots[age]] = c
        store = -1
        if row.keep and self.K > 0:
            free = [s for s in range(self.K) if s not in self.slots]
            store = free[0] if free else self.slots[-1]
            self.slots = [store] + [s for s in self.slots if s != store]
        return ops.sampler_coefs(row.m_x, row.m_e, row.z_x, row.z_m, zh, row.z_n, row.b_img, row.b_noise, row.in_scale, store)


def ddim_row(scheduler: "DDIMScheduler", t: int, eta: float = 0.0) -> SamplerRow:
    """The DDIM step at timestep ``t`` as a :class:`SamplerRow`, in float64: m = e and
        z' = (sqrt(a_prev) / sqrt(a_t)) z + (sqrt(1 - a_prev) - sqrt(a_prev) sqrt(1 - a_t) / sqrt(a_t)) e
    -- for the callers that give every latent row its own coefficients (``imd_sampler_step_rows``, the denoising session).  A function
    and not a ``plan`` method of :class:`DDIMScheduler`: the pipelines' loop picks the fused-sampler path by that attribute, and the
    default DDIM loop stays on ``imd_ddim_cfg_step``.
    ``eta`` > 0: the stochastic step of diffusers' ``DDIMScheduler.step`` with ``variance_noise`` -- sigma = ``scheduler.sigma(t, eta)``,
    the direction term becomes sqrt(1 - a_prev - sigma^2) and z_n = sigma scales the step's noise operand.  ``eta`` = 0 is the row
    above, bit for bit."""
    a_t, a_prev = float(scheduler.alpha(t)), float(scheduler.alpha_prev(t))
    sa_t, sa_p = np.sqrt(a_t), np.sqrt(a_prev)
    if float(eta) == 0.0:
        return SamplerRow(m_x=0.0, m_e=1.0, z_x=sa_p / sa_t, z_m=np.sqrt(1.0 - a_prev) - sa_p * np.sqrt(1.0 - a_t) / sa_t, keep=False)
    if float(eta) < 0.0:
        raise ValueError(f"eta must be >= 0, got {eta}")
    sigma = float(eta) * np.sqrt((1.0 - a_prev) / (1.0 - a_t) * (1.0 - a_t / a_prev))
    return SamplerRow(m_x=0.0, m_e=1.0, z_x=sa_p / sa_t, z_m=np.sqrt(1.0 - a_prev - sigma * sigma) - sa_p * np.sqrt(1.0 - a_t) / sa_t,
                      z_n=sigma, keep=False)


def _train_alphas_cumprod(num_train_timesteps, beta_start, beta_end, beta_schedule):
    if beta_schedule == "scaled_linear":
        betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=np.float64) ** 2
    elif beta_schedule == "linear":
        betas = np.linspace(beta_start, beta_end, num_train_timesteps, dtype=np.float64)
    else:
        raise NotImplementedError(f"beta_schedule {beta_schedule!r}")
    return np.cumprod(1.0 - betas)


def _karras_sigmas(sigma_min, sigma_max, n, rho=7.0):
    """Karras et al. 2022 eq. (5): n sigmas from sigma_max down to sigma_min (the library's ``_convert_to_karras``)"""
    lo, hi = sigma_min ** (1.0 / rho), sigma_max ** (1.0 / rho)
    return (hi + np.linspace(0.0, 1.0, n) * (lo - hi)) ** rho


def _sigma_to_t(sigma, log_sigmas):
    """the (fractional) training timestep whose sigma, interpolated in log space, is ``sigma`` (the library's ``_sigma_to_t``)"""
    ls = np.log(sigma)
    low = int(np.clip(np.searchsorted(log_sigmas, ls, side="right") - 1, 0, len(log_sigmas) - 2))
    w = float(np.clip((log_sigmas[low] - ls) / (log_sigmas[low] - log_sigmas[low + 1]), 0.0, 1.0))
    return (1.0 - w) * low + w * (low + 1)


class _AffineSampler:
    """What the four samplers below share: the training schedule, the diffusers-0.24 tensor surface (``step`` /
    ``scale_model_input`` / ``add_noise`` run on the GPU through the same kernel as the pipelines) and the host protocol the
    pipelines drive -- ``plan(i, start, blend)`` -> :class:`SamplerRow` in float64 for the i-th step of a run that begins at schedule
    position ``start``, ``history`` (slots of the device buffer), ``stochastic``, ``input_scale(pos)``."""
    order = 1
    history = 0
    stochastic = False
    init_noise_sigma = 1.0

    def _init_schedule(self, num_train_timesteps, beta_start, beta_end, beta_schedule, prediction_type, timestep_spacing, steps_offset):
        if prediction_type != "epsilon":
            raise NotImplementedError(f"{type(self).__name__}: prediction_type {prediction_type!r} (epsilon only, the reference's models)")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise NotImplementedError(f"{type(self).__name__}: timestep_spacing {timestep_spacing!r}")
        self.num_train_timesteps = num_train_timesteps
        self._ac = _train_alphas_cumprod(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self._sig_all = np.sqrt((1.0 - self._ac) / self._ac)
        self.alphas_cumprod = torch.from_numpy(self._ac.astype(np.float32))
        self.timestep_spacing, self.steps_offset = timestep_spacing, steps_offset
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self._run = None

    # ---- host protocol ----
    def plan(self, i: int, start: int = 0, blend: bool = False) -> SamplerRow:
        raise NotImplementedError

    def steps(self, start: int = 0) -> int:
        """number of steps (= UNet calls) of a run that begins at schedule position ``start``"""
        return len(self.timesteps) - int(start)

    def input_scale(self, pos: int) -> float:
        return 1.0

    def _alpha_blend(self, t_next):
        """coefficients of ``add_noise`` at timestep ``t_next`` (None: after the last step, the clean image latents)"""
        if t_next is None:
            return 1.0, 0.0
        a = float(self._ac[int(t_next)])
        return a ** 0.5, (1.0 - a) ** 0.5

    # ---- diffusers-compatible tensor API (NCHW in / out) ----
    def _position(self, timestep) -> int:
        ts = self.timesteps.double().numpy()
        return int(np.argmin(np.abs(ts - float(torch.as_tensor(timestep).reshape(-1)[0]))))

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, return_dict: bool = False, **unused):
        """One sampler step on tensors; call once per entry of ``timesteps``, in order (the first call after ``set_timesteps`` fixes
        where the run starts).  A stochastic sampler draws its noise like diffusers: ``variance_noise``, or a standard-normal draw
        of ``model_output``'s shape and dtype from ``generator``."""
        B, Cc, H, W = sample.shape
        if self._run is None:
            self._run = dict(start=self._position(timestep), i=0, ring=SamplerHistory(self.history),
                             hist=torch.zeros(self.history, B, H * W, Cc, dtype=torch.float32, device=sample.device) if self.history else None)
        run = self._run
        z = sample.float().permute(0, 2, 3, 1).reshape(B, H * W, Cc).contiguous()
        e = model_output.float().permute(0, 2, 3, 1).reshape(B, H * W, Cc).contiguous()
        noise = None
        if self.stochastic:
            if variance_noise is None:
                from .dressing_sd.pipelines._base import randn_tensor
                variance_noise = randn_tensor(tuple(model_output.shape), generator=generator, device=model_output.device, dtype=model_output.dtype)
            noise = variance_noise.to(sample.device).float().permute(0, 2, 3, 1).reshape(B, H * W, Cc).contiguous()
        ops.sampler_step(z, torch.cat([e, e]), None, guidance=1.0, coefs=run["ring"].coefs(self.plan(run["i"], run["start"])),
                         hist=run["hist"], noise=noise)
        run["i"] += 1
        return (z.view(B, H, W, Cc).permute(0, 3, 1, 2).to(sample.dtype),)

    def add_noise(self, original_samples, noise, timesteps):
        a = float(self._ac[int(round(float(torch.as_tensor(timesteps).reshape(-1)[0])))])
        return a ** 0.5 * original_samples + (1 - a) ** 0.5 * noise


class DPMSolverMultistepScheduler(_AffineSampler):
    """DPM-Solver++ (Lu et al. 2022) multistep sampler, orders 1 and 2 ("2M", midpoint), with the surface of diffusers==0.24.0
    ``DPMSolverMultistepScheduler``.  diffusers is un-vendored and the reference holds no vectors for it: **parity unpinned**; the
    class is anchored by properties tested in tests/ (order 1 == DDIM with eta = 0; a constant data prediction is integrated
    exactly; first / second order convergence on the Gaussian case) and by tests/sampler_oracle.py, the tensor-form restatement.

    sigma_t = sqrt((1 - abar_t) / abar_t), alpha = 1 / sqrt(sigma^2 + 1), sigma^ = sigma alpha, lambda = -ln sigma, h = lambda' - lambda:
        x0 = (z - sigma^ e) / alpha;   z' = (sigma^' / sigma^) z - alpha' (e^-h - 1) D;   D = x0 (order 1), x0 + (x0 - x0_prev) / (2 r), r = h_prev / h
    The final sigma is 0 (the last step returns the data prediction), so the last step is first order whatever ``lower_order_final``
    says (r would be 0), as the library does for a zero final sigma; the first step has no history and is first order.
    On the device: m = x0, one history slot, ONE ``imd_sampler_step`` per step."""
    history = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", solver_order=2,
                 prediction_type="epsilon", thresholding=False, algorithm_type="dpmsolver++", solver_type="midpoint",
                 lower_order_final=True, use_karras_sigmas=False, lambda_min_clipped=-float("inf"), variance_type=None,
                 timestep_spacing="linspace", steps_offset=0, trained_betas=None, **unused):
        if algorithm_type != "dpmsolver++":
            raise NotImplementedError(f"DPMSolverMultistepScheduler: algorithm_type {algorithm_type!r} (dpmsolver++ only)")
        if solver_type != "midpoint":
            raise NotImplementedError(f"DPMSolverMultistepScheduler: solver_type {solver_type!r} (midpoint only)")
        if solver_order not in (1, 2):
            raise NotImplementedError(f"DPMSolverMultistepScheduler: solver_order {solver_order} (1 or 2)")
        if thresholding:
            raise NotImplementedError("DPMSolverMultistepScheduler: thresholding")
        if variance_type is not None:
            raise NotImplementedError(f"DPMSolverMultistepScheduler: variance_type {variance_type!r}")
        if lambda_min_clipped != -float("inf"):
            raise NotImplementedError("DPMSolverMultistepScheduler: lambda_min_clipped")
        if trained_betas is not None:
            raise NotImplementedError("DPMSolverMultistepScheduler: trained_betas")
        self._init_schedule(num_train_timesteps, beta_start, beta_end, beta_schedule, prediction_type, timestep_spacing, steps_offset)
        self.solver_order, self.lower_order_final, self.use_karras_sigmas = solver_order, lower_order_final, use_karras_sigmas
        self.config = dict(num_train_timesteps=num_train_timesteps, solver_order=solver_order, algorithm_type=algorithm_type,
                           solver_type=solver_type, lower_order_final=lower_order_final, use_karras_sigmas=use_karras_sigmas,
                           timestep_spacing=timestep_spacing, steps_offset=steps_offset)

    def set_timesteps(self, num_inference_steps: int, device=None):
        T, N = self.num_train_timesteps, num_inference_steps
        if self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, N + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif self.timestep_spacing == "leading":
            ts = (np.arange(0, N + 1) * (T // (N + 1))).round()[::-1][:-1].copy().astype(np.int64) + self.steps_offset
        else:
            ts = (np.arange(T, 0, -T / N).round() - 1).astype(np.int64)
        if self.use_karras_sigmas:
            sig = _karras_sigmas(self._sig_all[0], self._sig_all[-1], N)          # between the extremes of the training schedule
            log_sigmas = np.log(self._sig_all)
            ts = np.array([_sigma_to_t(s, log_sigmas) for s in sig]).round().astype(np.int64)
        else:
            sig = self._sig_all[ts]
        self._sig = np.concatenate([sig, [0.0]])
        self.sigmas = torch.from_numpy(self._sig.astype(np.float32))
        self.num_inference_steps = N
        self.timesteps = torch.from_numpy(ts)
        self._run = None

    def plan(self, i: int, start: int = 0, blend: bool = False) -> SamplerRow:
        pos = int(start) + int(i)
        N = len(self.timesteps)
        s, t = self._sig[pos], self._sig[pos + 1]
        a_s, a_t = 1.0 / np.sqrt(s * s + 1.0), 1.0 / np.sqrt(t * t + 1.0)
        last = pos == N - 1
        if t > 0.0:
            h = np.log(s) - np.log(t)
            em = np.expm1(-h)
        else:
            h, em = np.inf, -1.0
        row = dict(m_x=1.0 / a_s, m_e=-s, z_x=(t * a_t) / (s * a_s), keep=True)
        if self.solver_order == 1 or i == 0 or last:
            row.update(z_m=-a_t * em)
        else:
            r = (np.log(self._sig[pos - 1]) - np.log(s)) / h
            row.update(z_m=-a_t * em * (1.0 + 0.5 / r), z_h=(a_t * em * 0.5 / r,))
        if blend:
            b = self._alpha_blend(None if last else self.timesteps[pos + 1])
            row.update(b_img=b[0], b_noise=b[1])
        return SamplerRow(**row)


class EulerDiscreteScheduler(_AffineSampler):
    """Euler sampler of Karras et al. 2022 (Algorithm 2 without churn) with the surface of diffusers==0.24.0
    ``EulerDiscreteScheduler``: the sample lives in sigma space (z = x0 + sigma n), the UNet sees z / sqrt(sigma^2 + 1)
    (``scale_model_input``; on the device the ``in_scale`` of the step that produced z) and z' = z + (sigma' - sigma) e.
    ``init_noise_sigma`` is max sigma for "linspace" / "trailing" spacing and sqrt(max sigma^2 + 1) for "leading", as in the library.
    The timesteps of "linspace" spacing and of Karras sigmas are fractional and reach the time embedding unrounded.
    diffusers is un-vendored and the reference holds no vectors for it: **parity unpinned**; anchored in tests/ by: on the same grid
    the trajectory equals DDIM's after dividing by sqrt(sigma^2 + 1); first-order convergence on the Gaussian case;
    tests/sampler_oracle.py.  No history: ONE ``imd_sampler_step`` per step with m = e."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", prediction_type="epsilon",
                 interpolation_type="linear", use_karras_sigmas=False, timestep_spacing="linspace", steps_offset=0,
                 trained_betas=None, **unused):
        name = type(self).__name__
        if interpolation_type != "linear":
            raise NotImplementedError(f"{name}: interpolation_type {interpolation_type!r} (linear only)")
        if trained_betas is not None:
            raise NotImplementedError(f"{name}: trained_betas")
        self._init_schedule(num_train_timesteps, beta_start, beta_end, beta_schedule, prediction_type, timestep_spacing, steps_offset)
        self.use_karras_sigmas = use_karras_sigmas
        self.config = dict(num_train_timesteps=num_train_timesteps, use_karras_sigmas=use_karras_sigmas, timestep_spacing=timestep_spacing,
                           steps_offset=steps_offset, interpolation_type=interpolation_type)
        self._set_sigmas(self._sig_all[::-1].copy(), np.arange(0, num_train_timesteps)[::-1].astype(np.float64))

    def _set_sigmas(self, sig, ts):
        self._sig = np.concatenate([sig, [0.0]])
        self.sigmas = torch.from_numpy(self._sig.astype(np.float32))
        self.timesteps = torch.from_numpy(np.ascontiguousarray(ts, dtype=np.float64))
        smax = float(self._sig.max())
        self.init_noise_sigma = smax if self.timestep_spacing in ("linspace", "trailing") else (smax * smax + 1.0) ** 0.5
        self._run = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        T, N = self.num_train_timesteps, num_inference_steps
        if self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, N, dtype=np.float64)[::-1].copy()
        elif self.timestep_spacing == "leading":
            ts = (np.arange(0, N) * (T // N)).round()[::-1].copy().astype(np.float64) + self.steps_offset
        else:
            ts = np.arange(T, 0, -T / N).round().astype(np.float64) - 1
        sig = np.interp(ts, np.arange(0, T), self._sig_all)
        if self.use_karras_sigmas:
            sig = _karras_sigmas(sig[-1], sig[0], N)                              # between the extremes of THIS schedule, as the library does
            log_sigmas = np.log(self._sig_all)
            ts = np.array([_sigma_to_t(s, log_sigmas) for s in sig])
        self.num_inference_steps = N
        self._set_sigmas(sig, ts)

    def input_scale(self, pos: int) -> float:
        return float(1.0 / np.sqrt(self._sig[pos] ** 2 + 1.0))

    def _sigma_steps(self, s, t):
        """-> (coefficient of e, coefficient of the noise) of the step sigma s -> t"""
        return t - s, 0.0

    def plan(self, i: int, start: int = 0, blend: bool = False) -> SamplerRow:
        pos = int(start) + int(i)
        s, t = self._sig[pos], self._sig[pos + 1]
        c_e, c_n = self._sigma_steps(s, t)
        return SamplerRow(m_x=0.0, m_e=1.0, z_x=1.0, z_m=c_e, z_n=c_n, in_scale=1.0 / np.sqrt(t * t + 1.0),
                          b_img=1.0, b_noise=t if blend else 0.0)

    def scale_model_input(self, sample, timestep=None):
        return sample * self.input_scale(self._position(timestep))

    def add_noise(self, original_samples, noise, timesteps):
        return original_samples + float(self._sig[self._position(timesteps)]) * noise


class EulerAncestralDiscreteScheduler(EulerDiscreteScheduler):
    """Ancestral Euler sampler (k-diffusion ``sample_euler_ancestral``) with the surface of diffusers==0.24.0
    ``EulerAncestralDiscreteScheduler``: sigma_up = sqrt(sigma'^2 (sigma^2 - sigma'^2) / sigma^2), sigma_down = sqrt(sigma'^2 - sigma_up^2),
    z' = z + (sigma_down - sigma) e + sigma_up noise.  The noise of step i is ``variance_noise[i]`` or a standard-normal draw in the
    UNet's element type from ``generator`` (what the library's ``step`` does with the reference's ``noise_pred``), like DDIM's
    eta > 0 path; the pipelines run it eagerly (no step-graph replay).  **Parity with the library unpinned** (see
    :class:`EulerDiscreteScheduler`); the host rows are checked against tests/sampler_oracle.py."""
    stochastic = True

    def __init__(self, *args, use_karras_sigmas=False, **kw):
        if use_karras_sigmas:
            raise NotImplementedError("EulerAncestralDiscreteScheduler: use_karras_sigmas (the library's class has no such option)")
        super().__init__(*args, **kw)

    def _sigma_steps(self, s, t):
        up = np.sqrt(t * t * (s * s - t * t) / (s * s))
        down = np.sqrt(t * t - up * up)
        return down - s, up


class PNDMScheduler(_AffineSampler):
    """PNDM (Liu et al. 2022) in its PLMS form -- ``skip_prk_steps=True``, the SD1.5 base model's own ``scheduler_config.json`` -- with
    the surface of diffusers==0.24.0 ``PNDMScheduler``: N + 1 UNet calls for N steps (``timesteps`` repeats its second entry), the
    linear-multistep state machine of ``step_plms`` and the transfer formula (9) of the paper (``_get_prev_sample``):

        z' = c_s z - c_e E,   c_s = sqrt(a' / a),   c_e = (a' - a) / (a sqrt(1 - a') + sqrt(a (1 - a) a'))
        E = e_0 | (e_1 + e_0) / 2 from the SAVED sample | (3, -1) / 2 | (23, -16, 5) / 12 | (55, -59, 37, -9) / 24 over the newest epsilons

    On the device m = e and three history slots hold the older epsilons (the newest is this step's m).  The second call does not
    keep the sample of the first step in a slot: z_0 = (z_1 + c_e e_0) / c_s is substituted, so that step is
    z' = (c_s1 / c_s0) z + (c_s1 c_e0 / c_s0 - c_e1 / 2) e_0 - (c_e1 / 2) e -- exact except under an inpainting mask with fractional
    values, where the library would restart from the unblended sample (the pipelines' masks are binary).
    diffusers is un-vendored and the reference holds no vectors for it: **parity unpinned**; anchored in tests/ by the
    Adams-Bashforth weights, the timestep list and tests/sampler_oracle.py, the tensor-form restatement."""
    history = 3

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", skip_prk_steps=False,
                 set_alpha_to_one=False, prediction_type="epsilon", timestep_spacing="leading", steps_offset=0, trained_betas=None,
                 **unused):
        if not skip_prk_steps:
            raise NotImplementedError("PNDMScheduler: skip_prk_steps=False (the Runge-Kutta warm-up; SD1.5's config sets skip_prk_steps)")
        if trained_betas is not None:
            raise NotImplementedError("PNDMScheduler: trained_betas")
        self._init_schedule(num_train_timesteps, beta_start, beta_end, beta_schedule, prediction_type, timestep_spacing, steps_offset)
        self._final_ac = 1.0 if set_alpha_to_one else float(self._ac[0])
        self.config = dict(num_train_timesteps=num_train_timesteps, skip_prk_steps=True, set_alpha_to_one=set_alpha_to_one,
                           timestep_spacing=timestep_spacing, steps_offset=steps_offset)

    def set_timesteps(self, num_inference_steps: int, device=None):
        T, N = self.num_train_timesteps, num_inference_steps
        if self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, N).round().astype(np.int64)
        elif self.timestep_spacing == "leading":
            ts = (np.arange(0, N) * (T // N)).round().astype(np.int64) + self.steps_offset
        else:
            ts = np.round(np.arange(T, 0, -T / N))[::-1].astype(np.int64) - 1
        self.num_inference_steps = N
        self.timesteps = torch.from_numpy(np.concatenate([ts[:-1], ts[-2:-1], ts[-1:]])[::-1].copy())
        self._run = None

    @staticmethod
    def plms_weights(counter: int):
        """weights of the newest .. oldest epsilon at call ``counter`` of a run"""
        return ([1.0], [0.5, 0.5], [1.5, -0.5], [23 / 12, -16 / 12, 5 / 12])[counter] if counter < 4 else [55 / 24, -59 / 24, 37 / 24, -9 / 24]

    def _transfer(self, t: int, prev: int):
        """(c_s, c_e) of ``_get_prev_sample``: sample at timestep t -> timestep prev"""
        a = float(self._ac[min(int(t), self.num_train_timesteps - 1)])
        ap = float(self._ac[int(prev)]) if prev >= 0 else self._final_ac
        return (ap / a) ** 0.5, (ap - a) / (a * (1.0 - ap) ** 0.5 + (a * (1.0 - a) * ap) ** 0.5)

    def _levels(self, counter: int, start: int):
        """(t, prev) of call ``counter`` of a run that begins at schedule position ``start``, as ``step_plms`` sets them"""
        d = self.num_train_timesteps // self.num_inference_steps
        t = int(self.timesteps[start + counter])
        return (t + d, t) if counter == 1 else (t, t - d)

    def plan(self, i: int, start: int = 0, blend: bool = False) -> SamplerRow:
        i, start = int(i), int(start)
        c_s, c_e = self._transfer(*self._levels(i, start))
        w = self.plms_weights(i)
        if i == 1:
            c_s0, c_e0 = self._transfer(*self._levels(0, start))
            row = dict(z_x=c_s / c_s0, z_m=-c_e * w[0], z_h=(c_s * c_e0 / c_s0 - c_e * w[1],), keep=False)
        else:
            row = dict(z_x=c_s, z_m=-c_e * w[0], z_h=tuple(-c_e * x for x in w[1:]), keep=True)
        if blend:
            last = start + i == len(self.timesteps) - 1
            b = self._alpha_blend(None if last else self.timesteps[start + i + 1])
            row.update(b_img=b[0], b_noise=b[1])
        return SamplerRow(m_x=0.0, m_e=1.0, **row)
