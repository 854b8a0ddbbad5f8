"""In-flight batching: a denoising session with a fixed number of slots that admits requests at any step.

A request-batched pipeline call needs all its requests in hand before it starts, and all of them run the same number of steps.  A
session keeps ONE batch of ``slots`` latent rows alive across calls instead: a request enters a free slot at the start of any step,
runs its own schedule (its own step count, its own position in it) and leaves when done.  Every :meth:`DenoiseSession.step` is one
UNet forward (plus ControlNet) over all 2 x slots rows of the CFG batch and one fused step launch (``imd_sampler_step_rows``) that
gives every latent row its own coefficients, its own history slots and its own "this row is not running" flag.

Two layers, so that the logic is testable without a GPU:

* :class:`SessionPlan` -- pure Python: slot allocation (lowest free index first), the FIFO queue, one scheduler instance /
  :class:`~imagdressing_amd.scheduler.SamplerHistory` / position per request, and per step one 16-float coefficient row and one
  timestep per slot.
* :class:`DenoiseSession` -- the device state: fixed-address buffers for every slot, admission (prompt encoding, the garment UNet at
  batch 1, in-place writes of the slot's rows), the step, tickets.

The session always runs all slots: an under-full session pays for its idle rows (tools/session_bench.py measures how much).
"""
from __future__ import annotations

import copy
from collections import deque
from typing import Any, Dict, List, Optional

import torch

from . import ops
from .scheduler import DDIMScheduler, SamplerHistory, ddim_row


# ---- refusals (pure: nothing here touches a device) ----
def check_scheduler(scheduler) -> None:
    """The samplers a session can drive: every deterministic one whose step is ONE affine row -- DPM-Solver++, Euler, PNDM
    (``plan``) and DDIM (``ddim_row``)."""
    name = type(scheduler).__name__
    if hasattr(scheduler, "step_guided"):
        raise NotImplementedError(f"open_session: scheduler {name} (UniPC) updates the latents with host-built linear combinations of "
                                  "whole tensors, not one affine row per latent row; use DPM-Solver++, Euler, PNDM or DDIM")
    if getattr(scheduler, "stochastic", False):
        raise NotImplementedError(f"open_session: scheduler {name} (Euler-ancestral) draws noise at every step; a session runs the "
                                  "deterministic samplers (DPM-Solver++, Euler, PNDM, DDIM)")
    if not hasattr(scheduler, "plan") and not isinstance(scheduler, DDIMScheduler):
        raise NotImplementedError(f"open_session: scheduler {name} has no affine step row (scheduler.SamplerRow)")


def check_pipeline(pipe) -> None:
    """what ``open_session`` and every ``step`` refuse about the pipeline's switches"""
    if getattr(pipe, "_deepcache", None) is not None:
        raise NotImplementedError("enable_deepcache is on: the feature cache belongs to one denoising call whose rows share the step "
                                  "index, the rows of a session do not; disable_deepcache() first")


def check_request(*, size, width=None, height=None, num_inference_steps, guidance_scale, image_scale=1.0, eta=0.0,
                  shard_over_ranks=False, control_guidance_start=0.0, control_guidance_end=1.0, num_images_per_prompt=1, slots=1) -> None:
    """what ``submit`` refuses, before anything is launched or queued.  ``size`` = (width, height) of the session."""
    for name, v in (("num_inference_steps", num_inference_steps), ("guidance_scale", guidance_scale), ("image_scale", image_scale)):
        if isinstance(v, (list, tuple)):
            raise ValueError(f"{name} is per request in a session: submit one request per call, got {list(v)}")
    if float(eta) > 0.0:
        raise NotImplementedError("eta > 0: the stochastic DDIM step draws noise per step; a session runs the deterministic samplers")
    if shard_over_ranks:
        raise NotImplementedError("shard_over_ranks: a session lives on one rank (sessions over several ranks are a later change)")
    if (width is not None and int(width) != int(size[0])) or (height is not None and int(height) != int(size[1])):
        raise ValueError(f"width x height {width} x {height}: this session was opened for {size[0]} x {size[1]} (one geometry per session)")
    if float(control_guidance_start) != 0.0 or float(control_guidance_end) != 1.0:
        raise NotImplementedError("control_guidance_start / control_guidance_end other than 0 / 1: the ControlNet gate is one scalar "
                                  "per launch (the zero-conv epilogue), the rows of a session are at different steps")
    if float(guidance_scale) <= 1.0:
        raise NotImplementedError("guidance_scale <= 1: the reference's loop indexes the CFG pair unconditionally "
                                  "(IMAGDressing_v1_pipeline.py:476-479, :511); sample with guidance_scale > 1")
    if int(num_inference_steps) < 1:
        raise ValueError(f"num_inference_steps must be >= 1, got {num_inference_steps}")
    if not 1 <= int(num_images_per_prompt) <= int(slots):
        raise ValueError(f"num_images_per_prompt = {num_images_per_prompt} takes that many slots; the session has {slots}")


# ---- the plan ----
class PlanRun:
    """One latent row's run: its own scheduler instance (``set_timesteps(n)``), history bookkeeping and position."""
    __slots__ = ("scheduler", "ring", "timesteps", "steps", "i", "slot", "payload")

    def __init__(self, scheduler, num_inference_steps: int, payload=None):
        sch = copy.copy(scheduler)          # the class and configuration of the pipeline's scheduler; set_timesteps rebinds, never mutates
        sch.set_timesteps(int(num_inference_steps))
        self.scheduler = sch
        if self.affine:
            self.timesteps = [t.item() for t in sch.timesteps]          # (fractional ones reach the time embedding unrounded)
            self.steps = sch.steps()                                       # UNet calls: PNDM has one more than it has steps
            self.ring = SamplerHistory(sch.history)
        else:
            self.timesteps = [int(t) for t in sch.timesteps]
            self.steps = len(self.timesteps)
            self.ring = SamplerHistory(0)
        self.i = 0
        self.slot: Optional[int] = None
        self.payload = payload

    @property
    def affine(self) -> bool:
        """a ``plan`` sampler (DPM-Solver++, Euler, PNDM); otherwise DDIM through ``ddim_row``"""
        return hasattr(self.scheduler, "plan")

    @property
    def done(self) -> bool:
        return self.i >= self.steps

    def first_input_scale(self) -> float:
        """``scale_model_input`` of the first step (later inputs come scaled out of the step launch)"""
        return float(self.scheduler.input_scale(0)) if self.affine else 1.0

    def next_coefs(self) -> List[float]:
        """the 13 coefficients of step ``i`` -- and the history bookkeeping advances"""
        row = self.scheduler.plan(self.i) if self.affine else ddim_row(self.scheduler, self.timesteps[self.i])
        return self.ring.coefs(row)


class PlanStep:
    """What one step launches: ``rows`` [slots][16] floats, ``timesteps`` [slots] (None for a free slot), ``running`` = (slot, run,
    position) of every row that takes this step, ``finished`` = the runs for which it is the last."""
    __slots__ = ("rows", "timesteps", "running", "finished")

    def __init__(self, rows, timesteps, running, finished):
        self.rows, self.timesteps, self.running, self.finished = rows, timesteps, running, finished


class SessionPlan:
    def __init__(self, slots: int, scheduler):
        if int(slots) < 1:
            raise ValueError(f"slots must be >= 1, got {slots}")
        check_scheduler(scheduler)
        self.S = int(slots)
        self.scheduler = scheduler
        self.K = int(getattr(scheduler, "history", 0)) if hasattr(scheduler, "plan") else 0          # history slots of the device buffer
        self._slots: List[Optional[PlanRun]] = [None] * self.S
        self.queue = deque()
        self.idle_row = ops.sampler_coef_row(ops.sampler_coefs(), active=False)

    def submit(self, num_inference_steps: int, payload=None) -> PlanRun:
        run = PlanRun(self.scheduler, num_inference_steps, payload)
        self.queue.append(run)
        return run

    def admit(self) -> List[PlanRun]:
        """Move queued runs into free slots: the queue is FIFO, slots are taken lowest index first."""
        taken = []
        for s in range(self.S):
            if not self.queue:
                break
            if self._slots[s] is None:
                run = self.queue.popleft()
                run.slot = s
                self._slots[s] = run
                taken.append(run)
        return taken

    def cancel(self, run: PlanRun) -> None:
        """drop a run that has not finished (a failed admission): its slot is free again"""
        if run in self.queue:
            self.queue.remove(run)
        if run.slot is not None and self._slots[run.slot] is run:
            self._slots[run.slot] = None

    def next_rows(self) -> PlanStep:
        """The coming step: one coefficient row and one timestep per slot (inactive rows for free slots).  Every running request
        advances; one that takes its last step is reported finished and its slot is free from the next step on."""
        rows, ts, running, finished = [], [], [], []
        for s, run in enumerate(self._slots):
            if run is None:
                rows.append(list(self.idle_row))
                ts.append(None)
                continue
            ts.append(run.timesteps[run.i])
            running.append((s, run, run.i))
            rows.append(ops.sampler_coef_row(run.next_coefs(), active=True))
            run.i += 1
            if run.done:
                finished.append(run)
                self._slots[s] = None
        return PlanStep(rows, ts, running, finished)

    def slot_runs(self) -> List[Optional[PlanRun]]:
        return list(self._slots)

    @property
    def running(self) -> int:
        return sum(r is not None for r in self._slots)

    @property
    def pending(self) -> int:
        return len(self.queue)

    @property
    def free_slots(self) -> List[int]:
        return [s for s, r in enumerate(self._slots) if r is None]


# ---- tickets ----
class SessionTicket:
    """Handle of one submitted request: ``done``, ``slot`` (None while it waits in the queue; the first of ``slots`` for a request of
    several images), ``steps_done``, ``latents`` ([n, 4, h, w] fp32 once done) and ``result()`` -- the pipeline's output object."""

    def __init__(self, request: "_Request"):
        self._request = request
        self._runs: List[PlanRun] = []
        self._latents: List[Optional[torch.Tensor]] = []
        self._output = None
        self.error: Optional[BaseException] = None
        self.latents: Optional[torch.Tensor] = None

    @property
    def done(self) -> bool:
        return self._output is not None

    @property
    def slots(self) -> List[Optional[int]]:
        return [r.slot for r in self._runs]

    @property
    def slot(self) -> Optional[int]:
        return self._runs[0].slot

    @property
    def steps_done(self) -> int:
        return min(r.i for r in self._runs)

    def result(self):
        if self.error is not None:
            raise RuntimeError("the request was dropped by the session") from self.error
        if not self.done:
            raise RuntimeError(f"the request has not finished ({self.steps_done} of {self._runs[0].steps} steps done): step() or drain() "
                               "the session first")
        return self._output


class _Request:
    """the arguments of one ``submit`` and, from the first admission on, what was computed from them"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.prepared = False
        self.temb: Dict[int, list] = {}          # image j -> per-encoder time-embedding table of its schedule, while it runs


# ---- the device state ----
class DenoiseSession:
    """``pipe.open_session(slots=S, width=W, height=H)``; a context manager.  See the module docstring."""

    def __init__(self, pipe, slots: int, width: int, height: int, controlnet_conditioning_scale: float = 1.0, with_controlnet: bool = False):
        check_pipeline(pipe)
        self.plan = SessionPlan(slots, pipe.scheduler)
        self.pipe = pipe
        vsf = pipe.vae_scale_factor
        if int(width) % vsf or int(height) % vsf:
            raise ValueError(f"width x height {width} x {height} must be multiples of {vsf}")
        self.S, self.width, self.height = int(slots), int(width), int(height)
        self.h, self.w = self.height // vsf, self.width // vsf
        self.HW = self.h * self.w
        self.controlnet = pipe.controlnet if with_controlnet else None
        if with_controlnet and self.controlnet is None:
            raise ValueError("open_session: this pipeline was built without a ControlNet")
        self.control_scale = float(controlnet_conditioning_scale)
        dev, dt, S = pipe.device, pipe.unet.dtype, self.S
        self.device, self.dtype = dev, dt
        ops.ensure_device(dev)
        # fixed-address buffers, one row (or CFG pair of rows) per slot.  Zero-filled: the rows of a free slot stay finite
        self.z = torch.zeros(S, self.HW, 4, dtype=torch.float32, device=dev)
        self.x_in = torch.zeros(2 * S, self.h, self.w, 8, dtype=dt, device=dev)
        self.hist = torch.zeros(self.plan.K, S, self.HW, 4, dtype=torch.float32, device=dev) if self.plan.K else None
        self.mask_rows = torch.zeros(2 * S, dtype=torch.float32, device=dev)          # [image_scale of the cond rows; 0 for the uncond rows]
        self.guidance = torch.ones(S, dtype=torch.float32, device=dev)
        self.coef_rows = torch.zeros(S, ops.SAMPLER_ROW_FLOATS, dtype=torch.float32, device=dev)
        self.encoders = [m for m in [pipe.unet] + ([self.controlnet] if self.controlnet is not None else []) if hasattr(m, "use_time_embedding")]
        if len(self.encoders) != (2 if self.controlnet is not None else 1):
            raise TypeError("open_session needs the engine UNet / ControlNet (imagdressing_amd.unet): per-row time embeddings")
        self.temb = [torch.zeros(2 * S, e.temb_proj.weight.shape[0], dtype=torch.float32, device=dev) for e in self.encoders]
        self.ctrl_img = torch.zeros(2 * S, self.height, self.width, 8, dtype=dt, device=dev) if self.controlnet is not None else None
        self.ehs = None                                   # [2S, T, C] text context, [cond; uncond]: allocated at the first admission
        self.garment: Optional[Dict[str, torch.Tensor]] = None          # name -> [S, M_l, C_l]
        self.cak = None
        self.closed = False
        self.steps_run = 0
        self._tickets: List[SessionTicket] = []

    # ---- context manager ----
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        """Release every buffer and the encoders' time-embedding state; unfinished tickets are dropped."""
        for e in getattr(self, "encoders", []):
            e.clear_time_embeddings()
        if self.closed:
            return
        self.closed = True
        for t in self._tickets:
            if not t.done and t.error is None:
                t.error = RuntimeError("the session was closed")
        self._tickets = []
        self.plan = None
        for name in ("z", "x_in", "hist", "mask_rows", "guidance", "coef_rows", "temb", "ctrl_img", "ehs", "garment", "cak"):
            setattr(self, name, None)

    def _check_open(self):
        if self.closed:
            raise RuntimeError("the session is closed")

    # ---- requests ----
    def submit(self, prompt=None, null_prompt=None, negative_prompt=None, ref_image=None, *, num_inference_steps: int,
               guidance_scale: float, ref_clip_image=None, pose_image=None, image_scale: float = 1.0, num_images_per_prompt: int = 1,
               generator=None, output_type: Optional[str] = "pil", clip_skip: Optional[int] = None, prompt_embeds=None,
               negative_prompt_embeds=None, ref_clip_hidden_states=None, ref_image_latents=None, latents=None,
               width: Optional[int] = None, height: Optional[int] = None, eta: float = 0.0, shard_over_ranks: bool = False,
               control_guidance_start: float = 0.0, control_guidance_end: float = 1.0) -> SessionTicket:
        """Queue one request (the per-request arguments of the pipeline's ``__call__``, with ``num_inference_steps``, ``guidance_scale``
        and ``image_scale`` per request) and return its ticket.  Never blocks and launches nothing: the request is admitted at the
        start of the first ``step()`` in which a slot is free.  ``num_images_per_prompt`` = n takes n slots."""
        self._check_open()
        check_request(size=(self.width, self.height), width=width, height=height, num_inference_steps=num_inference_steps,
                      guidance_scale=guidance_scale, image_scale=image_scale, eta=eta, shard_over_ranks=shard_over_ranks,
                      control_guidance_start=control_guidance_start, control_guidance_end=control_guidance_end,
                      num_images_per_prompt=num_images_per_prompt, slots=self.S)
        n = int(num_images_per_prompt)
        if self.controlnet is not None and pose_image is None:
            raise ValueError("pose_image: every request of a ControlNet session brings its pose image")
        if self.controlnet is None and pose_image is not None:
            raise ValueError("pose_image: this session was opened on the pipeline without a ControlNet")
        if latents is not None and tuple(latents.shape) != (n, 4, self.h, self.w):
            raise ValueError(f"latents {tuple(latents.shape)}: this session's requests have latents {(n, 4, self.h, self.w)} "
                             f"({self.width} x {self.height}, one geometry per session)")
        req = _Request(prompt=prompt, null_prompt=null_prompt, negative_prompt=negative_prompt, ref_image=ref_image, ref_clip_image=ref_clip_image,
                       pose_image=pose_image, guidance_scale=float(guidance_scale), image_scale=float(image_scale), n=n, generator=generator,
                       output_type=output_type, clip_skip=clip_skip, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                       ref_clip_hidden_states=ref_clip_hidden_states, ref_image_latents=ref_image_latents, latents=latents)
        ticket = SessionTicket(req)
        for j in range(n):
            ticket._runs.append(self.plan.submit(num_inference_steps, payload=(ticket, j)))
            ticket._latents.append(None)
        self._tickets.append(ticket)
        return ticket

    def _prepare(self, req: _Request, run: PlanRun):
        """Once per request, at its first admission: prompt encoding, the garment UNet at batch 1, the pose image, the start latents."""
        from .dressing_sd.pipelines._base import as_batch, randn_tensor
        from .unet import nchw_to_nhwc8
        pipe, dev, dt = self.pipe, self.device, self.dtype
        pe, ne = pipe.encode_prompt(req.prompt, dev, 1, True, req.negative_prompt, prompt_embeds=req.prompt_embeds,
                                    negative_prompt_embeds=req.negative_prompt_embeds, clip_skip=req.clip_skip)
        if pe.shape[0] != 1 or ne.shape[0] != 1:
            raise ValueError(f"a session request has one prompt: prompt embeds {tuple(pe.shape)}, negative {tuple(ne.shape)}")
        req.pe, req.ne = pe.to(device=dev, dtype=dt), ne.to(device=dev, dtype=dt)
        ref_lat, cloth_tokens, _ = pipe._request_garments(1, req.null_prompt, req.ref_image, req.ref_image_latents, req.ref_clip_image,
                                                          req.ref_clip_hidden_states, dev)
        # (the tensors returned are the garment UNet's own caches: the next admission overwrites them, the slot rows are copies)
        req.features = {k: v.clone() for k, v in pipe._garment_features(ref_lat, cloth_tokens).items()}
        req.pose = None
        if self.controlnet is not None:
            img, hw = pipe._image_tensor(as_batch(req.pose_image, "pose_image"), dev, normalize=False, size=(self.height, self.width),
                                         multiple=pipe.vae_scale_factor, layout="nhwc8")
            if tuple(hw) != (self.height, self.width) or img.shape[0] != 1:
                raise ValueError(f"pose_image gives {img.shape[0]} image(s) of {tuple(hw)}: a session request has one of {(self.height, self.width)}")
            req.pose = img if (img.dim() == 4 and img.shape[-1] == 8 and img.dtype == dt) else nchw_to_nhwc8(img.to(dev), dt)
        lat = req.latents
        if lat is None:
            lat = randn_tensor((req.n, 4, self.h, self.w), generator=req.generator, device=dev, dtype=torch.float32)
        req.z0 = (lat.to(device=dev, dtype=torch.float32) * run.scheduler.init_noise_sigma).permute(0, 2, 3, 1).reshape(req.n, self.HW, 4).contiguous()
        req.prepared = True

    def _allocate_context(self, req: _Request):
        S, dev, dt = self.S, self.device, self.dtype
        self.ehs = torch.zeros(2 * S, req.pe.shape[1], req.pe.shape[2], dtype=dt, device=dev)
        self.garment = {k: torch.zeros(S, v.shape[1], v.shape[2], dtype=v.dtype, device=dev) for k, v in req.features.items()}
        # sa_pair_layout: garment on for the cond rows [0, S) (weight = the slot's image_scale), off for the uncond rows [S, 2S)
        self.cak = {"sa_hidden_states": self.garment, "sa_batch_mask": self.mask_rows, "sa_pair_layout": True}

    def _admit(self, run: PlanRun):
        """Write the slot's rows of every buffer in place (nothing outside the slot is touched).  The writes bump the tensors'
        versions, so the processors' step-invariant K / V caches and the ControlNet's conditioning embedding refresh for ALL slots
        on the next forward."""
        ticket, j = run.payload
        req, s, S = ticket._request, run.slot, self.S
        if not req.prepared:
            self._prepare(req, run)
        if self.ehs is None:
            self._allocate_context(req)
        if tuple(req.pe.shape[1:]) != tuple(self.ehs.shape[1:]) or tuple(req.ne.shape[1:]) != tuple(self.ehs.shape[1:]):
            raise ValueError(f"prompt embeds {tuple(req.pe.shape)} / {tuple(req.ne.shape)}: this session's text context rows are {tuple(self.ehs.shape[1:])}")
        for k, v in req.features.items():
            if k not in self.garment or tuple(v.shape[1:]) != tuple(self.garment[k].shape[1:]):
                raise ValueError(f"garment features of layer {k}: {tuple(v.shape)} does not fit this session's {tuple(self.garment.get(k, v).shape)}")
        z0 = req.z0[j]
        self.z[s].copy_(z0)
        scale = run.first_input_scale()
        zin = (z0 if scale == 1.0 else z0 * scale).view(self.h, self.w, 4)
        self.x_in[s, ..., :4] = zin
        self.x_in[S + s, ..., :4] = zin
        self.ehs[s].copy_(req.pe[0])
        self.ehs[S + s].copy_(req.ne[0])
        for k, v in req.features.items():
            self.garment[k][s].copy_(v[0])
        self.mask_rows[s] = req.image_scale
        self.guidance[s] = req.guidance_scale
        if self.ctrl_img is not None:
            self.ctrl_img[s].copy_(req.pose[0])
            self.ctrl_img[S + s].copy_(req.pose[0])
        ts = torch.tensor([float(t) for t in run.timesteps], dtype=torch.float32).to(self.device)
        req.temb[j] = [e._time_embed_rows(ts) for e in self.encoders]          # the request's whole schedule, once

    # ---- the step ----
    @torch.no_grad()
    def step(self) -> List[SessionTicket]:
        """Admit from the queue, run ONE UNet (+ ControlNet) forward over all slots and ONE fused step launch; returns the tickets
        that finished, decoded for their own ``output_type``."""
        self._check_open()
        check_pipeline(self.pipe)
        with ops.tuning_scope(**(getattr(self.pipe, "_tuning", None) or {})):
            return self._step()

    def _step(self) -> List[SessionTicket]:
        pipe, S = self.pipe, self.S
        for run in self.plan.admit():
            try:
                self._admit(run)
            except BaseException as e:
                ticket = run.payload[0]
                ticket.error = e
                for r in ticket._runs:          # the whole request leaves: its slots and queue entries are free again
                    if not r.done:
                        self.plan.cancel(r)
                raise
        if not self.plan.running:
            return []
        st = self.plan.next_rows()
        for s, run, i in st.running:          # each slot's time-embedding row, the same in both CFG halves
            ticket, j = run.payload
            for buf, table in zip(self.temb, ticket._request.temb[j]):
                buf.view(2, S, -1)[:, s].copy_(table[i])
        self.coef_rows.copy_(torch.tensor(st.rows, dtype=torch.float32))
        pipe.set_scale(1.0)                   # the slots' image scales ride in the sa_batch_mask rows
        try:
            for e, buf in zip(self.encoders, self.temb):
                e.use_time_embedding(buf)
            down = mid = None
            if self.controlnet is not None:
                down, mid = self.controlnet.forward_nhwc(self.x_in, 0, self.ehs, self.ctrl_img, self.control_scale)
            eps = pipe.unet.forward_nhwc(self.x_in, 0, self.ehs, self.cak, down, mid, cfg_pair=True)
        finally:
            for e in self.encoders:
                e.clear_time_embeddings()
        ops.sampler_step_rows(self.z, eps, self.x_in.view(2 * S, self.HW, 8), guidance=self.guidance, coef_rows=self.coef_rows, hist=self.hist)
        self.steps_run += 1
        finished = []
        for run in st.finished:
            ticket, j = run.payload
            ticket._latents[j] = self.z[run.slot].view(1, self.h, self.w, 4).permute(0, 3, 1, 2).contiguous()
            ticket._request.temb.pop(j, None)
            if all(t is not None for t in ticket._latents):
                ticket.latents = torch.cat(ticket._latents)
                ticket._output = pipe._decode(ticket.latents, ticket._request.output_type, ticket._request.generator)
                self._tickets.remove(ticket)
                finished.append(ticket)
        return finished

    def drain(self) -> List[SessionTicket]:
        """step until nothing is running or queued -> every ticket that finished on the way"""
        out = []
        while not self.closed and (self.plan.running or self.plan.pending):
            out += self.step()
        return out

    @property
    def free_slots(self) -> List[int]:
        self._check_open()
        return self.plan.free_slots


__all__ = ["SessionPlan", "PlanRun", "PlanStep", "DenoiseSession", "SessionTicket", "check_scheduler", "check_pipeline", "check_request"]
