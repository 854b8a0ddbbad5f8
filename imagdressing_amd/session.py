"""In-flight batching: a denoising session with a fixed number of slots that admits requests at any step.

A request-batched pipeline call needs all its requests in hand before it starts, and all of them run the same number of steps.  A
session keeps ONE batch of ``slots`` latent rows alive across calls instead: a request enters a free slot at the start of any step,
runs its own schedule (its own step count, its own position in it) and leaves when done.  Every :meth:`DenoiseSession.step` is one
UNet forward (plus ControlNet) over all 2 x slots rows of the CFG batch and one fused step launch (``imd_sampler_step_rows``) that
gives every latent row its own coefficients, its own history slots and its own "this row is not running" flag.  A session has ONE
scheduler, so every row of a step goes through the same kernel: a UniPC whose fused-step switch is on runs on ``imd_unipc_step_rows``
(24-float rows, ``solver_order + 1`` history planes), every other sampler on ``imd_sampler_step_rows``.

Two kinds of index.  A SLOT is the home of a request's per-latent state -- the fp32 latent ``z[S, HW, 4]`` and the history
``hist[K, S, HW, 4]``; slots are taken lowest free index first and these buffers never move.  A ROW is a position in the batch the
forward runs: at width B the batch is [cond rows 0..B-1 ; uncond rows B..2B-1].  By default the width is always ``slots`` and row =
slot: an under-full session pays for its idle rows (tools/session_bench.py measures how much).  With ``compact=True`` the width is
the smallest entry of the ``widths`` ladder that holds the running requests; when it changes the step REPACKS (the running slots take
rows 0, 1, ... in ascending slot order and their rows of every batch buffer are rewritten from what the request keeps, the UNet input
from the fp32 latent by ``imd_session_input_rows``), otherwise rows stay where they are.  The step launch then goes through the device
map row -> slot (``imd_sampler_step_rows_at``).  A forward at another batch width may be dispatched to other tile configurations, so
with ``compact=True`` a request's bits depend on the sequence of widths it ran under; the default session is unchanged bit for bit.

Two layers, so that the logic is testable without a GPU:

* :class:`SessionPlan` -- pure Python: slot allocation (lowest free index first), the FIFO queue, one scheduler instance /
  :class:`~imagdressing_amd.scheduler.SamplerHistory` (UniPC: ``UniPCHistory``) / position per request, the width and the row of every
  slot, and per step one 16-float (UniPC: 24-float) coefficient row and one timestep per slot and per row.
* :class:`DenoiseSession` -- the device state: fixed-address buffers for every slot and, at capacity, for every row (one view object
  per width and buffer), admission (prompt encoding, the garment UNet at batch 1, in-place writes of the row), the step, tickets.
"""
from __future__ import annotations

import copy
import math
from collections import deque
from typing import Any, Dict, List, Optional

import torch

from . import ops
from .noise import RequestNoise, check_seed, resolve_seeds, step_draw
from .scheduler import DDIMScheduler, SamplerHistory, UniPCHistory, ddim_row, unipc_fused


# ---- refusals (pure: nothing here touches a device) ----
def check_scheduler(scheduler, *, device_noise: bool = False) -> None:
    """The samplers a session can drive: every deterministic one whose step is ONE affine row -- DPM-Solver++, Euler, PNDM
    (``plan``), DDIM (``ddim_row``) and UniPC with ``enable_fused_step()`` (``plan_fused``).  ``device_noise`` (the session draws its
    noise per request on the device, ``imd_noise_rows``): Euler-ancestral too."""
    name = type(scheduler).__name__
    if unipc_fused(scheduler):
        return
    if hasattr(scheduler, "step_guided"):
        raise NotImplementedError(f"open_session: scheduler {name} (UniPC) updates the latents with host-built linear combinations of "
                                  "whole tensors, not one affine row per latent row; use DPM-Solver++, Euler, PNDM or DDIM")
    if getattr(scheduler, "stochastic", False) and not device_noise:
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
                  shard_over_ranks=False, control_guidance_start=0.0, control_guidance_end=1.0, num_images_per_prompt=1, slots=1,
                  guidance_rescale=0.0, device_noise=False, scheduler=None, seed=None, controlnet_conditioning_scale=None,
                  control_rows=False) -> None:
    """what ``submit`` refuses, before anything is launched or queued.  ``size`` = (width, height) of the session.  ``device_noise``
    (the session draws its noise per request on the device): ``eta`` > 0 is accepted where ``scheduler`` is DDIM and raises ValueError
    for any other sampler, ``seed`` must be None or an int in [0, 2^64); without it ``eta`` > 0 and ``seed`` are refused.
    ``control_rows`` (the session scales the ControlNet residuals per batch row): ``controlnet_conditioning_scale`` is None (the
    session's) or one finite value and the window needs 0 <= start < end <= 1; without it a scale per request and any window other
    than 0 / 1 are refused."""
    for name, v in (("num_inference_steps", num_inference_steps), ("guidance_scale", guidance_scale), ("image_scale", image_scale),
                    ("guidance_rescale", guidance_rescale)):
        if isinstance(v, (list, tuple)):
            raise ValueError(f"{name} is per request in a session: submit one request per call, got {list(v)}")
    if float(eta) > 0.0 and not device_noise:
        raise NotImplementedError("eta > 0: the stochastic DDIM step draws noise per step; a session runs the deterministic samplers")
    if not device_noise and seed is not None:
        raise ValueError("seed= is the request seed of the device noise source: open the session with device_noise=True or call "
                         "pipe.enable_device_noise() first")
    if device_noise:
        if isinstance(eta, (list, tuple)) or not (math.isfinite(float(eta)) and float(eta) >= 0.0):
            raise ValueError(f"eta must be one finite value >= 0 per request, got {eta!r}")
        if float(eta) > 0.0 and scheduler is not None and not isinstance(scheduler, DDIMScheduler):
            raise ValueError(f"eta > 0 is the stochastic DDIM step; this session's sampler is {type(scheduler).__name__}")
        if seed is not None:
            check_seed(seed)
    if shard_over_ranks:
        raise NotImplementedError("shard_over_ranks: a session lives on one rank (sessions over several ranks are a later change)")
    if (width is not None and int(width) != int(size[0])) or (height is not None and int(height) != int(size[1])):
        raise ValueError(f"width x height {width} x {height}: this session was opened for {size[0]} x {size[1]} (one geometry per session)")
    if control_rows:
        for name, v in (("controlnet_conditioning_scale", controlnet_conditioning_scale), ("control_guidance_start", control_guidance_start),
                        ("control_guidance_end", control_guidance_end)):
            if isinstance(v, (list, tuple)):
                raise ValueError(f"{name} is per request in a session: submit one request per call, got {list(v)}")
        if controlnet_conditioning_scale is not None and not math.isfinite(float(controlnet_conditioning_scale)):
            raise ValueError(f"controlnet_conditioning_scale must be finite, got {controlnet_conditioning_scale}")
        a, b = float(control_guidance_start), float(control_guidance_end)
        if not (math.isfinite(a) and math.isfinite(b) and 0.0 <= a < b <= 1.0):
            raise ValueError(f"control_guidance_start / control_guidance_end: need 0 <= start < end <= 1, got start = {a}, end = {b}")
    elif controlnet_conditioning_scale is not None:
        raise NotImplementedError("controlnet_conditioning_scale per request: this session was opened without control_rows, its ControlNet "
                                  "scale is the one given at open_session (out_scale of the zero-conv launches)")
    elif float(control_guidance_start) != 0.0 or float(control_guidance_end) != 1.0:
        raise NotImplementedError("control_guidance_start / control_guidance_end other than 0 / 1: the ControlNet gate is one scalar "
                                  "per launch (the zero-conv epilogue), the rows of a session are at different steps")
    if float(guidance_scale) <= 1.0:
        raise NotImplementedError("guidance_scale <= 1: the reference's loop indexes the CFG pair unconditionally "
                                  "(IMAGDressing_v1_pipeline.py:476-479, :511); sample with guidance_scale > 1")
    if int(num_inference_steps) < 1:
        raise ValueError(f"num_inference_steps must be >= 1, got {num_inference_steps}")
    if not (math.isfinite(float(guidance_rescale)) and 0.0 <= float(guidance_rescale) <= 1.0):
        raise ValueError(f"guidance_rescale must be finite and in [0, 1], got {guidance_rescale}")
    if not 1 <= int(num_images_per_prompt) <= int(slots):
        raise ValueError(f"num_images_per_prompt = {num_images_per_prompt} takes that many slots; the session has {slots}")


# ---- the plan ----
class PlanRun:
    """One latent row's run: its own scheduler instance (``set_timesteps(n)``), history bookkeeping and position."""
    __slots__ = ("scheduler", "ring", "timesteps", "steps", "i", "slot", "row", "in_scale", "ready", "payload", "seed", "image", "eta", "control")

    def __init__(self, scheduler, num_inference_steps: int, payload=None, seed: Optional[int] = None, image: int = 0, eta: float = 0.0,
                 control=None):
        # the noise key of the run (a plan with device_noise): the request's seed and the image index inside the request; eta: DDIM's
        self.seed, self.image, self.eta = seed, int(image), float(eta)
        sch = copy.copy(scheduler)          # the class and configuration of the pipeline's scheduler; set_timesteps rebinds, never mutates
        sch.set_timesteps(int(num_inference_steps))
        self.scheduler = sch
        if self.unipc:
            self.timesteps = [t.item() for t in sch.timesteps]
            self.steps = sch.steps()
            self.ring = UniPCHistory(sch.history)
        elif self.affine:
            self.timesteps = [t.item() for t in sch.timesteps]          # (fractional ones reach the time embedding unrounded)
            self.steps = sch.steps()                                       # UNet calls: PNDM has one more than it has steps
            self.ring = SamplerHistory(sch.history)
        else:
            self.timesteps = [int(t) for t in sch.timesteps]
            self.steps = len(self.timesteps)
            self.ring = SamplerHistory(0)
        # control = (scale, start, end) of a plan with control_rows -> the effective ControlNet scale of every UNet call of the run:
        # scale * controlnet_keep(num_inference_steps, start, end)[i]; a call past the gate (PNDM's extra one) keeps the last entry
        self.control: Optional[List[float]] = None
        if control is not None:
            scale, start, end = (float(c) for c in control)
            n = int(num_inference_steps)
            keep = [1.0 - float(k / n < start or (k + 1) / n > end) for k in range(n)]          # diffusers' gate (pipelines._base.controlnet_keep)
            self.control = [scale * keep[min(k, n - 1)] for k in range(self.steps)]
        self.i = 0
        self.slot: Optional[int] = None
        self.row: Optional[int] = None          # its position in the batch the forward runs (== slot unless the plan compacts)
        self.in_scale = self.first_input_scale()          # what its current UNet input was scaled with: coefficient [11] of its last step
        self.ready = False          # for the plan's caller: what an admission has to set up (device state) is in place
        self.payload = payload

    @property
    def affine(self) -> bool:
        """a ``plan`` sampler (DPM-Solver++, Euler, PNDM); otherwise DDIM through ``ddim_row``"""
        return hasattr(self.scheduler, "plan")

    @property
    def unipc(self) -> bool:
        """UniPC on the fused step (``plan_fused``, 19 coefficients)"""
        return unipc_fused(self.scheduler)

    @property
    def done(self) -> bool:
        return self.i >= self.steps

    def first_input_scale(self) -> float:
        """``scale_model_input`` of the first step (later inputs come scaled out of the step launch)"""
        return float(self.scheduler.input_scale(0)) if self.affine else 1.0

    def next_coefs(self) -> List[float]:
        """the 13 coefficients of step ``i`` (UniPC: the 19 of ``ops.unipc_coefs``) -- and the history bookkeeping advances"""
        if self.unipc:
            coefs = self.ring.coefs(self.scheduler.plan_fused(self.i))
            self.in_scale = coefs[ops.UNIPC_IN_SCALE]
            return coefs
        row = self.scheduler.plan(self.i) if self.affine else ddim_row(self.scheduler, self.timesteps[self.i], self.eta)
        coefs = self.ring.coefs(row)
        self.in_scale = coefs[11]
        return coefs

    @property
    def noisy(self) -> bool:
        """its steps read the noise operand: Euler-ancestral, or DDIM with eta > 0"""
        return bool(getattr(self.scheduler, "stochastic", False)) or (not self.affine and not self.unipc and self.eta > 0.0)


class PlanStep:
    """What one step launches: ``rows`` [slots][16] floats, ``timesteps`` [slots] (None for a free slot), ``running`` = (slot, run,
    position) of every row that takes this step, ``finished`` = the runs for which it is the last.  And the same step seen by batch
    ROW: ``width`` rows ran, row r carried slot ``row_slot[r]`` (-1: idle) with the coefficient row ``coef_rows[r]`` and the timestep
    ``row_timesteps[r]``; ``repack`` = the rows were laid out anew before this step.  A plan that does not compact has width =
    slots, row r = slot r and never repacks.  A plan with ``device_noise``: ``noise`` = (slot, seed, image, draw) of every running
    row whose step reads noise and ``key_rows`` [slots][8] = the ``ops.noise_key_row`` of every SLOT for this step (inactive for
    every other slot), whether the plan compacts or not; otherwise both are None.  A plan with ``control_rows``: ``control_rows``
    [2 width] = the effective ControlNet scale of every batch ROW for this step, the cond rows then the same values for their uncond
    twins, 1.0 for an idle row (``imd_residual_scale_rows`` skips it); otherwise None."""
    __slots__ = ("rows", "timesteps", "running", "finished", "width", "row_slot", "repack", "coef_rows", "row_timesteps", "noise", "key_rows",
                 "control_rows")

    def __init__(self, rows, timesteps, running, finished, width=None, row_slot=None, repack=False, coef_rows=None, row_timesteps=None,
                 noise=None, key_rows=None, control_rows=None):
        self.rows, self.timesteps, self.running, self.finished = rows, timesteps, running, finished
        self.noise, self.key_rows, self.control_rows = noise, key_rows, control_rows
        self.width = len(rows) if width is None else width
        self.row_slot = list(range(len(rows))) if row_slot is None else row_slot
        self.repack = repack
        self.coef_rows = rows if coef_rows is None else coef_rows
        self.row_timesteps = timesteps if row_timesteps is None else row_timesteps


class PlanLayout:
    """The batch of the coming step: ``width`` rows, ``rows`` [width] = the run of each row or None, ``repack`` = every running
    request was given a new row (ascending slot order), ``placed`` = the runs that entered a row without one (none at a repack)."""
    __slots__ = ("width", "rows", "repack", "placed")

    def __init__(self, width, rows, repack, placed):
        self.width, self.rows, self.repack, self.placed = width, rows, repack, placed


def check_widths(slots: int, widths) -> tuple:
    """the ladder of batch widths of a compacting plan: None = every width 1..slots, else strictly increasing ints in 1..slots
    that end at slots"""
    S = int(slots)
    if widths is None:
        return tuple(range(1, S + 1))
    try:
        w = tuple(widths)
    except TypeError:
        raise ValueError(f"widths must be None or a tuple of ints, got {widths!r}") from None
    if not w or any(isinstance(v, bool) or not isinstance(v, int) for v in w):
        raise ValueError(f"widths must be a non-empty tuple of ints, got {widths!r}")
    if any(not 1 <= v <= S for v in w) or any(a >= b for a, b in zip(w, w[1:])) or w[-1] != S:
        raise ValueError(f"widths must be strictly increasing, within 1..{S} and end at slots = {S}, got {widths!r}")
    return w


class SessionPlan:
    def __init__(self, slots: int, scheduler, compact: bool = False, widths=None, *, device_noise: bool = False, control_rows: bool = False,
                 control_scale: float = 1.0):
        if int(slots) < 1:
            raise ValueError(f"slots must be >= 1, got {slots}")
        check_scheduler(scheduler, device_noise=bool(device_noise))
        self.device_noise = bool(device_noise)
        # control_rows: every run carries its own ControlNet scale and window (control_scale: the scale of a run that names none)
        self.control_rows, self.control_scale = bool(control_rows), float(control_scale)
        # the step launch may be handed a noise operand: the session's sampler can be stochastic (Euler-ancestral, or DDIM -- eta is per request)
        self.noisy = self.device_noise and not unipc_fused(scheduler) and (bool(getattr(scheduler, "stochastic", False))
                                                                         or isinstance(scheduler, DDIMScheduler))
        self.S = int(slots)
        self.compact = bool(compact)
        if widths is not None and not self.compact:
            raise ValueError("widths is the ladder of a compacting session: pass compact=True with it")
        self.widths = check_widths(self.S, widths) if self.compact else (self.S,)
        self.scheduler = scheduler
        self.unipc = unipc_fused(scheduler)          # every row of a step goes through ONE kernel: imd_unipc_step_rows or imd_sampler_step_rows
        self.K = int(getattr(scheduler, "history", 0)) if hasattr(scheduler, "plan") or self.unipc else 0          # history slots of the device buffer
        self._slots: List[Optional[PlanRun]] = [None] * self.S
        self.queue = deque()
        self.coef_row = ops.unipc_coef_row if self.unipc else ops.sampler_coef_row
        self.row_floats = ops.UNIPC_ROW_FLOATS if self.unipc else ops.SAMPLER_ROW_FLOATS
        self.idle_row = self.coef_row(ops.unipc_coefs() if self.unipc else ops.sampler_coefs(), active=False)
        # the batch: width 0 until the first step lays it out (nothing to move: that is no repack)
        self.width = 0 if self.compact else self.S
        self._rows: List[Optional[PlanRun]] = [] if self.compact else [None] * self.S
        self._laid: Optional[PlanLayout] = None
        self.repacks = 0

    def submit(self, num_inference_steps: int, payload=None, *, seed: Optional[int] = None, image: int = 0, eta: float = 0.0,
               control=None) -> PlanRun:
        """``seed`` / ``image`` (a plan with ``device_noise``): the noise key of the run; ``eta`` > 0: the stochastic DDIM step;
        ``control`` (a plan with ``control_rows``): (scale or None = the plan's, start, end) of the run's ControlNet gate"""
        if control is not None and not self.control_rows:
            raise NotImplementedError("a ControlNet scale or window per run: the plan was made without control_rows")
        if self.control_rows:
            scale, start, end = control if control is not None else (None, 0.0, 1.0)
            control = (self.control_scale if scale is None else scale, start, end)
        if unipc_fused(self.scheduler) != self.unipc:
            raise RuntimeError("the scheduler's fused-step switch changed since the session was opened: its buffers and its step kernel "
                               "were chosen for the other setting; open a new session")
        if float(eta) > 0.0 and not self.device_noise:
            raise NotImplementedError("eta > 0: the stochastic DDIM step draws noise per step; a session runs the deterministic samplers")
        if float(eta) > 0.0 and not isinstance(self.scheduler, DDIMScheduler):
            raise ValueError(f"eta > 0 is the stochastic DDIM step; this session's sampler is {type(self.scheduler).__name__}")
        run = PlanRun(self.scheduler, num_inference_steps, payload, seed=seed, image=image, eta=eta, control=control)
        if self.noisy and run.noisy and seed is None:
            raise ValueError("a run whose steps read noise needs its request's seed (DenoiseSession.submit resolves it)")
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
        """drop a run that has not finished (a failed admission): its slot is free again (and its row, had it one).  Call it
        before ``layout()`` of the step, which counts the running slots."""
        if run in self.queue:
            self.queue.remove(run)
        if run.slot is not None and self._slots[run.slot] is run:
            self._slots[run.slot] = None
        if run.row is not None and run.row < len(self._rows) and self._rows[run.row] is run:
            self._rows[run.row] = None
        run.row = None

    def required_width(self) -> int:
        """the smallest entry of the ladder that holds every running slot"""
        n = self.running
        return next(w for w in self.widths if w >= n)

    def layout(self) -> PlanLayout:
        """Give every running slot its batch row for the coming step (after ``admit``; ``next_rows`` calls it if the caller did
        not).  The width is the smallest ladder entry >= the running slots.  If it differs from the current width the step REPACKS:
        the running slots take rows 0, 1, ... in ascending slot order, the rest of the width idles.  Otherwise every row stays where
        it is and each slot without a row (just admitted) takes the lowest idle one.  A plan that does not compact keeps row = slot."""
        if self._laid is not None:
            return self._laid
        live = [r for r in self._slots if r is not None]
        if not self.compact:
            placed = [r for r in live if r.row is None]
            for r in placed:
                r.row = r.slot
                self._rows[r.slot] = r
            self._laid = PlanLayout(self.S, list(self._rows), False, placed)
            return self._laid
        need = self.required_width()
        repack = need != self.width and self.width != 0
        if need != self.width:
            self.width = need
            self._rows = [None] * need
            if repack:
                self.repacks += 1
                for r in live:
                    r.row = None
        placed = []
        for r in live:                                   # ascending slot order
            if r.row is None:
                r.row = self._rows.index(None)
                self._rows[r.row] = r
                placed.append(r)
        self._laid = PlanLayout(need, list(self._rows), repack, [] if repack else placed)
        return self._laid

    def next_rows(self) -> PlanStep:
        """The coming step: one coefficient row and one timestep per slot (inactive rows for free slots).  Every running request
        advances; one that takes its last step is reported finished and its slot (and batch row) is free from the next step on."""
        lay = self.layout()
        self._laid = None
        rows, ts, running, finished = [], [], [], []
        noise = [] if self.noisy else None          # (slot, seed, image, draw): draw 1 + i, i the step index of the run's own schedule
        keys = [ops.noise_key_row(0, 0, 0, active=False) for _ in range(self.S)] if self.noisy else None
        gate = {}                                   # slot -> the effective ControlNet scale of its run for this step
        for s, run in enumerate(self._slots):
            if run is None:
                rows.append(list(self.idle_row))
                ts.append(None)
                continue
            if self.control_rows:
                gate[s] = run.control[run.i]
            ts.append(run.timesteps[run.i])
            running.append((s, run, run.i))
            if self.noisy and run.noisy:
                noise.append((s, run.seed, run.image, step_draw(run.i)))
                keys[s] = ops.noise_key_row(run.seed, run.image, step_draw(run.i))
            rows.append(self.coef_row(run.next_coefs(), active=True))
            run.i += 1
            if run.done:
                finished.append(run)
                self._slots[s] = None
                self._rows[run.row] = None
        if not self.compact:
            ctrl = [gate.get(s, 1.0) for s in range(self.S)] * 2 if self.control_rows else None
            return PlanStep(rows, ts, running, finished, noise=noise, key_rows=keys, control_rows=ctrl)
        row_slot = [-1 if r is None else r.slot for r in lay.rows]
        ctrl = [gate.get(s, 1.0) for s in row_slot] * 2 if self.control_rows else None          # by batch ROW: what a repack moved is written anew
        return PlanStep(rows, ts, running, finished, width=lay.width, row_slot=row_slot, repack=lay.repack, noise=noise, key_rows=keys,
                        control_rows=ctrl,
                        coef_rows=[list(self.idle_row) if s < 0 else rows[s] for s in row_slot],
                        row_timesteps=[None if s < 0 else ts[s] for s in row_slot])

    def slot_runs(self) -> List[Optional[PlanRun]]:
        return list(self._slots)

    def row_runs(self) -> List[Optional[PlanRun]]:
        """the run of every batch row (the rows of the last layout, minus the requests that have finished since)"""
        return list(self._rows)

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
        self.seed: Optional[int] = None          # the request's noise seed (a session with device_noise)

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
class _WidthViews:
    """The first 2B (or B) rows of every batch buffer, as ONE object per buffer for the life of the session: the processors' K / V
    caches and the ControlNet's conditioning cache are keyed on the identity, address and version of the tensors they are handed
    (adapter/attention_processor.py::_TensorCache), a fresh view per step would miss them every step."""

    def __init__(self, ses: "DenoiseSession", B: int):
        self.B = B
        self.x_in = ses.x_in[:2 * B]
        self.x_flat = self.x_in.view(2 * B, ses.HW, 8)
        self.mask_rows = ses.mask_rows[:2 * B]
        self.temb = [t[:2 * B] for t in ses.temb]
        self.temb_pairs = [t.view(2, B, -1) for t in self.temb]
        self.ctrl_img = ses.ctrl_img[:2 * B] if ses.ctrl_img is not None else None
        self.coef_rows = ses.coef_rows[:B]
        self.guidance_rows = ses.guidance_rows[:B] if ses.guidance_rows is not None else None
        self.rescale_rows = ses.rescale_rows[:B] if ses.rescale_rows is not None else None
        self.row_slot = ses.row_slot[:B]
        self.control_rows = ses.control_scale_rows[:2 * B] if ses.control_scale_rows is not None else None
        self.ehs = self.garment = self.cak = None          # with the context buffers, at the first admission

    def bind_context(self, ses: "DenoiseSession"):
        B = self.B
        self.ehs = ses.ehs[:2 * B]
        self.garment = {k: v[:B] for k, v in ses.garment.items()}
        # sa_pair_layout: garment on for the cond rows [0, B) (weight = the row's image_scale), off for the uncond rows [B, 2B)
        self.cak = {"sa_hidden_states": self.garment, "sa_batch_mask": self.mask_rows, "sa_pair_layout": True}


class DenoiseSession:
    """``pipe.open_session(slots=S, width=W, height=H, compact=False, widths=None)``; a context manager.  See the module docstring."""

    def __init__(self, pipe, slots: int, width: int, height: int, controlnet_conditioning_scale: float = 1.0, with_controlnet: bool = False,
                 compact: bool = False, widths=None, device_noise: Optional[bool] = None, control_rows: Optional[bool] = None):
        check_pipeline(pipe)
        # device_noise None: follow the pipeline's switch (enable_device_noise) as it stands when the session opens
        self.device_noise = bool(getattr(pipe, "_device_noise", False)) if device_noise is None else bool(device_noise)
        # control_rows None: follow enable_request_control_scales as it stands when the session opens; a session without a ControlNet has no such rows
        self.control_rows = bool(with_controlnet) and (bool(getattr(pipe, "_request_control_scales", False)) if control_rows is None
                                                       else bool(control_rows))
        if control_rows and not with_controlnet:
            raise ValueError("open_session: control_rows needs a ControlNet; this session has none")
        self.plan = SessionPlan(slots, pipe.scheduler, compact=compact, widths=widths, device_noise=self.device_noise,
                                control_rows=self.control_rows, control_scale=float(controlnet_conditioning_scale))
        self.pipe = pipe
        self.compact = self.plan.compact
        vsf = pipe.vae_scale_factor
        if int(width) % vsf or int(height) % vsf:
            raise ValueError(f"width x height {width} x {height} must be multiples of {vsf}")
        self.S, self.image_width, self.image_height = int(slots), int(width), int(height)
        self.h, self.w = self.image_height // vsf, self.image_width // vsf
        self.HW = self.h * self.w
        # (a MultiControlNetModel of one net is that net; several nets are refused by the pipeline's open_session)
        self.controlnet = (pipe._single_controlnet() if hasattr(pipe, "_single_controlnet") else pipe.controlnet) if with_controlnet else None
        if with_controlnet and self.controlnet is None:
            raise ValueError("open_session: this pipeline was built without a ControlNet")
        self.control_scale = float(controlnet_conditioning_scale)
        dev, dt, S = pipe.device, pipe.unet.dtype, self.S
        self.device, self.dtype = dev, dt
        ops.ensure_device(dev)
        # fixed-address buffers.  Per SLOT (the home of a request's state, never moved): z, hist, guidance.  Per batch ROW, allocated
        # at capacity (width B uses the first 2B or B rows): everything the forward reads.  Zero-filled: idle rows stay finite
        self.z = torch.zeros(S, self.HW, 4, dtype=torch.float32, device=dev)
        self.x_in = torch.zeros(2 * S, self.h, self.w, 8, dtype=dt, device=dev)
        self.hist = torch.zeros(self.plan.K, S, self.HW, 4, dtype=torch.float32, device=dev) if self.plan.K else None
        self.mask_rows = torch.zeros(2 * S, dtype=torch.float32, device=dev)          # [image_scale of the cond rows; 0 for the uncond rows]
        self.guidance = torch.ones(S, dtype=torch.float32, device=dev)
        self.guidance_rows = torch.ones(S, dtype=torch.float32, device=dev) if self.compact else None
        # guidance_rescale beside the guidance: 0 = imd_guidance_rescale leaves the row alone -- the value of every idle slot / row, always
        self.rescale = torch.zeros(S, dtype=torch.float32, device=dev)
        self.rescale_rows = torch.zeros(S, dtype=torch.float32, device=dev) if self.compact else None
        self._rescale_seen = False          # a request with a non-zero value was admitted: repacks then clear the rows first
        # device noise, where the sampler can be stochastic: both by SLOT in plain and compacting sessions alike (imd_sampler_step_rows_at
        # reads noise by slot).  noise is ZERO-FILLED: a row with z_n = 0 multiplies it, so it must never hold uninitialised bytes
        self.noise = torch.zeros(S, self.HW, 4, dtype=torch.float32, device=dev) if self.plan.noisy else None
        self.key_rows = torch.zeros(S, ops.NOISE_ROW_WORDS, dtype=torch.int32, device=dev) if self.plan.noisy else None
        # control_rows: the effective ControlNet scale of every batch ROW, [cond; uncond] at the current width, rewritten whole every step
        # (idle rows 1.0: imd_residual_scale_rows leaves them alone)
        self.control_scale_rows = torch.ones(2 * S, dtype=torch.float32, device=dev) if self.control_rows else None
        self.coef_rows = torch.zeros(S, self.plan.row_floats, dtype=torch.float32, device=dev)
        self.row_slot = torch.arange(S, dtype=torch.int32, device=dev)
        self._row_slot_host = list(range(S))
        self.encoders = [m for m in [pipe.unet] + ([self.controlnet] if self.controlnet is not None else []) if hasattr(m, "use_time_embedding")]
        if len(self.encoders) != (2 if self.controlnet is not None else 1):
            raise TypeError("open_session needs the engine UNet / ControlNet (imagdressing_amd.unet): per-row time embeddings")
        self.temb = [torch.zeros(2 * S, e.temb_proj.weight.shape[0], dtype=torch.float32, device=dev) for e in self.encoders]
        self.ctrl_img = torch.zeros(2 * S, self.image_height, self.image_width, 8, dtype=dt, device=dev) if self.controlnet is not None else None
        self.ehs = None                                   # [2S, T, C] text context, [cond; uncond]: allocated at the first admission
        self.garment: Optional[Dict[str, torch.Tensor]] = None          # name -> [S, M_l, C_l]
        self._views: Dict[int, _WidthViews] = {}          # one per width of the ladder, made at its first use
        self.closed = False
        self.steps_run = 0
        self.steps_at_width: Dict[int, int] = {}          # width -> steps run at it (at most one entry per ladder width)
        self._last_width = 0
        self._tickets: List[SessionTicket] = []

    # ---- introspection ----
    @property
    def width(self) -> int:
        """rows of the last step's batch (0 before the first; always ``slots`` unless the session compacts)"""
        return self._last_width

    @property
    def rows(self) -> List[Optional[int]]:
        """slot of every batch row, None for an idle row (the last layout, minus the requests that have finished since)"""
        self._check_open()
        return [None if r is None else r.slot for r in self.plan.row_runs()]

    @property
    def repacks(self) -> int:
        self._check_open()
        return self.plan.repacks

    @property
    def cak(self):
        """the UNet's cross-attention kwargs at full width (None before the first admission)"""
        v = self._views.get(self.S) if self._views is not None else None
        return None if v is None else v.cak

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
        for name in ("z", "x_in", "hist", "noise", "key_rows", "mask_rows", "guidance", "guidance_rows", "rescale", "rescale_rows", "control_scale_rows", "coef_rows", "row_slot", "temb", "ctrl_img", "ehs",
                     "garment", "_views"):
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
               control_guidance_start: float = 0.0, control_guidance_end: float = 1.0, guidance_rescale: float = 0.0,
               seed: Optional[int] = None, controlnet_conditioning_scale: Optional[float] = None) -> SessionTicket:
        """Queue one request (the per-request arguments of the pipeline's ``__call__``, with ``num_inference_steps``, ``guidance_scale``,
        ``image_scale`` and ``guidance_rescale`` per request) and return its ticket.  Never blocks and launches nothing: the request is admitted at the
        start of the first ``step()`` in which a slot is free.  ``num_images_per_prompt`` = n takes n slots.
        A session with ``device_noise``: ``seed`` (an int in [0, 2^64); else ``generator.initial_seed()``, else 8 bytes of
        ``os.urandom``; kept in ``ticket.seed``) keys the request's noise -- draw 0 its initial latents (unless ``latents`` is given),
        draw 1 + i its step i -- and ``eta`` > 0 is the stochastic DDIM step of this request alone.
        A session with ``control_rows``: ``controlnet_conditioning_scale`` (None: the value given at ``open_session``),
        ``control_guidance_start`` and ``control_guidance_end`` are this request's; its step i of n runs the ControlNet at
        ``scale * controlnet_keep(n, start, end)[i]``."""
        self._check_open()
        check_request(size=(self.image_width, self.image_height), width=width, height=height, num_inference_steps=num_inference_steps,
                      guidance_scale=guidance_scale, image_scale=image_scale, eta=eta, shard_over_ranks=shard_over_ranks,
                      control_guidance_start=control_guidance_start, control_guidance_end=control_guidance_end,
                      num_images_per_prompt=num_images_per_prompt, slots=self.S, guidance_rescale=guidance_rescale,
                      device_noise=self.device_noise, scheduler=self.plan.scheduler, seed=seed,
                      controlnet_conditioning_scale=controlnet_conditioning_scale, control_rows=self.control_rows)
        control = (controlnet_conditioning_scale, float(control_guidance_start), float(control_guidance_end)) if self.control_rows else None
        if self.device_noise:
            if isinstance(generator, (list, tuple)):
                raise ValueError("generator: a session request has one seed; pass one generator or seed=")
            seed = resolve_seeds(seed, generator, 1)[0]
        n = int(num_images_per_prompt)
        if self.controlnet is not None and pose_image is None:
            raise ValueError("pose_image: every request of a ControlNet session brings its pose image")
        if self.controlnet is None and pose_image is not None:
            raise ValueError("pose_image: this session was opened on the pipeline without a ControlNet")
        if latents is not None and tuple(latents.shape) != (n, 4, self.h, self.w):
            raise ValueError(f"latents {tuple(latents.shape)}: this session's requests have latents {(n, 4, self.h, self.w)} "
                             f"({self.image_width} x {self.image_height}, one geometry per session)")
        req = _Request(prompt=prompt, null_prompt=null_prompt, negative_prompt=negative_prompt, ref_image=ref_image, ref_clip_image=ref_clip_image,
                       pose_image=pose_image, guidance_scale=float(guidance_scale), image_scale=float(image_scale), guidance_rescale=float(guidance_rescale),
                       n=n, generator=generator, seed=seed, eta=float(eta),
                       output_type=output_type, clip_skip=clip_skip, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                       ref_clip_hidden_states=ref_clip_hidden_states, ref_image_latents=ref_image_latents, latents=latents)
        ticket = SessionTicket(req)
        ticket.seed = seed
        for j in range(n):
            ticket._runs.append(self.plan.submit(num_inference_steps, payload=(ticket, j), seed=seed, image=j, eta=float(eta), control=control))
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
            img, hw = pipe._image_tensor(as_batch(req.pose_image, "pose_image"), dev, normalize=False, size=(self.image_height, self.image_width),
                                         multiple=pipe.vae_scale_factor, layout="nhwc8")
            if tuple(hw) != (self.image_height, self.image_width) or img.shape[0] != 1:
                raise ValueError(f"pose_image gives {img.shape[0]} image(s) of {tuple(hw)}: a session request has one of "
                                 f"{(self.image_height, self.image_width)}")
            req.pose = img if (img.dim() == 4 and img.shape[-1] == 8 and img.dtype == dt) else nchw_to_nhwc8(img.to(dev), dt)
        lat = req.latents
        if lat is None and self.device_noise:          # draw 0 of the request's seed, image j in row j: what the solo call draws
            lat = RequestNoise([req.seed], req.n, dev).initial(self.h, self.w)
        if lat is None:
            lat = randn_tensor((req.n, 4, self.h, self.w), generator=req.generator, device=dev, dtype=torch.float32)
        req.z0 = (lat.to(device=dev, dtype=torch.float32) * run.scheduler.init_noise_sigma).permute(0, 2, 3, 1).reshape(req.n, self.HW, 4).contiguous()
        req.prepared = True

    def _allocate_context(self, req: _Request):
        S, dev, dt = self.S, self.device, self.dtype
        self.ehs = torch.zeros(2 * S, req.pe.shape[1], req.pe.shape[2], dtype=dt, device=dev)
        self.garment = {k: torch.zeros(S, v.shape[1], v.shape[2], dtype=v.dtype, device=dev) for k, v in req.features.items()}
        for v in self._views.values():
            v.bind_context(self)

    def _view(self, B: int) -> _WidthViews:
        v = self._views.get(B)
        if v is None:
            v = self._views[B] = _WidthViews(self, B)
            if self.ehs is not None:
                v.bind_context(self)
        return v

    def _admit(self, run: PlanRun):
        """What an admission does before the run has a batch row: prepare the request (once), check that it fits the session's
        context buffers, write the SLOT's latent and compute the time-embedding table of its schedule."""
        ticket, j = run.payload
        req, s = ticket._request, run.slot
        if not req.prepared:
            self._prepare(req, run)
        if self.ehs is None:
            self._allocate_context(req)
        if tuple(req.pe.shape[1:]) != tuple(self.ehs.shape[1:]) or tuple(req.ne.shape[1:]) != tuple(self.ehs.shape[1:]):
            raise ValueError(f"prompt embeds {tuple(req.pe.shape)} / {tuple(req.ne.shape)}: this session's text context rows are {tuple(self.ehs.shape[1:])}")
        for k, v in req.features.items():
            if k not in self.garment or tuple(v.shape[1:]) != tuple(self.garment[k].shape[1:]):
                raise ValueError(f"garment features of layer {k}: {tuple(v.shape)} does not fit this session's {tuple(self.garment.get(k, v).shape)}")
        self.z[s].copy_(req.z0[j])
        self.guidance[s] = req.guidance_scale
        if req.guidance_rescale:          # (a released slot is back at 0: a request that does not ask costs no launch)
            self.rescale[s] = req.guidance_rescale
            self._rescale_seen = True
        ts = torch.tensor([float(t) for t in run.timesteps], dtype=torch.float32).to(self.device)
        req.temb[j] = [e._time_embed_rows(ts) for e in self.encoders]          # the request's whole schedule, once

    def _write_row(self, v: _WidthViews, run: PlanRun):
        """Write batch row ``run.row`` (and its uncond twin B + row) of every buffer the forward reads, in place, from what the request
        keeps while it runs; nothing outside the row is touched.  The writes bump the tensors' versions, so the processors'
        step-invariant K / V caches and the ControlNet's conditioning embedding refresh for ALL rows on the next forward."""
        req, r, B = run.payload[0]._request, run.row, v.B
        v.ehs[r].copy_(req.pe[0])
        v.ehs[B + r].copy_(req.ne[0])
        for k, f in req.features.items():
            v.garment[k][r].copy_(f[0])
        v.mask_rows[r] = req.image_scale
        if self.compact:
            v.guidance_rows[r] = req.guidance_scale
            if req.guidance_rescale:
                v.rescale_rows[r] = req.guidance_rescale
        if v.ctrl_img is not None:
            v.ctrl_img[r].copy_(req.pose[0])
            v.ctrl_img[B + r].copy_(req.pose[0])

    def _release_rescale(self, run: PlanRun):
        """the slot -- and, compacting, the batch row -- of a run that leaves goes back to guidance_rescale 0: an idle row of eps may
        hold anything and must not be read"""
        if not run.payload[0]._request.guidance_rescale:
            return
        if run.slot is not None:
            self.rescale[run.slot] = 0.0
        if self.compact and run.row is not None:
            self.rescale_rows[run.row] = 0.0

    def _write_inputs(self, v: _WidthViews, runs: List[PlanRun]):
        """the UNet input of the rows of ``runs`` from their slots' fp32 latents, both CFG halves (``imd_session_input_rows``; the
        other rows keep their bytes): for a fresh request in_scale is its first step's, for a moved one its last step's"""
        rs, sc = [-1] * v.B, [1.0] * v.B
        for run in runs:
            rs[run.row], sc[run.row] = run.slot, run.in_scale
        ops.session_input_rows(self.z, torch.tensor(rs, dtype=torch.int32).to(self.device), torch.tensor(sc, dtype=torch.float32).to(self.device),
                               v.x_flat)

    # ---- the step ----
    @torch.no_grad()
    def step(self) -> List[SessionTicket]:
        """Admit from the queue, run ONE UNet (+ ControlNet) forward over the batch -- all slots, or with ``compact=True`` as many rows
        as the width ladder needs for the running ones -- and ONE fused step launch; returns the tickets that finished, decoded for
        their own ``output_type``."""
        self._check_open()
        check_pipeline(self.pipe)
        with ops.tuning_scope(**(getattr(self.pipe, "_tuning", None) or {})):
            return self._step()

    def _step(self) -> List[SessionTicket]:
        pipe = self.pipe
        self.plan.admit()
        for run in [r for r in self.plan.slot_runs() if r is not None and not r.ready]:          # (also what a failed step left waiting)
            try:
                self._admit(run)
                run.ready = True
            except BaseException as e:
                ticket = run.payload[0]
                ticket.error = e
                for r in ticket._runs:          # the whole request leaves: its slots and queue entries are free again
                    if not r.done:
                        self._release_rescale(r)
                        self.plan.cancel(r)
                raise
        if not self.plan.running:
            return []
        lay = self.plan.layout()
        B = lay.width
        v = self._view(B)
        moved = [r for r in lay.rows if r is not None] if lay.repack else lay.placed
        if lay.repack:
            v.mask_rows.zero_()
            if self._rescale_seen:
                v.rescale_rows.zero_()
        for run in moved:
            self._write_row(v, run)
        if moved:
            self._write_inputs(v, moved)
        st = self.plan.next_rows()
        for s, run, i in st.running:          # each row's time-embedding row, the same in both CFG halves
            ticket, j = run.payload
            for pair, table in zip(v.temb_pairs, ticket._request.temb[j]):
                pair[:, run.row].copy_(table[i])
        v.coef_rows.copy_(torch.tensor(st.coef_rows, dtype=torch.float32))
        if self.compact and st.row_slot != self._row_slot_host[:B]:
            v.row_slot.copy_(torch.tensor(st.row_slot, dtype=torch.int32))
            self._row_slot_host[:B] = st.row_slot
        pipe.set_scale(1.0)                   # the rows' image scales ride in the sa_batch_mask rows
        try:
            for e, buf in zip(self.encoders, v.temb):
                e.use_time_embedding(buf)
            down = mid = None
            if self.controlnet is not None:
                if self.control_rows:          # ALWAYS the rows route: a request's bits do not depend on its company's values
                    v.control_rows.copy_(torch.tensor(st.control_rows, dtype=torch.float32))
                    down, mid = self.controlnet.forward_nhwc(v.x_in, 0, v.ehs, v.ctrl_img, 1.0, scale_rows=v.control_rows)
                else:
                    down, mid = self.controlnet.forward_nhwc(v.x_in, 0, v.ehs, v.ctrl_img, self.control_scale)
            eps = pipe.unet.forward_nhwc(v.x_in, 0, v.ehs, v.cak, down, mid, cfg_pair=True)
        finally:
            for e in self.encoders:
                e.clear_time_embeddings()
        # guidance_rescale: ONE launch in front of the step, only while a running request asks for it; eps and both arrays by ROW
        if any(run.payload[0]._request.guidance_rescale for _, run, _ in st.running):
            ops.guidance_rescale(eps.view(2 * B, self.HW, 4), guidance=v.guidance_rows if self.compact else self.guidance,
                                 rescale=v.rescale_rows if self.compact else self.rescale)
        # device noise: the key rows of the slots whose step reads noise (every other slot inactive), ONE imd_noise_rows launch over all
        # slots, and the noise operand of the step -- only while such a row runs: a deterministic step keeps its launches and its bits
        kw = {}
        if st.noise:
            self.key_rows.copy_(ops.noise_key_rows(st.key_rows))
            ops.noise_rows(self.noise, self.key_rows)
            kw["noise"] = self.noise
        step_rows_at, step_rows = (ops.unipc_step_rows_at, ops.unipc_step_rows) if self.plan.unipc else (ops.sampler_step_rows_at, ops.sampler_step_rows)
        if self.compact:
            step_rows_at(self.z, eps, v.x_flat, guidance=v.guidance_rows, coef_rows=v.coef_rows, row_slot=v.row_slot, hist=self.hist, **kw)
        else:
            step_rows(self.z, eps, v.x_flat, guidance=self.guidance, coef_rows=v.coef_rows, hist=self.hist, **kw)
        self.steps_run += 1
        self._last_width = B
        self.steps_at_width[B] = self.steps_at_width.get(B, 0) + 1
        finished = []
        for run in st.finished:
            ticket, j = run.payload
            self._release_rescale(run)
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


__all__ = ["SessionPlan", "PlanRun", "PlanStep", "PlanLayout", "check_widths", "DenoiseSession", "SessionTicket", "check_scheduler", "check_pipeline", "check_request"]
