"""Host side of the device noise source (``imd_noise_rows``, csrc/noise.hip): which (seed, image, draw) a latent row reads.

The noise of a pixel is a pure function of (request seed, image, draw, pixel), so a request gets the same noise alone, inside a
request batch, under graph replay and in any slot of a denoising session.  Draw numbering:

* draw 0 -- the request's initial noise: the initial latent before ``init_noise_sigma``; in the inpainting pipeline the same tensor is
  the ``noise`` of ``add_noise`` and of the blend;
* draw 1 + i -- the variance noise of step index i of the request's FULL schedule (``strength`` < 1 starts at 1 + t_start);
* image j of ``num_images_per_prompt`` is counter word ``image`` = j.

Nothing here needs a GPU but :meth:`RequestNoise.key_table` / :meth:`RequestNoise.initial`, which launch.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import ops

INITIAL_DRAW = 0


def step_draw(step_index: int) -> int:
    """the draw of the variance noise of step index ``step_index`` (absolute: counted over the request's full schedule)"""
    step_index = int(step_index)
    if step_index < 0:
        raise ValueError(f"step index must be >= 0, got {step_index}")
    return 1 + step_index


def step_draws(t_start: int, steps_run: int) -> List[int]:
    """the draws of a call that skips the first ``t_start`` steps of its schedule (``strength`` < 1) and runs ``steps_run``: the index
    stays absolute, so the same request at another strength reads the same noise at the same timestep"""
    return [step_draw(int(t_start) + i) for i in range(int(steps_run))]


def check_seed(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < (1 << 64):
        raise ValueError(f"seed must be an int in [0, 2^64), got {seed!r}")
    return seed


def fresh_seed() -> int:
    return int.from_bytes(os.urandom(8), "little")


def resolve_seeds(seed, generator, requests: int) -> List[int]:
    """The seed of each of ``requests`` requests: ``seed`` (an int in [0, 2^64) for all of them, or a list / tuple with one per
    request), else ``generator[r].initial_seed()`` (one generator: its seed for all of them), else 8 bytes of ``os.urandom`` each.
    Anything else raises ValueError."""
    R = int(requests)
    if seed is not None:
        if isinstance(seed, (list, tuple)):
            if len(seed) != R:
                raise ValueError(f"seed has {len(seed)} entries for {R} requests (give one int, or one per request)")
            return [check_seed(s) for s in seed]
        return [check_seed(seed)] * R
    if generator is not None:
        gens = list(generator) if isinstance(generator, (list, tuple)) else [generator] * R
        if len(gens) != R:
            raise ValueError(f"generator has {len(gens)} entries for {R} requests: the device noise source takes one seed per request")
        return [check_seed(int(g.initial_seed()) & ((1 << 64) - 1)) for g in gens]
    return [fresh_seed() for _ in range(R)]


class RequestNoise:
    """The noise keys of one pipeline call: latent row b reads (``seeds[b // n]``, image ``b % n``) -- request-major rows, as
    ``RequestLayout`` -- or the rows ``[lo, hi)`` of that list (a rank's share)."""

    def __init__(self, seeds: Sequence[int], images_per_request: int, device=None, rows: Optional[Tuple[int, int]] = None):
        self.seeds = [check_seed(s) for s in seeds]
        self.images_per_request = int(images_per_request)
        if self.images_per_request < 1 or not self.seeds:
            raise ValueError("RequestNoise: at least one request and one image per request")
        self.device = device
        pairs = [(s, j) for s in self.seeds for j in range(self.images_per_request)]
        self.pairs = pairs if rows is None else pairs[rows[0]:rows[1]]

    @property
    def rows(self) -> int:
        return len(self.pairs)

    def shard(self, bounds: Tuple[int, int]) -> "RequestNoise":
        return RequestNoise(self.seeds, self.images_per_request, self.device, rows=bounds)

    def key_rows(self, draw: int) -> List[List[int]]:
        """the ``ops.noise_key_row`` of every latent row for ``draw``"""
        return [ops.noise_key_row(s, j, draw) for s, j in self.pairs]

    def key_table(self, draws: Sequence[int]) -> torch.Tensor:
        """[len(draws), rows, 8] int32 on the device: one upload for a whole call; entry i is the ``key_rows`` of a launch"""
        return ops.noise_key_rows([r for d in draws for r in self.key_rows(d)], self.device).view(len(draws), self.rows, ops.NOISE_ROW_WORDS)

    def initial(self, h: int, w: int) -> torch.Tensor:
        """draw 0 as [rows, 4, h, w] fp32 (NCHW, what the pipelines carry; the kernel's pixel index is the NHWC one)"""
        out = torch.empty(self.rows, h * w, 4, dtype=torch.float32, device=self.device)
        ops.noise_rows(out, self.key_table([INITIAL_DRAW])[0])
        return out.view(self.rows, h, w, 4).permute(0, 3, 1, 2).contiguous()
