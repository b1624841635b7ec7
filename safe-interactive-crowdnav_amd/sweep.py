"""Multi-GPU evaluation sweep: independent episodes shard across ranks (one process per GPU), no collective on the
data path; a single gather of the per-episode metrics over RCCL (``torch.distributed`` backend "nccl" on ROCm) at
the end.  JMID attention is intra-episode, so an episode is never split.

The reference has no distributed code; this is the build's own harness for BASELINE configs 3 and 5.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist


def shard_range(total: int, rank: int, world: int) -> Tuple[int, int]:
    """Block partition: rank g owns episodes [g*total/world, (g+1)*total/world) (balanced to +-1)."""
    base, rem = divmod(total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def gather_metrics(local: torch.Tensor, total: int, dst: int = 0, force: bool = False) -> Optional[np.ndarray]:
    """Gather per-episode metric rows [E_local, M] from every rank to ``dst`` in episode order.
    One collective of a few KB (latency-bound; payload is independent of the model size).  ``force`` runs the collective
    even in a one-rank group (tests of the RCCL call on a one-GPU box)."""
    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size() == 1 and not force):
        return local.detach().cpu().numpy()
    world, rank = dist.get_world_size(), dist.get_rank()
    if dist.get_backend() == "gloo" and local.is_cuda:     # host collective (CPU tests; several ranks sharing one GPU)
        local = local.detach().cpu()
    width = local.shape[1]
    cap = max(shard_range(total, r, world)[1] - shard_range(total, r, world)[0] for r in range(world))
    buf = torch.full((cap, width), float("nan"), dtype=local.dtype, device=local.device)
    buf[: local.shape[0]] = local
    gl = [torch.empty_like(buf) for _ in range(world)] if rank == dst else None
    dist.gather(buf, gl, dst=dst)
    if rank != dst:
        return None
    rows = []
    for r in range(world):
        lo, hi = shard_range(total, r, world)
        rows.append(gl[r][: hi - lo].cpu().numpy())
    return np.concatenate(rows, axis=0)


def statistics_rows(agent, scene):
    """One shard's evaluation statistics (``JmidEngine.eval_statistics``: agent [E, A, 10], scene [E, 6]; tensors or arrays) as
    per-episode rows [E, A * 10 + 6], the form ``gather_metrics`` carries."""
    if isinstance(agent, torch.Tensor):
        return torch.cat([agent.reshape(agent.shape[0], -1), scene.reshape(scene.shape[0], -1)], dim=1)
    return np.concatenate([agent.reshape(agent.shape[0], -1), scene.reshape(scene.shape[0], -1)], axis=1)


def split_statistics_rows(rows, n_agents: int):
    """Undo ``statistics_rows`` (on the destination rank, after ``gather_metrics``): [E, A * 10 + 6] -> (agent [E, A, 10],
    scene [E, 6])."""
    from .metrics import STAT_AGENT_COLUMNS, STAT_SCENE_COLUMNS
    na, ns = len(STAT_AGENT_COLUMNS), len(STAT_SCENE_COLUMNS)
    if rows.ndim != 2 or rows.shape[1] != n_agents * na + ns:
        raise ValueError(f"expected rows [E, {n_agents} * {na} + {ns}]")
    return rows[:, : n_agents * na].reshape(rows.shape[0], n_agents, na), rows[:, n_agents * na:]


def masked_statistics_rows(agent, cut, scene):
    """One shard's masked evaluation statistics (``JmidEngine.eval_statistics_masked``: agent [E, A, 12], cut [E, A, C, 5],
    scene [E, 6]; tensors or arrays) as per-episode rows [E, A * (12 + 5 C) + 6] - every agent's columns followed by its cut-offs',
    then the scene's - the form ``gather_metrics`` carries."""
    E, A = agent.shape[0], agent.shape[1]
    if isinstance(agent, torch.Tensor):
        return torch.cat([torch.cat([agent, cut.reshape(E, A, -1)], dim=2).reshape(E, -1), scene.reshape(E, -1)], dim=1)
    return np.concatenate([np.concatenate([agent, cut.reshape(E, A, -1)], axis=2).reshape(E, -1), scene.reshape(E, -1)], axis=1)


def split_masked_statistics_rows(rows, n_agents: int, n_cut: int):
    """Undo ``masked_statistics_rows`` (on the destination rank, after ``gather_metrics``): [E, A * (12 + 5 C) + 6] ->
    (agent [E, A, 12], cut [E, A, C, 5], scene [E, 6])."""
    from .metrics import STAT_CUTOFF_COLUMNS, STAT_MASKED_AGENT_COLUMNS, STAT_SCENE_COLUMNS
    na, nc, ns = len(STAT_MASKED_AGENT_COLUMNS), len(STAT_CUTOFF_COLUMNS), len(STAT_SCENE_COLUMNS)
    w = na + nc * n_cut
    if rows.ndim != 2 or rows.shape[1] != n_agents * w + ns:
        raise ValueError(f"expected rows [E, {n_agents} * ({na} + {nc} * {n_cut}) + {ns}]")
    per_agent = rows[:, : n_agents * w].reshape(rows.shape[0], n_agents, w)
    return per_agent[..., :na], per_agent[..., na:].reshape(rows.shape[0], n_agents, n_cut, nc), rows[:, n_agents * w:]
