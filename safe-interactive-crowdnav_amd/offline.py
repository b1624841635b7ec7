"""Per-sample sampling used by the reference's offline evaluation, on the HIP engine.

Mirrors ``DiffusionTraj.sample`` (``sicnav_diffusion/JMID/MID/models/diffusion.py:544-613``) and the tail of
``AutoEncoder.generate`` (``MID/models/autoencoder.py:50-103``): unlike ``sample_sicnav_inference`` (the MPC-step path,
``engine.JmidEngine.denoise`` with K samples in one batch), every sample is denoised on its own with the context
rows as the batch, so for JMID a sample is one attention sequence of B*T tokens.  On the engine that is
``E = sample`` independent "episodes" with K = 1 that share the context - one batched launch instead of the
reference's Python loop over samples.

RNG contract: the global torch CPU generator is consumed exactly as the reference does - per sample ``x_T``
(``bestof``; zeros otherwise, no draw), then one ``randn_like`` per step for t > 1 (``z``; drawn for "ddim" as well,
where it is unused).  ``seed=`` (opt-in; None is the contract above) draws nothing on the host: x_T and every step's z come from the
library's counter generator (``noise.py``, ``jmid_denoise_seeded``) with sample i as episode id i - no [n_steps, ...] tensor is drawn
or uploaded.  Statistically, not seed-, compatible with the reference.

``get_loss`` / ``validation`` mirror ``AutoEncoder.get_loss`` (``MID/models/autoencoder.py:105-122``) and ``MID.validation()``
(``MID/mid.py:252-296``): the denoising loss of ``DiffusionTraj.get_loss`` (``diffusion.py:448-476``) on recorded futures, one device
call per batch (``JmidEngine.loss``), with the reference's draws of t and e.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .engine import JmidEngine
from .forecaster import denoise_stage, repair_stage, sampling_constraints
from .metrics import rejection_totals


def sample(engine: JmidEngine, num_points: int, context, sample: int, bestof: bool, point_dim: int = 2,
           flexibility: float = 0.0, ret_traj: bool = False, sampling: str = "ddpm", step: int = 100,
           precision: str = "f32", _integrate=None, seed: Optional[int] = None, with_constraints: bool = False,
           collision_threshold: float = 0.2, max_rounds: int = 3, static_obstacles=None,
           wall_radius: Optional[float] = None, constraint_type: Optional[str] = None,
           repair_options: Optional[dict] = None, guidance: Optional[dict] = None) -> Tuple[np.ndarray, int, int, int, int]:
    """-> (vel [sample, B, num_points, 2] float32, number_of_steps, 0, 0, 0)   (diffusion.py:603-613).
    ``_integrate`` = (p0 [B, 2], dt): used by ``generate`` - the same call also integrates on the device (integrate_kernel) and
    the first element of the result is the positions instead.
    ``with_constraints=True`` (the reference's flag, whose loop body is gone there): collision-free sampling,
    ``JmidEngine.denoise_reject`` - a sample in which two agents come closer than ``collision_threshold`` is redrawn up to
    ``max_rounds`` times (sample i is episode i with K = 1, so a redraw is exactly the reference's per-sample loop), and the last three
    values are the real (num_iter, samples with collisions, samples fixed) of ``metrics.rejection_totals``.  Needs ``seed=``,
    ``bestof=True``, ``sampling="ddim"`` and positions (``_integrate``: ``generate`` passes it); ``ValueError`` otherwise.
    ``static_obstacles=`` [L, 2, 2] or [L, 4] with ``wall_radius=`` (with ``with_constraints=True`` only; no default radius): a sample in
    which an agent's path, the step from p0 included, comes closer than ``wall_radius`` to a wall is redrawn too; the five returned
    values keep their meaning ("with collisions": not acceptable for either cause).
    ``constraint_type="opt_softplus"`` (with ``with_constraints=True``; the reference's name for its second mechanism): collision repair
    INSTEAD of redraws (``JmidEngine.repair_collisions``, every sample an episode with K = 1) - the samples are drawn exactly as without
    constraints, on either RNG contract and under either sampler, and a sample in which two agents come closer than
    ``collision_threshold`` is pushed apart until the predicate holds or comes back as it was.  Needs positions only; the last three
    values are (the largest iteration count, samples with collisions, samples repaired).  ``repair_options`` = {margin, tau, step,
    max_iter}.  Not with ``static_obstacles=``: walls are not in the objective.
    ``constraint_type="opt_softplus_walls"``: the same with the walls of ``static_obstacles=`` / ``wall_radius=`` (both needed) in the
    objective and in both gates (``jmid_repair_collisions_walls``): a sample whose paths, the step from p0 included, come closer than
    ``wall_radius`` to a wall is a candidate too; "with collisions" then reads "not acceptable for either cause".
    ``guidance=`` {scale, n_inner, margin, tau, weights, walls, table} (with ``with_constraints=True`` and ``sampling="ddim"``; needs
    positions): guided sampling INSTEAD of redraws (``JmidEngine.denoise(guidance=)``, every sample an episode with K = 1) - softplus
    collision steps at ``collision_threshold`` between the denoise steps, on either RNG contract; with ``constraint_type`` the repair
    follows on what is left, and without one the last three values are (the largest iteration total of a sample, samples that were
    guided, 0)."""
    if guidance is not None and not with_constraints:
        raise ValueError("guidance needs with_constraints=True")
    if guidance is not None and _integrate is None:
        raise ValueError("guidance needs positions (generate, or _integrate)")
    limits = sampling_constraints(max_rounds if with_constraints and guidance is None else None, collision_threshold, static_obstacles, wall_radius,
                                  constraint_type, repair_options, guidance=guidance, step=step, sampling=sampling)
    # (here the repair, or the guidance, stands in for the redraws; in the forecaster the repair follows them)
    redraw = with_constraints and limits.repair is None and limits.guidance is None
    if limits.repair is not None and not with_constraints:
        raise ValueError("constraint_type needs with_constraints=True")
    if limits.repair is not None and _integrate is None:
        raise ValueError("with_constraints=True needs positions (generate, or _integrate)")
    if redraw:
        missing = [w for w, ok in (("seed=", seed is not None), ("bestof=True", bool(bestof)), ('sampling="ddim"', sampling == "ddim"),
                                   ("positions (generate, or _integrate)", _integrate is not None)) if not ok]
        if missing:
            raise ValueError("with_constraints=True needs " + ", ".join(missing))
    if point_dim != 2:
        raise ValueError("point_dim must be 2")
    if ret_traj:
        raise NotImplementedError("ret_traj=True (every intermediate x_t) is a training-time debugging aid")
    if sampling not in ("ddpm", "ddim"):
        raise ValueError("sampling must be 'ddpm' or 'ddim'")      # the reference drops into pdb here (:595)
    ctx = torch.as_tensor(np.asarray(context, dtype=np.float32))
    B = int(ctx.shape[0])
    engine.set_step(step, sampling, flexibility)
    n_steps, stride = engine.n_steps, int(100 / step)
    if seed is not None:
        if not bestof:
            raise ValueError("seed= needs bestof=True: the seeded entry draws x_T (bestof=False starts from zeros)")
        x_T, noise = None, dict(seed=int(seed), episode_ids=np.arange(sample, dtype=np.uint32), K=1, T=int(num_points))
    else:
        x_T = torch.zeros([sample, B, num_points, 2])
        z = torch.zeros([n_steps, sample, B, num_points, 2])
        for i in range(sample):
            if bestof:
                x_T[i] = torch.randn([B, num_points, point_dim])
            for k, t in enumerate(range(engine.schedule.num_steps, 0, -stride)):
                if t > 1:
                    z[k, i] = torch.randn([B, num_points, point_dim])
        x_T, noise = x_T.numpy(), dict(z=z.numpy() if sampling == "ddpm" else None)
    ctx_e = ctx.unsqueeze(0).expand(sample, B, ctx.shape[1]).contiguous().numpy()
    number_of_steps = sample * (engine.schedule.num_steps // stride + 1)
    if _integrate is None:
        vel, _ = engine.denoise(x_T, ctx_e, None, precision=precision, want_pos=False, **noise)
        return vel.reshape(sample, B, num_points, 2), number_of_steps, 0, 0, 0
    # every sample is an "episode" of B agents with K = 1: p0 repeats per sample
    p0, dt = np.ascontiguousarray(np.broadcast_to(np.asarray(_integrate[0], dtype=np.float32)[None], (sample, B, 2))), float(_integrate[1])
    totals = (0, 0, 0)
    if redraw:
        pos, rejection = denoise_stage(engine, ctx_e, p0, limits, dt, seeded=noise)(precision, True)
        totals = rejection_totals(rejection.episodes)
    elif limits.guidance is not None:
        _, pos, guide = engine.denoise(x_T, ctx_e, p0, dt=dt, precision=precision, want_vel=False, guidance=limits.guidance, want_guide=True,
                                       **{key: v for key, v in noise.items() if key != "z"})
        totals = (int(guide[..., 1].max()), int((guide[..., 0] > 0).sum()), 0)
    else:
        _, pos = engine.denoise(x_T, ctx_e, p0, dt=dt, precision=precision, want_vel=False, **noise)
    if limits.repair is not None:
        pos, episode, _ = repair_stage(engine, pos, (sample, B, 1, num_points), limits.threshold, limits.repair, p0=p0, dt=dt)
        totals = rejection_totals(episode)      # (the same three columns: largest iteration count, samples with collisions, repaired)
    return (pos.reshape(sample, B, num_points, 2), number_of_steps, *totals)


def generate(engine: JmidEngine, context, p0, dt: float, num_points: int, sample_n: int, bestof: bool,
             flexibility: float = 0.0, sampling: str = "ddpm", step: int = 100, precision: str = "f32", seed: Optional[int] = None,
             with_constraints: bool = False, collision_threshold: float = 0.2, max_rounds: int = 3, static_obstacles=None,
             wall_radius: Optional[float] = None, constraint_type: Optional[str] = None, repair_options: Optional[dict] = None,
             guidance: Optional[dict] = None):
    """Tail of ``AutoEncoder.generate``: ``sample`` + ``SingleIntegrator.integrate_samples``
    (``single_integrator.py:290-321``): pos = cumsum(vel, T) * dt + p0[b].  ``context`` [B, ctx] is the encoder
    output (``JmidEngine.encode``), ``p0`` [B, 2] the current positions.  -> (pos [sample, B, T, 2], steps, 0, 0, 0); with
    ``with_constraints=True`` (see ``sample``) the zeros are (num_iter, samples with collisions, samples fixed); ``static_obstacles`` /
    ``wall_radius`` as there; with ``constraint_type="opt_softplus"`` they are (the largest iteration count, samples with collisions,
    samples repaired) of the collision repair; ``"opt_softplus_walls"`` needs ``static_obstacles`` / ``wall_radius`` and repairs for either
    cause; ``guidance=`` as there."""
    pos, nsteps, a, b, c = sample(engine, num_points, context, sample_n, bestof, flexibility=flexibility,
                                  sampling=sampling, step=step, precision=precision, _integrate=(p0, dt), seed=seed,
                                  with_constraints=with_constraints, collision_threshold=collision_threshold, max_rounds=max_rounds,
                                  static_obstacles=static_obstacles, wall_radius=wall_radius, constraint_type=constraint_type,
                                  repair_options=repair_options, guidance=guidance)
    return np.asarray(pos, dtype=np.float32), nsteps, a, b, c


def agent_counts_from_futures(y_t, batch_size: int) -> np.ndarray:
    """The real agents per scene of a NaN-padded batch of futures, by ``generate_mask``'s rule (MID/dataset/preprocessing.py:35-89).
    y_t [batch_size * A, T, 2] -> n_agents int32 [batch_size].  The reference makes two masks from the NaNs: attention sees the agents in
    front of the first row with ANY NaN (:63-73), the loss drops the rows that are ALL NaN (:85).  They describe one padded batch only
    when the padding is trailing and whole rows; anything else raises ``ValueError``."""
    y = np.asarray(y_t.detach().cpu() if torch.is_tensor(y_t) else y_t)
    if y.ndim != 3 or batch_size < 1 or y.shape[0] % batch_size != 0:
        raise ValueError("expected y_t [batch_size * A, T, 2]")
    A = y.shape[0] // batch_size
    nan = np.isnan(y).reshape(batch_size, A, -1)
    any_nan, all_nan = nan.any(axis=-1), nan.all(axis=-1)
    n = np.where(any_nan.any(axis=1), any_nan.argmax(axis=1), A).astype(np.int32)       # attention: agents before the first NaN row
    for b in range(batch_size):
        if (any_nan[b] != all_nan[b]).any():
            raise ValueError(f"scene {b}: agent {int((any_nan[b] != all_nan[b]).argmax())} is partly NaN - the reference's two masks disagree there "
                             "(attention drops the row and every later one, the loss keeps it)")
        if not all_nan[b, n[b]:].all():
            raise ValueError(f"scene {b}: a NaN agent (row {int(n[b])}) in front of a real one - the reference's two masks disagree there "
                             "(attention stops at the first NaN row, the loss keeps the real rows behind it): padding must be trailing")
        if n[b] < 1:
            raise ValueError(f"scene {b} has no real agent")
    return n


def get_loss(engine: JmidEngine, x_st, nbr_sum, edge_mask, y_t, batch_size: Optional[int] = None, t=None, precision: str = "f32",
             seed: Optional[int] = None, episode_ids=None, want_rows: bool = False, want_e_theta: bool = False,
             first_history_index=None):
    """``AutoEncoder.get_loss`` (MID/models/autoencoder.py:105-122) on the engine: encode, then ``DiffusionTraj.get_loss``
    (MID/models/diffusion.py:448-476) as one device call (``JmidEngine.loss``).  x_st [R, hist, 6], nbr_sum [R, 2, hist, 6], edge_mask
    [R, 2] the encoder's inputs, y_t [R, T, 2] the futures.  ``batch_size`` (the joint predictor's validation, MID/mid.py:275-281): R =
    batch_size * A rows, scenes padded to A agents with NaN rows in y_t - the counts come from ``agent_counts_from_futures``
    (``generate_mask``), NaNs are zeroed as ``masked_fill`` does (preprocessing.py:29-33).  None: the unmasked branch, all R rows one scene.
    RNG contract (the reference's): ``t`` from ``np.random.choice(np.arange(1, num_steps + 1), R)`` when not given
    (``uniform_sample_t``, diffusion.py:55-57), then e from one global ``torch.randn`` of y_t's shape.  ``seed=`` draws e on the device
    instead (scene b is episode id ``episode_ids[b]``, default b); t is still drawn on the host.
    ``first_history_index`` [R] (the batch's own, MID/dataset/preprocessing.py:468; the loaders admit rows with two history frames,
    MID/mid.py:1334, 1427): row r is encoded from that frame on (``JmidEngine.encode(first_index=)``); nothing else in the loss changes.
    -> ``engine.LossResult``."""
    y = torch.as_tensor(np.asarray(y_t.detach().cpu() if torch.is_tensor(y_t) else y_t, dtype=np.float32))
    if y.ndim != 3 or y.shape[-1] != 2:
        raise ValueError("expected y_t [R, T, 2]")
    R, T = int(y.shape[0]), int(y.shape[1])
    E = 1 if batch_size is None else int(batch_size)
    n_agents = None if batch_size is None else agent_counts_from_futures(y, E)
    A = R // E
    clean = [np.nan_to_num(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float32), nan=0.0) for a in (x_st, nbr_sum, edge_mask)]
    if first_history_index is not None and torch.is_tensor(first_history_index):
        first_history_index = first_history_index.detach().cpu().numpy()
    ctx = engine.encode(*clean, first_index=first_history_index).reshape(E, A, -1)
    if t is None:
        t = np.random.choice(np.arange(1, engine.schedule.num_steps + 1), R)
    t = np.asarray(t, dtype=np.int32).reshape(E, A)
    x0 = torch.nan_to_num(y, nan=0.0).numpy().reshape(E, A, T, 2)
    if n_agents is not None and (n_agents == A).all():
        n_agents = None if not engine.joint else n_agents       # (iMID rows are independent: nothing to mask)
    kw = dict(n_agents=n_agents, precision=precision, want_rows=want_rows, want_e_theta=want_e_theta)
    if seed is not None:
        return engine.loss(x0, ctx, t, seed=seed, episode_ids=np.arange(E) if episode_ids is None else episode_ids, **kw)
    e = torch.randn(y.shape).numpy().reshape(E, A, T, 2)
    return engine.loss(x0, ctx, t, e=e, **kw)


def validation(engine: JmidEngine, batches, precision: str = "f32", seed: Optional[int] = None) -> float:
    """``MID.validation`` (MID/mid.py:252-296): the mean of the per-batch losses ("Avg. Val Loss").  ``batches``: an iterable of dicts
    with the keyword arguments of ``get_loss`` (x_st, nbr_sum, edge_mask, y_t and optionally batch_size, t, first_history_index).  ``seed``: batch i draws its
    e on the device with scene b as episode id (number of scenes before the batch) + b."""
    losses, first = [], 0
    for b in batches:
        kw = dict(b)
        if seed is not None:
            E = 1 if kw.get("batch_size") is None else int(kw["batch_size"])
            kw.update(seed=seed, episode_ids=np.arange(first, first + E))
            first += E
        losses.append(float(get_loss(engine, precision=precision, **kw).loss))
    return sum(losses) / len(losses)
