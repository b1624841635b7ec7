"""The evaluation statistics of the reference's test loop on the host: column names, the NumPy float64 twin of the device kernel
(``csrc/eval_stats.hpp``, ``jmid_eval_statistics``) and the table of means the reference prints.

Reference: ``compute_batch_statistics`` (MID/evaluation/evaluation.py:456-739, the branch without ``is_eval_hst``), its helpers
``compute_ade`` / ``compute_fde`` (:11-36), ``compute_kde_nll`` (:191-232), ``get_most_likely_trajectory_idx`` (:445-453) and the
summary of ``MID.eval`` (MID/mid.py:965-1003).  The reference fits its per-step densities with ``scipy.stats.gaussian_kde``; the
package does not import scipy - the two routines are restated here in closed form for the 2-D case.

The masked form (``eval_statistics_masked_host``, ``summarise_masked``; ``jmid_eval_statistics_masked``) is the ``is_eval_hst`` branch
of the same function (:540-545, :556-577, :624-715; summarised at MID/mid.py:978-1000, 1051-1075): only the horizon steps whose ground
truth is real are scored, agents without any are left out, and the fixed-horizon ("one / two / three fourth") columns are added.

The collision statistics (``collision_statistics_host``, ``summarise_collisions``; ``csrc/collision_stats.hpp``,
``jmid_collision_statistics``) follow MID/models/collision_check_utils.py: ``calc_min_dists`` (:58-80) with ``lineseg_dist`` (:20-55)
for the clearance of every agent pair of one joint sample, ``get_agents_in_collision`` (:83-97) for the agents that collide.

Collision repair (``repair_collisions_host``; ``csrc/repair.hpp``, ``jmid_repair_collisions``) is the twin of the rule include/jmid_hip.h
states for the reference's ``constraint_type: opt_softplus``: colliding samples are pushed apart under a softplus penalty on that
clearance until the predicate holds, or come back as they were.

Guided sampling (``guide_step_host``; ``csrc/guide.hpp``, ``jmid_guide_step``) is the twin of one guidance step of the denoise loop: the
velocity state integrated to positions, at most ``n_inner`` steps of the repair's own iteration, the displacement written back.

The wall statistics (``wall_statistics_host``, ``summarise_walls``; ``csrc/wall_stats.hpp``, ``jmid_wall_statistics``) take the
reference simulator's predicate: a step hits a wall when ``closest_distance_between_line_segments(wall, step) - radius < 0``
(crowd_sim_plus/envs/crowd_sim_plus.py:885-893, crowd_sim_plus/envs/utils/utils_plus.py:205-338).

The denoising loss (``loss_host``, ``loss_by_timestep``; ``csrc/loss.hpp``, ``jmid_loss``) is the reduction of ``DiffusionTraj.get_loss``
(MID/models/diffusion.py:465-475): ``F.mse_loss(reduction="none")`` in fp32, the mean over the rows the loss mask keeps in fp64.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

STAT_AGENT_COLUMNS = ("ade_min", "ade_mean", "ade_std", "ade_ml", "fde_min", "fde_mean", "fde_std", "fde_ml", "kde_nll", "ml_idx")
STAT_SCENE_COLUMNS = ("sade_min", "sade_mean", "sade_std", "sfde_min", "sfde_mean", "sfde_std")
STAT_MASKED_AGENT_COLUMNS = STAT_AGENT_COLUMNS + ("n_valid", "fde_valid")
STAT_CUTOFF_COLUMNS = ("ade_min", "ade_mean", "ade_ml", "kde", "valid")
CUTOFF_NAMES = ("one_fourth", "two_fourth", "three_fourth")      # the reference's names of cut-off positions 0, 1, 2
LOG_PDF_LOWER_BOUND = -20.0      # evaluation.py:203, :271
COLLISION_SAMPLE_COLUMNS = ("min_dist", "closest_pair", "n_pairs_colliding", "n_agents_colliding")
COLLISION_SCENE_COLUMNS = ("collision_rate", "agent_collision_rate", "min_dist_min", "min_dist_mean", "min_dist_std")
COLLISION_THRESHOLD = 0.2        # metres; collision_check_utils.py:88
WALL_SAMPLE_COLUMNS = ("min_clear", "n_agents_hitting", "n_hits")
WALL_SCENE_COLUMNS = ("wall_hit_rate", "agent_wall_hit_rate", "min_clear_min", "min_clear_mean", "min_clear_std")

# the reference's summary keys (mid.py:965-1003) -> the column each one averages
_SUMMARY_AGENT = {"ade": "ade_min", "fde": "fde_min", "kde": "kde_nll", "ade_most_likely": "ade_ml", "fde_most_likely": "fde_ml",
                  "ade_mean": "ade_mean", "ade_std": "ade_std", "fde_mean": "fde_mean", "fde_std": "fde_std"}
_SUMMARY_SCENE = {"sade": "sade_min", "sfde": "sfde_min", "sade_mean": "sade_mean", "sfde_mean": "sfde_mean",
                  "sade_std": "sade_std", "sfde_std": "sfde_std"}


def step_logpdf(points: np.ndarray, gt: np.ndarray):
    """``gaussian_kde(points.T)`` with scipy's defaults for one horizon step: points [K, 2] float64, gt [2].
    Returns (log-pdf at the K points [K], log-pdf at gt), unclipped, or None when the Cholesky factorisation of the data
    covariance fails (scipy raises LinAlgError)."""
    K = points.shape[0]
    c = points - points.mean(axis=0)
    cov = c.T @ c / (K - 1)
    if not cov[0, 0] > 0.0:
        return None
    l11 = np.sqrt(cov[0, 0])
    l21 = cov[1, 0] / l11
    piv = cov[1, 1] - l21 * l21
    if not piv > 0.0:
        return None
    f = float(K) ** (-1.0 / 6.0)         # scotts_factor: n^(-1 / (d + 4)), d = 2; the covariance is scaled by its square
    l11, l21, l22 = l11 * f, l21 * f, np.sqrt(piv) * f
    x = np.concatenate([points, gt[None]], axis=0)                     # [K + 1, 2] evaluation points
    y0 = (x[:, None, 0] - points[None, :, 0]) / l11                    # whitened differences [K + 1, K]
    y1 = ((x[:, None, 1] - points[None, :, 1]) - l21 * y0) / l22
    en = -0.5 * (y0 * y0 + y1 * y1)
    m = en.max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = np.where(np.isneginf(m), m, m + np.log(np.exp(en - m[:, None]).sum(axis=1)))
    lp = lse - np.log(K) - np.log(2.0 * np.pi) - np.log(l11 * l22)     # ln K + 1/2 ln det(2 pi C)
    return lp[:K], lp[K]


def step_logpdf_1d(points: np.ndarray, x: float):
    """``gaussian_kde(points)`` with scipy's defaults for one coordinate: points [K] float64 -> its log-pdf at ``x``, unclipped, or
    None when the data have no variance (the 1 x 1 Cholesky factorisation fails: scipy raises LinAlgError).  Variance with divisor
    K - 1, Scott's factor K^(-1/5) (d = 1)."""
    K = points.shape[0]
    c = points - points.mean()
    var = (c * c).sum() / (K - 1)
    if not var > 0.0:
        return None
    l = np.sqrt(var) * float(K) ** (-1.0 / 5.0)
    y0 = (x - points) / l
    en = -0.5 * (y0 * y0)
    m = en.max()
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = m if np.isneginf(m) else m + np.log(np.exp(en - m).sum())
    return lse - np.log(K) - 0.5 * np.log(2.0 * np.pi) - np.log(l)


def _min_mean_std(v: np.ndarray) -> np.ndarray:
    """min, mean and population std (np.std) over axis 1 of v [E, K, ...] -> [E, ..., 3].  Mean and deviations are taken relative to
    the first sample, as the kernel does: K equal values (a degenerate agent) then have exactly their value as mean and exactly 0
    as std instead of the rounding noise of a sum of K large numbers."""
    c = v - v[:, :1]
    return np.stack([v.min(axis=1), v[:, 0] + c.mean(axis=1), c.std(axis=1)], axis=-1)


def eval_statistics_host(pos: np.ndarray, gt: np.ndarray, return_details: bool = False):
    """pos [E, K, A, T, 2], gt [E, A, T, 2] -> (agent [E, A, 10], scene [E, 6]) float64, columns ``STAT_AGENT_COLUMNS`` /
    ``STAT_SCENE_COLUMNS``: what ``JmidEngine.eval_statistics`` computes on the device, without its size limits.
    ``return_details``: additionally a dictionary with ``gt_logpdf`` [E, A, T] (unclipped; NaN where the step's KDE does not exist)
    and ``ml_gap`` [E, A] (best minus second-best step-mean self log-pdf; NaN on degenerate rows)."""
    pos = np.asarray(pos, dtype=np.float64)
    gt = np.asarray(gt, dtype=np.float64)
    E, K, A, T, _ = pos.shape
    if gt.shape != (E, A, T, 2):
        raise ValueError("gt must be [E, A, T, 2]")
    if K < 2:
        raise ValueError("the statistics need at least two samples")
    d = np.linalg.norm(pos - gt[:, None], axis=-1)                     # [E, K, A, T]
    ade, fde = d.mean(axis=-1), d[..., -1]                             # [E, K, A]
    agent = np.empty((E, A, len(STAT_AGENT_COLUMNS)))
    agent[..., 0:3] = _min_mean_std(ade)
    agent[..., 4:7] = _min_mean_std(fde)
    gt_lp = np.full((E, A, T), np.nan)
    gap = np.full((E, A), np.nan)
    for e in range(E):
        for a in range(A):
            self_ll, ok = np.zeros(K), True
            for t in range(T):
                r = step_logpdf(pos[e, :, a, t], gt[e, a, t])
                if r is None:
                    ok = False
                    continue
                self_ll += np.maximum(r[0], LOG_PDF_LOWER_BOUND)
                gt_lp[e, a, t] = r[1]
            if ok:
                self_ll /= T
                ml = int(np.argmax(self_ll))                           # the first maximum, as min(dict, key = nll) keeps it
                agent[e, a, 3], agent[e, a, 7] = ade[e, ml, a], fde[e, ml, a]
                agent[e, a, 8] = -np.mean(np.maximum(gt_lp[e, a], LOG_PDF_LOWER_BOUND))
                agent[e, a, 9] = ml
                top2 = np.sort(self_ll)[-2:]
                gap[e, a] = top2[1] - top2[0]
            else:
                agent[e, a, 3] = agent[e, a, 7] = agent[e, a, 8] = np.nan
                agent[e, a, 9] = -1
    sade, sfde = ade.mean(axis=2), fde.mean(axis=2)                    # [E, K]
    scene = np.concatenate([_min_mean_std(sade), _min_mean_std(sfde)], axis=1)
    if return_details:
        return agent, scene, {"gt_logpdf": gt_lp, "ml_gap": gap}
    return agent, scene


def eval_statistics_masked_host(pos: np.ndarray, gt: np.ndarray, interp_future: np.ndarray, interp_history=None,
                                cutoffs=(2, 5, 8), return_details: bool = False):
    """The ``is_eval_hst`` branch: pos [E, K, A, T, 2], gt [E, A, T, 2], interp_future [E, A, T] bool (True = the step is not scored),
    interp_history [E, A, F] bool or None (an agent whose history is all True is left out, like one without a scored step, :544-545)
    -> (agent [E, A, 12], cut [E, A, len(cutoffs), 5], scene [E, 6]) float64 with the columns ``STAT_MASKED_AGENT_COLUMNS``,
    ``STAT_CUTOFF_COLUMNS``, ``STAT_SCENE_COLUMNS``: what ``JmidEngine.eval_statistics_masked`` computes on the device, without its
    size limits.  Absent values are NaN with their flag column 0 (``n_valid`` = 0: the agent is left out; ``fde_valid``; a
    cut-off's ``valid``).  The cut-offs' ``kde`` reproduces the reference's quirk: the mean of two 1-D negative log-pdfs (x and y),
    not a 2-D single-step density (``compute_kde_nll`` with ``cutoff_idx``, :209-222).  This project's conventions where the
    reference raises: sfde runs over the kept agents whose last step is scored, and a scene block without a qualifying agent is NaN.
    ``return_details``: additionally ``ml_gap`` [E, A] as in ``eval_statistics_host``."""
    pos = np.asarray(pos, dtype=np.float64)
    gt = np.asarray(gt, dtype=np.float64)
    E, K, A, T, _ = pos.shape
    if gt.shape != (E, A, T, 2):
        raise ValueError("gt must be [E, A, T, 2]")
    masked = np.asarray(interp_future).astype(bool)
    if masked.shape != (E, A, T):
        raise ValueError("interp_future must be [E, A, T]")
    if K < 2:
        raise ValueError("the statistics need at least two samples")
    cutoffs = tuple(int(c) for c in cutoffs)
    if any(c < 0 or c >= T for c in cutoffs):
        raise ValueError("every cut-off step must be in [0, T)")
    valid = ~masked
    if interp_history is not None:
        hist = np.asarray(interp_history).astype(bool)
        if hist.shape[:2] != (E, A):
            raise ValueError("interp_history must be [E, A, F]")
        valid = valid & ~hist.reshape(E, A, -1).all(axis=-1)[..., None]
    n_valid = valid.sum(axis=-1)                                       # [E, A]
    kept, fde_ok = n_valid > 0, valid[..., -1]
    d = np.linalg.norm(pos - gt[:, None], axis=-1)                     # [E, K, A, T]
    with np.errstate(divide="ignore", invalid="ignore"):
        ade = np.where(valid[:, None], d, 0.0).sum(axis=-1) / n_valid[:, None]        # [E, K, A]; NaN for an agent left out
    fde = np.where(fde_ok[:, None], d[..., -1], np.nan)
    agent = np.full((E, A, len(STAT_MASKED_AGENT_COLUMNS)), np.nan)
    cut = np.full((E, A, len(cutoffs), len(STAT_CUTOFF_COLUMNS)), np.nan)
    agent[..., 0:3] = _min_mean_std(ade)
    agent[..., 4:7] = _min_mean_std(fde)
    agent[..., 9], agent[..., 10], agent[..., 11] = -1, n_valid, fde_ok
    cut[..., 4] = 0
    gap = np.full((E, A), np.nan)
    for e in range(E):
        for a in range(A):
            if not kept[e, a]:
                continue
            steps = np.flatnonzero(valid[e, a])
            self_ll, gt_lp, ok = np.zeros(K), np.full(T, np.nan), True
            for t in steps:
                r = step_logpdf(pos[e, :, a, t], gt[e, a, t])
                if r is None:
                    ok = False
                    continue
                self_ll += np.maximum(r[0], LOG_PDF_LOWER_BOUND)
                gt_lp[t] = r[1]
            ml = -1
            if ok:
                self_ll /= len(steps)
                ml = int(np.argmax(self_ll))
                agent[e, a, 3], agent[e, a, 7] = ade[e, ml, a], fde[e, ml, a]
                agent[e, a, 8] = -np.mean(np.maximum(gt_lp[steps], LOG_PDF_LOWER_BOUND))
                agent[e, a, 9] = ml
                top2 = np.sort(self_ll)[-2:]
                gap[e, a] = top2[1] - top2[0]
            for j, c in enumerate(cutoffs):
                if not valid[e, a, c]:
                    continue
                dc = d[e, :, a, c]
                lps = [step_logpdf_1d(pos[e, :, a, c, k], gt[e, a, c, k]) for k in range(2)]
                kde = np.nan if None in lps else -(max(lps[0], LOG_PDF_LOWER_BOUND) / 2 + max(lps[1], LOG_PDF_LOWER_BOUND) / 2)
                cut[e, a, j] = [dc.min(), dc.mean(), dc[ml] if ml >= 0 else np.nan, kde, 1]
    n_kept, n_last = kept.sum(axis=1), (kept & fde_ok).sum(axis=1)     # [E]
    with np.errstate(divide="ignore", invalid="ignore"):
        sade = np.where(kept[:, None], ade, 0.0).sum(axis=2) / n_kept[:, None]            # [E, K]
        sfde = np.where((kept & fde_ok)[:, None], fde, 0.0).sum(axis=2) / n_last[:, None]
    scene = np.concatenate([_min_mean_std(sade), _min_mean_std(sfde)], axis=1)
    if return_details:
        return agent, cut, scene, {"ml_gap": gap}
    return agent, cut, scene


def summarise_masked(agent: np.ndarray, cut: np.ndarray, scene: np.ndarray) -> Dict[str, float]:
    """The reference's table of means for the ``is_eval_hst`` branch (mid.py:978-1000, 1051-1075) from the rows of all episodes:
    agent [..., 12], cut [..., n_cut, 5], scene [..., 6].  Each key is a plain ``np.mean`` over the rows that are present - the
    reference appends nothing for the others: ``n_valid`` > 0 for the ADE / KDE columns, ``fde_valid`` for the FDE columns, the
    cut-off's ``valid`` for its columns (named ``*_one_fourth``, ``*_two_fourth``, ``*_three_fourth`` for cut-off positions 0, 1,
    2); the scene keys average the episodes whose block exists.  A key without any row is NaN.  NaN rows from degenerate samples
    propagate as in ``summarise``; their number comes back as ``nan_rows``."""
    na, nc = len(STAT_MASKED_AGENT_COLUMNS), len(STAT_CUTOFF_COLUMNS)
    cut = np.asarray(cut, dtype=np.float64)
    n_cut = cut.shape[-2]
    if n_cut > len(CUTOFF_NAMES):
        raise ValueError("the reference names three cut-offs")
    agent = np.asarray(agent, dtype=np.float64).reshape(-1, na)
    cut = cut.reshape(-1, n_cut, nc)
    scene = np.asarray(scene, dtype=np.float64).reshape(-1, len(STAT_SCENE_COLUMNS))
    mean = lambda v: float(np.mean(v)) if v.size else float("nan")
    kept = agent[:, STAT_MASKED_AGENT_COLUMNS.index("n_valid")] > 0
    with_fde = kept & (agent[:, STAT_MASKED_AGENT_COLUMNS.index("fde_valid")] > 0)
    out = {}
    for k, c in _SUMMARY_AGENT.items():
        out[k] = mean(agent[with_fde if c.startswith("fde") else kept, STAT_AGENT_COLUMNS.index(c)])
    for j in range(n_cut):
        rows = cut[cut[:, j, STAT_CUTOFF_COLUMNS.index("valid")] > 0, j]
        for key, c in (("ade", "ade_min"), ("ade_most_likely", "ade_ml"), ("ade_mean", "ade_mean"), ("kde", "kde")):
            out[f"{key}_{CUTOFF_NAMES[j]}"] = mean(rows[:, STAT_CUTOFF_COLUMNS.index(c)])
    for k, c in _SUMMARY_SCENE.items():
        col = scene[:, STAT_SCENE_COLUMNS.index(c)]
        # an absent block (no qualifying agent) is NaN in all three of its columns; its minimum is NaN for no other reason
        present = ~np.isnan(scene[:, STAT_SCENE_COLUMNS.index("sade_min" if c.startswith("sade") else "sfde_min")])
        out[k] = mean(col[present])
    out["nan_rows"] = int(np.isnan(agent[kept, STAT_AGENT_COLUMNS.index("kde_nll")]).sum())
    return out


def summarise(agent: np.ndarray, scene: np.ndarray, rejection=None) -> Dict[str, float]:
    """The means the reference prints after an evaluation (mid.py:965-1003) from the rows of all episodes: agent [..., 10],
    scene [..., 6].  Plain ``np.mean`` as there: one agent without a KDE makes ``kde`` (and the most-likely columns) NaN; the
    number of such rows comes back as ``nan_rows``.  ``rejection`` = the (num_iter, colliding, fixed) of ``rejection_totals``: the
    reference's sentence about them (mid.py:1046-1049) is printed and the three come back under ``rejection_*``."""
    agent = np.asarray(agent, dtype=np.float64).reshape(-1, len(STAT_AGENT_COLUMNS))
    scene = np.asarray(scene, dtype=np.float64).reshape(-1, len(STAT_SCENE_COLUMNS))
    out = {k: float(np.mean(agent[:, STAT_AGENT_COLUMNS.index(c)])) for k, c in _SUMMARY_AGENT.items()}
    out.update({k: float(np.mean(scene[:, STAT_SCENE_COLUMNS.index(c)])) for k, c in _SUMMARY_SCENE.items()})
    out["nan_rows"] = int(np.isnan(agent[:, STAT_AGENT_COLUMNS.index("kde_nll")]).sum())
    if rejection is not None:
        num_iter, colliding, fixed, *causes = (int(v) for v in rejection)
        print(rejection_sentence(colliding, fixed, causes or None))
        out.update(rejection_num_iter=num_iter, rejection_colliding=colliding, rejection_fixed=fixed)
        if causes:
            out.update(rejection_pedestrian=causes[0], rejection_wall=causes[1])
    return out


def rejection_totals(episodes, cause=None) -> tuple:
    """The three counts ``DiffusionTraj.sample`` returns behind its samples (MID/models/diffusion.py:606-613; placeholders there) from the
    ``episodes`` [..., 3] rows of ``JmidEngine.denoise_reject`` = (colliding at round 0, fixed, last round rerun):
    -> (num_iter = the largest round over the batch, samples with collisions, samples fixed).  With walls ("collisions" then counts a
    sample that fails either predicate) ``cause`` [..., 2] = (fails the pedestrian predicate, fails the wall predicate) at round 0 adds
    its two sums: five counts."""
    ep = np.asarray(episodes.detach().cpu() if hasattr(episodes, "detach") else episodes).reshape(-1, 3).astype(np.int64)
    totals = (int(ep[:, 2].max()), int(ep[:, 0].sum()), int(ep[:, 1].sum())) if ep.shape[0] else (0, 0, 0)
    if cause is None:
        return totals
    ca = np.asarray(cause.detach().cpu() if hasattr(cause, "detach") else cause).reshape(-1, 2).astype(np.int64)
    return totals + (int(ca[:, 0].sum()), int(ca[:, 1].sum()))


def rejection_sentence(colliding: int, fixed: int, causes=None) -> str:
    """The line the reference prints after an evaluation with constraints (MID/mid.py:1048).  ``causes`` = (samples that fail the
    pedestrian predicate, samples that fail the wall predicate), when walls were asked for: both are named (a sample may count in
    both)."""
    line = f"Rejection sampling fixed {int(fixed)} samples out of {int(colliding)} samples with collisions"
    if causes is None:
        return line
    return line + f" ({int(causes[0])} between pedestrians, {int(causes[1])} with walls)"


def fill_slots(acceptable_by_round):
    """The pairing rule of collision-free sampling (include/jmid_hip.h, ``jmid_denoise_reject_seeded``) for ONE episode, the host twin of
    the device loop.  ``acceptable_by_round``: a callable j -> bool [K] (the acceptability of the K candidates of round j, asked for
    round 0 and then only for the rounds in which the episode is rerun; None ends the loop: ``max_rounds`` is reached), or a sequence
    of such rows, whose length is ``max_rounds`` + 1.
    Round 0: slot s holds candidate s, bad = the unacceptable slots.  Round j >= 1, only while bad is not empty: the i-th smallest bad
    slot takes the i-th smallest acceptable candidate, i < min(|bad|, |good|).
    -> (slots int32 [K, 3] = (round, candidate, still not acceptable), episode int32 [3] = (bad at round 0, fixed, last round rerun))."""
    if callable(acceptable_by_round):
        ask = acceptable_by_round
    else:
        rows = [np.asarray(r, dtype=bool) for r in acceptable_by_round]
        ask = lambda j: rows[j] if j < len(rows) else None
    ok0 = np.asarray(ask(0), dtype=bool)
    K = ok0.size
    slots = np.stack([np.zeros(K, np.int32), np.arange(K, dtype=np.int32), (~ok0).astype(np.int32)], axis=1)
    episode = np.array([int((~ok0).sum()), 0, 0], dtype=np.int32)
    j = 1
    while slots[:, 2].any():
        ok = ask(j)
        if ok is None:
            break
        bad, good = np.flatnonzero(slots[:, 2]), np.flatnonzero(np.asarray(ok, dtype=bool))
        n = min(bad.size, good.size)
        slots[bad[:n], 0], slots[bad[:n], 1], slots[bad[:n], 2] = j, good[:n], 0
        episode[1] += n
        episode[2] = j
        j += 1
    return slots, episode


def pair_index(i, j, A: int):
    """The ``pdist`` index of pair (i, j), i < j, among A agents: i A - i (i + 1) / 2 + (j - i - 1)."""
    return i * A - i * (i + 1) // 2 + (j - i - 1)


def _counts(n_agents, E: int, A: int) -> np.ndarray:
    n = np.asarray(n_agents, dtype=np.int64).reshape(-1)
    if n.size != E or np.any(n < 1) or np.any(n > A):
        raise ValueError("n_agents must hold one count in 1..A per episode")
    return n


def _collision_statistics_padded(pos: np.ndarray, threshold: float, n_agents):
    """The plain twin on every compacted episode, scattered to the layout at A (``jmid_collision_statistics_padded``)."""
    pos = np.asarray(pos)
    E, K, A, T, _ = pos.shape
    n = _counts(n_agents, E, A)
    pair = np.full((E, K, A * (A - 1) // 2), np.nan)
    agent = np.zeros((E, K, A), dtype=np.uint8)
    sample, scene = np.empty((E, K, len(COLLISION_SAMPLE_COLUMNS))), np.empty((E, len(COLLISION_SCENE_COLUMNS)))
    for e in range(E):
        ne = int(n[e])
        pr, ag, sm, sc = collision_statistics_host(pos[e:e + 1, :, :ne], threshold)
        i, j = np.triu_indices(ne, 1)
        at_A = pair_index(i, j, A)                                     # monotone in the index at n_e
        pair[e][:, at_A] = pr[0]
        agent[e, :, :ne] = ag[0]
        sample[e] = sm[0]
        has = sm[0, :, 1] >= 0
        sample[e, has, 1] = at_A[sm[0, has, 1].astype(np.int64)]
        scene[e] = sc[0]
    return pair, agent, sample, scene


def collision_statistics_host(pos: np.ndarray, threshold: float = COLLISION_THRESHOLD, n_agents=None):
    """pos [E, K, A, T, 2] -> (pair [E, K, P] float64, agent [E, K, A] uint8, sample [E, K, 4] float64, scene [E, 5] float64), the
    columns ``COLLISION_SAMPLE_COLUMNS`` / ``COLLISION_SCENE_COLUMNS``: what ``JmidEngine.collision_statistics`` computes on the
    device, without its size limits.  Pairs in ``pdist`` order, P = A (A - 1) / 2; a pair's value is the minimum over the T - 1
    segments of the distance from the origin to the segment of the relative position (``calc_min_dists`` / ``lineseg_dist``); an
    agent is flagged when one of its pairs is closer than ``threshold`` (``get_agents_in_collision``).  A = 1: no pairs, ``min_dist``
    +inf, ``closest_pair`` -1, ``min_dist_std`` NaN.  A non-finite position makes its pairs and the sample's ``min_dist`` NaN
    (``closest_pair`` -1); NaN pairs never collide.  T >= 2 (with one step the reference collapses to a scalar over all pairs).
    ``n_agents`` [E] (``jmid_collision_statistics_padded``): a padded batch, episode e has n_agents[e] <= A real agents.  Defined as
    this function on each compacted episode ``pos[e, :, :n_e]``, scattered to the shapes at A: pair (i, j) at ``pair_index(i, j, A)``,
    NaN in the pairs of a padded agent (they take part in nothing), 0 in a padded agent's byte, ``closest_pair`` the index at A,
    ``agent_collision_rate`` over K * n_e.  Padded rows are never read."""
    if n_agents is not None:
        return _collision_statistics_padded(pos, threshold, n_agents)
    pos = np.asarray(pos, dtype=np.float64)
    E, K, A, T, _ = pos.shape
    if T < 2:
        raise ValueError("the collision statistics need at least two horizon steps")
    if not (np.isfinite(threshold) and threshold >= 0.0):
        raise ValueError("the threshold must be finite and >= 0")
    i, j = np.triu_indices(A, 1)                                       # pdist order
    P = i.size
    rel = pos[:, :, i] - pos[:, :, j]                                  # [E, K, P, T, 2]
    a, b = rel[..., :-1, :], rel[..., 1:, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        still = (a == b).all(axis=-1)
        u = b - a
        d = u / np.sqrt(u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1])[..., None]
        s = a[..., 0] * d[..., 0] + a[..., 1] * d[..., 1]
        t = (-b[..., 0]) * d[..., 0] + (-b[..., 1]) * d[..., 1]
        h = np.maximum(np.maximum(s, t), 0.0)
        c = (-a[..., 0]) * d[..., 1] - (-a[..., 1]) * d[..., 0]
        seg = np.where(still, np.sqrt(a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]), np.hypot(h, np.abs(c)))
        seg = np.where(np.isfinite(a).all(axis=-1) & np.isfinite(b).all(axis=-1), seg, np.nan)
        pair = seg.min(axis=-1)                                        # [E, K, P]; np.min keeps a NaN
        hit = pair < threshold
    agent = np.zeros((E, K, A), dtype=np.uint8)
    for p in range(P):
        agent[:, :, i[p]] |= hit[:, :, p]
        agent[:, :, j[p]] |= hit[:, :, p]
    sample = np.empty((E, K, len(COLLISION_SAMPLE_COLUMNS)))
    if P:
        sample[..., 0] = pair.min(axis=-1)
        sample[..., 1] = np.where(np.isnan(sample[..., 0]), -1, np.argmin(pair, axis=-1))      # the first minimum
    else:
        sample[..., 0], sample[..., 1] = np.inf, -1
    sample[..., 2] = hit.sum(axis=-1)
    sample[..., 3] = agent.sum(axis=-1)
    md = sample[..., 0]
    with np.errstate(invalid="ignore"):
        scene = np.stack([(sample[..., 2] > 0).mean(axis=1), agent.reshape(E, -1).mean(axis=1), md.min(axis=1), md.mean(axis=1),
                          md.std(axis=1)], axis=-1)
    return pair, agent, sample, scene


def summarise_collisions(scene: np.ndarray) -> Dict[str, float]:
    """The means of the scene columns over all episodes: scene [..., 5] -> {column name: mean}.  Plain ``np.mean``: an episode with a
    NaN column (a non-finite position, or ``min_dist_std`` with A = 1) makes that key NaN."""
    scene = np.asarray(scene, dtype=np.float64).reshape(-1, len(COLLISION_SCENE_COLUMNS))
    with np.errstate(invalid="ignore"):
        return {c: float(np.mean(scene[:, k])) for k, c in enumerate(COLLISION_SCENE_COLUMNS)}


REPAIR_SAMPLE_COLUMNS = ("min_dist_before", "min_dist_after", "iterations", "state")
REPAIR_EPISODE_COLUMNS = ("colliding", "repaired", "max_iterations")
REPAIR_WALL_COLUMNS = ("min_clear_before", "min_clear_after")
REPAIR_UNTOUCHED, REPAIR_REPAIRED, REPAIR_REVERTED, REPAIR_NAN = 0, 1, 2, 3
# the defaults of collision repair (include/jmid_hip.h, ``jmid_repair_collisions``): arguments of the entry, not constants of the rule
REPAIR_DEFAULTS = {"margin": 0.02, "tau": 0.005, "step": 0.02, "max_iter": 32}


def _repair_segments(x: np.ndarray, lo: np.ndarray, hi: np.ndarray, m: float, tau: float, exp):
    """The closest-point form of the rule for the pairs (lo[a], hi[a]) of x [S, n, T, 2], every segment: -> (d, u, nx, ny, sigma), each
    [S, n, T - 1].  The operations and their order are the device function's (``csrc/repair.hpp::rpr_segment``)."""
    rel = x[:, lo] - x[:, hi]
    ax, ay, bx, by = rel[:, :, :-1, 0], rel[:, :, :-1, 1], rel[:, :, 1:, 0], rel[:, :, 1:, 1]
    abx, aby = bx - ax, by - ay
    den = abx * abx + aby * aby
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(den > 0.0, np.clip(-(ax * abx + ay * aby) / den, 0.0, 1.0), 0.0)
        cx, cy = ax + u * abx, ay + u * aby
        d = np.sqrt(cx * cx + cy * cy)
        nx, ny = np.where(d > 0.0, cx / d, 1.0), np.where(d > 0.0, cy / d, 0.0)
    z = (m - d) / tau
    e = exp(-np.abs(z))
    sigma = np.where(z >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))
    return d, u, nx, ny, sigma


def _repair_wall_segments(q: np.ndarray, wall, m: float, tau: float, exp):
    """The wall term's closest-point form for the steps q[:, :, s] -> q[:, :, s + 1] of q [S, n, NP, 2] and ONE wall {x1, y1, x2, y2}:
    -> (d, w0, w1, nx, ny, sigma), each [S, n, NP - 1]; w0 / w1 are the weights of the step's two ends.  The operations and their order are
    the device function's (``csrc/repair.hpp::rpr_wall_segment``)."""
    w0x, w0y, w1x, w1y = (float(v) for v in wall)
    b0x, b0y, b1x, b1y = q[:, :, :-1, 0], q[:, :, :-1, 1], q[:, :, 1:, 0], q[:, :, 1:, 1]
    p00x, p00y, p01x, p01y = b0x - w0x, b0y - w0y, b0x - w1x, b0y - w1y
    p10x, p10y, p11x, p11y = b1x - w0x, b1y - w0y, b1x - w1x, b1y - w1y

    def closest(ax, ay, bx, by):                             # the origin against the segment a -> b, rpr_segment's closed form
        abx, aby = bx - ax, by - ay
        den = abx * abx + aby * aby
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(den > 0.0, np.clip(-(ax * abx + ay * aby) / den, 0.0, 1.0), 0.0)
        cx, cy = ax + u * abx, ay + u * aby
        return u, cx, cy, cx * cx + cy * cy

    _, cx, cy, best = closest(p00x, p00y, p01x, p01y)        # b0 onto the wall
    wa, wb = np.ones_like(best), np.zeros_like(best)
    _, c1x, c1y, s1 = closest(p10x, p10y, p11x, p11y)        # b1 onto the wall
    # a step that properly crosses the wall: the four orientation products, strictly opposite signs twice
    Wx, Wy, Bx, By = w1x - w0x, w1y - w0y, b1x - b0x, b1y - b0y
    o1, o2 = Wx * p00y - Wy * p00x, Wx * p10y - Wy * p10x
    o3, o4 = By * p00x - Bx * p00y, By * p01x - Bx * p01y
    cross = (((o1 > 0.0) & (o2 < 0.0)) | ((o1 < 0.0) & (o2 > 0.0))) & (((o3 > 0.0) & (o4 < 0.0)) | ((o3 < 0.0) & (o4 > 0.0)))
    take = s1 < best
    cx, cy, best, wa, wb = np.where(take, c1x, cx), np.where(take, c1y, cy), np.where(take, s1, best), np.where(take, 0.0, wa), np.where(take, 1.0, wb)
    for ax, ay, bx, by in ((p00x, p00y, p10x, p10y), (p01x, p01y, p11x, p11y)):      # the wall's start, then its end, onto the step
        u, c2x, c2y, s2 = closest(ax, ay, bx, by)
        take = s2 < best
        cx, cy, best, wa, wb = np.where(take, c2x, cx), np.where(take, c2y, cy), np.where(take, s2, best), np.where(take, 1.0 - u, wa), np.where(take, u, wb)
    cx, cy, best, wa, wb = np.where(cross, c1x, cx), np.where(cross, c1y, cy), np.where(cross, s1, best), np.where(cross, 0.0, wa), np.where(cross, 1.0, wb)
    d = np.sqrt(best)
    with np.errstate(divide="ignore", invalid="ignore"):
        nx, ny = np.where(d > 0.0, cx / d, 1.0), np.where(d > 0.0, cy / d, 0.0)
    d, nx, ny = np.where(cross, -d, d), np.where(cross, -nx, nx), np.where(cross, -ny, ny)
    z = (m - d) / tau
    e = exp(-np.abs(z))
    sigma = np.where(z >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))
    return d, wa, wb, nx, ny, sigma


def _repair_iterate(x: np.ndarray, threshold: float, margin: float, tau: float, step: float, max_iter: int, exp, walls=None,
                    wall_radius: float = 0.0, lead=None):
    """The iteration of the rule on the candidates x [S, n, T, 2] float64 -> (x at the end, iterations used [S]).  ``walls`` [L, 4]: the
    wall terms of ``jmid_repair_collisions_walls`` behind the pairs' (``lead`` [n, 2] or None: the fixed point p0 in front of every path)."""
    S, n, T, _ = x.shape
    m, stop = threshold + margin, threshold + margin * 0.5
    mw, wstop = wall_radius + margin, wall_radius + margin * 0.5
    x, iters, active = x.copy(), np.zeros(S, dtype=np.int64), np.ones(S, dtype=bool)
    agents = np.arange(n)
    for _ in range(int(max_iter)):
        idx = np.flatnonzero(active)
        if not idx.size:
            break
        xa = x[idx]
        g = np.zeros_like(xa)
        dmin = np.full(idx.size, np.inf)
        for b in range(n if T > 1 else 0):                   # partners ascending; a partner's segment t - 1 before its segment t (T = 1: no segment)
            lo, hi = np.minimum(agents, b), np.maximum(agents, b)
            d, u, nx, ny, sigma = _repair_segments(xa, lo, hi, m, tau, exp)
            real = (agents != b)[None, :, None]
            sign = np.where(agents < b, -1.0, 1.0)[None, :, None]      # the pair's i subtracts, its j adds
            w1, w0 = sigma * u, sigma * (1.0 - u)
            for c, nc in ((0, nx), (1, ny)):
                far, near = w1 * nc, w0 * nc
                g[:, :, 1:, c] = np.where(real, np.where(sign < 0, g[:, :, 1:, c] - far, g[:, :, 1:, c] + far), g[:, :, 1:, c])
                g[:, :, :-1, c] = np.where(real, np.where(sign < 0, g[:, :, :-1, c] - near, g[:, :, :-1, c] + near), g[:, :, :-1, c])
            dmin = np.minimum(dmin, np.where(real, d, np.inf).min(axis=(1, 2)))
        go = dmin < stop
        if walls is not None:                                # walls ascending; per wall the step that ends in the point, then the one that starts there
            q = xa if lead is None else np.concatenate([np.broadcast_to(lead[None, :, None, :], (idx.size, n, 1, 2)), xa], axis=2)
            wmin = np.full(idx.size, np.inf)
            for wall in walls:
                d, wa, wb, nx, ny, sigma = _repair_wall_segments(q, wall, mw, tau, exp)
                we, ws = sigma * wb, sigma * wa
                for c, nc in ((0, nx), (1, ny)):
                    end, start = we * nc, ws * nc
                    if lead is None:
                        g[:, :, 1:, c] = g[:, :, 1:, c] - end
                        g[:, :, :-1, c] = g[:, :, :-1, c] - start
                    else:                                    # step s ends in x[s]; p0 takes no gradient
                        g[:, :, :, c] = g[:, :, :, c] - end
                        g[:, :, :-1, c] = g[:, :, :-1, c] - start[:, :, 1:]
                wmin = np.minimum(wmin, d.min(axis=(1, 2)))
            go = go | (wmin < wstop)
        active[idx[~go]] = False
        moved = idx[go]
        x[moved] = xa[go] - step * g[go]
        iters[moved] += 1
    return x, iters


def repair_collisions_host(pos: np.ndarray, threshold: float = COLLISION_THRESHOLD, margin: float = REPAIR_DEFAULTS["margin"],
                           tau: float = REPAIR_DEFAULTS["tau"], step: float = REPAIR_DEFAULTS["step"],
                           max_iter: int = REPAIR_DEFAULTS["max_iter"], p0: Optional[np.ndarray] = None, dt: Optional[float] = None,
                           vel: Optional[np.ndarray] = None, n_agents=None, exp=np.exp, walls=None, wall_radius: Optional[float] = None):
    """The NumPy twin of collision repair (``jmid_repair_collisions``; include/jmid_hip.h states the rule, ``csrc/repair.hpp`` is the
    kernel): the same candidates, the same operations in the same order, the same outputs.  pos [E, K, A, T, 2] float32 ->
    (pos_out float32 [E, K, A, T, 2], vel_out float32 or None, sample float64 [E, K, 4] = ``REPAIR_SAMPLE_COLUMNS``, episode int32 [E, 3] =
    ``REPAIR_EPISODE_COLUMNS``).  A sample is a candidate iff ``collision_statistics_host`` counts a colliding agent in it at
    ``threshold``; a NaN ``min_dist`` is state 3; everything that is not repaired comes back bit for bit.  ``vel`` [E, K, A, T, 2] with
    ``p0`` [E, A, 2] and ``dt``: the velocities, of which the rows of repaired samples are rewritten as
    float32((float64(x32[t]) - float64(x32[t - 1])) / dt), x32[-1] = p0.  ``n_agents`` [E]: a padded batch - the rule on every compacted
    episode, the padded rows as they are.  ``exp``: the exponential (the tests perturb it).
    ``walls`` [L, 4] or [L, 2, 2] with ``wall_radius`` (``jmid_repair_collisions_walls``): the wall terms join the objective and
    ``wall_statistics_host`` at (walls, wall_radius, p0) joins both gates - a sample that hits a wall is a candidate too (a single agent
    included), a NaN in either minimum is state 3, and a sample is kept only when both predicates accept it.  ``p0``, when given, is the
    fixed first point of every path.  A fifth value comes back: wall float64 [E, K, 2] = ``REPAIR_WALL_COLUMNS``.  L = 0: the first four
    values are those without walls, bit for bit."""
    pos = np.asarray(pos)
    if pos.dtype != np.float32:
        raise ValueError("pos must be float32 (the rule is defined on the fp32 samples)")
    E, K, A, T, _ = pos.shape
    for name, v, low in (("threshold", threshold, True), ("margin", margin, True), ("tau", tau, False), ("step", step, False)):
        if not (np.isfinite(v) and (v >= 0.0 if low else v > 0.0)):
            raise ValueError(f"{name} must be finite and {'>= 0' if low else '> 0'}")
    if not 0 <= int(max_iter) <= 1024:
        raise ValueError("max_iter must lie in 0..1024")
    if vel is not None and (p0 is None or dt is None):
        raise ValueError("vel needs p0 and dt")
    if walls is None and wall_radius is not None:
        raise ValueError("wall_radius is given without walls")
    if walls is not None:
        walls = np.asarray(walls, dtype=np.float64).reshape(-1, 4)
        if wall_radius is None or not (np.isfinite(wall_radius) and wall_radius >= 0.0):
            raise ValueError("walls need a wall_radius that is finite and >= 0")
        if not np.isfinite(walls).all():
            raise ValueError("a wall has a non-finite coordinate")
        if p0 is not None and np.asarray(p0).shape != (E, A, 2):
            raise ValueError("p0 must be [E, A, 2]")
    counts = _counts(n_agents, E, A) if n_agents is not None else np.full(E, A, dtype=np.int64)
    out = pos.copy()
    vel_out = None if vel is None else np.array(vel, dtype=np.float32, copy=True)
    sample, episode = np.zeros((E, K, 4)), np.zeros((E, 3), dtype=np.int32)
    wall = np.full((E, K, 2), np.inf)
    for e in range(E):
        n = int(counts[e])
        x32 = pos[e, :, :n]
        _, _, cs, _ = collision_statistics_host(x32[None], threshold)
        before, hit = cs[0, :, 0], cs[0, :, 3]
        sample[e, :, 0] = sample[e, :, 1] = before
        is_nan = np.isnan(before)
        flagged = (hit > 0) & (n >= 2)
        lead = None
        if walls is not None:
            lead32 = None if p0 is None else np.asarray(p0, dtype=np.float32)[e:e + 1, :n]
            lead = None if lead32 is None else lead32[0].astype(np.float64)
            _, _, ws, _ = wall_statistics_host(x32[None], walls, wall_radius, lead32)
            wall[e, :, 0] = wall[e, :, 1] = ws[0, :, 0]
            is_nan = is_nan | np.isnan(ws[0, :, 0])
            flagged = flagged | (ws[0, :, 1] > 0)
        sample[e, is_nan, 3] = REPAIR_NAN
        cand = np.flatnonzero(~is_nan & flagged)
        if not cand.size:
            continue
        x, iters = _repair_iterate(x32[cand].astype(np.float64), float(threshold), float(margin), float(tau), float(step), max_iter, exp,
                                   walls, 0.0 if walls is None else float(wall_radius), lead)
        r32 = x.astype(np.float32)
        _, _, rs, _ = collision_statistics_host(r32[None], threshold)
        after = rs[0, :, 0]
        ok = ~np.isnan(after) & (rs[0, :, 3] == 0)
        if walls is not None:
            _, _, ws, _ = wall_statistics_host(r32[None], walls, wall_radius, lead32)
            ok = ok & ~np.isnan(ws[0, :, 0]) & (ws[0, :, 1] == 0)
            wall[e, cand[ok], 1] = ws[0, ok, 0]
        sample[e, cand, 2] = iters
        sample[e, cand, 3] = np.where(ok, REPAIR_REPAIRED, REPAIR_REVERTED)
        sample[e, cand[ok], 1] = after[ok]
        out[e, cand[ok], :n] = r32[ok]
        if vel_out is not None:
            r = r32[ok].astype(np.float64)
            prev = np.concatenate([np.broadcast_to(np.asarray(p0, dtype=np.float32)[e, :n].astype(np.float64)[None, :, None], r[:, :, :1].shape),
                                   r[:, :, :-1]], axis=2)
            vel_out[e, cand[ok], :n] = ((r - prev) / float(np.float32(dt))).astype(np.float32)
        episode[e] = (cand.size, int(ok.sum()), int(iters.max()))
    if walls is None:
        return out, vel_out, sample, episode
    return out, vel_out, sample, episode, wall


GUIDE_COLUMNS = ("steps", "iterations")
# the defaults of guided sampling (include/jmid_hip.h, ``jmid_denoise_guided``): arguments of the entries, not constants of the rule
GUIDE_DEFAULTS = {"margin": 0.02, "tau": 0.005, "scale": 0.02, "n_inner": 4}


def guide_step_host(x: np.ndarray, p0: np.ndarray, dt: float, threshold: float = COLLISION_THRESHOLD, margin: float = GUIDE_DEFAULTS["margin"],
                    tau: float = GUIDE_DEFAULTS["tau"], weight: float = GUIDE_DEFAULTS["scale"], n_inner: int = GUIDE_DEFAULTS["n_inner"],
                    n_agents=None, walls=None, wall_radius: Optional[float] = None, exp=np.exp, return_positions: bool = False):
    """The NumPy twin of one guidance step (``jmid_guide_step``; include/jmid_hip.h states the rule, ``csrc/guide.hpp`` is the kernel):
    x [E, K*A, T, 2] float32 velocities (row s*A + a), p0 [E, A, 2] -> (x_out float32, rows float64 [E, K, 2] = ``GUIDE_COLUMNS``: 1 if the
    sample iterated, the iterations it used).  Per joint sample, in float64: integrate from p0 (ascending t), run at most ``n_inner``
    iterations of the repair's own iteration (``_repair_iterate``, the functions ``repair_collisions_host`` runs) with step := ``weight``
    metres, and write the displacement back as velocity differences, one rounding per point.  A sample that stops before its first
    iteration - or has a point that is not finite - keeps its bits; ``weight = 0`` returns the input.  ``n_agents`` [E]: a padded block -
    the rule on every compacted episode, the padded rows as they are.  ``walls`` [L, 4] or [L, 2, 2] with ``wall_radius``: the wall terms
    of ``jmid_repair_collisions_walls`` with p0 as the fixed first point of every path.  ``return_positions``: a third value, the pair
    (q_initial, q_final) float64 [E, K, A, T, 2] (NaN in padded rows)."""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 4 or x.shape[-1] != 2:
        raise ValueError("x must be float32 [E, K*A, T, 2] (the rule is defined on the fp32 state)")
    if p0 is None:
        raise ValueError("p0 is required (the guidance is defined on positions)")
    p0 = np.asarray(p0, dtype=np.float32)
    E, KA, T, _ = x.shape
    if p0.ndim != 3 or p0.shape[0] != E or p0.shape[2] != 2 or KA % p0.shape[1]:
        raise ValueError("p0 must be [E, A, 2] with K*A rows of x per episode")
    A = int(p0.shape[1])
    K = KA // A
    for name, v, low in (("threshold", threshold, True), ("margin", margin, True), ("tau", tau, False), ("weight", weight, True)):
        if not (np.isfinite(v) and (v >= 0.0 if low else v > 0.0)):
            raise ValueError(f"{name} must be finite and {'>= 0' if low else '> 0'}")
    if not (np.isfinite(dt) and dt > 0.0):
        raise ValueError("dt must be finite and > 0")
    if not 1 <= int(n_inner) <= 64:
        raise ValueError("n_inner must lie in 1..64")
    if walls is None and wall_radius is not None:
        raise ValueError("wall_radius is given without walls")
    if walls is not None:
        walls = np.asarray(walls, dtype=np.float64).reshape(-1, 4)
        if wall_radius is None or not (np.isfinite(wall_radius) and wall_radius >= 0.0):
            raise ValueError("walls need a wall_radius that is finite and >= 0")
        if not np.isfinite(walls).all():
            raise ValueError("a wall has a non-finite coordinate")
        if walls.shape[0] > 64:
            raise ValueError("at most 64 walls")
        if walls.shape[0] == 0:
            walls = None
    counts = _counts(n_agents, E, A) if n_agents is not None else np.full(E, A, dtype=np.int64)
    dtd = float(np.float32(dt))
    out = x.copy()
    view = out.reshape(E, K, A, T, 2)
    rows = np.zeros((E, K, 2))
    q_init, q_fin = np.full((E, K, A, T, 2), np.nan), np.full((E, K, A, T, 2), np.nan)
    for e in range(E):
        n = int(counts[e])
        v = x.reshape(E, K, A, T, 2)[e, :, :n].astype(np.float64)
        lead = p0[e, :n].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            q0 = lead[None, :, None, :] + dtd * np.cumsum(v, axis=2)      # (a sequential sum, ascending t)
        q_init[e, :, :n] = q_fin[e, :, :n] = q0
        ok = np.flatnonzero(np.isfinite(q0).all(axis=(1, 2, 3)))
        if not (weight > 0.0) or not ok.size or (T == 1 and walls is None):
            continue
        q, iters = _repair_iterate(q0[ok], float(threshold), float(margin), float(tau), float(weight), int(n_inner), exp, walls,
                                   0.0 if walls is None else float(wall_radius), lead if walls is not None else None)
        moved = iters > 0
        D = q[moved] - q0[ok[moved]]
        dD = D - np.concatenate([np.zeros_like(D[:, :, :1]), D[:, :, :-1]], axis=2)
        view[e, ok[moved], :n] = (v[ok[moved]] + dD / dtd).astype(np.float32)
        q_fin[e, ok[moved], :n] = q[moved]
        rows[e, ok, 0] = moved
        rows[e, ok, 1] = iters
    if return_positions:
        return out, rows, (q_init, q_fin)
    return out, rows


def repair_causes(sample, wall, threshold: float, wall_radius: float) -> Dict[str, int]:
    """The candidates of a repair with walls split by cause, from its ``sample`` [..., 4] and ``wall`` [..., 2] outputs: how many samples
    failed the pedestrian predicate on entry (min_dist < threshold), how many the wall predicate (min_clear - wall_radius < 0), how many
    both, and of each how many came back repaired.  -> {"pedestrians", "walls", "both", "pedestrians_repaired", "walls_repaired",
    "both_repaired", "candidates", "repaired", "reverted"}.  (State 3 counts nowhere.)"""
    to_np = lambda a: np.asarray(a.detach().cpu() if hasattr(a, "detach") else a, dtype=np.float64)
    sample, wall = to_np(sample).reshape(-1, 4), to_np(wall).reshape(-1, 2)
    state = sample[:, 3]
    tried, fixed = (state == REPAIR_REPAIRED) | (state == REPAIR_REVERTED), state == REPAIR_REPAIRED
    with np.errstate(invalid="ignore"):
        ped, hit = tried & (sample[:, 0] < threshold), tried & (wall[:, 0] - float(wall_radius) < 0)
    n = lambda m: int(m.sum())
    return {"pedestrians": n(ped), "walls": n(hit), "both": n(ped & hit), "pedestrians_repaired": n(ped & fixed),
            "walls_repaired": n(hit & fixed), "both_repaired": n(ped & hit & fixed), "candidates": n(tried), "repaired": n(fixed),
            "reverted": n(tried & ~fixed)}


def _wall_step_distance(a0, a1, b0, b1):
    """``closest_distance_between_line_segments`` (crowd_sim_plus/envs/utils/utils_plus.py:205-338) on arrays: walls a0 -> a1 and steps
    b0 -> b1, [..., 2] each and broadcast against each other -> the distance [...].  Every branch of the scalar
    ``crowd_env._closest_between_segments`` (the yardstick this is pinned to) is evaluated and chosen with ``np.where``, in its
    arithmetic and its order of operations; only the distance is kept.  Finite inputs."""
    dot = lambda u, v: u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]
    dist = lambda p, q: np.sqrt(dot(p - q, p - q))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a0, a1, b0, b1 = np.broadcast_arrays(a0, a1, b0, b1)
        A, B = a1 - a0, b1 - b0
        magA, magB = np.sqrt(dot(A, A)), np.sqrt(dot(B, B))
        degA, degB = magA < 1e-8, magB < 1e-8
        a1, b1 = np.where(degA[..., None], a0, a1), np.where(degB[..., None], b0, b1)
        uA, uB = np.where(degA[..., None], 0.0, A / magA[..., None]), np.where(degB[..., None], 0.0, B / magB[..., None])
        cross = uA[..., 0] * uB[..., 1] - uA[..., 1] * uB[..., 0]
        denom = cross * cross
        # exactly parallel (or a degenerate segment): before the wall, behind it, or an overlap
        d0, d1 = dot(uA, b0 - a0), dot(uA, b1 - a0)
        first = np.abs(d0) < np.abs(d1)
        before, behind = (d0 <= 0) & (0 >= d1), (d0 >= magA) & (magA <= d1)
        same = (dist(uA, uB) < 1e-8) | degB
        a0f, uAf = np.where(same[..., None], a0, a1), np.where(same[..., None], uA, -uA)
        d0f = dot(uAf, b0 - a0f)
        onto_wall = dist(a0f + uAf * d0f[..., None], b0)
        onto_step = dist(a0f, b0 + uB * dot(uB, a0f - b0)[..., None])
        parallel = np.where(before, np.where(first, dist(a0, b0), dist(a0, b1)),
                            np.where(behind, np.where(first, dist(a1, b0), dist(a1, b1)), np.where(d0f >= 0, onto_wall, onto_step)))
        # crossing lines: the two projections, each clamped, each clamp re-projecting the other point
        t = b0 - a0
        t0 = cross * (t[..., 0] * uB[..., 1] - t[..., 1] * uB[..., 0]) / denom
        t1 = cross * (t[..., 0] * uA[..., 1] - t[..., 1] * uA[..., 0]) / denom
        lowA, highA, lowB, highB = t0 < 0, t0 > magA, t1 < 0, t1 > magB
        pA = np.where(lowA[..., None], a0, np.where(highA[..., None], a1, a0 + uA * t0[..., None]))
        pB = np.where(lowB[..., None], b0, np.where(highB[..., None], b1, b0 + uB * t1[..., None]))
        pB = np.where((lowA | highA)[..., None], b0 + uB * np.minimum(np.maximum(dot(uB, pA - b0), 0.0), magB)[..., None], pB)
        pA = np.where((lowB | highB)[..., None], a0 + uA * np.minimum(np.maximum(dot(uA, pB - a0), 0.0), magA)[..., None], pA)
        return np.where(denom == 0, parallel, dist(pA, pB))


def _wall_statistics_padded(pos, walls, radius, p0, n_agents):
    """The plain twin on every compacted episode, scattered to the layout at A (``jmid_wall_statistics_padded``)."""
    pos = np.asarray(pos)
    E, K, A, T, _ = pos.shape
    n = _counts(n_agents, E, A)
    L = np.asarray(walls, dtype=np.float64).reshape(-1, 4).shape[0]
    if p0 is not None and np.asarray(p0).shape != (E, A, 2):
        raise ValueError("p0 must be [E, A, 2]")
    d = np.full((E, K, A, L), np.nan)
    agent = np.zeros((E, K, A), dtype=np.uint8)
    sample, scene = np.empty((E, K, len(WALL_SAMPLE_COLUMNS))), np.empty((E, len(WALL_SCENE_COLUMNS)))
    for e in range(E):
        ne = int(n[e])
        de, ag, sm, sc = wall_statistics_host(pos[e:e + 1, :, :ne], walls, radius, None if p0 is None else np.asarray(p0)[e:e + 1, :ne])
        d[e, :, :ne], agent[e, :, :ne], sample[e], scene[e] = de[0], ag[0], sm[0], sc[0]
    return d, agent, sample, scene


def wall_statistics_host(pos: np.ndarray, walls: np.ndarray, radius: float, p0: Optional[np.ndarray] = None, n_agents=None):
    """pos [E, K, A, T, 2], walls [L, 4] or [L, 2, 2], p0 [E, A, 2] or None -> (dist [E, K, A, L] float64, agent [E, K, A] uint8,
    sample [E, K, 3] float64, scene [E, 5] float64), the columns ``WALL_SAMPLE_COLUMNS`` / ``WALL_SCENE_COLUMNS``: what
    ``JmidEngine.wall_statistics`` computes on the device (include/jmid_hip.h, ``jmid_wall_statistics``), without its size limits.
    Agent a walks pos[t-1] -> pos[t] (and p0 -> pos[0] first when ``p0`` is given); dist[a, l] is the minimum over its segments of the
    reference's closest distance between wall l and the segment, the agent hits wall l iff dist - radius < 0.  A segment with a
    non-finite end makes the agent's row NaN (NaN never hits, and decides ``min_clear``).  L = 0: ``min_clear`` +inf, counts and rates
    0, ``min_clear_std`` NaN.  fp64 on the fp32 positions; vectorised over everything (the samples in blocks, for the memory).
    ``n_agents`` [E] (``jmid_wall_statistics_padded``): defined as this function on each compacted episode (``pos[e, :, :n_e]``,
    ``p0[e, :n_e]``), scattered to the shapes at A: NaN in a padded agent's row of dist, 0 in its byte, it counts nowhere and
    ``agent_wall_hit_rate`` is over K * n_e.  Padded rows of pos and p0 are never read."""
    if n_agents is not None:
        return _wall_statistics_padded(pos, walls, radius, p0, n_agents)
    pos = np.asarray(np.asarray(pos, dtype=np.float32), dtype=np.float64)
    E, K, A, T, _ = pos.shape
    if T < 2:
        raise ValueError("the wall statistics need at least two horizon steps")
    if not (np.isfinite(radius) and radius >= 0.0):
        raise ValueError("the radius must be finite and >= 0")
    walls = np.asarray(walls, dtype=np.float64).reshape(-1, 4)
    if not np.isfinite(walls).all():
        raise ValueError("a wall has a non-finite coordinate")
    L = walls.shape[0]
    if p0 is not None:
        p0 = np.asarray(np.asarray(p0, dtype=np.float32), dtype=np.float64)
        if p0.shape != (E, A, 2):
            raise ValueError("p0 must be [E, A, 2]")
        pos = np.concatenate([np.broadcast_to(p0[:, None, :, None, :], (E, K, A, 1, 2)), pos], axis=3)
    S = pos.shape[3] - 1
    d = np.empty((E, K, A, L))
    a0, a1 = walls[:, None, :2], walls[:, None, 2:]                    # [L, 1, 2] against the steps [..., 1, S, 2]
    block = max(1, (1 << 21) // max(1, E * A * S * L))
    for k0 in range(0, K, block):
        b0, b1 = pos[:, k0:k0 + block, :, None, :-1, :], pos[:, k0:k0 + block, :, None, 1:, :]
        ok = np.isfinite(b0).all(axis=-1) & np.isfinite(b1).all(axis=-1)
        seg = np.where(ok, _wall_step_distance(a0, a1, np.where(ok[..., None], b0, 0.0), np.where(ok[..., None], b1, 0.0)), np.nan)
        d[:, k0:k0 + block] = seg.min(axis=-1)                         # [E, block, A, L]; np.min keeps a NaN
    with np.errstate(invalid="ignore"):
        hit = d - float(radius) < 0
    agent = hit.any(axis=-1).astype(np.uint8)
    sample = np.empty((E, K, len(WALL_SAMPLE_COLUMNS)))
    sample[..., 0] = d.reshape(E, K, -1).min(axis=-1) if L else np.inf
    sample[..., 1] = agent.sum(axis=-1)
    sample[..., 2] = hit.reshape(E, K, -1).sum(axis=-1)
    mc = sample[..., 0]
    with np.errstate(invalid="ignore"):
        scene = np.stack([(sample[..., 1] > 0).mean(axis=1), agent.reshape(E, -1).mean(axis=1), mc.min(axis=1), mc.mean(axis=1),
                          mc.std(axis=1)], axis=-1)
    return d, agent, sample, scene


def summarise_walls(scene: np.ndarray) -> Dict[str, float]:
    """The means of the wall scene columns over all episodes: scene [..., 5] -> {column name: mean}.  Plain ``np.mean``, as
    ``summarise_collisions``: an episode with a NaN column (a non-finite position, or ``min_clear_std`` without walls) makes that key
    NaN."""
    scene = np.asarray(scene, dtype=np.float64).reshape(-1, len(WALL_SCENE_COLUMNS))
    with np.errstate(invalid="ignore"):
        return {c: float(np.mean(scene[:, k])) for k, c in enumerate(WALL_SCENE_COLUMNS)}


def _real_rows(E: int, A: int, n_agents) -> np.ndarray:
    """[E, A] bool: agent a of episode e is real (a < n_agents[e]); every row when ``n_agents`` is None."""
    if n_agents is None:
        return np.ones((E, A), dtype=bool)
    n = np.asarray(n_agents, dtype=np.int64).reshape(-1)
    if n.size != E or np.any(n < 1) or np.any(n > A):
        raise ValueError("n_agents must hold one count in 1..A per episode")
    return np.arange(A)[None, :] < n[:, None]


def loss_host(e_theta: np.ndarray, e: np.ndarray, n_agents=None):
    """The host twin of the device loss reduction (``csrc/loss.hpp``, ``jmid_loss``): ``DiffusionTraj.get_loss``'s
    ``F.mse_loss(reduction="none")`` and masked mean (MID/models/diffusion.py:465-475).  e_theta, e [E, A, T, 2]: the difference and its
    square in fp32, sums in fp64 -> (loss, count, rows): the mean over the real rows' T * 2 components, their number, and the sum of
    squared errors per row [E, A] float64 (NaN for padded rows, whose values are never read)."""
    e_theta, e = np.asarray(e_theta, dtype=np.float32), np.asarray(e, dtype=np.float32)
    if e_theta.ndim != 4 or e_theta.shape != e.shape or e.shape[-1] != 2:
        raise ValueError("expected e_theta and e [E, A, T, 2]")
    E, A, T, _ = e.shape
    real = _real_rows(E, A, n_agents)
    with np.errstate(invalid="ignore"):
        d = np.where(real[:, :, None, None], e_theta - e, np.float32(0))
    sq = (d * d).astype(np.float32)
    rows = sq.astype(np.float64).reshape(E, A, T * 2).sum(axis=-1)
    count = int(real.sum()) * T * 2
    loss = float(rows[real].sum() / count)
    rows[~real] = np.nan
    return loss, count, rows


def loss_by_timestep(rows: np.ndarray, t: np.ndarray, T: int, n_agents=None) -> Dict[int, float]:
    """The usual diagnostic of a denoising loss: the mean squared error per distinct timestep.  rows [E, A] (sum of squared errors per
    row, as ``loss_host`` / ``JmidEngine.loss`` return them), t [E, A] the rows' timesteps, T the horizon -> {t: mean over the real rows at
    that t of rows / (T * 2)}."""
    rows, t = np.asarray(rows, dtype=np.float64), np.asarray(t)
    if rows.ndim != 2 or t.shape != rows.shape:
        raise ValueError("expected rows and t [E, A]")
    real = _real_rows(rows.shape[0], rows.shape[1], n_agents)
    return {int(v): float(rows[real & (t == v)].sum() / (int((real & (t == v)).sum()) * T * 2)) for v in np.unique(t[real])}
