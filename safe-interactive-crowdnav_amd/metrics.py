"""The evaluation statistics of the reference's test loop on the host: column names, the NumPy float64 twin of the device kernel
(``csrc/eval_stats.hpp``, ``jmid_eval_statistics``) and the table of means the reference prints.

Reference: ``compute_batch_statistics`` (MID/evaluation/evaluation.py:456-739, the branch without ``is_eval_hst``), its helpers
``compute_ade`` / ``compute_fde`` (:11-36), ``compute_kde_nll`` (:191-232), ``get_most_likely_trajectory_idx`` (:445-453) and the
summary of ``MID.eval`` (MID/mid.py:965-1003).  The reference fits its per-step densities with ``scipy.stats.gaussian_kde``; the
package does not import scipy - the two routines are restated here in closed form for the 2-D case.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

STAT_AGENT_COLUMNS = ("ade_min", "ade_mean", "ade_std", "ade_ml", "fde_min", "fde_mean", "fde_std", "fde_ml", "kde_nll", "ml_idx")
STAT_SCENE_COLUMNS = ("sade_min", "sade_mean", "sade_std", "sfde_min", "sfde_mean", "sfde_std")
LOG_PDF_LOWER_BOUND = -20.0      # evaluation.py:203, :271

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


def summarise(agent: np.ndarray, scene: np.ndarray) -> Dict[str, float]:
    """The means the reference prints after an evaluation (mid.py:965-1003) from the rows of all episodes: agent [..., 10],
    scene [..., 6].  Plain ``np.mean`` as there: one agent without a KDE makes ``kde`` (and the most-likely columns) NaN; the
    number of such rows comes back as ``nan_rows``."""
    agent = np.asarray(agent, dtype=np.float64).reshape(-1, len(STAT_AGENT_COLUMNS))
    scene = np.asarray(scene, dtype=np.float64).reshape(-1, len(STAT_SCENE_COLUMNS))
    out = {k: float(np.mean(agent[:, STAT_AGENT_COLUMNS.index(c)])) for k, c in _SUMMARY_AGENT.items()}
    out.update({k: float(np.mean(scene[:, STAT_SCENE_COLUMNS.index(c)])) for k, c in _SUMMARY_SCENE.items()})
    out["nan_rows"] = int(np.isnan(agent[:, STAT_AGENT_COLUMNS.index("kde_nll")]).sum())
    return out
