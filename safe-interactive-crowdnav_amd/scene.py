"""Host-side batch builder: agent histories -> the arrays the device encoder consumes.

A NumPy restatement (no pandas, no Scene/Node objects) of what the reference does between
``update_state_hists`` and ``Trajectron.get_latent``:

  * history frame table, resampling to the ``time_step`` grid from the last stamp backwards, keep-last per
    bin, linear interpolation of empty bins      (``JMID/mid_sim_wrapper.py:244-310``)
  * cluster selection around the human nearest the robot, constant-velocity forecasts for everybody else
                                                 (``mid_sim_wrapper.py:313-437``)
  * per-node state [pos, vel, acc] by first differences   (``MID/environment/data_utils.py:24-37``)
  * standardisation, neighbour sets, edge scaling (``MID/dataset/preprocessing.py:428-620``,
    ``MID/environment/scene_graph.py:111-250, 280-313``)
  * the reductions the encoder applies before its LSTMs: per edge type the SUM of neighbour histories and
    clamp(sum(edge values), 1)                    (``MID/models/encoders/mgcvae.py:726-768``)

All arithmetic is float64 until the final cast to float32, as in the reference
(``preprocessing.py:495-499``: ``torch.tensor(..., dtype=torch.float)``).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

ATTENTION_RADIUS = 3.0                       # mid_sim_wrapper.py:234-238
STATE_STD = np.array([3.0, 3.0, 2.0, 2.0, 1.0, 1.0])   # pos std overridden by the attention radius
                                                        # (mid_sim_wrapper.py:219-231, preprocessing.py:477-478)
EDGE_ADDITION_FILTER = (0.25, 0.5, 0.75, 1.0)           # trajectron_hypers.py:83
EDGE_REMOVAL_FILTER = (1.0, 0.0)                        # trajectron_hypers.py:84
TYPE_VALUE_PED, TYPE_VALUE_ROBOT = 1, 2                 # NodeType enum values (environment/node_type.py)
ROBOT_ID = -1


class HistoryTooShortError(TypeError):
    """Fewer resampled frames than ``past_num_frames``.  The reference fails in the same situation
    (``get_timesteps_data`` returns None -> ``TypeError`` at MID/mid.py:326); callers catch and re-raise
    (``sicnav_diffusion/policy/sicnav_acados.py:1176-1180``)."""


def derivative_of(x: np.ndarray, dt: float) -> np.ndarray:
    """data_utils.py:24-37 for NaN-free input: first difference, first element duplicated."""
    if x.shape[0] < 2:
        return np.zeros_like(x)
    d = np.empty_like(x)                 # (x: [F] or [F, C], differences along the first axis; the values np.ediff1d(x, to_begin=x[1] - x[0]) gives)
    np.subtract(x[1:], x[:-1], out=d[1:])
    d[0] = d[1]
    return d / dt


# --------------------------------------------------------------------------------------------- history table
def frame_table(prev_states: Sequence[Sequence[Sequence[float]]], prev_robot_states: Sequence[Sequence[float]],
                time_step: float, num_hist_frames: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """mid_sim_wrapper.py:244-298.

    prev_states: per human a list of [x, y, t]; prev_robot_states: list of [x, y, t].
    Returns (human_xy [F, N, 2], robot_xy [F, 2], pose_now [N, 2]) with F <= num_hist_frames resampled frames.
    """
    N = len(prev_states)
    h0 = np.asarray(prev_states[0], dtype=np.float64).reshape(-1, 3)
    times = h0[:, 2]
    table = np.full((len(times), 2 * N + 2), np.nan)
    table[:, 0:2] = h0[:, 0:2]
    for i in range(1, N):                       # left-join on exactly equal stamps
        hi = np.asarray(prev_states[i], dtype=np.float64).reshape(-1, 3)
        lut = {t: k for k, t in enumerate(hi[:, 2])}
        for r, t in enumerate(times):
            k = lut.get(t)
            if k is not None:
                table[r, 2 * i:2 * i + 2] = hi[k, 0:2]
    pose_now = table[-1, :2 * N].reshape(N, 2).copy()      # agent_df.tail(1), before the robot join
    rob = np.asarray(prev_robot_states, dtype=np.float64).reshape(-1, 3)
    lut = {t: k for k, t in enumerate(rob[:, 2])}
    for r, t in enumerate(times):
        k = lut.get(t)
        if k is not None:
            table[r, 2 * N:2 * N + 2] = rob[k, 0:2]
    keep = ~np.isnan(table).any(axis=1)         # dropna
    table, times = table[keep], times[keep]
    order = np.argsort(times, kind="stable")
    table, times = table[order], times[order]
    if len(times) == 0:
        raise HistoryTooShortError("no complete history frame")
    # subsample_df: stamps*100 -> integer nanoseconds (truncation), bins of round(time_step*100) ns anchored at
    # the LAST stamp, right-closed; keep the last row per bin; interpolate empty bins linearly
    ns = np.trunc(times * 100.0).astype(np.int64)
    w = int(round(time_step * 100))
    k = (ns[-1] - ns) // w                      # bin index counted backwards from the end
    nb = int(k.max()) + 1
    out = np.full((nb, table.shape[1]), np.nan)
    for r in range(len(times)):                 # ascending time: later rows overwrite -> "last"
        out[nb - 1 - int(k[r])] = table[r]
    idx = np.arange(nb)
    good = ~np.isnan(out[:, 0])
    if not good.all():
        for c in range(out.shape[1]):
            out[:, c] = np.interp(idx, idx[good], out[good, c])
    out = out[-num_hist_frames:]
    human_xy = out[:, :2 * N].reshape(-1, N, 2)
    robot_xy = out[:, 2 * N:2 * N + 2]
    return human_xy, robot_xy, pose_now


def frame_table_frames(stamps: np.ndarray, human_xy: np.ndarray, robot_xy: np.ndarray, time_step: float,
                       num_hist_frames: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``frame_table`` for histories given as raw FRAMES - stamps [R], human_xy [R, N, 2], robot_xy [R, 2], oldest-pushed first, every
    human and the robot sharing the stamp of a frame (what ``update_state_hists`` produces) - and the host twin of the device
    ``frames_kernel`` (csrc/frames.hpp), in its operation order.  Same returns, bit for bit.

    Only the ``num_hist_frames`` newest bins are produced: the ``nb = max(bin) + 1`` rows of the full table are never materialised (a
    stale frame makes ``nb`` huge).  An empty bin is interpolated between the last frames of the nearest filled bin on either side - the
    older one may lie beyond the cut - as ``np.interp`` does it: ``slope = (y1 - y0) / (x1 - x0); y = slope * (x - x0) + y0``."""
    stamps = np.asarray(stamps, dtype=np.float64).reshape(-1)
    R = len(stamps)
    human_xy = np.asarray(human_xy, dtype=np.float64).reshape(R, -1, 2)
    N = human_xy.shape[1]
    tab = np.concatenate([human_xy.reshape(R, 2 * N), np.asarray(robot_xy, dtype=np.float64).reshape(R, 2)], axis=1)
    if R == 0:
        raise HistoryTooShortError("no complete history frame")
    pose_now = human_xy[-1].copy()                       # agent_df.tail(1): before anything is dropped or sorted
    keep = ~(np.isnan(tab).any(axis=1) | np.isnan(stamps))
    tab, t = tab[keep], stamps[keep]
    if len(t) == 0:
        raise HistoryTooShortError("no complete history frame")
    order = np.argsort(t, kind="stable")
    tab, t = tab[order], t[order]
    ns = np.trunc(t * 100.0).astype(np.int64)
    w = int(round(time_step * 100))
    k = (ns[-1] - ns) // w                               # bin counted backwards from the newest stamp (ascending in time: non-increasing)
    nb = int(k.max()) + 1
    n_grid = min(int(num_hist_frames), nb)
    out = np.empty((n_grid, tab.shape[1]))
    for b in range(n_grid):
        hit = np.nonzero(k == b)[0]
        if len(hit):
            out[n_grid - 1 - b] = tab[hit[-1]]           # the LAST sorted frame of the bin
            continue
        bo = int(k[k > b].min())                         # the nearest filled older bin (the oldest kept frame's bin is filled)
        bn = int(k[k < b].max())                         # the nearest filled newer bin (bin 0 is filled)
        y0, y1 = tab[np.nonzero(k == bo)[0][-1]], tab[np.nonzero(k == bn)[0][-1]]
        x0, x1, x = float(nb - 1 - bo), float(nb - 1 - bn), float(nb - 1 - b)
        slope = (y1 - y0) / (x1 - x0)
        out[n_grid - 1 - b] = slope * (x - x0) + y0
    return out[:, :2 * N].reshape(n_grid, N, 2), out[:, 2 * N:2 * N + 2], pose_now


def frame_table_frames_batched(stamps: np.ndarray, human_xy: np.ndarray, robot_xy: np.ndarray, n_frames: Optional[np.ndarray],
                               time_step: float, num_hist_frames: int) -> Dict[str, np.ndarray]:
    """``frame_table_frames`` for E episodes: stamps [E, R], human_xy [E, R, N, 2], robot_xy [E, R, 2]; the first ``n_frames[e]`` (1..R;
    None: all R) raw frames of episode e are valid.  Returns ``human_xy`` [E, F, N, 2], ``robot_xy`` [E, F, 2], ``pose_now`` [E, N, 2]
    float64 and ``n_grid`` [E] int32 with F = ``num_hist_frames``: episode e has ``n_grid[e]`` grid frames, oldest first in its rows
    0 .. n_grid[e]-1, zeros behind them (``n_grid[e]`` = 0: no complete frame) - the layout ``jmid_build_scene_stamped`` leaves."""
    stamps = np.asarray(stamps, dtype=np.float64)
    human_xy = np.asarray(human_xy, dtype=np.float64)
    robot_xy = np.asarray(robot_xy, dtype=np.float64)
    E, R, N, _ = human_xy.shape
    F = int(num_hist_frames)
    n_frames = np.full(E, R, dtype=np.int64) if n_frames is None else np.asarray(n_frames)
    if n_frames.shape != (E,) or (n_frames < 1).any() or (n_frames > R).any():
        raise ValueError("n_frames must hold E values in 1..R")
    out = {"human_xy": np.zeros((E, F, N, 2)), "robot_xy": np.zeros((E, F, 2)), "pose_now": np.empty((E, N, 2)),
           "n_grid": np.zeros(E, dtype=np.int32)}
    for e in range(E):
        n = int(n_frames[e])
        out["pose_now"][e] = human_xy[e, n - 1]
        try:
            h, r, _ = frame_table_frames(stamps[e, :n], human_xy[e, :n], robot_xy[e, :n], time_step, F)
        except HistoryTooShortError:
            continue
        out["n_grid"][e] = len(h)
        out["human_xy"][e, :len(h)] = h
        out["robot_xy"][e, :len(h)] = r
    return out


class TrackAbsentError(ValueError):
    """A pedestrian is not seen in the anchor frame (the newest frame with a finite stamp and robot position) of an episode handed to
    ``engine.build_scene_stamped(tracks=True)``: the resident scene cannot hold a node that is absent now.  Leave the track out."""

    def __init__(self, episode: int, track: int, message: Optional[str] = None):
        super().__init__(message or f"episode {episode}: track {track} is not seen in the anchor frame")
        self.episode, self.track = int(episode), int(track)


def _track_column(k: np.ndarray, nb: int, n_grid: int, F: int, seen: np.ndarray, y: np.ndarray, b_new: int = 0):
    """One track's column [F, 2] of the per-track frame table and its oldest filled bin b_old: k [n] the shared bins of the kept frames
    in sorted order, seen [n] bool where the track is seen, y [n, 2] its positions; ``b_new`` its newest filled bin (0: the anchor's).
    The bins b_new .. min(b_old, n_grid-1) are written, the rows of the others stay NaN."""
    ks = np.where(seen, k, -1)
    b_old = int(ks.max())
    col = np.full((F, 2), np.nan)
    for b in range(b_new, min(b_old, n_grid - 1) + 1):
        hit = np.nonzero(ks == b)[0]
        if len(hit):
            col[F - 1 - b] = y[hit[-1]]              # the LAST sorted seen frame of the bin
            continue
        bo = int(ks[ks > b].min())                   # the nearest filled older bin of THIS track (b < b_old: there is one)
        bn = int(ks[(ks < b) & seen].max())          # the nearest filled newer one (bin b_new is filled)
        y0, y1 = y[np.nonzero(ks == bo)[0][-1]], y[np.nonzero(ks == bn)[0][-1]]
        x0, x1, x = float(nb - 1 - bo), float(nb - 1 - bn), float(nb - 1 - b)
        slope = (y1 - y0) / (x1 - x0)
        col[F - 1 - b] = slope * (x - x0) + y0
    return col, b_old


def _coast_tracks(table, stamps, human_xy, robot_xy, time_step: float, F: int, max_coast: int):
    """The ``max_coast`` half of ``_track_table``: ``table`` is its result without coasting, in which a pedestrian who is not seen in the
    anchor frame has first_frame -1; every such column, first_frame and pose_now entry is decided again here.  Returns table + (coast,)."""
    hum, rob, pose_now, first, n_grid = table
    N = hum.shape[1]
    coast = np.where(first[1:] >= 0, 0, -1).astype(np.int32)
    if n_grid == 0:                                      # no kept frame: nobody is seen anywhere
        pose_now[:] = np.nan
    if n_grid == 0 or (coast == 0).all():
        return hum, rob, pose_now, first, n_grid, coast
    stamps = np.asarray(stamps, dtype=np.float64).reshape(-1)
    R = len(stamps)
    human_xy = np.asarray(human_xy, dtype=np.float64).reshape(R, N, 2)
    robot_xy = np.asarray(robot_xy, dtype=np.float64).reshape(R, 2)
    keep = ~(np.isnan(stamps) | np.isnan(robot_xy).any(axis=1))
    order = np.argsort(stamps[keep], kind="stable")
    t, H = stamps[keep][order], human_xy[keep][order]
    ns = np.trunc(t * 100.0).astype(np.int64)
    k = (ns[-1] - ns) // int(round(time_step * 100))
    nb = int(k.max()) + 1
    for j in np.nonzero(coast < 0)[0]:
        pose_now[j] = np.nan                             # not seen in the anchor frame: the coasted position, or left out
        seen = ~np.isnan(H[:, j]).any(axis=1)
        if not seen.any():
            continue
        b_new = int(k[seen].min())
        if b_new > max_coast or b_new > n_grid - 1:
            continue
        col, b_old = _track_column(k, nb, n_grid, F, seen, H[:, j], b_new)
        y_new = col[F - 1 - b_new]
        # (a grid row behind b_new, real or interpolated, gives the step; a single observation stands still)
        step = y_new - col[F - 2 - b_new] if b_new + 1 <= min(b_old, n_grid - 1) else np.zeros(2)
        for b in range(b_new):
            col[F - 1 - b] = y_new + float(b_new - b) * step
        hum[:, j] = col
        first[j + 1] = F - 1 - min(b_old, n_grid - 1)
        pose_now[j] = col[F - 1]
        coast[j] = b_new
    return hum, rob, pose_now, first, n_grid, coast


def _check_max_coast(max_coast, F: int) -> Optional[int]:
    if max_coast is None:
        return None
    if int(max_coast) != max_coast or not 0 <= int(max_coast) <= F - 2:
        raise ValueError("max_coast must be an integer in 0..F-2")
    return int(max_coast)


def _track_table(stamps: np.ndarray, human_xy: np.ndarray, robot_xy: np.ndarray, time_step: float, F: int, max_coast: Optional[int] = None):
    """``frame_table_tracks`` without its refusal: (human_xy [F, N, 2], robot_xy [F, 2], pose_now [N, 2], first_frame [N + 1], n_grid)
    whatever ``n_grid`` is (0: no kept frame - everything NaN, the robot's first_frame F, every pedestrian's -1).  With ``max_coast``
    (see ``frame_table_tracks``) ``coast`` [N] int32 comes behind them."""
    if max_coast is not None:
        out = _track_table(stamps, human_xy, robot_xy, time_step, F)
        return _coast_tracks(out, stamps, human_xy, robot_xy, time_step, F, max_coast)
    stamps = np.asarray(stamps, dtype=np.float64).reshape(-1)
    R = len(stamps)
    human_xy = np.asarray(human_xy, dtype=np.float64).reshape(R, -1, 2)
    robot_xy = np.asarray(robot_xy, dtype=np.float64).reshape(R, 2)
    N = human_xy.shape[1]
    hum, rob = np.full((F, N, 2), np.nan), np.full((F, 2), np.nan)
    first = np.full(N + 1, -1, dtype=np.int32)
    first[0] = F
    pose_now = human_xy[-1].copy() if R else np.full((N, 2), np.nan)      # before anything is dropped or sorted
    keep = ~(np.isnan(stamps) | np.isnan(robot_xy).any(axis=1))          # a human NaN drops nothing
    if not keep.any():
        return hum, rob, pose_now, first, 0
    order = np.argsort(stamps[keep], kind="stable")
    t, H, Rb = stamps[keep][order], human_xy[keep][order], robot_xy[keep][order]
    ns = np.trunc(t * 100.0).astype(np.int64)
    w = int(round(time_step * 100))
    k = (ns[-1] - ns) // w                               # the shared bins, counted back from the anchor (the last sorted kept frame)
    nb = int(k.max()) + 1
    n_grid = min(F, nb)
    first[0] = F - n_grid

    def column(seen, y):                                 # y [n, 2] of one track, seen [n] bool with the anchor seen -> its b_old
        return _track_column(k, nb, n_grid, F, seen, y)

    rob, _ = column(np.ones(len(t), dtype=bool), Rb)
    for j in range(N):
        seen = ~np.isnan(H[:, j]).any(axis=1)
        if not seen[-1]:                                 # absent now: first_frame -1, the column stays NaN
            continue
        hum[:, j], b_old = column(seen, H[:, j])
        first[j + 1] = F - 1 - min(b_old, n_grid - 1)
    return hum, rob, pose_now, first, n_grid


def frame_table_tracks(stamps: np.ndarray, human_xy: np.ndarray, robot_xy: np.ndarray, time_step: float,
                       num_hist_frames: int, max_coast: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, int]:
    """The frame table PER TRACK from raw frames - stamps [R], human_xy [R, N, 2], robot_xy [R, 2], oldest-pushed first - and the host
    twin of the device ``track_frames_kernel`` (csrc/frames.hpp), in its operation order.  A NaN coordinate of pedestrian j means "track
    j was not seen in this frame" and drops nothing:

      1. ``pose_now`` = the human positions of the last pushed frame, before anything is dropped or sorted (NaN where not seen)
      2. a frame is dropped iff its stamp or a robot coordinate is NaN
      3. the kept frames in stable sort order by stamp share one grid: ns = trunc(stamp * 100), w = round(time_step * 100), bin
         b = (ns_last - ns) // w counted back from the newest kept frame (the ANCHOR), nb = max(b) + 1, n_grid = min(F, nb); the robot's
         column is ``frame_table_frames``'s
      4. pedestrian j's frames are the kept ones where both its coordinates are non-NaN; a bin holds the last sorted of them, an empty
         bin between filled ones is interpolated between the nearest filled older and newer bin of THAT track in index space
         x = nb-1-b (``slope = (y1 - y0) / (x1 - x0); y = slope * (x - x0) + y0``), nothing is extrapolated in front of its oldest filled
         bin b_old(j), which may lie beyond the window

    Returns (human_xy [F, N, 2], robot_xy [F, 2], pose_now [N, 2], first_frame [N + 1] int32, n_grid) with F = ``num_hist_frames``:
    right-aligned, NaN in front, the newest frame in row F-1 (the layout of ``pad_short_window``); ``first_frame`` (robot first) is
    F - n_grid for the robot, F-1 - min(b_old(j), n_grid-1) for pedestrian j and -1 for a pedestrian not seen in the anchor frame (absent
    now: its column is NaN; leave it out of the scene).  Without human NaN the rows F-n_grid .. F-1 are the bytes of
    ``frame_table_frames``.  Raises ``HistoryTooShortError`` (``.n_grid`` attached) when n_grid < 2.

    ``max_coast`` (0 .. F-2 bins; None: everything above, and the five returns): a pedestrian who is not seen in the anchor frame is
    COASTED to it when his newest filled bin b_new is at most ``max_coast`` (and inside the window), and left out otherwise - the twin
    of ``track_frames_coast_kernel``.  Coasted: the bins b >= b_new of his column follow rule 4; the bins b < b_new are
    ``y(b) = y(b_new) + float(b_new - b) * step`` with ``step = y(b_new) - y(b_new + 1)`` when the grid row b_new + 1 exists in his window
    (real or interpolated) and 0 otherwise; ``first_frame`` by the same formula; ``pose_now`` = y(0).  Left out: ``first_frame`` -1, the
    column and ``pose_now`` NaN.  ``coast`` [N] int32 is returned as a sixth value: 0 seen in the anchor frame (everything as without
    ``max_coast``), b_new coasted (0: seen in the anchor's bin but not in the anchor frame itself), -1 left out."""
    F = int(num_hist_frames)
    out = _track_table(stamps, human_xy, robot_xy, time_step, F, _check_max_coast(max_coast, F))
    if out[4] < 2:
        err = HistoryTooShortError(f"{out[4]} history frames on the time_step grid, at least 2 needed")
        err.n_grid = out[4]
        raise err
    return out


def frame_table_tracks_batched(stamps: np.ndarray, human_xy: np.ndarray, robot_xy: np.ndarray, n_frames: Optional[np.ndarray],
                               time_step: float, num_hist_frames: int, max_coast: Optional[int] = None) -> Dict[str, np.ndarray]:
    """``frame_table_tracks`` for E episodes: stamps [E, R], human_xy [E, R, N, 2], robot_xy [E, R, 2]; the first ``n_frames[e]`` (1..R;
    None: all R) raw frames of episode e are valid.  Returns ``human_xy`` [E, F, N, 2], ``robot_xy`` [E, F, 2], ``pose_now`` [E, N, 2]
    float64, ``first_frame`` [E, N + 1] and ``n_grid`` [E] int32 - what ``jmid_build_scene_stamped_var`` leaves.  Nothing is raised for
    an episode: ``n_grid[e]`` < 2 is the too-short one, ``first_frame[e, 1 + j]`` = -1 the pedestrian who is absent now.
    ``max_coast``: as in ``frame_table_tracks``, with ``coast`` [E, N] int32 - what ``jmid_build_scene_stamped_coast`` leaves."""
    stamps = np.asarray(stamps, dtype=np.float64)
    human_xy = np.asarray(human_xy, dtype=np.float64)
    robot_xy = np.asarray(robot_xy, dtype=np.float64)
    E, R, N, _ = human_xy.shape
    F = int(num_hist_frames)
    max_coast = _check_max_coast(max_coast, F)
    n_frames = np.full(E, R, dtype=np.int64) if n_frames is None else np.asarray(n_frames)
    if n_frames.shape != (E,) or (n_frames < 1).any() or (n_frames > R).any():
        raise ValueError("n_frames must hold E values in 1..R")
    out = {"human_xy": np.empty((E, F, N, 2)), "robot_xy": np.empty((E, F, 2)), "pose_now": np.empty((E, N, 2)),
           "first_frame": np.empty((E, N + 1), dtype=np.int32), "n_grid": np.empty(E, dtype=np.int32)}
    if max_coast is not None:
        out["coast"] = np.empty((E, N), dtype=np.int32)
    for e in range(E):
        n = int(n_frames[e])
        parts = _track_table(stamps[e, :n], human_xy[e, :n], robot_xy[e, :n], time_step, F, max_coast)
        for key, v in zip(("human_xy", "robot_xy", "pose_now", "first_frame", "n_grid", "coast"), parts):
            out[key][e] = v
    return out


def histories_as_frames(prev_states, prev_robot_states, joined: bool = True):
    """The per-human lists of ``update_state_hists`` as raw frames (stamps [R], human_xy [R, N, 2], robot_xy [R, 2]) when they ARE frames:
    every human's list has the same stamps, entry by entry, as the robot's last R entries, and a stamp that occurs twice comes with
    NaN-free data (``frame_table`` joins on stamp VALUES, so a duplicated stamp next to a dropped frame is not a frame-wise table).
    None otherwise (somebody edited the lists by hand): ``frame_table`` handles those.  ``joined=False``: for ``frame_table_tracks``,
    which never joins on stamp values - the last condition does not apply."""
    R = len(prev_states[0]) if len(prev_states) else 0
    if R == 0 or len(prev_robot_states) < R or any(len(h) != R for h in prev_states):
        return None
    try:
        hum = np.asarray(prev_states, dtype=np.float64)                     # [N, R, 3]
        rob = np.asarray(prev_robot_states[-R:], dtype=np.float64)          # [R, 3]
    except ValueError:
        return None
    if hum.ndim != 3 or hum.shape[2] != 3 or rob.shape != (R, 3):
        return None
    stamps = rob[:, 2]
    if not (hum[:, :, 2] == stamps[None]).all():                            # (a NaN stamp fails this too)
        return None
    if joined and len(np.unique(stamps)) != R and (np.isnan(hum).any() or np.isnan(rob).any()):
        return None
    # (the robot's list is unbounded, but frame_table's join takes the LAST entry with a stamp: always one of these R)
    return stamps.copy(), np.ascontiguousarray(hum[:, :, 0:2].transpose(1, 0, 2)), np.ascontiguousarray(rob[:, 0:2])


def assemble_forecasts(in_cluster: np.ndarray, sel_or_pos: np.ndarray, logw_in: Optional[np.ndarray], cv,
                       pose_now: np.ndarray, k: int, K: int, n_agents: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The result assembly of ``predict_ret_best`` (mid_sim_wrapper.py:493-510, :444-454) and the host twin of the device
    ``assemble_kernel`` (csrc/frames.hpp), for one scene or, with a leading episode axis on every array, for E of them.

    in_cluster [N] bool; k < K: sel_or_pos = the kept samples [A, k, H, 2] and logw_in [A, k] (float32, as ``predict_scene`` returns
    them); k == K: sel_or_pos = all samples [K, A, H, 2] (``pos``) and logw_in is ignored; cv [N, H, 2] float64 (every pedestrian's
    constant-velocity row) or, for one scene, ``SceneBatch.cv_forecasts`` (the rows of the pedestrians outside the cluster by track id:
    nothing is made dense for the others); pose_now [N, 2].  Returns (forecasts [N, k, H+1, 2], log-weights [N, k]) float64: the in-cluster rows
    scattered by ascending track id, the others their ``cv`` row under the cluster's weight row, the current pose prepended.
    ``n_agents`` [E]: episodes of different counts, A = the largest and episode e's agents in its first n_agents[e] rows (``pad_agents``;
    the others are not read).  None: every episode has A."""
    in_cluster, rows, pose_now = np.asarray(in_cluster, dtype=bool), np.asarray(sel_or_pos), np.asarray(pose_now)
    if k < K:
        lw = np.asarray(logw_in).astype(np.float64)
    else:
        rows = np.swapaxes(rows, -4, -3)                                     # [K, A, H, 2] -> agents by ascending id
        lw = _uniform_logw(rows.shape[-4], K)
    H = rows.shape[-2]
    forecasts = np.empty(in_cluster.shape + (k, H + 1, 2), dtype=np.float64)
    logw = np.empty(in_cluster.shape + (k,), dtype=np.float64)
    forecasts[..., 0, :] = pose_now[..., None, :]
    # everybody the constant-velocity row under the cluster's first weight row, then the in-cluster rows over them (no loop over
    # pedestrians): both masks take their (episode, row) pairs in row-major order, an episode's n tracks against its first n rows
    future = forecasts[..., 1:, :]
    if isinstance(cv, dict):
        for i, row in cv.items():
            future[i] = row
    else:
        future[...] = np.asarray(cv)[..., None, :, :]
    logw[...] = lw[..., :1, :]
    real = Ellipsis if n_agents is None else np.arange(rows.shape[-4]) < np.asarray(n_agents)[:, None]
    future[in_cluster] = rows[real].reshape(-1, k, H, 2)
    if k < K:                                                                # (k == K: every weight row is the one just written)
        logw[in_cluster] = lw[real].reshape(-1, k)
    return forecasts, logw


@functools.lru_cache(maxsize=None)
def _uniform_logw(A: int, K: int) -> np.ndarray:
    """The weight rows of a call that returns all K samples (mid_sim_wrapper.py:507), [A, K]; read-only, computed once per shape."""
    lw = np.log(np.ones((A, K), dtype=np.float64) / K)
    lw.setflags(write=False)
    return lw


# --------------------------------------------------------------------------------------------- scene batch
@dataclass
class SceneBatch:
    ids_in: np.ndarray               # pedestrian track ids inside the chosen cluster, ascending == batch row order
    ids_out: np.ndarray              # pedestrian track ids outside the cluster (constant-velocity fill)
    x: np.ndarray                    # [A, F, 6] f32 raw state  [px, py, vx, vy, ax, ay]
    x_st: np.ndarray                 # [A, F, 6] f32 standardized
    nbr_sum: np.ndarray              # [A, 2, F, 6] f32   edge types (PED->PED, PED->ROBOT)
    edge_mask: np.ndarray            # [A, 2] f32
    p0: np.ndarray                   # [A, 2] f32 current positions (integrator initial condition)
    cv_forecasts: Dict[int, np.ndarray] = field(default_factory=dict)   # id -> [H, 2] f64
    pose_now: Optional[np.ndarray] = None                               # [N, 2] f64
    robot_in_cluster: bool = False
    first_index: Optional[np.ndarray] = None   # [A] int32 first history frame of every row (the reference's first_history_index)


def edge_scaling_last(adj3: np.ndarray) -> np.ndarray:
    """scene_graph.py:203-225 evaluated at the last of 3 frames.  adj3 [3, n, n] (type-valued adjacency).
    conv with the addition filter, clamp 1, zero where not adjacent now; the removal filter [1, 0] is the
    identity at this frame."""
    f = EDGE_ADDITION_FILTER
    s = np.minimum(f[0] * adj3[2] + f[1] * adj3[1] + f[2] * adj3[0], 1.0)
    s = np.where(adj3[2] == 0, 0.0, s)
    return np.minimum(s, 1.0)


def pad_short_window(human_xy: np.ndarray, robot_xy: np.ndarray, F: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The episode-start case of ``first_frame``: L < F shared frames (human_xy [L, N, 2], robot_xy [L, 2], oldest first) as F-frame arrays
    that are NaN in front, with ``first_frame`` = F - L for the robot and every pedestrian.  L >= F: the last F frames, first_frame 0."""
    human_xy = np.asarray(human_xy, dtype=np.float64)
    robot_xy = np.asarray(robot_xy, dtype=np.float64)
    L, N, _ = human_xy.shape
    if L < 1 or robot_xy.shape != (L, 2):
        raise ValueError("expected human_xy [L, N, 2] and robot_xy [L, 2] with L >= 1")
    pad = max(int(F) - L, 0)
    hum = np.concatenate([np.full((pad, N, 2), np.nan), human_xy[-int(F):]], axis=0)
    rob = np.concatenate([np.full((pad, 2), np.nan), robot_xy[-int(F):]], axis=0)
    return hum, rob, np.full(N + 1, pad, dtype=np.int32)


def _check_first_frame(first_frame, E: int, N: int, F: int, force_all_in_cluster: bool, allow_absent: bool = False) -> np.ndarray:
    ff = np.asarray(first_frame)
    if ff.shape != (E, N + 1) or not np.issubdtype(ff.dtype, np.integer):
        raise ValueError("first_frame must hold N + 1 integers per episode, robot first")
    if allow_absent:
        if (ff[:, 0] < 0).any() or (ff[:, 1:] < -1).any() or (ff > F - 1).any():
            raise ValueError("first_frame must lie in 0..F-1, or be -1 for a pedestrian who is not in the scene")
        if (ff[:, 1:] == -1).all(axis=1).any():
            e = int(np.nonzero((ff[:, 1:] == -1).all(axis=1))[0][0])
            raise ValueError(f"episode {e}: every pedestrian is left out (first_frame -1)")
    elif (ff < 0).any() or (ff > F - 1).any():
        raise ValueError("first_frame must lie in 0..F-1")
    if not force_all_in_cluster and (ff[:, 0] > F - 2).any():
        raise ValueError("the robot needs at least 2 frames unless force_all_in_cluster is set")
    return ff.astype(np.int32)


def build_scene(human_xy: np.ndarray, robot_xy: np.ndarray, time_step: float, horizon: int,
                num_hist_frames: int = 6, force_all_in_cluster: bool = False, first_frame=None, allow_absent: bool = False) -> SceneBatch:
    """mid_sim_wrapper.py:313-437 + preprocessing.py:428-694 for one scene.

    human_xy [F, N, 2], robot_xy [F, 2] on the ``time_step`` grid (oldest first).  ``first_frame`` [N + 1] (robot first): see
    ``build_scenes_batched``, whose episode this then is - the rows are the EGO rows (in-cluster pedestrians with at least two frames),
    a one-frame pedestrian is listed in ``ids_out`` with its position repeated as its constant-velocity row.  ``allow_absent``: a
    pedestrian with first_frame -1 is not in the scene - neither in ``ids_in`` nor in ``ids_out``.
    """
    F, N, _ = human_xy.shape
    if F < num_hist_frames:
        raise HistoryTooShortError(f"{F} history frames available, {num_hist_frames} needed")
    if first_frame is not None:
        b = build_scenes_batched(np.asarray(human_xy, dtype=np.float64)[None], np.asarray(robot_xy, dtype=np.float64)[None], time_step,
                                 force_all_in_cluster=force_all_in_cluster, horizon=horizon, first_frame=np.asarray(first_frame)[None],
                                 allow_absent=allow_absent)
        rows = np.nonzero(b["in_cluster"][0])[0]
        out = np.nonzero(~b["in_cluster"][0] & (b["first_index"][0] >= 0))[0]
        return SceneBatch(ids_in=rows.astype(np.int64), ids_out=out.astype(np.int64), x=b["x"][0, rows], x_st=b["x_st"][0, rows],
                          nbr_sum=b["nbr_sum"][0, rows], edge_mask=b["edge_mask"][0, rows], p0=b["p0"][0, rows],
                          cv_forecasts={int(i): b["cv"][0, i] for i in out}, robot_in_cluster=bool(b["robot_in_cluster"][0]),
                          first_index=b["first_index"][0, rows])
    dt = time_step
    # positions at the last frame, sorted by track id: robot (-1) first
    pos_last = np.concatenate([robot_xy[-1:], human_xy[-1]], axis=0)           # [N+1, 2]
    track_ids = np.concatenate([[ROBOT_ID], np.arange(N)])
    sq = np.square(pos_last[:, None] - pos_last[None, :])
    dists = np.sqrt(np.sum(sq, axis=2))
    mask = dists < ATTENTION_RADIUS
    if force_all_in_cluster:
        in_mask = np.ones(N + 1, dtype=bool)
    else:
        cluster_means = (mask @ pos_last) / mask.sum(axis=1, keepdims=True)
        robot_dist = np.linalg.norm(cluster_means - pos_last[0], axis=1)
        chosen = int(np.argmin(robot_dist[1:])) + 1
        in_mask = mask[chosen]
    ids_in_all = track_ids[in_mask]
    ids_out_all = track_ids[~in_mask]

    # scene nodes in track-id order (robot first when it is in the cluster); node state [pos, vel, acc] by first differences for all
    # of them at once (element-wise, so the values derivative_of gives per coordinate)
    node_ids = list(ids_in_all)
    n = len(node_ids)
    pos_all = np.concatenate([robot_xy[:, None, :], human_xy], axis=1)         # [F, N+1, 2], robot first like track_ids

    def deriv(a):                                                              # [n, F, 2], differences along the frames
        if F < 2:
            return np.zeros_like(a)
        d = np.empty_like(a)
        np.subtract(a[:, 1:], a[:, :-1], out=d[:, 1:])
        d[:, 0] = d[:, 1]
        return d / dt

    P = np.ascontiguousarray(pos_all[:, in_mask].transpose(1, 0, 2))           # [n, F, 2]
    V = deriv(P)
    S = np.concatenate([P, V, deriv(V)], axis=2)                               # [n, F, 6]
    types = np.where(ids_in_all == ROBOT_ID, TYPE_VALUE_ROBOT, TYPE_VALUE_PED)

    # constant-velocity forecasts for pedestrians outside the cluster (mid_sim_wrapper.py:413-429)
    cv = {}
    out_peds = [int(i) for i in ids_out_all if i != ROBOT_ID]
    if out_peds:
        last = human_xy[-1, out_peds]                                          # [m, 2]
        v_last = (last - human_xy[-2, out_peds]) / dt if F >= 2 else np.zeros_like(last)
        fc_all = last[:, None, :] + np.cumsum(np.repeat((v_last * dt)[:, None, :], horizon, axis=1), axis=1)
        for r, i in enumerate(out_peds):
            cv[i] = fc_all[r]

    # temporal scene graph over the last 3 frames (scene.py:67-110, scene_graph.py:111-201)
    P3 = S[:, F - 3:F, 0:2].transpose(1, 0, 2)                                 # [3, n, 2]
    d3 = np.sqrt(np.square(P3[:, :, None] - P3[:, None, :]).sum(-1))           # [3, n, n]
    type_mat = np.tile(types[None, :], (n, 1)).astype(np.float64)
    np.fill_diagonal(type_mat, 0)
    adj3 = (d3 <= ATTENTION_RADIUS).astype(np.float64) * type_mat[None]
    eye = np.eye(n, dtype=bool)
    adj3[:, eye] = 0.0
    scaling = edge_scaling_last(adj3)                                          # [n, n]
    connected = scaling > 1e-2

    ped_rows = np.nonzero(ids_in_all != ROBOT_ID)[0]
    A = len(ped_rows)
    x = S[ped_rows]                                                            # [A, F, 6]
    rel = np.zeros((A, 1, 6))
    rel[:, 0, 0:2] = x[:, -1, 0:2]
    x_st = (x - rel) / STATE_STD
    nbr_sum = np.zeros((A, 2, F, 6), dtype=np.float32)
    edge_mask = np.zeros((A, 2), dtype=np.float32)
    for r, k in enumerate(ped_rows):
        # edge values are NOT filtered by edge type (scene_graph.py:293-299): both types see the same sum
        ev = scaling[k, connected[k]].astype(np.float32)
        edge_mask[r, :] = np.float32(min(float(ev.sum(dtype=np.float32)), 1.0)) if ev.size else np.float32(0.0)
    # neighbour state relative to the ego's WHOLE present state (preprocessing.py:531-550), summed per edge type in node order in
    # float32: one pass over the neighbours j for all egos at once (a neighbour that is not connected adds +0.0, which leaves a
    # float32 partial sum as it is - the sums start at +0.0 and never become -0.0)
    if A and n:
        conn = connected[ped_rows]                                             # [A, n]
        tm = type_mat[ped_rows]
        sel = np.stack([conn & (tm == TYPE_VALUE_PED), conn & (tm == TYPE_VALUE_ROBOT)], axis=1)   # [A, 2, n]
        ego_now = x[:, -1, :]                                                  # [A, 6]
        for j in range(n):
            if not sel[:, :, j].any():
                continue
            term = ((S[j][None] - ego_now[:, None, :]) / STATE_STD).astype(np.float32)             # [A, F, 6]
            nbr_sum += np.where(sel[:, :, j, None, None], term[:, None], np.float32(0.0))
    ids_in = np.array([i for i in node_ids if i != ROBOT_ID], dtype=np.int64)
    ids_out = np.array(out_peds, dtype=np.int64)
    return SceneBatch(ids_in=ids_in, ids_out=ids_out, x=x.astype(np.float32), x_st=x_st.astype(np.float32),
                      nbr_sum=nbr_sum, edge_mask=edge_mask, p0=x[:, -1, 0:2].astype(np.float32),
                      cv_forecasts=cv, robot_in_cluster=bool(in_mask[0]), first_index=np.zeros(A, dtype=np.int32))


# --------------------------------------------------------------------------------------------- batched builder
def build_scenes_batched(human_xy: np.ndarray, robot_xy: np.ndarray, time_step: float,
                         force_all_in_cluster: bool = False, horizon: Optional[int] = None, first_frame=None,
                         allow_absent: bool = False) -> Dict[str, np.ndarray]:
    """``build_scene`` for E independent episodes at once (no Python loop over episodes): the feed of the
    256-4096-episode evaluation sweeps.

    human_xy [E, F, N, 2], robot_xy [E, F, 2].  Every pedestrian gets a row; ``in_cluster`` [E, N] tells which rows
    the reference would have sent through the network (the others get constant-velocity forecasts there).
    Returns x, x_st [E, N, F, 6], nbr_sum [E, N, 2, F, 6], edge_mask [E, N, 2], p0 [E, N, 2] (all float32),
    in_cluster [E, N] bool, robot_in_cluster [E] bool.  Rows outside the cluster are computed as if they had no
    neighbours in the graph (they are not graph nodes in the reference).  Bit-identical to ``build_scene`` per episode.
    With ``horizon`` the constant-velocity forecasts of EVERY pedestrian (what the reference returns for the ones
    outside the cluster, mid_sim_wrapper.py:413-429) come back as ``cv`` [E, N, horizon, 2] float64.

    ``first_frame`` [E, N + 1] integers in 0..F-1, robot first (the host twin of ``jmid_build_scene_var``, csrc/scene.hpp): node j is
    present on frames first_frame[j] .. F-1 and its earlier positions are never read.  Velocity and acceleration are first differences
    over the node's own span (data_utils.py:24-37; one frame: zero), x and x_st are NaN in front of it (``node.get(padding=nan)``), the
    scene graph has no adjacency on a frame where a node is absent (environment/scene.py:84-106), and a connected neighbour is taken
    with padding 0.0 and THEN standardised (preprocessing.py:531-550): absent, it adds (0 - ego_now) / std.  A pedestrian with one frame
    is no ego row (``in_cluster`` False) but counts in the cluster choice and as a neighbour.  ``first_index`` [E, N] int32 is returned
    in every case (zeros without ``first_frame``); all-zero ``first_frame`` gives the bits of None.

    ``allow_absent`` (the host twin of ``jmid_build_scene_absent``): ``first_frame[e, 1 + j]`` may be -1 - pedestrian j is NOT IN THE SCENE
    of episode e.  His positions are never read, he is no candidate of the cluster choice, no member of a cluster mean, no graph node,
    no neighbour and no ego row; his rows come back NaN (x, x_st, nbr_sum, edge_mask, p0, cv), ``in_cluster`` False, ``first_index`` -1,
    and every output of every other track is what the episode gives with his column removed.  The robot may not be -1; an episode in
    which every pedestrian is -1 raises ValueError.  Without a -1 the bits of ``allow_absent=False``.
    """
    E, F, N, _ = human_xy.shape
    dt = time_step
    ff = None if first_frame is None else _check_first_frame(first_frame, E, N, F, force_all_in_cluster, allow_absent)
    absent = None                                                                  # [E, N+1] the nodes that are not in the scene
    if ff is not None and (ff < 0).any():
        absent, ff_in = ff < 0, ff
        ff = np.where(absent, F, ff)                                               # present on no frame: NaN wherever a position is taken
    pos = np.concatenate([robot_xy[:, :, None, :], human_xy], axis=2)              # [E, F, N+1, 2], robot first
    if ff is not None:
        present = np.arange(F)[None, None, :] >= ff[:, :, None]                    # [E, N+1, F]
        pos = np.where(present.transpose(0, 2, 1)[..., None], pos, np.nan)
    last = pos[:, -1]                                                              # [E, N+1, 2]
    d_last = np.sqrt(np.square(last[:, :, None] - last[:, None, :]).sum(-1))
    near = d_last < ATTENTION_RADIUS
    if force_all_in_cluster:
        inc = np.ones((E, N + 1), dtype=bool)
    else:
        # (a node that is not in the scene is near nobody: a zero in its place keeps its NaN out of the others' sums)
        with np.errstate(invalid="ignore"):                                        # (its own row: 0 / 0)
            means = (near.astype(np.float64) @ (last if absent is None else np.where(absent[..., None], 0.0, last))) / near.sum(axis=2, keepdims=True)
        rdist = np.linalg.norm(means - last[:, :1], axis=2)
        if absent is not None:                                                     # no candidate (its 0 / 0 would be the minimum)
            rdist = np.where(absent, np.inf, rdist)
        chosen = np.argmin(rdist[:, 1:], axis=1) + 1
        inc = near[np.arange(E), chosen]                                           # [E, N+1]
    if absent is not None:
        inc = inc & ~absent
    # node states [E, N+1, F, 6] by first differences (first element duplicated)
    P = pos.transpose(0, 2, 1, 3)                                                  # [E, N+1, F, 2]

    def deriv(a):
        dd = np.diff(a, axis=2) / dt
        d = np.concatenate([dd[:, :, :1], dd], axis=2)
        if ff is None:
            return d
        # the node's own span: the first present element duplicates the second, a single element is zero, NaN in front
        nxt = np.take_along_axis(d, np.minimum(ff + 1, F - 1)[:, :, None, None], axis=2)               # [E, N+1, 1, 2]
        first_val = np.where((ff < F - 1)[:, :, None, None], nxt, 0.0)
        d = np.where((np.arange(F)[None, None, :] == ff[:, :, None])[..., None], first_val, d)
        return np.where(present[..., None], d, np.nan)

    with np.errstate(invalid="ignore"):
        V = deriv(P)
        A_ = deriv(V)
    S = np.concatenate([P, V, A_], axis=3)                                         # [E, N+1, F, 6]
    # temporal scene graph over the last three frames, in-cluster nodes only
    P3 = P[:, :, F - 3:F].transpose(0, 2, 1, 3)                                    # [E, 3, N+1, 2]
    with np.errstate(invalid="ignore"):
        d3 = np.sqrt(np.square(P3[:, :, :, None] - P3[:, :, None, :]).sum(-1))     # [E, 3, n, n]; NaN where a node is absent: not <= radius
        near3 = d3 <= ATTENTION_RADIUS
    types = np.full(N + 1, float(TYPE_VALUE_PED))
    types[0] = float(TYPE_VALUE_ROBOT)
    tmat = np.tile(types[None, :], (N + 1, 1))
    np.fill_diagonal(tmat, 0)
    pair_in = (inc[:, :, None] & inc[:, None, :]).astype(np.float64)               # [E, n, n]
    adj3 = near3.astype(np.float64) * tmat[None, None] * pair_in[:, None]
    f = EDGE_ADDITION_FILTER
    scal = np.minimum(f[0] * adj3[:, 2] + f[1] * adj3[:, 1] + f[2] * adj3[:, 0], 1.0)
    scal = np.where(adj3[:, 2] == 0, 0.0, scal)                                    # [E, n, n]
    conn = scal > 1e-2
    ego = inc[:, 1:]
    Sn = S                                                                          # what a neighbour contributes
    if ff is not None:
        ego = ego & (ff[:, 1:] <= F - 2)                                            # an ego row needs two frames
        conn = conn & np.concatenate([np.ones((E, 1), dtype=bool), ego], axis=1)[:, :, None]     # the others have no graph row
        Sn = np.where(present[..., None], S, 0.0)                                   # padding 0.0, standardised below
    xs = S[:, 1:]                                                                   # pedestrians [E, N, F, 6]
    rel = np.zeros((E, N, 1, 6))
    rel[:, :, 0, 0:2] = xs[:, :, -1, 0:2]
    x_st = (xs - rel) / STATE_STD
    em = np.minimum((scal[:, 1:] * conn[:, 1:]).astype(np.float32).sum(axis=2, dtype=np.float32), np.float32(1.0))
    edge_mask = np.repeat(em[:, :, None], 2, axis=2).astype(np.float32)
    nbr_sum = np.zeros((E, N, 2, F, 6), dtype=np.float32)
    ego_now = xs[:, :, -1:, :]                                                      # [E, N, 1, 6]
    for j in range(N + 1):                                                          # neighbours in node order
        relj = ((Sn[:, j][:, None] - ego_now) / STATE_STD).astype(np.float32)       # [E, N, F, 6]
        w = conn[:, 1:, j].astype(np.float32)[:, :, None, None]
        e_idx = 1 if j == 0 else 0                                                  # robot -> edge type PED->ROBOT
        nbr_sum[:, :, e_idx] = nbr_sum[:, :, e_idx] + relj * w
    out = dict(x=xs.astype(np.float32), x_st=x_st.astype(np.float32), nbr_sum=nbr_sum, edge_mask=edge_mask,
               p0=xs[:, :, -1, 0:2].astype(np.float32), in_cluster=ego, robot_in_cluster=inc[:, 0],
               first_index=np.zeros((E, N), dtype=np.int32) if ff is None else np.ascontiguousarray((ff if absent is None else ff_in)[:, 1:]))
    if ff is not None:                                                              # (one NaN, whatever the arithmetic made of its payload)
        gone = ~present[:, 1:, :, None]
        out["x"] = np.where(gone, np.float32(np.nan), out["x"])
        out["x_st"] = np.where(gone, np.float32(np.nan), out["x_st"])
    if horizon is not None:      # same operations, in the same order, as build_scene's per-pedestrian loop
        step = np.repeat((xs[:, :, -1, 2:4] * dt)[:, :, None, :], horizon, axis=2)     # [E, N, H, 2]
        out["cv"] = xs[:, :, -1:, 0:2] + np.cumsum(step, axis=2)
    if absent is not None:                                                          # not in the scene: NaN rows
        for key in ("x", "x_st", "nbr_sum", "edge_mask", "p0", "cv"):
            if key in out:
                g = absent[:, 1:].reshape(absent[:, 1:].shape + (1,) * (out[key].ndim - 2))
                out[key] = np.where(g, out[key].dtype.type(np.nan), out[key])
    return out


# --------------------------------------------------------------------------------------------- synthetic feeds
# ---------------------------------------------------------------------------------------------- padded scene batches
# Episodes of different in-cluster counts n[e] in ONE device call of the uniform shape [E, K * A, ...], A = max(n) (the *_padded
# entries of include/jmid_hip.h): agent a of episode e is real iff a < n[e]; sample s of agent a is row s * A + a.

def pad_agents(arr: np.ndarray, in_cluster: np.ndarray, A: int) -> np.ndarray:
    """Per-track arrays [E, N, ...] -> [E, A, ...]: episode e's in-cluster rows in ascending track id, then zero rows."""
    E = arr.shape[0]
    out = np.zeros((E, A) + arr.shape[2:], dtype=arr.dtype)
    for e in range(E):
        rows = np.nonzero(in_cluster[e])[0]
        out[e, :rows.size] = arr[e, rows]
    return out


def pad_samples(per_episode: Sequence[np.ndarray], n_agents: np.ndarray, A: int, K: int) -> np.ndarray:
    """Per-episode sample rows [K * n[e], ...] (row s * n[e] + a, as the plain call takes them) -> [E, K * A, ...] with the row of
    (s, a) at s * A + a and zeros in the padded agents' rows."""
    first = np.asarray(per_episode[0])
    out = np.zeros((len(per_episode), K * A) + first.shape[1:], dtype=first.dtype)
    for e, x in enumerate(per_episode):
        n = int(n_agents[e])
        out[e].reshape((K, A) + first.shape[1:])[:, :n] = np.asarray(x).reshape((K, n) + first.shape[1:])
    return out


def unpad_samples(arr: np.ndarray, n_agents: np.ndarray, e: int) -> np.ndarray:
    """The inverse for one episode of an output [E, K, A, ...]: its real agents [K, n[e], ...]."""
    return arr[e][:, :int(n_agents[e])]


def key_mask_words(n_agents: np.ndarray, A: int, K: int, T: int) -> np.ndarray:
    """NumPy twin of the device's key-mask words (csrc/padded.hpp): uint32 [E, ceil(S / 32)], S = K * A * T; bit i of word w of
    episode e is set iff key 32 w + i < S belongs to a real agent - token j = (s * A + a) * T + t is a valid key iff a < n[e]."""
    S = K * A * T
    nw = (S + 31) // 32
    key = np.arange(nw * 32)
    valid = (key[None, :] < S) & (((key // T) % A)[None, :] < np.asarray(n_agents).reshape(-1, 1))
    bits = valid.reshape(len(valid), nw, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return bits.sum(axis=2).astype(np.uint32)


def synthetic_episodes(E: int, N: int, seed: int, time_step: float = 0.25, num_hist_frames: int = 6,
                       horizon: int = 12) -> Dict[str, np.ndarray]:
    """Synthetic scene batches for measurement: per episode pos0 ~ U(-2,2)^2,
    vel ~ U(-0.5,0.5)^2 m/s, 7 frames at dt (6 kept), robot at (0,-3) + 0.2 t y; all agents forced into the
    cluster (A = N).  Returns stacked encoder inputs and the constant-velocity ground truth."""
    rng = np.random.default_rng(seed)
    pos0 = rng.uniform(-2.0, 2.0, (E, N, 2))
    vel = rng.uniform(-0.5, 0.5, (E, N, 2))
    t = np.arange(num_hist_frames + 1) * time_step
    hum = pos0[:, None] + vel[:, None] * t[None, :, None, None]                    # [E, F+1, N, 2]
    rob = np.array([0.0, -3.0])[None, None] + np.array([0.0, 0.2])[None, None] * t[None, :, None]
    rob = np.broadcast_to(rob, (E, num_hist_frames + 1, 2))
    b = build_scenes_batched(hum[:, -num_hist_frames:], rob[:, -num_hist_frames:], time_step, force_all_in_cluster=True)
    steps = (np.arange(horizon) + 1)[None, None, :, None] * time_step
    gt = (hum[:, -1][:, :, None, :] + vel[:, :, None, :] * steps).astype(np.float32)
    return dict(x=b["x"], x_st=b["x_st"], nbr_sum=b["nbr_sum"], edge_mask=b["edge_mask"], p0=b["p0"], gt=gt)
