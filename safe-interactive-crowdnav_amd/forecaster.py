"""Drop-in predictor: same call surface as the reference's ``HumanTrajectoryForecasterSim``.

Reference: ``sicnav_diffusion/JMID/mid_sim_wrapper.py:173-510`` (class at ``:207``).  The only caller,
``SICNavAcados`` (``sicnav_diffusion/policy/sicnav_acados.py:996-1000, 1171-1182, 1641-1651``), uses

    f = HumanTrajectoryForecasterSim(env_config, mid_config_file)
    f.num_hist_frames
    f.update_state_hists(robot_state, human_states, time_stamp)
    forecasts, log_weights = f.predict_ret_best()      # [N, k, H+1, 2] f64, [N, k] f64

and nothing else.  Here the history buffers and the scene/batch construction are NumPy on the host
(``scene.py``), and everything from the context encoder to the integrated sample trajectories runs in the HIP
library through the C ABI (``engine.py`` -> ``include/jmid_hip.h``).  There is no CPU fallback for that part.

Arithmetic (``precision``): since round 6 the class default is the mode ``bench.py`` quotes, ``"f16mx"`` (fp16 activation x
split-fp16 weight, ``A_hi . W_hi`` on the fp16 matrix cores plus the correction term as ONE bf8 x bf8 MFMA per 64-deep block;
5e-6 m on the 50-step cfg3 sample, worst fixture 5.7e-5 m against the 1e-4 m gate) TOGETHER WITH ``self_check=True``: every
accuracy figure in this repository is on seeded random-init weights (the trained blobs are absent from the reference), so the
first call of every input shape is also run in ``"f16x3"`` - fp32-class three-term split-fp16 products, ~1e-6 m from the
reference (the fp32-vs-fp64 noise floor) - on the call's own inputs, and the instance moves to ``"f16x3"`` for good (with a
``RuntimeWarning``) when the mean displacement between the two exceeds ``self_check_tol`` (5e-5 m: half the gate, so a mode that
passes holds the gate with 2x margin on that checkpoint and shape).  ``"f16x2"`` (the same products with fp16 correction terms),
``"f16x3"`` and ``"f32"`` (exact-fp32 MFMA) can be asked for by name; ``self_check`` only acts on ``"f16mx"`` / ``"f16x2"``.  If an activation ever leaves the fp16 range (``JMID_ERANGE``) the call is repeated in the exact-fp32 mode: same
result, ~5x the latency - counted in ``erange_fallbacks`` / ``forecaster.ERANGE_FALLBACKS`` and warned about once.

RNG contract (``rng_compat``): ``x_T`` is always the first draw of torch's CPU default generator
(``MID/models/diffusion.py:499``).  The reference also draws one (unused, DDIM) ``randn_like(x_T)`` per reverse step
(``:509``) on the device ``x_T`` was moved to: the CPU generator in a CPU-only run (what the golden captures are),
the CUDA generator on a GPU host (``MID/mid.py:91``).  ``rng_compat="cpu"`` consumes those draws from the CPU
generator, ``"cuda"`` from the device generator (the CPU generator then advances by ``x_T`` only; the device generator is
moved by what the draws would consume without launching them, ``advance_cuda_generator``), and the default
``"auto"`` does what the reference itself would do on this host (``"cuda"`` iff ``torch.cuda.is_available()``).
``rng_compat="device"`` (opt-in) leaves that contract: ``x_T`` comes from the library's counter generator (``noise.py``,
``jmid_noise_fill``) as a pure function of (``seed``, ``episode_id``, draw number), the draw number advancing by one block of
``n_steps + 1`` per ``predict_ret_best()``, and the torch generators are not touched.  Statistically, not seed-, compatible with
the reference.
``collision_free_rounds=R`` > 0 (opt-in, with ``rng_compat="device"``; 0 is today's behaviour, draw numbering included): collision-free
sampling (``JmidEngine.denoise_reject``; the rule stands in include/jmid_hip.h) - a joint sample in which two pedestrians come closer
than ``collision_threshold`` is redrawn, the whole scene's K samples together, up to R times; the ranking then runs on the accepted
set.  The route is staged, the draw number advances by ``max(n_steps + 1, R + 1)`` per call, and ``self.rejection`` holds the last
call's (num_iter, samples with collisions, samples fixed).  A slot that no round could fix keeps its round-0 sample.
``static_obstacles=`` [L, 2, 2] or [L, 4] with ``wall_radius=`` (opt-in, with ``collision_free_rounds`` > 0; the wall segments the MPC
receives as ``static_obs``, in the forecasts' world frame): a joint sample in which a pedestrian's path - the step from his present
position included - comes closer than ``wall_radius`` to a wall is redrawn too (``jmid_denoise_reject_walls_seeded``), and
``self.rejection`` gains the two cause counts (samples that fail the pedestrian predicate, the wall predicate).  The forecaster knows
no agent radius: ``wall_radius`` has no default.
``constraint_type="opt_softplus"`` (opt-in, under EVERY ``rng_compat``; the name is the reference's, ``DiffusionTraj.sample``'s second
mechanism and what every shipped config sets): collision repair (``JmidEngine.repair_collisions``; the rule stands in include/jmid_hip.h) -
a joint sample in which two pedestrians come closer than ``collision_threshold`` is pushed apart on the device under a softplus penalty
until the predicate holds, or comes back as it was when ``max_iter`` steps do not get it there: no redraw, no second denoise loop, no
download.  The route is staged (denoise -> repair -> ranking on the repaired set), ``self.repair`` holds the last call's (samples with
collisions, repaired, reverted, largest iteration count), and ``repair_options`` = {margin, tau, step, max_iter} overrides the defaults.
Together with ``collision_free_rounds=R`` the redraw loop runs first and the repair takes whatever is still flagged.  Not with
``static_obstacles=``: walls are not in the objective.
``constraint_type="opt_softplus_walls"`` (opt-in; needs ``static_obstacles=`` and ``wall_radius=``, with or without a redraw loop): the same
stage with the walls in the objective and in both gates (``jmid_repair_collisions_walls``) - a sample whose paths, the step from the present
position included, come closer than ``wall_radius`` to a wall is a candidate too, a single pedestrian included, and a repaired sample is
kept only when both predicates accept it.  ``self.repair_causes`` holds the last call's candidates split by cause
(``metrics.repair_causes``).
``guidance={scale, n_inner, margin, tau, weights, walls, table}`` (opt-in, under EVERY ``rng_compat``; ``{}``: the defaults): guided
sampling - softplus collision steps at ``collision_threshold`` BETWEEN the denoise steps (``JmidEngine.denoise(guidance=)``,
``jmid_denoise_guided``; include/jmid_hip.h states the rule), so the net's remaining steps run on the corrected state; the route is staged
and ``self.guide`` [K, 2] holds the last call's rows (``metrics.GUIDE_COLUMNS``).  With ``constraint_type`` the repair follows on the guided
set; ``walls=True`` takes ``static_obstacles=`` / ``wall_radius=`` into the objective.  Not with ``collision_free_rounds`` (a rerun would
have to be guided too), ``device_scene`` or ``device_frames`` (the one-entry chains) - unless ``constraint_route="chain"``.
``constraint_route="chain"`` (opt-in; ``"staged"`` is the default, with the refusals above): ``guidance=`` and ``constraint_type=`` ride INSIDE
the one-entry chains (``JmidEngine.predict(constraints=)`` ... ``forecast_scene(constraints=)``; the ``jmid_*_constrained`` entries) - one
call per ``predict_ret_best()``, with ``device_scene``, ``device_frames``, ``track_presence`` and ``coast_frames`` too, the bits of the staged
route, and ``self.guide`` / ``self.repair`` / ``self.repair_causes`` filled from the chain's reports.  The first-call self check and a
JMID_ERANGE repeat still take the staged route.  Not with ``collision_free_rounds`` (the redraw loop has no chain).

Differences from the reference that a caller can observe:
  * the engine (weights on the GPU) is cached across instances: the reference rebuilds the model and reloads the
    checkpoint at the start of every episode (``sicnav_acados.py:1171``); the cache key holds the checkpoint file's
    identity (path, size, mtime) or the weight checksum (computed once per ``JMIDWeights`` object), the engine is
    one per (weights, net, device, history length, step size) and calls on it are serialised by a lock;
  * ``model_path`` may point to the neutral ``.npz`` written by ``export_checkpoint`` instead of the pickled
    ``nn.ModuleDict`` container (which needs the reference tree on ``sys.path`` to unpickle);
  * a too-short history raises ``HistoryTooShortError`` (a ``TypeError``, like the reference's failure mode) - unless the instance was
    made with ``short_history=True`` (opt-in): then a call with 2 .. past_num_frames - 1 shared frames predicts, every track encoded from
    its first frame on as the reference's MODEL does it (``first_history_index``, MID/dataset/preprocessing.py:468);
  * ``track_presence=True`` (opt-in, with ``short_history=True``): ``update_state_hists`` may be fed NaN positions for a pedestrian who is not
    seen.  The reference's table drops such a frame for everybody (``mid_sim_wrapper.py:266``); here every track keeps a window of its own
    (``scene.frame_table_tracks``), and a pedestrian who is NaN in the newest frame is left out of the call - his rows come back NaN;
  * ``coast_frames=c`` > 0 (opt-in, with ``track_presence=True``): such a pedestrian is instead COASTED to the newest frame when he was seen
    at most c grid bins ago (``scene.frame_table_tracks(max_coast=c)``: his last step repeated, or his position when he was seen once)
    and forecast like everybody else from there; seen longer ago, he is left out as above.
"""
from __future__ import annotations

import configparser
import os
import time
import warnings
from functools import partial
from threading import Lock, RLock
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch
import yaml

from . import scene as SC
from ._lib import EINVAL, ERANGE
from .engine import ChainConstraints, Guidance, JmidEngine, JmidError, wall_segments
from .kde import most_likely_samples
from .metrics import GUIDE_DEFAULTS, rejection_totals, repair_causes
from .schedule import guidance_weights
from .weights import JMIDWeights, NetDims

_ENGINE_CACHE: Dict[tuple, JmidEngine] = {}
_ENGINE_LOCKS: Dict[int, RLock] = {}
_WEIGHTS_CACHE: Dict[tuple, JMIDWeights] = {}     # (path, size, mtime_ns, dims) -> weights (re-created every episode)
_CACHE_LOCK = Lock()            # guards the three caches above (forecasters may be built from several threads)
ERANGE_FALLBACKS = 0            # calls of this process that were repeated in "f32" after JMID_ERANGE
SELF_CHECK_DOWNGRADES = 0       # instances whose opt-in precision was replaced by "f16x3" by the first-call self check
# what HumanTrajectoryForecasterSim's keyword arguments default to (safe_interactive_crowdnav_amd.install(**defaults) edits it)
DEFAULTS = {"device_id": 0, "precision": "f16mx", "rng_compat": "auto", "self_check": True, "device_topk": True,
            "device_scene": False, "device_frames": False}


_PHILOX_STEP: Dict[Tuple[int, Tuple[int, ...]], int] = {}     # (device, shape) -> what one randn_like of that shape adds to the Philox offset


def wall_arguments(static_obstacles, wall_radius, rounds: int, repair_walls: bool = False) -> dict:
    """The ``static_obstacles`` / ``wall_radius`` keywords of the forecaster, ``predict_batch`` and ``offline.sample`` as the keywords of
    ``JmidEngine.denoise_reject``: {} without walls (the call, its route and its bits are then what they were), else
    {"walls": [L, 4] float64, "wall_radius": float}.  Walls need collision-free sampling (``rounds`` > 0) and a radius - the sampler
    knows no agent radius, so there is no default.  ``repair_walls``: ``constraint_type="opt_softplus_walls"`` reads the walls too
    (``repair_arguments`` holds its copy), so without a redraw loop there is nothing to hand to one: {}."""
    if static_obstacles is None:
        if wall_radius is not None:
            raise ValueError("wall_radius is given without static_obstacles")
        return {}
    if rounds <= 0 and repair_walls:
        return {}
    if rounds <= 0:
        raise ValueError("static_obstacles needs collision-free sampling (collision_free_rounds > 0 / with_constraints=True)")
    if wall_radius is None:
        raise ValueError("static_obstacles needs wall_radius (the sampler knows no agent radius)")
    walls, radius = wall_segments(static_obstacles), float(wall_radius)
    if not np.isfinite(walls).all():
        raise ValueError("static_obstacles holds a non-finite coordinate")
    if walls.shape[0] > 64:
        raise ValueError("static_obstacles holds more than 64 segments")
    if not (np.isfinite(radius) and radius >= 0.0):
        raise ValueError("wall_radius must be finite and >= 0")
    return {"walls": walls, "wall_radius": radius}


REPAIR_OPTIONS = ("margin", "tau", "step", "max_iter")


CONSTRAINT_TYPES = ("opt_softplus", "opt_softplus_walls")


def repair_arguments(constraint_type, repair_options=None, static_obstacles=None, wall_radius=None) -> Optional[dict]:
    """The ``constraint_type`` / ``repair_options`` keywords of the forecaster, ``predict_batch`` and ``offline.sample`` as the keywords of
    ``JmidEngine.repair_collisions``: None without a constraint type (nothing changes), else the options that were given ({}: the
    defaults).  ``"opt_softplus"`` is the reference configs' name; walls are not in its objective, so ``static_obstacles`` is refused with
    it.  ``"opt_softplus_walls"`` (``jmid_repair_collisions_walls``) has them in the objective and in both gates: it NEEDS
    ``static_obstacles`` and ``wall_radius`` (no default: the sampler knows no agent radius), which come back as the keys ``walls`` /
    ``wall_radius``."""
    if constraint_type is None:
        if repair_options:
            raise ValueError("repair_options is given without constraint_type")
        return None
    if constraint_type not in CONSTRAINT_TYPES:
        raise ValueError(f"unknown constraint_type {constraint_type!r} (known: {list(CONSTRAINT_TYPES)})")
    if constraint_type == "opt_softplus" and static_obstacles is not None:
        raise ValueError("static_obstacles cannot be combined with constraint_type='opt_softplus': walls are not in the repair's objective "
                         "(a repaired sample could be pushed into one); constraint_type='opt_softplus_walls' has them")
    opts = dict(repair_options or {})
    unknown = sorted(set(opts) - set(REPAIR_OPTIONS))
    if unknown:
        raise ValueError(f"unknown repair_options {unknown} (known: {list(REPAIR_OPTIONS)})")
    for key in ("margin", "tau", "step"):
        if key in opts and not (np.isfinite(opts[key]) and (opts[key] >= 0.0 if key == "margin" else opts[key] > 0.0)):
            raise ValueError(f"repair_options[{key!r}] must be finite and {'>= 0' if key == 'margin' else '> 0'}")
    if "max_iter" in opts and not 0 <= int(opts["max_iter"]) <= 1024:
        raise ValueError("repair_options['max_iter'] must lie in 0..1024")
    if constraint_type == "opt_softplus_walls":
        if static_obstacles is None:
            raise ValueError("constraint_type='opt_softplus_walls' needs static_obstacles (and wall_radius)")
        opts.update(wall_arguments(static_obstacles, wall_radius, 1))
    return opts


GUIDANCE_OPTIONS = ("scale", "n_inner", "margin", "tau", "weights", "walls", "table")


def guidance_arguments(guidance, threshold: float, static_obstacles=None, wall_radius=None, step: Optional[int] = None,
                       sampling: str = "ddim") -> Optional[Guidance]:
    """The ``guidance=`` keyword of the forecaster, ``predict_batch`` and ``offline.sample`` - a dict {scale, n_inner, margin, tau, weights,
    walls: bool, table} - as the ``engine.Guidance`` of ``JmidEngine.denoise``: None without the keyword (nothing changes).  ``step``: the
    sampler's step count (one weight per entry of its DDIM table).  ``weights`` is the table itself; otherwise ``scale`` (0.02 m, the
    repair's step) and ``table`` ("alpha_bar") make it (``schedule.guidance_weights``).  ``walls=True`` takes ``static_obstacles`` /
    ``wall_radius`` into the objective and is refused without them.  The threshold is the call's ``collision_threshold``."""
    if guidance is None:
        return None
    if sampling != "ddim":
        raise ValueError("guidance needs the DDIM sampler (a DDPM step draws noise behind the correction)")
    opts = dict(guidance)
    unknown = sorted(set(opts) - set(GUIDANCE_OPTIONS))
    if unknown:
        raise ValueError(f"unknown guidance options {unknown} (known: {list(GUIDANCE_OPTIONS)})")
    if step is None:
        raise ValueError("guidance needs the sampler's step count")
    margin, tau = float(opts.get("margin", GUIDE_DEFAULTS["margin"])), float(opts.get("tau", GUIDE_DEFAULTS["tau"]))
    n_inner = int(opts.get("n_inner", GUIDE_DEFAULTS["n_inner"]))
    if not (np.isfinite(margin) and margin >= 0.0):
        raise ValueError("guidance['margin'] must be finite and >= 0")
    if not (np.isfinite(tau) and tau > 0.0):
        raise ValueError("guidance['tau'] must be finite and > 0")
    if not 1 <= n_inner <= 64:
        raise ValueError("guidance['n_inner'] must lie in 1..64")
    if opts.get("weights") is not None:
        if "scale" in opts or "table" in opts:
            raise ValueError("guidance takes either weights or scale / table")
        weights = np.asarray(opts["weights"], dtype=np.float64).reshape(-1)
        if weights.size != len(range(100, 0, -int(100 / step))):
            raise ValueError(f"guidance['weights'] must hold one weight per step-table entry ({len(range(100, 0, -int(100 / step)))})")
        if not (np.isfinite(weights).all() and (weights >= 0.0).all()):
            raise ValueError("guidance['weights'] must be finite and >= 0")
    else:
        weights = guidance_weights(float(opts.get("scale", GUIDE_DEFAULTS["scale"])), step, table=opts.get("table", "alpha_bar"))
    walls = {}
    if opts.get("walls"):
        if static_obstacles is None or wall_radius is None:
            raise ValueError("guidance with walls=True needs static_obstacles and wall_radius")
        walls = wall_arguments(static_obstacles, wall_radius, 1)
    return Guidance(float(threshold), margin, tau, weights, n_inner, walls.get("walls"), walls.get("wall_radius"))


def repair_totals(episode) -> Tuple[int, int, int, int]:
    """``episode`` [..., 3] of ``JmidEngine.repair_collisions`` -> (samples with collisions, repaired, reverted, largest iteration count)."""
    ep = np.asarray(episode.detach().cpu() if hasattr(episode, "detach") else episode).reshape(-1, 3).astype(np.int64)
    if not ep.shape[0]:
        return 0, 0, 0, 0
    return int(ep[:, 0].sum()), int(ep[:, 1].sum()), int(ep[:, 0].sum() - ep[:, 1].sum()), int(ep[:, 2].max())


CONSTRAINT_ROUTES = ("staged", "chain")


def constraint_route_arguments(constraint_route: str, rounds) -> bool:
    """The ``constraint_route=`` keyword of the forecaster and ``predict_batch`` -> whether guidance and repair ride inside the one-entry
    chains.  ``"chain"`` is refused with a redraw loop (``collision_free_rounds``: the loop has no chain)."""
    if constraint_route not in CONSTRAINT_ROUTES:
        raise ValueError(f"constraint_route must be one of {list(CONSTRAINT_ROUTES)}")
    if constraint_route == "chain" and rounds:
        raise ValueError("constraint_route='chain' cannot be combined with collision_free_rounds (the redraw loop has no one-entry chain)")
    return constraint_route == "chain"


def chain_constraints(limits: "Constraints") -> Optional[ChainConstraints]:
    """The guidance and the repair of ``limits`` as the ``constraints=`` of the engine's chained methods; None with neither."""
    if limits.guidance is None and limits.repair is None:
        return None
    return ChainConstraints(limits.threshold, limits.guidance, limits.repair)


def chain_report_causes(report, limits: "Constraints") -> Optional[dict]:
    """``metrics.repair_causes`` of a constrained chain's report, as ``repair_stage`` gives it: None unless the repair takes walls."""
    if report.wall is None:
        return None
    return repair_causes(report.sample, report.wall, limits.threshold, limits.repair["wall_radius"])


class Constraints(NamedTuple):
    """The sampling constraints of one call as data: everything the constraint keywords of the forecaster, ``predict_batch`` and
    ``offline.sample`` decide, decided once (``sampling_constraints``).  The callers read the fields and never the keywords."""
    rounds: Optional[int] = None      # the redraw loop (JmidEngine.denoise_reject) and its max_rounds; None: no loop
    threshold: float = 0.2            # the pedestrian predicate's distance, of the loop and of the repair
    walls: dict = {}                  # the loop's {walls, wall_radius} keywords, or {}
    repair: Optional[dict] = None     # the repair stage (JmidEngine.repair_collisions) and its keywords, the walls of "opt_softplus_walls" among them; None: no stage
    padded: bool = False              # predict_batch: ONE loop for the whole padded batch instead of one per count group
    guidance: Optional[Guidance] = None      # guided sampling (JmidEngine.denoise(guidance=)): the collision steps between the denoise steps; None: none


def sampling_constraints(rounds: Optional[int] = None, threshold: float = 0.2, static_obstacles=None, wall_radius=None,
                         constraint_type: Optional[str] = None, repair_options: Optional[dict] = None, padded: bool = False,
                         guidance: Optional[dict] = None, step: Optional[int] = None, sampling: str = "ddim") -> Constraints:
    """``Constraints`` from the public keywords, with every refusal that is about them: ``rounds`` is ``collision_free_rounds`` where it is
    > 0 (``offline.sample``: ``max_rounds`` under ``with_constraints=True``) and None otherwise, ``threshold`` is ``collision_threshold``,
    ``padded`` is ``collision_free_padded``.  What a caller refuses itself is what only it knows: its RNG contract, ``padded=``, the
    sampler's ``bestof`` / ``sampling``.  ``guidance`` (with the sampler's ``step`` and ``sampling``): ``guidance_arguments``; not with a
    redraw loop - a rerun would have to be guided too - and composed with the repair: guide, then repair what is left."""
    if rounds is not None and not 0 <= int(rounds) <= 64:
        raise ValueError("collision_free_rounds must lie in 0..64")
    threshold = float(threshold)
    if not (np.isfinite(threshold) and threshold >= 0.0):
        raise ValueError("collision_threshold must be finite and >= 0")
    repair = repair_arguments(constraint_type, repair_options, static_obstacles, wall_radius)
    guide = guidance_arguments(guidance, threshold, static_obstacles, wall_radius, step, sampling)
    if guide is not None and rounds is not None:
        raise ValueError("guidance cannot be combined with collision_free_rounds (a rerun would have to be guided too: not built)")
    walls = wall_arguments(static_obstacles, wall_radius, int(rounds is not None),
                           (repair is not None and "walls" in repair) or (guide is not None and guide.walls is not None))
    if padded and rounds is None:
        raise ValueError("collision_free_padded needs collision_free_rounds > 0")
    return Constraints(None if rounds is None else int(rounds), threshold, walls, repair, bool(padded), guide)


def repair_stage(engine: JmidEngine, pos, dims: Tuple[int, int, int, int], threshold: float, options: dict, n_agents=None, p0=None,
                 dt: Optional[float] = None):
    """The repair stage of a staged route behind a denoise (or rejection) call of ``dims`` = (E, A, K, H): ``pos`` [E, K, A, H, 2], or None
    when the samples stayed on the device - they are then repaired where they lie and the ranking reads them there.
    -> (pos repaired, or None; episode [E, 3]; ``metrics.repair_causes`` of the call, or None without walls).  With walls among the
    ``options`` (``"opt_softplus_walls"``) the call's ``p0`` [E, A, 2] and ``dt`` go along - the step from the present position is part of
    the wall predicate, as in the redraw loop."""
    where = dict(dims=dims if pos is None else None, n_agents=n_agents)
    if "walls" not in options:
        out = engine.repair_collisions(pos, threshold=threshold, **where, **options)
        return out[0], out[3], None
    on_device = pos is not None and torch.is_tensor(pos) and pos.is_cuda
    # p0 goes where pos lives (pos None: the resident set, host arrays out)
    if on_device:
        p0 = (p0 if torch.is_tensor(p0) else torch.from_numpy(np.ascontiguousarray(p0, dtype=np.float32))).to(pos.device, torch.float32).contiguous()
    else:
        p0 = np.ascontiguousarray(p0.detach().cpu().numpy() if torch.is_tensor(p0) else p0, dtype=np.float32)
    out = engine.repair_collisions(pos, threshold=threshold, **where, p0=p0, dt=float(dt), **options)      # (a fifth value: wall)
    return out[0], out[3], repair_causes(out[2], out[4], threshold, options["wall_radius"])


def advance_cuda_generator(device_id: int, shape: Tuple[int, ...], n: int) -> None:
    """Leave device ``device_id``'s default generator where ``n`` successive ``torch.randn_like(z)`` (z fp32 of ``shape`` on that
    device) leave it - the reference's unused per-step draws (``MID/models/diffusion.py:509``) - without launching them: a CUDA
    generator is (seed, Philox offset), and a draw of a given shape adds a fixed amount to the offset.  The first call for a
    (device, shape) makes ONE real draw to learn that amount; 49 launches per cfg2 call (0.2 ms of host time) otherwise."""
    if n <= 0:
        return
    gen = torch.cuda.default_generators[device_id] if len(torch.cuda.default_generators) > device_id else None
    if gen is None:                               # (CUDA not initialised yet: the first tensor on the device does it)
        torch.empty(1, device=f"cuda:{device_id}")
        gen = torch.cuda.default_generators[device_id]
    key = (int(device_id), tuple(int(v) for v in shape))
    if not (hasattr(gen, "get_offset") and hasattr(gen, "set_offset")):
        # an older torch (the reference pins 1.13.1) has no Philox-offset accessors: make the draws for real, as the reference does
        for _ in range(n):
            torch.randn(key[1], device=f"cuda:{device_id}")
        return
    step = _PHILOX_STEP.get(key)
    if step is None:
        before = gen.get_offset()
        torch.randn(key[1], device=f"cuda:{device_id}")
        step = gen.get_offset() - before
        _PHILOX_STEP[key] = step
        n -= 1
    if n > 0:
        gen.set_offset(gen.get_offset() + n * step)


def load_weights(model_path: str, dims: NetDims) -> JMIDWeights:
    """Weights from ``model_path``: the neutral ``.npz`` (preferred; also looked up next to a ``.pt`` path), or the
    reference's two-part checkpoint ``{"encoder": nn.ModuleDict, "ddpm": state_dict}`` (``MID/mid.py:1231-1232,
    1291, 1501-1509``) when it can be unpickled in this interpreter."""
    cand = [model_path] if model_path.endswith(".npz") else [os.path.splitext(model_path)[0] + ".npz", model_path]
    for p in cand:
        if not os.path.exists(p):
            continue
        st = os.stat(p)
        key = (os.path.abspath(p), st.st_size, st.st_mtime_ns, dims)
        with _CACHE_LOCK:
            if key in _WEIGHTS_CACHE:
                return _WEIGHTS_CACHE[key]
        if p.endswith(".npz"):
            w = JMIDWeights.load(p)
            if w.dims != dims:
                raise ValueError(f"{p} holds dims {w.dims}, config asks for {dims}")
        else:
            ckpt = torch.load(p, map_location="cpu", weights_only=False)
            w = JMIDWeights.from_reference_state(dims, ckpt["ddpm"], ckpt["encoder"])
        with _CACHE_LOCK:
            w = _WEIGHTS_CACHE.setdefault(key, w)
        return w
    raise FileNotFoundError(f"no checkpoint at {model_path} (or its .npz export)")


class ForecasterSimSuper:
    """History bookkeeping, identical to ``mid_sim_wrapper.py:172-204``."""

    def init_super(self, env_config):
        self.prev_states_lock = Lock()
        if env_config is None:     # mid_sim_wrapper.py:175-178: a file relative to the CWD (NoSectionError below when it is absent)
            env_config = configparser.RawConfigParser()
            env_config.read("./src/human_traj_forecaster/configs/env_utias_vicon.config")
        self.publish_freq = env_config.getfloat("human_trajectory_forecaster", "publish_freq")
        self.time_step = env_config.getfloat("env", "time_step")
        assert (self.time_step * 100).is_integer(), \
            "please only specify human time step to a hundredth of a second"
        self.num_hist_frames = env_config.getint("human_trajectory_forecaster", "past_num_frames")
        self.predict_horizon = env_config.getint("human_trajectory_forecaster", "prediction_horizon")
        self.num_ret_samples = env_config.getint("human_trajectory_forecaster", "num_samples")
        self.num_hums = env_config.getint("sim", "human_num")
        self.prev_states = [[] for _ in range(self.num_hums)]
        self.prev_robot_states = []

    def update_state_hists(self, robot_state, human_states, time_stamp):
        for i in range(self.num_hums):
            self.prev_states[i].append([*human_states[i].position, time_stamp])
            if len(self.prev_states[i]) > self.num_hist_frames:
                self.prev_states[i].pop(0)
        self.prev_robot_states.append([*robot_state.position, time_stamp])


class _ModelInfo:
    """What the reference exposes as ``.model`` / ``.mid_model`` (an ``MID`` object): kept as a plain record."""

    def __init__(self, config, engine, num_samples):
        self.config = config
        self.engine = engine
        self.num_samples = num_samples


class HumanTrajectoryForecasterSim(ForecasterSimSuper):
    def __init__(self, env_config=None, mid_config_file=None, *, weights: Optional[JMIDWeights] = None,
                 device_id: Optional[int] = None, precision: Optional[str] = None, rng_compat: Optional[str] = None,
                 self_check: Optional[bool] = None, self_check_tol: float = 5e-5, device_topk: Optional[bool] = None,
                 lib_path: Optional[str] = None, device_scene: Optional[bool] = None, device_frames: Optional[bool] = None,
                 seed: int = 0, episode_id: int = 0, short_history: bool = False, track_presence: bool = False, coast_frames: int = 0,
                 collision_free_rounds: int = 0, collision_threshold: float = 0.2, static_obstacles=None,
                 wall_radius: Optional[float] = None, constraint_type: Optional[str] = None, repair_options: Optional[dict] = None,
                 guidance: Optional[dict] = None, constraint_route: str = "staged"):
        # (lib_path: another build of the library - tests run both flavours in one process; the product leaves it at None)
        # keyword arguments left at None take the process-wide defaults (``DEFAULTS``; ``install(**defaults)`` sets them for
        # a caller that constructs the class with the reference's two positional arguments only, sicnav_acados.py:998-1000)
        device_id = DEFAULTS["device_id"] if device_id is None else device_id
        precision = DEFAULTS["precision"] if precision is None else precision
        rng_compat = DEFAULTS["rng_compat"] if rng_compat is None else rng_compat
        self_check = DEFAULTS["self_check"] if self_check is None else self_check
        device_topk = DEFAULTS["device_topk"] if device_topk is None else device_topk
        device_scene = DEFAULTS["device_scene"] if device_scene is None else device_scene
        device_frames = DEFAULTS["device_frames"] if device_frames is None else device_frames
        self.init_super(env_config)
        self.precision = precision
        self.self_check = bool(self_check) and precision in ("f16mx", "f16x2")
        self.self_check_tol = float(self_check_tol)
        self._checked_shapes = set()
        self.device_topk = bool(device_topk)
        # True: the scene batch (cluster choice, states, scene graph, neighbour sums) is built on the device (jmid_build_scene) and the
        # predictor runs on it where it lies (jmid_predict_scene); the history table stays on the host either way
        self.device_scene = bool(device_scene)
        # True: the raw stamped frames go to the device as they are (jmid_build_scene_stamped: frame table + scene batch) and the two
        # returned arrays come back assembled (jmid_forecast_scene); the staged path (self check, JMID_ERANGE repeat, k < K beyond the
        # top-k limits) reads its inputs back and assembles on the host.  Histories that are not frames (the per-human lists do not share
        # one stamp sequence with the robot's last entries) take the host frame table as before
        self.device_frames = bool(device_frames)
        # True (opt-in; False is the reference wrapper's refusal): a call with 2 <= L < past_num_frames shared grid frames predicts - the
        # window is padded in front (scene.pad_short_window) and every row is encoded from its first frame (the reference model's
        # first_history_index) - instead of raising HistoryTooShortError.  One frame still raises; from past_num_frames frames on
        # nothing changes
        self.short_history = bool(short_history)
        # True (opt-in, needs short_history): a history window PER TRACK.  update_state_hists may be fed NaN positions for a pedestrian who
        # is not seen; such a frame is not dropped (scene.frame_table_tracks), a track that appears mid-run is encoded from its own first
        # frame and a hole inside a track is interpolated.  A pedestrian who is NaN in the anchor frame (the newest frame with a stamp
        # and a robot position) is absent now: left out of the call, his rows NaN in both returned arrays; everybody absent raises
        # HistoryTooShortError.  With device_frames the raw frames go to the device as they are (jmid_build_scene_stamped_var): ONE build
        # and ONE chain, short windows included
        self.track_presence = bool(track_presence)
        if self.track_presence and not self.short_history:
            raise ValueError("track_presence needs short_history=True (a track that appears mid-run has a short window)")
        # > 0 (opt-in, needs track_presence): a pedestrian who is NaN in the anchor frame but was seen at most coast_frames grid bins ago is
        # coasted to it (scene.frame_table_tracks(max_coast=)) - a node like any other: a network forecast in the cluster with two grid
        # rows, his constant-velocity row otherwise, his coasted pose prepended.  Seen longer ago: left out of the SCENE, not of the
        # arrays (first_frame -1, jmid_build_scene_absent) - with device_frames all num_hums tracks go to the device as they are
        # (jmid_build_scene_stamped_coast), nothing is filtered on the host.  0: the host filter above, today's routes and bits
        self.coast_frames = int(coast_frames)
        if self.coast_frames and not self.track_presence:
            raise ValueError("coast_frames needs track_presence=True")
        if not 0 <= self.coast_frames <= self.num_hist_frames - 2:
            raise ValueError("coast_frames must lie in 0..past_num_frames-2")
        self.erange_fallbacks = 0
        self.timings: Dict[str, float] = {}     # ms of the last predict_ret_best(): scene, device, topk, assemble
        if rng_compat not in ("auto", "cpu", "cuda", "device"):
            raise ValueError("rng_compat must be 'auto', 'cpu', 'cuda' or 'device'")
        # rng_compat="device": the address of this instance's noise (seed, episode id) and the draw number its next call starts at
        # (_draw0: the draw number the last call's redraw loop started at)
        self.noise_seed, self.episode_id, self._noise_draw, self._draw0 = int(seed), int(episode_id), 0, 0
        self.rng_compat = rng_compat if rng_compat != "auto" else ("cuda" if torch.cuda.is_available() else "cpu")
        # > 0 (opt-in, needs rng_compat="device": a redraw is a draw number of the counter generator): collision-free sampling, up to that
        # many reruns of a scene whose joint samples collide at collision_threshold metres; rejection: the last call's totals
        self.collision_free_rounds, self.collision_threshold = int(collision_free_rounds), float(collision_threshold)
        # guidance={scale, n_inner, margin, tau, weights, walls, table} (opt-in, every RNG contract): softplus collision steps between the
        # denoise steps (JmidEngine.denoise(guidance=)) - the staged route, not with collision_free_rounds or the one-entry chains;
        # composes with constraint_type: guide, then repair what is left.  guide: the last call's rows [K, 2] (metrics.GUIDE_COLUMNS)
        # constraint_route="chain" (opt-in): guidance and repair inside the one-entry chains (the jmid_*_constrained entries) wherever the
        # unconstrained call would take a chain - device_scene and device_frames included; "staged": today's route and refusals
        self.constraint_route = constraint_route
        self._chain_constraints = constraint_route_arguments(constraint_route, collision_free_rounds)
        step = None
        if guidance is not None:
            if (device_scene or device_frames) and not self._chain_constraints:
                raise ValueError("guidance has no one-entry chain: not with device_scene or device_frames")
            with open(mid_config_file) as f:
                step = int(yaml.safe_load(f)["step_size"])
        self.constraints = sampling_constraints(self.collision_free_rounds or None, collision_threshold, static_obstacles, wall_radius,
                                                constraint_type, repair_options, guidance=guidance, step=step)
        self.guide: Optional[np.ndarray] = None
        self._walls, self._repair_options = self.constraints.walls, self.constraints.repair      # (read by tests/)
        if self.constraints.rounds is not None and self.rng_compat != "device":
            raise ValueError("collision_free_rounds needs rng_compat='device' (a redraw is a draw number of the library's counter generator)")
        # static_obstacles + wall_radius (opt-in, with collision_free_rounds > 0): the wall predicate joins the pedestrian one, and
        # rejection holds five counts (the three, then the samples that fail the pedestrian predicate, the wall predicate)
        # constraint_type="opt_softplus" (opt-in, every RNG contract): collision repair behind the denoise stage (and behind the redraw
        # loop, when both are asked for); repair: the last call's (samples with collisions, repaired, reverted, largest iteration count)
        # constraint_type="opt_softplus_walls": the same stage with the walls in the objective and in both gates (needs static_obstacles +
        # wall_radius, with or without a redraw loop); repair_causes: the last call's candidates split by cause (metrics.repair_causes)
        self.constraint_type = constraint_type
        self.repair: Optional[Tuple[int, int, int, int]] = None
        self.repair_causes: Optional[Dict[str, int]] = None
        self.rejection: Optional[Tuple[int, ...]] = None
        self._init_MID(mid_config_file, weights, device_id, lib_path)

    def _init_MID(self, mid_config_file, weights, device_id, lib_path=None):
        with open(mid_config_file) as f:
            cfg = yaml.safe_load(f)
        self.config = cfg
        dims = NetDims(ctx_dim=int(cfg["encoder_dim"]), tf_layer=int(cfg["tf_layer"]))
        self.joint = cfg["diffnet"] == "JointPredictionTransformerConcatLinear"
        if not self.joint and cfg["diffnet"] != "TransformerConcatLinear":
            raise ValueError(f"unsupported diffnet {cfg['diffnet']!r}")
        self.num_samples = int(cfg["num_samples"])
        self.step_size = int(cfg["step_size"])
        # the sampler runs with the YAML horizon / history length (MID/mid.py:1260-1261), the wrapper allocates its
        # output with the env-config ones (mid_sim_wrapper.py:494): they have to agree
        if int(cfg["prediction_horizon"]) != self.predict_horizon:
            raise ValueError("prediction_horizon differs between the MID yaml and [human_trajectory_forecaster]")
        if int(cfg["maximum_history_length"]) != self.num_hist_frames - 1:
            raise ValueError("maximum_history_length must equal past_num_frames - 1")
        if weights is None:
            weights = load_weights(cfg["model_path"], dims)
        key = (weights.checksum(), self.joint, device_id, self.num_hist_frames, self.step_size, lib_path)
        with _CACHE_LOCK:
            eng = _ENGINE_CACHE.get(key)
            if eng is None:
                eng = JmidEngine(weights, joint=self.joint, device_id=device_id, hist_len=self.num_hist_frames,
                                 step=self.step_size, lib_path=lib_path)
                _ENGINE_CACHE[key] = eng
                _ENGINE_LOCKS[id(eng)] = RLock()
            self.engine = eng
            self._engine_lock = _ENGINE_LOCKS[id(eng)]
        self.mid_model = _ModelInfo(cfg, eng, self.num_samples)
        self.model = self.mid_model

    # ------------------------------------------------------------------------------------------ prediction
    def _snapshot(self):
        with self.prev_states_lock:           # mid_sim_wrapper.py:251-258
            return [list(map(list, h)) for h in self.prev_states], list(map(list, self.prev_robot_states))

    def _first_call_check(self, key, nan_downgrades: bool, stage, pos, rejection):
        """First call per shape (``key``) in an opt-in mode: the call's denoise stage (``denoise_stage``) once more in "f16x3" on the same
        inputs - a redraw loop from the same draw0 - and the downgrade when the two disagree.  -> the (pos, rejection) to use: those of
        the run that produced the positions.  ``nan_downgrades``: whether a NaN delta downgrades as well (behind a redraw loop it does,
        behind a plain denoise call it does not: docs/NOTEBOOK.md)."""
        global SELF_CHECK_DOWNGRADES
        self._checked_shapes.add(key)
        (ref, ref_rejection), _ = repeat_in_fp32(lambda p: stage(p, True), "f16x3")
        with np.errstate(invalid="ignore"):
            delta = float(np.linalg.norm(pos - ref, axis=-1).mean())
        self.self_check_delta = delta
        if delta > self.self_check_tol or (nan_downgrades and np.isnan(delta)):
            warnings.warn(f"precision={self.precision!r} differs from 'f16x3' by {delta:.2e} m mean displacement on this "
                          f"checkpoint (> {self.self_check_tol:.1e}): this forecaster now runs 'f16x3'", RuntimeWarning,
                          stacklevel=4)
            self.precision, self.self_check = "f16x3", False
            SELF_CHECK_DOWNGRADES += 1
            return ref, ref_rejection
        return pos, rejection

    def _self_check(self, x_T, ctx, p0, pos):
        """``_first_call_check`` of a plain denoise call on given inputs and positions -> the positions to use."""
        key = tuple(x_T.shape)
        if key in self._checked_shapes:
            return pos
        return self._first_call_check(key, False, denoise_stage(self.engine, ctx, p0, Constraints(), self.time_step, x_T), pos, None)[0]

    def get_most_likely_samples(self, forecasts):
        """mid_sim_wrapper.py:440-441: the ``num_ret_samples`` most likely of the sampled joint futures under the per-step
        Gaussian KDE (``get_most_likely_samples``, ``:14-169``, joint branch).  forecasts [K, A, H, 2] (tensor or array) ->
        (kept [A, k, H, 2], log-weights [A, k]) as float32 torch tensors, ascending likelihood like the reference's
        ``argsort(...)[-k:]``.  On the device (``jmid_topk``) while the shape fits it, on the host twin otherwise."""
        f = forecasts.detach().cpu().numpy() if isinstance(forecasts, torch.Tensor) else np.asarray(forecasts)
        f = np.ascontiguousarray(f, dtype=np.float32)
        K, A, H, _ = f.shape
        k = self.num_ret_samples
        if self.device_topk and k <= K and topk_fits_device(A, K, H):
            with self._engine_lock:
                sel, lw = self.engine.topk(f[None], k)
            sel, lw = sel[0], lw[0]
        else:
            sel, lw = most_likely_samples(f, k)
        return torch.from_numpy(np.ascontiguousarray(sel)), torch.from_numpy(np.ascontiguousarray(lw))

    def predict_ret_best(self) -> Tuple[np.ndarray, np.ndarray]:
        """mid_sim_wrapper.py:482-510 -> (forecasts [N, k, H+1, 2] float64, log-weights [N, k] float64)."""
        if not (self.device_scene or self.device_frames):
            return self._predict_ret_best()
        with self._engine_lock:     # the engine holds ONE resident scene: nobody else builds between this call's build and its predict
            return self._predict_ret_best()

    def _scene(self, prev, rob):
        """Scene stage: the histories -> (``Route.scene``, ids_in: the in-cluster track ids, ascending; cv: the constant-velocity rows as
        ``scene.assemble_forecasts`` takes them; pose_now [N, 2] or None while it lies on the device; the host ``SceneBatch`` or None
        when the scene is resident; the padded short window's first_frame [N + 1] or None).  Raises HistoryTooShortError before
        anything is drawn."""
        F, H, ff = self.num_hist_frames, self.predict_horizon, None
        if self.track_presence:
            # (lists edited by hand are no frames: they take the table below, where a NaN position drops its frame)
            frames = SC.histories_as_frames(prev, rob, joined=False)
            if frames is not None:
                return self._scene_tracks(*frames)
        if self.short_history:
            hum_xy, rob_xy, pose_now = SC.frame_table(prev, rob, self.time_step, F)
            if 2 <= hum_xy.shape[0] < F:
                hum_xy, rob_xy, ff = SC.pad_short_window(hum_xy, rob_xy, F)
        frames = SC.histories_as_frames(prev, rob) if self.device_frames and ff is None else None     # (a short window is never stamped)
        source = scene_source(self.device_scene, self.device_frames, short=ff is not None, frames=frames is not None)
        if source == "stamped":
            # the frame table on the device too (JMID_EHISTORY -> HistoryTooShortError, where build_scene raises it on the host path);
            # the pose is read back only by the staged path (forecast_scene prepends it on the device)
            ds = self.engine.build_scene_stamped(*frames, self.time_step, H)
            return source, np.nonzero(ds["in_cluster"])[0], ds["cv"], None, None, None, None
        if not self.short_history:                          # (short_history has the table already)
            hum_xy, rob_xy, pose_now = SC.frame_table(prev, rob, self.time_step, F)
        if source == "resident":
            if hum_xy.shape[0] < F:
                raise SC.HistoryTooShortError(f"{hum_xy.shape[0]} history frames available, {F} needed")
            ds = self.engine.build_scene(hum_xy, rob_xy, self.time_step, H, first_frame=ff)
            return source, np.nonzero(ds["in_cluster"])[0], ds["cv"], pose_now, None, ff, None
        sb = SC.build_scene(hum_xy, rob_xy, self.time_step, H, F, first_frame=ff)
        return source, sb.ids_in, sb.cv_forecasts, pose_now, sb, ff, None

    def _scene_tracks(self, stamps, hum, rob):
        """``_scene`` with ``track_presence`` for histories that are frames: its returns for the pedestrians who are present now, and
        ``present`` [N] bool - the pedestrians seen in the anchor frame (the others are left out; nobody left: HistoryTooShortError)."""
        F, H = self.num_hist_frames, self.predict_horizon
        if self.coast_frames:
            return self._scene_coasted(stamps, hum, rob)
        kept = np.nonzero(~(np.isnan(stamps) | np.isnan(rob).any(axis=1)))[0]
        if not len(kept):
            raise SC.HistoryTooShortError("no history frame with a stamp and a robot position")
        anchor = kept[np.argsort(stamps[kept], kind="stable")[-1]]
        present = ~np.isnan(hum[anchor]).any(axis=1)
        if not present.any():
            raise SC.HistoryTooShortError("no pedestrian is seen in the newest history frame")
        hum = np.ascontiguousarray(hum[:, present])
        source = scene_source(self.device_scene, self.device_frames, short=True, tracks=True)
        if source == "stamped":      # raw frames in, short windows included: one build (first_index resident), one chain
            ds = self.engine.build_scene_stamped(stamps, hum, rob, self.time_step, H, tracks=True)
            return source, np.nonzero(ds["in_cluster"])[0], ds["cv"], None, None, ds["first_frame"], present
        hum_xy, rob_xy, pose_now, ff, _ = SC.frame_table_tracks(stamps, hum, rob, self.time_step, F)
        if not ff.any():             # everybody on every frame: the bits of a build without first_frame, and its routes
            ff = None
        if source == "resident":
            ds = self.engine.build_scene(hum_xy, rob_xy, self.time_step, H, first_frame=ff)
            return source, np.nonzero(ds["in_cluster"])[0], ds["cv"], pose_now, None, ff, present
        sb = SC.build_scene(hum_xy, rob_xy, self.time_step, H, F, first_frame=ff)
        return source, sb.ids_in, sb.cv_forecasts, pose_now, sb, ff, present

    def _scene_coasted(self, stamps, hum, rob):
        """``_scene_tracks`` with ``coast_frames``: every track stays in the arrays (``present`` all True); who is neither seen now nor
        coasted has first_frame -1 - not in the scene, his rows NaN.  Nobody left: HistoryTooShortError on both routes."""
        F, H, c = self.num_hist_frames, self.predict_horizon, self.coast_frames
        present = np.ones(hum.shape[1], dtype=bool)
        source = scene_source(self.device_scene, self.device_frames, short=True, tracks=True)
        if source == "stamped":      # all N tracks as raw frames: one build (coasting and leaving out on the device), one chain
            try:
                ds = self.engine.build_scene_stamped(stamps, hum, rob, self.time_step, H, tracks=True, max_coast=c)
            except JmidError as e:
                if e.code == EINVAL and "no pedestrian left" in str(e):
                    raise SC.HistoryTooShortError("no pedestrian is seen in, or coasted to, the newest history frame") from e
                raise
            return source, np.nonzero(ds["in_cluster"])[0], ds["cv"], None, None, ds["first_frame"], present
        hum_xy, rob_xy, pose_now, ff, _, _ = SC.frame_table_tracks(stamps, hum, rob, self.time_step, F, max_coast=c)
        if (ff[1:] < 0).all():
            raise SC.HistoryTooShortError("no pedestrian is seen in, or coasted to, the newest history frame")
        if not ff.any():             # everybody on every frame: the bits of a build without first_frame, and its routes
            ff = None
        if source == "resident":
            ds = self.engine.build_scene(hum_xy, rob_xy, self.time_step, H, first_frame=ff, allow_absent=ff is not None)
            return source, np.nonzero(ds["in_cluster"])[0], ds["cv"], pose_now, None, ff, present
        sb = SC.build_scene(hum_xy, rob_xy, self.time_step, H, F, first_frame=ff, allow_absent=ff is not None)
        return source, sb.ids_in, sb.cv_forecasts, pose_now, sb, ff, present

    def _draw_x_T(self, A: int) -> np.ndarray:
        """Noise stage -> x_T [1, K * A, H, 2].  RNG contract (module docstring): x_T is the first draw of the CPU default generator; the
        per-step z of the reference (unused by DDIM) comes from the generator of the device the reference would run on."""
        K, H, stride = self.num_samples, self.predict_horizon, int(100 / self.step_size)
        if self.rng_compat == "device" and self.collision_free_rounds:
            # collision-free sampling draws inside the entry: round j is draw number draw0 + j.  The block of this call is reserved here
            # (the self check and the JMID_ERANGE repeat start from the same draw0); nothing is drawn
            self._draw0 = self._noise_draw
            self._noise_draw += max(len(range(100, 0, -stride)) + 1, self.collision_free_rounds + 1)
            return None
        if self.rng_compat == "device":
            # the library's counter generator: this call's block of n_steps + 1 draw numbers (x_T is its first; a DDPM sampler would take
            # the others), drawn ONCE - the self check and the JMID_ERANGE repeat reuse the array
            with self._engine_lock:
                x_np = self.engine.noise(self.noise_seed, [self.episode_id], K * A, H, draw=self._noise_draw)
            self._noise_draw += len(range(100, 0, -stride)) + 1
            return x_np
        x_T = torch.randn([K * A, H, 2])
        n_z = sum(1 for t in range(100, 0, -stride) if t > 1)
        if self.rng_compat == "cpu":
            for _ in range(n_z):
                torch.randn_like(x_T)
        else:
            advance_cuda_generator(self.engine.device_id, tuple(x_T.shape), n_z)
        return x_T.numpy()[None]

    def _encoder_inputs(self, ids_in, sb, ff):
        """The staged path's (x_st, nbr_sum, edge_mask, p0, first_index): the host batch, or the in-cluster rows of the resident scene read
        back (the self-check call and the JMID_ERANGE repeat take their inputs from there)."""
        if sb is not None:
            return sb.x_st, sb.nbr_sum, sb.edge_mask, sb.p0, None if ff is None else sb.first_index
        sa = self.engine.scene_arrays()
        x_st, nbr_sum, edge_mask, p0 = (np.ascontiguousarray(sa[key][ids_in]) for key in ("x_st", "nbr_sum", "edge_mask", "p0"))
        return x_st, nbr_sum, edge_mask, p0, None if ff is None else np.ascontiguousarray(sa["first_index"][ids_in])

    def _predict_ret_best(self) -> Tuple[np.ndarray, np.ndarray]:
        """Snapshot -> scene -> noise -> route -> run (ONE chained library entry, or encode / denoise / rank) -> assembly -> timings."""
        t0 = time.perf_counter()
        source, ids_in, cv, pose_now, sb, ff, present = self._scene(*self._snapshot())
        A, K, H, k, limits = len(ids_in), self.num_samples, self.predict_horizon, self.num_ret_samples, self.constraints
        x_np = self._draw_x_T(A)             # after the scene: a call that raises HistoryTooShortError has drawn nothing
        t1 = time.perf_counter()
        check = self.self_check and (1, K * A, H, 2) not in self._checked_shapes
        route = plan_route(k=k, K=K, A=A, H=H, device_topk=self.device_topk, device_scene=self.device_scene,
                           device_frames=self.device_frames, check=check, short=ff is not None, frames=source == "stamped",
                           tracks=present is not None, collision_free=limits.rounds is not None, repair=limits.repair is not None,
                           guidance=limits.guidance is not None, chain_constraints=self._chain_constraints)
        result, call, report = None, dict(dt=self.time_step, precision=self.precision), None
        cons = chain_constraints(limits) if route.run == "chain" else None
        if cons is not None:      # (the chained methods then return a third value, the report)
            call["constraints"] = cons
        with self._engine_lock:               # the engine is shared between forecaster instances and not re-entrant
            if self.engine.step != self.step_size or self.engine.sampling != "ddim":
                self.engine.set_step(self.step_size, "ddim")   # eval_sicnav hard-codes sampling="ddim" (MID/mid.py:333)
            if route.run == "chain":
                try:
                    if source == "stamped":      # from raw frames, the assembled result itself: nothing left to do on the host
                        result, report = _split_report(self.engine.forecast_scene(x_np, k, **call))
                    elif sb is None:
                        (rows, logw), report = _split_report(self.engine.predict_scene(x_np, k, **call))
                    else:
                        (rows, logw), report = _split_report(self.engine.predict(sb.x_st, sb.nbr_sum, sb.edge_mask, x_np, sb.p0[None], k, **call))
                    if report is not None:      # what the staged run fills from its stages' outputs, from the chain's one download
                        if report.guide is not None:
                            self.guide = np.asarray(report.guide)[0]
                        if report.episode is not None:
                            self.repair, self.repair_causes = repair_totals(report.episode), chain_report_causes(report, limits)
                except JmidError as e:
                    if not _repeats_in_fp32(e, self.precision):
                        raise
                    route = route._replace(run="staged")      # whose denoise call repeats in exact fp32, warns once and counts
            t2 = time.perf_counter()
            if route.run == "staged":
                x_st, nbr_sum, edge_mask, p0, first_index = self._encoder_inputs(ids_in, sb, ff)
                if pose_now is None:
                    pose_now = self.engine.scene_frames()["pose_now"]
                ctx = self.engine.encode(x_st, nbr_sum, edge_mask, first_index=first_index)
                # (x_np None: a redraw loop draws inside the entry, from the draw number _draw_x_T reserved)
                seeded = dict(seed=self.noise_seed, episode_ids=[self.episode_id], K=K, T=H) if x_np is None else None
                out = run_staged(self.engine, ctx[None], p0[None], (1, A, K, H), limits, route.rank, k, self.time_step, self.precision,
                                 x_T=x_np, seeded=seeded, draw0=self._draw0,
                                 self_check=partial(self._first_call_check, (1, K * A, H, 2), limits.rounds is not None) if check else None)
                if out.fell_back:
                    if not self.erange_fallbacks:
                        warnings.warn("JMID_ERANGE: an activation left the fp16 range; the call was repeated in the exact-fp32 mode "
                                      "(same result, ~5x the latency).  Construct the forecaster with precision='f32' if this "
                                      "checkpoint does it often.", RuntimeWarning, stacklevel=2)
                    self.erange_fallbacks += 1
                if out.rejection is not None:
                    self.rejection = rejection_totals(out.rejection.episodes, out.rejection.cause)
                if out.repair is not None:
                    self.repair, self.repair_causes = repair_totals(out.repair), out.repair_causes
                if out.guide is not None:
                    self.guide = np.asarray(out.guide)[0]
                rows, logw, t2 = out.rows, out.logw, out.rank_started
        t3 = time.perf_counter()
        if result is None:
            in_cluster = np.zeros(self.num_hums if present is None else int(present.sum()), dtype=bool)
            in_cluster[ids_in] = True
            result = SC.assemble_forecasts(in_cluster, rows[0], None if logw is None else logw[0], cv, pose_now, k, K)
        if present is not None and not present.all():     # the rows of the pedestrians who are absent now: NaN
            full = np.full((self.num_hums,) + result[0].shape[1:], np.nan), np.full((self.num_hums,) + result[1].shape[1:], np.nan)
            full[0][present], full[1][present] = result
            result = full
        if present is not None and ff is not None and (ff[1:] < 0).any():      # coast_frames: the rows of the pedestrians left out of the scene
            result[0][ff[1:] < 0], result[1][ff[1:] < 0] = np.nan, np.nan
        t4 = time.perf_counter()
        self.timings = {"scene_ms": 1e3 * (t1 - t0), "device_ms": 1e3 * (t2 - t1), "topk_ms": 1e3 * (t3 - t2),
                        "assemble_ms": 1e3 * (t4 - t3), "total_ms": 1e3 * (t4 - t0)}
        return result


def get_most_likely_samples(forecasts, mid_model, num_ret_samples):
    """Module-level twin of ``mid_sim_wrapper.get_most_likely_samples`` (``:14-169``; joint branch - the predictor's model has
    no ``cfg``, ``:20-21``): forecasts [K, A, H, 2] -> (kept [A, k, H, 2], log-weights [A, k]) float32 tensors.  Host arithmetic
    (``kde.most_likely_samples``); the class method of the same name uses the device kernel."""
    f = forecasts.detach().cpu().numpy() if isinstance(forecasts, torch.Tensor) else np.asarray(forecasts)
    sel, lw = most_likely_samples(np.ascontiguousarray(f, dtype=np.float32), int(num_ret_samples))
    return torch.from_numpy(np.ascontiguousarray(sel)), torch.from_numpy(np.ascontiguousarray(lw))


# size limits of the device-side joint-KDE top-k (jmid_topk, include/jmid_hip.h): beyond them the host twin (kde.py) ranks
TOPK_MAX_AGENTS, TOPK_MAX_SAMPLES, TOPK_MAX_HORIZON = 32, 1024, 24


def topk_fits_device(A: int, K: int, H: int) -> bool:
    return A <= TOPK_MAX_AGENTS and K <= TOPK_MAX_SAMPLES and H <= TOPK_MAX_HORIZON


class Route(NamedTuple):
    """The path of one ``predict_ret_best()`` - or of one count group, or the padded form, of ``predict_batch`` - as data."""
    scene: str     # the scene batch: "host" (scene.py), "resident" (engine.build_scene) or "stamped" (engine.build_scene_stamped, raw frames)
    run: str       # "chain": ONE library entry (predict / predict_scene / forecast_scene / predict_padded / forecast_scene_padded); "staged": encode -> denoise -> rank
    rank: str      # the k of K samples: "device_resident" (jmid_topk on the positions the call left in the workspace; inside a chain), "device"
    #                (jmid_topk on given positions), "host" (kde.py, beyond the device's size limits) or "none" (k == K: uniform weights)


def scene_source(device_scene: bool, device_frames: bool, short: bool = False, frames: bool = True, batch: bool = False,
                 resident: bool = False, tracks: bool = False) -> str:
    """``Route.scene``.  ``predict_batch`` takes grid inputs: nothing to stamp.  A single call's histories that are not frames take the
    host frame table, and a short window has no stamped form (its padded table is built with ``first_frame``) - unless the windows are
    per track (``tracks``: ``track_presence`` on histories that are frames), whose stamped form builds short windows too.  ``resident``
    (``predict_batch(padded="resident")``): the whole batch is built on the device."""
    if batch:
        return "resident" if device_scene or device_frames or resident else "host"
    if tracks and device_frames and frames:
        return "stamped"
    if device_frames and frames and not short:
        return "stamped"
    return "resident" if device_scene or (device_frames and short) else "host"


def plan_route(*, k: int, K: int, A: int, H: int, device_topk: bool = True, device_scene: bool = False, device_frames: bool = False,
               check: bool = False, short: bool = False, frames: bool = True, batch: bool = False, padded: bool = False,
               resident: bool = False, tracks: bool = False, collision_free: bool = False, repair: bool = False,
               guidance: bool = False, chain_constraints: bool = False) -> Route:
    """Every decision of a call that does not need an array: the flags, k of K samples, A in-cluster pedestrians, horizon H, whether the
    first-call self check is due (``check``), whether the window is short (``short``) and whether the histories are frames (``frames``).
    ``batch``: a count group of ``predict_batch``, ``padded``: its one-call form with A the largest count, ``resident``: that form on the
    batch's resident scene (``padded="resident"``: forecast_scene_padded).  ``tracks``: per-track windows (``track_presence``).
    ``collision_free``: collision-free sampling (``collision_free_rounds`` > 0) - the rejection loop has no one-entry chain, so the run is
    staged (encode -> ``denoise_reject`` -> rank) and the ranking reads the accepted set where the loop left it.
    ``repair``: collision repair (``constraint_type="opt_softplus"``) - a stage between the denoise call and the ranking, so the run is
    staged too (encode -> denoise -> ``repair_collisions`` -> rank).  ``guidance``: guided sampling - the guided denoise call has no
    one-entry chain either, so the run is staged; with none of the three nothing changes.
    ``chain_constraints`` (``constraint_route="chain"``): ``repair`` and ``guidance`` ride inside the chain (the constrained entries) and no
    longer force the staged run; ``collision_free`` and the first-call self check still do.  False: every answer is what it was."""
    scene = scene_source(device_scene, device_frames, short, frames, batch, resident, tracks)
    # the K samples stay on the GPU (only the k kept ones come back) while jmid_topk takes the shape; beyond its limits - the reference
    # has none - the host twin ranks them
    on_dev = k < K and device_topk and topk_fits_device(A, K, H)
    if batch:       # the chains predict_batch has: predict_padded on host arrays, forecast_scene on a group's resident scenes,
        #             forecast_scene_padded on the batch's
        chain = padded or device_frames or resident
    else:           # a short window built on the host is staged: jmid_predict has no first_index (a resident one is predict_scene's)
        chain = not (short and scene == "host")
    chain = chain and (on_dev or k == K) and not check        # (the self check compares the staged denoise call's positions)
    chain = chain and not collision_free and (chain_constraints or not (repair or guidance))
    rank = "none" if k >= K else "host" if not on_dev else "device" if check else "device_resident"
    return Route(scene, "chain" if chain else "staged", rank)


def _split_report(out):
    """What a chained engine method returned -> (its two values, the ``ChainReport`` of a constrained call or None)."""
    return (out[:2], out[2]) if len(out) == 3 else (out, None)


def _repeats_in_fp32(err: JmidError, precision: str) -> bool:
    return err.code == ERANGE and precision != "f32"


def repeat_in_fp32(call, precision: str):
    """``call(precision)``; on JMID_ERANGE (an fp16 operand left the fp16 range) the same call in the exact-fp32 mode - what the
    reference computes in throughout (diffusion.py:478-541) - and counted.  -> (result, fell_back)."""
    global ERANGE_FALLBACKS
    try:
        return call(precision), False
    except JmidError as e:
        if not _repeats_in_fp32(e, precision):
            raise
    ERANGE_FALLBACKS += 1
    return call("f32"), True


def rank_samples(engine: JmidEngine, rank: str, pos, k: int, dims: Tuple[int, int, int, int], n_agents=None):
    """The ranking stage (``Route.rank``) after a denoise call of ``dims`` = (E, A, K, H), ``pos`` [E, K, A, H, 2] or None (left on the device)
    -> what ``scene.assemble_forecasts`` takes: (kept [E, A, k, H, 2], log-weights [E, A, k]), or (pos, None) when all K are returned.
    ``n_agents`` [E]: a padded batch - every episode is ranked over its real agents, the rows of the padded ones are NaN."""
    if rank == "none":
        return pos, None
    if rank == "host":
        E, A, _, H = dims
        sel, lw = np.full((E, A, k, H, 2), np.nan, dtype=np.float32), np.full((E, A, k), np.nan, dtype=np.float32)
        for e, n in enumerate([A] * E if n_agents is None else n_agents):
            sel[e, :n], lw[e, :n] = most_likely_samples(np.ascontiguousarray(pos[e][:, :n]), k)
        return sel, lw
    padded = {} if n_agents is None else {"n_agents": n_agents}      # (the call without counts is the one it always was)
    return engine.topk(pos if rank == "device" else None, k, dims=dims, **padded)


class Rejection(NamedTuple):
    """What a redraw loop (``JmidEngine.denoise_reject``) reports next to its samples."""
    slots: np.ndarray                  # [E, K, 3] int32
    episodes: np.ndarray               # [E, 3] int32
    cause: Optional[np.ndarray]        # [E, 2] int32 of a loop with walls or with counts, else None


class Staged(NamedTuple):
    """What ``run_staged`` returns."""
    rows: np.ndarray                   # what ``scene.assemble_forecasts`` takes (``rank_samples``)
    logw: Optional[np.ndarray]
    rejection: Optional[Rejection]     # of the loop whose samples were used; None: no loop
    repair: Optional[np.ndarray]       # the repair's episode rows [E, 3] (``repair_totals``); None: no repair stage
    repair_causes: Optional[dict]      # ``metrics.repair_causes`` of a repair with walls
    fell_back: bool                    # JMID_ERANGE: the denoise stage was repeated in exact fp32
    rank_started: float                # ``time.perf_counter()`` between the repair and the ranking (the forecaster's timings split there)
    guide: Optional[np.ndarray] = None      # the guided denoise call's rows [E, K, 2] (``metrics.GUIDE_COLUMNS``); None: no guidance


def denoise_stage(engine: JmidEngine, ctx, p0, constraints: Constraints, dt: float, x_T=None, seeded: Optional[dict] = None, draw0: int = 0,
                  n_agents=None):
    """The denoise stage of a staged run as a callable (precision, want_pos) -> (pos [E, K, A, H, 2] or None when the samples stay on the
    device, ``Rejection`` or None): the redraw loop from ``draw0`` when the constraints ask for one, else one denoise call.  Either
    ``x_T`` or ``seeded``, the seed / episode_ids / K / T keywords of a seeded call (a repeat then draws the same noise).  With guidance
    among the constraints the call is the guided one, and ``stage.guide`` holds the rows [E, K, 2] of its last run."""
    seeded = seeded or {}

    def stage(precision: str, want_pos: bool):
        if constraints.guidance is not None:
            _, pos, stage.guide = engine.denoise(x_T, ctx, p0, dt=dt, precision=precision, want_vel=False, want_pos=want_pos,
                                                 guidance=constraints.guidance, want_guide=True, **seeded)
            return pos, None
        if constraints.rounds is None:
            return engine.denoise(x_T, ctx, p0, dt=dt, precision=precision, want_vel=False, want_pos=want_pos, **seeded)[1], None
        out = engine.denoise_reject(ctx, p0, dt=dt, precision=precision, threshold=constraints.threshold, max_rounds=constraints.rounds,
                                    draw0=draw0, want_vel=False, want_pos=want_pos, n_agents=n_agents, **constraints.walls, **seeded)
        return out[1], Rejection(out[2], out[3], out[4] if len(out) > 4 else None)      # (the engine gives four values, or five)
    stage.guide = None
    return stage


def run_staged(engine: JmidEngine, ctx, p0, dims: Tuple[int, int, int, int], constraints: Constraints, rank: str, k: int, dt: float,
               precision: str, x_T=None, seeded: Optional[dict] = None, draw0: int = 0, n_agents=None, self_check=None) -> Staged:
    """The staged run behind ``encode``, for every caller: ctx [E, A, ctx_dim], p0 [E, A, 2], ``dims`` = (E, A, K, H) -> the denoise stage
    (``denoise_stage``) under ``repeat_in_fp32``, the repair stage when the constraints hold one, the ranking (``Route.rank``; k of K).
    The samples come back from the device only when the ranking needs them there.  ``n_agents`` [E]: a padded batch.
    ``self_check`` (stage, pos, rejection) -> (pos, rejection): the forecaster's first-call check, given the stage to run again."""
    stage = denoise_stage(engine, ctx, p0, constraints, dt, x_T, seeded, draw0, n_agents)
    (pos, rejection), fell_back = repeat_in_fp32(lambda p: stage(p, rank != "device_resident"), precision)
    if self_check is not None:
        pos, rejection = self_check(stage, pos, rejection)
    episode = causes = None
    if constraints.repair is not None:      # on the set the stage above left: in place on the device, or on the host copy
        pos, episode, causes = repair_stage(engine, pos, dims, constraints.threshold, constraints.repair, n_agents=n_agents, p0=p0, dt=dt)
    rank_started = time.perf_counter()
    rows, logw = rank_samples(engine, rank, pos, k, dims, n_agents)
    return Staged(rows, logw, rejection, episode, causes, fell_back, rank_started, stage.guide)


def _engine_lock_of(engine: JmidEngine) -> RLock:
    with _CACHE_LOCK:
        return _ENGINE_LOCKS.setdefault(id(engine), RLock())


def predict_batch(engine: JmidEngine, human_xy: np.ndarray, robot_xy: np.ndarray, seeds, *, num_samples: int,
                  num_ret_samples: int, horizon: int, time_step: float, precision: Optional[str] = None,
                  device_topk: bool = True, device_scene: bool = False,
                  device_frames: bool = False, noise: str = "torch", seed: int = 0,
                  padded=False, short_history: bool = False, first_frame=None, collision_free_rounds: int = 0,
                  collision_threshold: float = 0.2, stats: Optional[dict] = None, static_obstacles=None,
                  wall_radius: Optional[float] = None, collision_free_padded: bool = False, constraint_type: Optional[str] = None,
                  repair_options: Optional[dict] = None, guidance: Optional[dict] = None,
                  constraint_route: str = "staged") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``predict_ret_best()`` for E independent episodes in as few device calls as their cluster sizes allow: the feed
    of the multi-episode evaluation sweeps.

    human_xy [E, F, N, 2], robot_xy [E, F, 2] on the ``time_step`` grid (oldest first); ``seeds[e]`` seeds the torch
    generator episode e draws its x_T from (== ``torch.manual_seed(seeds[e])`` before the per-episode call).
    The host batch comes from ``scene.build_scenes_batched`` (``device_scene=True``: from ``engine.build_scene`` +
    ``engine.scene_arrays()``, the device twin) with the reference's own clustering (the pedestrians
    within 3 m of the cluster nearest the robot go through the network, mid_sim_wrapper.py:335-355; the others get
    constant-velocity forecasts, :413-429); episodes with the same number A of in-cluster pedestrians share one
    ``encode`` + ``denoise`` call (the C ABI takes one A per call).  Returns (forecasts [E, N, k, H+1, 2] float64,
    log-weights [E, N, k] float64, in_cluster [E, N] bool), each episode as ``predict_ret_best`` would return it.
    ``device_frames=True``: the inputs are on the grid already, so only the assembly moves - every count group is built on the device
    and comes back as its assembled arrays (``engine.forecast_scene``: one call per group instead of encode + denoise + top-k + the
    host scatter); a group whose ranking does not fit the device top-k takes the staged path.
    ``noise="device"`` (opt-in; ``"torch"`` is the reference's contract above): x_T is drawn on the device by the library's counter
    generator (``noise.py``) with ``seed`` as its key and ``seeds[e]`` as episode e's GLOBAL id, so an episode's forecasts are the same
    bits whichever batch, count group or shard it is part of (in JMID_PREC_F32 at any width and in every mode below head_dim 128; at
    head_dim 128 the split modes agree to rounding across batch sizes, include/jmid_hip.h at jmid_set_chunk_episodes) - statistically,
    not seed-, compatible with the reference.
    ``padded=True`` (opt-in): instead of one call per count, EVERY episode goes through one ``engine.predict_padded`` call with
    A = the largest count; episodes with fewer in-cluster pedestrians carry padding rows, which the attention kernels mask as keys
    (the reference's attn_mask, diffusion.py:186-195) - the forecasts equal the grouped path's up to rounding, the torch draws are the
    same (episode e draws [K * n_e, H, 2] from ``seeds[e]``, scattered to the padded rows).  One loop at the batch's launch rate against
    one per count at a group's; the padded share of the rows is wasted work.  Host arrays and torch noise only:
    not with ``device_scene``, ``device_frames`` or ``noise="device"``; a batch whose ranking does not fit the device top-k, or
    with an empty cluster, takes the grouped path.
    ``short_history=True`` (opt-in): human_xy / robot_xy may hold 2 <= L < hist_len frames (every episode the same L: the episode start);
    the windows are padded in front (``scene.pad_short_window``) and every row is encoded from its first frame.  Not with ``padded=True``.
    ``padded="resident"`` (opt-in): the one-call form on the device scene - ONE ``engine.build_scene`` for all E episodes, then ONE
    ``engine.forecast_scene_padded`` with A = the largest count (the counts are the resident scene's).  With ``noise="device"`` the call is
    seeded and episode e draws what it draws alone and in its count group; otherwise the torch draws of ``padded=True``.  It combines with
    ``short_history``.  A batch with an empty cluster, or whose ranking does not fit the device top-k, takes the grouped device path
    (``device_frames=True``).
    ``first_frame`` [E, N + 1] integers, robot first (opt-in; human_xy / robot_xy hold hist_len frames and are never read in front of a
    node's first frame): every node of every episode with a window of its own, as ``engine.build_scene(first_frame=)`` takes it - it
    supersedes the common-L padding of ``short_history``.  A pedestrian's entry may be -1: he is NOT IN THE SCENE of that episode
    (``jmid_build_scene_absent``; not seen now) - the episodes of a batch keep one N, his rows come back NaN in both arrays with
    ``in_cluster`` False, everybody else as if his column were removed.  On the host route, the grouped device route and
    ``padded="resident"``; not with ``padded=True``.
    ``collision_free_rounds=R`` > 0 (opt-in, with ``noise="device"``): collision-free sampling per count group
    (``engine.denoise_reject`` from draw 0: a joint sample in which two pedestrians come closer than ``collision_threshold`` is redrawn,
    its episode's K samples together, up to R times) - every group is staged and ranked on its accepted set, and an episode's rows stay
    the same bits whichever batch it is part of.  ``stats`` (a dict) is filled with ``episodes`` [E, 3] int32 = (samples colliding at
    round 0, fixed, last round rerun) and ``slots`` [E, K, 3] int32, rows in input order (an episode with an empty cluster: zeros).
    Not with ``padded=``.
    ``static_obstacles=`` [L, 2, 2] or [L, 4] with ``wall_radius=`` (opt-in, with ``collision_free_rounds`` > 0): a joint sample in which
    a pedestrian's path, the step from his present position included, comes closer than ``wall_radius`` to a wall is redrawn too
    (``jmid_denoise_reject_walls_seeded``); ``stats`` also gets ``cause`` [E, 2] int32 = (samples that fail the pedestrian predicate,
    the wall predicate, at round 0).  ``wall_radius`` has no default: the sampler knows no agent radius.
    ``collision_free_padded=True`` (opt-in, with ``collision_free_rounds`` > 0 and ``noise="device"``; not with ``padded=``): ONE
    rejection loop for the whole batch instead of one per count group (``jmid_denoise_reject_padded_seeded``) - the staged route on
    padded inputs with A = the largest count: the scene as above, ONE ``engine.encode`` over E * A rows, ONE
    ``engine.denoise_reject(n_agents=)`` from draw 0, the ranking by ``engine.topk(n_agents=)`` on the accepted set (the host twin beyond
    its limits).  Episode e draws what it draws in its count group; its forecasts equal the grouped path's up to the rounding of a
    padded call's attention (bit for bit when every count is the same).  ``stats`` gets ``episodes``, ``slots`` and ``cause`` in input
    order.  A batch with an empty cluster takes the count groups.
    ``constraint_type="opt_softplus"`` (opt-in, with either ``noise``; ``repair_options`` = {margin, tau, step, max_iter}): collision repair
    (``engine.repair_collisions``) behind every group's denoise call - or behind its rejection loop, ``collision_free_padded`` included,
    when ``collision_free_rounds`` is given too - and the ranking on the repaired set; every group is staged.  ``stats`` gets ``repair``
    [E, 3] int32 = (samples with collisions, repaired, largest iteration count), rows in input order (an empty cluster: zeros).  Not with
    ``static_obstacles=`` (walls are not in the objective); with ``padded=`` the batch takes the count groups.
    ``constraint_type="opt_softplus_walls"`` (needs ``static_obstacles=`` and ``wall_radius=``): the repair with the walls in its objective and
    in both gates, every call with its group's ``p0``; ``stats`` also gets ``repair_causes``, the sums of ``metrics.repair_causes``.
    ``guidance=`` {scale, n_inner, margin, tau, weights, walls, table} (opt-in, with either ``noise``; ``guidance_arguments``): guided
    sampling - every group's denoise call runs softplus collision steps at ``collision_threshold`` between its denoise steps
    (``engine.denoise(guidance=)``), every group is staged, and ``stats`` gets ``guide`` [E, K, 2] = ``metrics.GUIDE_COLUMNS``, rows in
    input order.  It composes with ``constraint_type``: guide, then repair what is left.  Not with ``collision_free_rounds`` (a rerun
    would have to be guided too), a DDPM table, ``padded=``, ``device_scene`` or ``device_frames`` (the one-entry chains).
    ``constraint_route="chain"`` (opt-in; ``"staged"`` is everything above): ``guidance=`` and ``constraint_type=`` ride inside the one-entry
    chains (``engine.forecast_scene(constraints=)``, ``predict_padded(constraints=)``, ``forecast_scene_padded(constraints=)``), so they
    combine with ``device_frames``, ``padded=True`` and ``padded="resident"`` in one call per group or batch; ``stats`` gets the same keys,
    filled from the chains' reports.  A group or batch that has no chain (its ranking does not fit the device top-k, an empty cluster) is
    staged as before.  Not with ``collision_free_rounds``.
    """
    if noise not in ("torch", "device"):
        raise ValueError("noise must be 'torch' or 'device'")
    if padded not in (False, True, "resident"):
        raise ValueError("padded must be False, True or 'resident'")
    sampler = {} if guidance is None else dict(step=engine.step, sampling=engine.sampling)      # (one weight per entry of the engine's table)
    limits = sampling_constraints(int(collision_free_rounds) or None, collision_threshold, static_obstacles, wall_radius, constraint_type,
                                  repair_options, collision_free_padded, guidance=guidance, **sampler)
    chained = constraint_route_arguments(constraint_route, collision_free_rounds)
    cons = chain_constraints(limits) if chained else None
    kw = {} if cons is None else {"constraints": cons}      # (a chained method then returns a third value, the report)
    if limits.guidance is not None and (padded or device_scene or device_frames) and not chained:
        raise ValueError("guidance has no one-entry chain: not with padded=, device_scene or device_frames")
    if limits.rounds is not None:
        if padded:
            raise ValueError("collision_free_rounds has no padded form (jmid_denoise_reject_seeded takes one agent count per call)")
        if noise != "device":
            raise ValueError("collision_free_rounds needs noise='device' (a redraw is a draw number of the library's counter generator)")
    resident = isinstance(padded, str)
    if resident:
        padded, device_frames = False, True       # (what it falls back to: the grouped device path)
    if padded and (device_scene or device_frames or noise == "device"):
        raise ValueError("padded=True takes host scene arrays and torch noise only: not with device_scene, device_frames or noise='device' "
                         "(the padded entries have no scene-resident or seeded form)")
    ff = None                                    # short_history: first_frame [E, N + 1] of the padded windows
    absent = first_frame is not None             # (the builds that take a -1; without one they leave the bits of the others)
    ab = {"allow_absent": True} if absent else {}
    if absent:
        if padded:
            raise ValueError("first_frame has no padded form (jmid_predict_padded takes no first_index)")
        if human_xy.shape[1] != engine.hist_len:
            raise ValueError("first_frame needs hist_len frames in human_xy / robot_xy")
        ff = SC._check_first_frame(first_frame, human_xy.shape[0], human_xy.shape[2], engine.hist_len, False, allow_absent=True)
    elif short_history and 2 <= human_xy.shape[1] < engine.hist_len:
        if padded:
            raise ValueError("short_history has no padded form (jmid_predict_padded takes no first_index)")
        parts = [SC.pad_short_window(human_xy[e], robot_xy[e], engine.hist_len) for e in range(human_xy.shape[0])]
        human_xy, robot_xy, ff = (np.stack([p[i] for p in parts]) for i in range(3))
    E, F, N, _ = human_xy.shape
    K, k, H = int(num_samples), int(num_ret_samples), int(horizon)
    precision = DEFAULTS["precision"] if precision is None else precision      # (no self check here: an engine-level call)
    lock = _engine_lock_of(engine)               # an engine may be shared with forecaster instances; it is not re-entrant

    def plan(A, padded=False, resident=False):
        return plan_route(k=k, K=K, A=A, H=H, device_topk=device_topk, device_scene=device_scene, device_frames=device_frames,
                          short=ff is not None, batch=True, padded=padded, resident=resident, collision_free=limits.rounds is not None,
                          repair=limits.repair is not None, guidance=limits.guidance is not None, chain_constraints=chained)

    def batch_stats(report):
        """``stats`` of a one-call form from its chain's report: the keys and rows the count groups fill."""
        if report is None or stats is None:
            return
        if report.guide is not None:
            stats["guide"] = report.guide
        if report.episode is not None:
            stats["repair"] = report.episode
        if report.wall is not None:
            stats["repair_causes"] = chain_report_causes(report, limits)

    def torch_x_T(e, A):
        return torch.randn([K * A, H, 2], generator=torch.Generator().manual_seed(int(seeds[e])))

    if scene_source(device_scene, device_frames, batch=True, resident=resident) == "resident":
        with lock:                               # the same batch from the device kernel (jmid_build_scene)
            b = engine.build_scene(human_xy, robot_xy, time_step, horizon=H, first_frame=ff, **ab)
            n_in = b["in_cluster"].sum(axis=1)
            if resident and n_in.min() >= 1 and plan(int(n_in.max()), resident=True).run == "chain":
                # the scene stays where it is: predictor + assembly for every count in one entry
                if noise == "device":
                    x_T, nz = None, dict(seed=int(seed), episode_ids=np.asarray(seeds), K=K, T=H)
                else:
                    x_T, nz = SC.pad_samples([torch_x_T(e, int(n_in[e])).numpy() for e in range(E)], n_in, int(n_in.max()), K), {}
                ((forecasts, logw), report), _ = repeat_in_fp32(
                    lambda p: _split_report(engine.forecast_scene_padded(x_T, k, dt=time_step, precision=p, **nz, **kw)), precision)
                batch_stats(report)
                return forecasts, logw, b["in_cluster"]
            if not device_frames:
                b.update(engine.scene_arrays())
    else:
        b = SC.build_scenes_batched(human_xy, robot_xy, time_step, horizon=H, first_frame=ff, **ab)
    inc, pose_now = b["in_cluster"], human_xy[:, -1]
    left_out = ff[:, 1:] < 0 if absent else None      # [E, N] not in the scene: NaN rows
    if absent:
        pose_now = np.where(left_out[..., None], np.nan, pose_now)
    n_in = inc.sum(axis=1)

    if padded and n_in.min() >= 1 and plan(int(n_in.max()), padded=True).run == "chain":
        A = int(n_in.max())
        x_T = SC.pad_samples([torch_x_T(e, int(n_in[e])).numpy() for e in range(E)], n_in, A, K)
        args = (SC.pad_agents(b["x_st"], inc, A).reshape(E * A, F, 6), SC.pad_agents(b["nbr_sum"], inc, A).reshape(E * A, 2, F, 6),
                SC.pad_agents(b["edge_mask"], inc, A).reshape(E * A, 2), x_T, SC.pad_agents(b["p0"], inc, A), k, n_in)
        with lock:
            ((rows, lw), report), _ = repeat_in_fp32(lambda p: _split_report(engine.predict_padded(*args, dt=time_step, precision=p, **kw)), precision)
        batch_stats(report)
        return (*SC.assemble_forecasts(inc, rows, lw, b["cv"], pose_now, k, K, n_agents=n_in), inc)
    if limits.padded and n_in.min() >= 1:
        # the staged route on the whole batch: padded inputs, one encode, one rejection loop, one ranking of the accepted set
        A = int(n_in.max())
        if "p0" not in b:           # (device_frames built without reading the encoder inputs back)
            with lock:
                engine.build_scene(human_xy, robot_xy, time_step, horizon=H, first_frame=ff, **ab)
                b.update(engine.scene_arrays())
        counts = n_in.astype(np.int32)
        with lock:
            ctx = engine.encode(SC.pad_agents(b["x_st"], inc, A).reshape(E * A, F, 6), SC.pad_agents(b["nbr_sum"], inc, A).reshape(E * A, 2, F, 6),
                                SC.pad_agents(b["edge_mask"], inc, A).reshape(E * A, 2),
                                first_index=None if ff is None else SC.pad_agents(b["first_index"], inc, A).reshape(-1)).reshape(E, A, -1)
            out = run_staged(engine, ctx, SC.pad_agents(b["p0"], inc, A), (E, A, K, H), limits, plan(A).rank, k, time_step, precision,
                             seeded=dict(seed=int(seed), episode_ids=np.asarray(seeds), K=K, T=H), n_agents=counts)
        if stats is not None:
            stats["episodes"], stats["slots"], stats["cause"] = out.rejection.episodes, out.rejection.slots, out.rejection.cause
            if out.repair is not None:
                stats["repair"] = out.repair
            if out.repair_causes is not None:
                stats["repair_causes"] = out.repair_causes
        forecasts, logw = SC.assemble_forecasts(inc, out.rows, out.logw, b["cv"], pose_now, k, K, n_agents=counts)
        if absent:
            forecasts[left_out], logw[left_out] = np.nan, np.nan
        return forecasts, logw, inc
    forecasts = np.empty((E, N, k, H + 1, 2), dtype=np.float64)
    logw = np.empty((E, N, k), dtype=np.float64)
    if limits.repair is not None and stats is not None:
        stats["repair"] = np.zeros((E, 3), dtype=np.int32)
    if limits.guidance is not None and stats is not None:
        stats["guide"] = np.zeros((E, K, 2), dtype=np.float32)
    if limits.rounds is not None and stats is not None:
        stats["episodes"], stats["slots"] = np.zeros((E, 3), dtype=np.int32), np.zeros((E, K, 3), dtype=np.int32)
        if limits.walls:
            stats["cause"] = np.zeros((E, 2), dtype=np.int32)
    causes = []                                 # metrics.repair_causes of every group's repair with walls
    for A in np.unique(n_in):                   # episodes with the same count share their device calls
        eps = np.nonzero(n_in == A)[0]
        A = int(A)
        route = plan(A)
        if noise == "device":       # (seed, global episode id) is the whole address: nothing to draw here
            x_T, nz = None, dict(seed=int(seed), episode_ids=np.asarray(seeds)[eps], K=K, T=H)
        else:
            x_T, nz = torch.stack([torch_x_T(e, A) for e in eps]).numpy(), {}
        if route.run == "chain":
            with lock:              # the group's scenes resident, then predictor + assembly in one entry
                engine.build_scene(human_xy[eps], robot_xy[eps], time_step, horizon=H, first_frame=None if ff is None else ff[eps], **ab)
                ((forecasts[eps], logw[eps]), report), _ = repeat_in_fp32(
                    lambda p: _split_report(engine.forecast_scene(x_T, k, dt=time_step, precision=p, **nz, **(kw if A else {}))), precision)
            if report is not None and stats is not None:
                if report.guide is not None:
                    stats["guide"][eps] = report.guide
                if report.episode is not None:
                    stats["repair"][eps] = report.episode
            if report is not None and report.wall is not None:
                causes.append(chain_report_causes(report, limits))
            continue
        if "p0" not in b:           # (device_frames built without reading the encoder inputs back)
            with lock:
                engine.build_scene(human_xy, robot_xy, time_step, horizon=H, first_frame=ff, **ab)
                b.update(engine.scene_arrays())
        rows = np.stack([np.nonzero(inc[e])[0] for e in eps])                       # [Eg, A] ascending track ids
        ei, n = eps[:, None], len(eps) * A
        p0 = np.ascontiguousarray(b["p0"][ei, rows])
        with lock:                  # every episode of the group in ONE encode, denoise and jmid_topk call
            ctx = engine.encode(b["x_st"][ei, rows].reshape(n, F, 6), b["nbr_sum"][ei, rows].reshape(n, 2, F, 6),
                                b["edge_mask"][ei, rows].reshape(n, 2),
                                first_index=None if ff is None else b["first_index"][ei, rows].reshape(-1)).reshape(len(eps), A, -1)
            # (an empty cluster: no loop and no repair - its stats rows stay zero)
            out = run_staged(engine, ctx, p0, (len(eps), A, K, H), limits if A else Constraints(), route.rank, k, time_step, precision,
                             x_T=x_T, seeded=nz)
        if out.rejection is not None and stats is not None:
            stats["episodes"][eps], stats["slots"][eps] = out.rejection.episodes, out.rejection.slots
            if out.rejection.cause is not None:
                stats["cause"][eps] = out.rejection.cause
        if out.repair is not None and stats is not None:
            stats["repair"][eps] = out.repair
        if out.repair_causes is not None:
            causes.append(out.repair_causes)
        if out.guide is not None and stats is not None:
            stats["guide"][eps] = out.guide
        forecasts[eps], logw[eps] = SC.assemble_forecasts(inc[eps], out.rows, out.logw, b["cv"][eps], pose_now[eps], k, K)
    if causes and stats is not None:            # the groups' counts, summed
        stats["repair_causes"] = {key: sum(c[key] for c in causes) for key in causes[0]}
    if absent:
        forecasts[left_out], logw[left_out] = np.nan, np.nan
    return forecasts, logw, inc


def write_configs(directory: str, *, joint: bool, ctx_dim: int, N: int, K: int, k_ret: int, H: int, step: int,
                  past: int = 6, time_step: float = 0.25, model_path: str = "weights.npz"):
    """Helper for tests / demos: writes an env.config + MID yaml pair with the keys the predictor reads
    (``configs/env.config:8-13``, ``JMID/test_time_configs/mid_jp.yaml``) and returns (RawConfigParser, yaml path)."""
    os.makedirs(directory, exist_ok=True)
    cfg = dict(model_path=model_path,
               diffnet="JointPredictionTransformerConcatLinear" if joint else "TransformerConcatLinear",
               encoder_dim=ctx_dim, tf_layer=3, num_samples=K, step_size=step, prediction_horizon=H,
               maximum_history_length=past - 1, sampling="ddim", eval_mode=True, time=False,
               override_attention_radius=[])
    ypath = os.path.join(directory, "mid_jp.yaml" if joint else "mid.yaml")
    with open(ypath, "w") as f:
        yaml.safe_dump(cfg, f)
    env = configparser.RawConfigParser()
    env.add_section("env")
    env.set("env", "time_step", str(time_step))
    env.add_section("human_trajectory_forecaster")
    env.set("human_trajectory_forecaster", "publish_freq", "0.08")
    env.set("human_trajectory_forecaster", "past_num_frames", str(past))
    env.set("human_trajectory_forecaster", "prediction_horizon", str(H))
    env.set("human_trajectory_forecaster", "num_samples", str(k_ret))
    env.add_section("sim")
    env.set("sim", "human_num", str(N))
    return env, ypath
