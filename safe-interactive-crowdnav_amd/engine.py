"""JmidEngine: Python handle around the C ABI (``include/jmid_hip.h``).

This is the device half of the predictor: context encoder, the batched DDIM
reverse-denoising loop and the integrator, i.e. what ``AutoEncoder.generate_sicnav_inference``
(``sicnav_diffusion/JMID/MID/models/autoencoder.py:17-47``) does, for one scene or for a
batch of independent episodes.  No arithmetic happens in Python.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, NamedTuple, Optional, Tuple, Union

import numpy as np

from . import _lib
from ._lib import JmidError
from .schedule import VarianceSchedule, ddim_steps, ddpm_steps, loss_tables
from .weights import JMIDWeights

try:  # torch is optional plumbing here (device tensors in / out)
    import torch
except Exception:  # pragma: no cover
    torch = None

ArrayLike = Union[np.ndarray, "torch.Tensor"]

# every JMID_ERANGE any engine of this process has returned (the tests assert that no fixture ever produces one)
ERANGE_EVENTS: list = []
# every JMID_ETIMEOUT (a workgroup of a one-launch GEMM + LayerNorm gave up waiting for its partners: include/jmid_hip.h) - the engine
# repeats such a call once in the SAME precision (the handle has dropped that kernel by then) and records it here
TIMEOUT_EVENTS: list = []


def _is_cuda(t) -> bool:
    return torch is not None and isinstance(t, torch.Tensor) and t.is_cuda


def _out(shape, dtype=np.float32, device=None):
    """An uninitialised output array: a torch tensor on ``device`` (a device-mode call: the device its input lives on), or NumPy."""
    if device is None:
        return np.empty(shape, dtype=dtype)
    name = np.dtype(dtype).name
    return torch.empty(shape, dtype=getattr(torch, "int32" if name == "uint32" else name), device=device)     # (Philox words: the bits)


def _ptr(a) -> Optional[C.c_void_p]:
    """The raw pointer of a torch tensor or a NumPy array; None (an output that was not asked for) stays None."""
    if a is None:
        return None
    return C.c_void_p(a.data_ptr() if torch is not None and isinstance(a, torch.Tensor) else a.ctypes.data)


def kde_bandwidths(T: int):
    """The per-step KDE bandwidths of the joint top-k exactly as the reference computes them (fp32 torch ops, mid_sim_wrapper.py:26-30):
    a contiguous float32 CPU tensor [T]."""
    return torch.exp(torch.linspace(math.log(0.01), math.log(0.1), steps=T))


def agent_counts(n_agents, E: int) -> np.ndarray:
    """The ``n_agents`` argument of a padded call as the library takes it: a contiguous HOST int32 array [E] (the library checks the
    range 1..A and answers JMID_EINVAL)."""
    n = np.ascontiguousarray(np.asarray(n_agents.cpu() if torch is not None and torch.is_tensor(n_agents) else n_agents), dtype=np.int32).reshape(-1)
    if n.size != E:
        raise ValueError(f"n_agents must hold one count per episode ({E}), got {n.size}")
    return n


def wall_segments(walls) -> np.ndarray:
    """The ``walls`` argument of the wall entries as the library takes it: a contiguous HOST float64 array [L, 4] = {x1, y1, x2, y2}
    from [L, 4] or [L, 2, 2] (``crowd_env.static_obstacles(rule)[0]``); None or empty: L = 0.  The library checks the values."""
    if walls is None:
        return np.zeros((0, 4), dtype=np.float64)
    w = np.asarray(walls.detach().cpu() if torch is not None and torch.is_tensor(walls) else walls, dtype=np.float64)
    if w.size and (w.ndim < 2 or int(np.prod(w.shape[1:])) != 4):
        raise ValueError("walls must be [L, 4] or [L, 2, 2]")
    return np.ascontiguousarray(w.reshape(-1, 4))


def seeded_noise_args(x_T, seed, episode_ids, E: Optional[int] = None):
    """The noise source of a call: either the caller's ``x_T`` or ``seed`` + ``episode_ids`` (the library's counter generator,
    ``noise.py``), never both.  -> None for an explicit call, else (seed, ids uint32 [E])."""
    if seed is None:
        if episode_ids is not None:
            raise ValueError("episode_ids needs seed")
        if x_T is None:
            raise ValueError("either x_T or seed + episode_ids")
        return None
    if x_T is not None:
        raise ValueError("x_T and seed are mutually exclusive: a seeded call draws x_T itself")
    if episode_ids is None:
        raise ValueError("seed needs episode_ids (the global number of every episode of the call)")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits")
    ids = np.atleast_1d(np.asarray(episode_ids))
    if ids.ndim != 1 or (E is not None and ids.size != E) or ids.size < 1:
        raise ValueError("episode_ids must hold one id per episode")
    if np.any(ids.astype(np.int64) < 0) or np.any(ids.astype(np.int64) > 0xFFFFFFFF):
        raise ValueError("episode ids are uint32")
    return seed, np.ascontiguousarray(ids, dtype=np.uint32)


class Guidance(NamedTuple):
    """The guidance of a guided denoise call (``jmid_denoise_guided``; include/jmid_hip.h states the rule): after every step-table entry
    i with ``weights[i] > 0`` each joint sample is integrated, pushed apart by at most ``n_inner`` iterations of the repair's iteration
    with step ``weights[i]`` metres, and written back as velocities.  ``weights``: one per entry of the installed DDIM table
    (``schedule.guidance_weights``).  ``walls`` [L, 4] or [L, 2, 2] with ``wall_radius``: the wall terms too."""
    threshold: float
    margin: float = 0.02
    tau: float = 0.005
    weights: Any = None
    n_inner: int = 4
    walls: Any = None
    wall_radius: Optional[float] = None


REPAIR_DEFAULTS = {"margin": 0.02, "tau": 0.005, "step": 0.02, "max_iter": 32}      # those of ``JmidEngine.repair_collisions``


class ChainConstraints(NamedTuple):
    """The constraints of a one-entry chain (``predict(constraints=)`` ... ``forecast_scene_padded(constraints=)``; the
    ``jmid_*_constrained`` entries of include/jmid_hip.h): guided sampling inside the chain's denoise stage and collision repair between
    that stage and the ranking, at one ``threshold``.  ``guidance``: a ``Guidance`` (its threshold must be this one), or None.
    ``repair``: the keywords of ``JmidEngine.repair_collisions`` - margin, tau, step, max_iter, and ``walls`` with ``wall_radius`` for the
    repair with walls - ({}: the defaults), or None: no repair.  Where both mechanisms take walls they are the same walls."""
    threshold: float = 0.2
    guidance: Optional[Guidance] = None
    repair: Optional[dict] = None


class ChainReport(NamedTuple):
    """What a constrained chain reports next to its results, with the one download: the rows of the staged entries, unchanged.  ``guide``
    [E, K, 2] (``metrics.GUIDE_COLUMNS``) or None without guidance; ``sample`` [E, K, 4] and ``episode`` [E, 3] int32
    (``metrics.REPAIR_SAMPLE_COLUMNS`` / ``REPAIR_EPISODE_COLUMNS``) or None without repair; ``wall`` [E, K, 2]
    (``metrics.REPAIR_WALL_COLUMNS``) or None unless the repair takes walls.  The episode axis is always there."""
    guide: Optional[np.ndarray] = None
    sample: Optional[np.ndarray] = None
    episode: Optional[np.ndarray] = None
    wall: Optional[np.ndarray] = None


def chain_constraint_arguments(constraints: ChainConstraints, n_steps: int):
    """The ``<constraints>`` arguments of the constrained chains from a ``ChainConstraints`` (threshold, guide_weights, n_inner,
    guide_margin, guide_tau, guide_walls, repair, margin, tau, step, max_iter, repair_walls, L, walls, wall_radius) as plain Python values
    and arrays - ``guide_weights`` float64 [n_steps] or None, ``walls`` float64 [L, 4] - with every refusal that needs no device."""
    c = constraints
    if not isinstance(c, ChainConstraints):
        raise TypeError("constraints must be an engine.ChainConstraints")
    threshold = float(c.threshold)
    if not (np.isfinite(threshold) and threshold >= 0.0):
        raise ValueError("constraints.threshold must be finite and >= 0")
    g, walls, radius = c.guidance, None, None
    weights, n_inner, g_margin, g_tau, g_walls = None, 0, 0.0, 0.0, 0
    if g is not None:
        if float(g.threshold) != threshold:
            raise ValueError("constraints.guidance.threshold differs from constraints.threshold (a chain has one threshold)")
        if g.weights is None:
            raise ValueError("guidance needs weights: one per step-table entry (schedule.guidance_weights)")
        weights = np.ascontiguousarray(np.asarray(g.weights, dtype=np.float64).reshape(-1))
        if weights.size != n_steps:
            raise ValueError(f"guidance.weights must hold one weight per step-table entry ({n_steps}), got {weights.size}")
        if (g.walls is None) != (g.wall_radius is None):
            raise ValueError("guidance: walls and wall_radius go together (the guidance knows no agent radius)")
        n_inner, g_margin, g_tau = int(g.n_inner), float(g.margin), float(g.tau)
        if g.walls is not None:
            walls, radius, g_walls = wall_segments(g.walls), float(g.wall_radius), 1
    margin, tau, step, max_iter, r_walls = 0.0, 0.0, 0.0, 0, 0
    if c.repair is not None:
        opts = dict(c.repair)
        unknown = sorted(set(opts) - set(REPAIR_DEFAULTS) - {"walls", "wall_radius"})
        if unknown:
            raise ValueError(f"unknown repair options {unknown} (known: {sorted(REPAIR_DEFAULTS) + ['wall_radius', 'walls']})")
        if (opts.get("walls") is None) != (opts.get("wall_radius") is None):
            raise ValueError("repair: walls and wall_radius go together (the repair knows no agent radius)")
        margin, tau, step = (float(opts.get(key, REPAIR_DEFAULTS[key])) for key in ("margin", "tau", "step"))
        max_iter = int(opts.get("max_iter", REPAIR_DEFAULTS["max_iter"]))
        if opts.get("walls") is not None:
            rw, rr = wall_segments(opts["walls"]), float(opts["wall_radius"])
            if walls is not None and (rw.shape != walls.shape or not np.array_equal(rw, walls) or rr != radius):
                raise ValueError("the guidance and the repair of one chain take the same walls and wall_radius")
            walls, radius, r_walls = rw, rr, 1
    if walls is None:
        walls, radius = np.zeros((0, 4), dtype=np.float64), 0.0
    if (g_walls or r_walls) and walls.shape[0] == 0:
        raise ValueError("walls are asked for, and there are none (L = 0)")
    return (threshold, weights, n_inner, g_margin, g_tau, g_walls, int(c.repair is not None), margin, tau, step, max_iter, r_walls,
            int(walls.shape[0]), walls, radius)


class LossResult:
    """What ``JmidEngine.loss`` returns: ``loss``, ``count``, and ``rows`` / ``e_theta`` where they were asked for (else None)."""
    __slots__ = ("loss", "count", "rows", "e_theta")

    def __init__(self, loss, count, rows=None, e_theta=None):
        self.loss, self.count, self.rows, self.e_theta = loss, count, rows, e_theta

    def __repr__(self):
        return f"LossResult(loss={float(self.loss):.6g}, count={int(self.count)})"


class _Buf:
    """fp32 contiguous view of an input + its raw pointer."""

    def __init__(self, a: ArrayLike, device_mode: bool):
        if device_mode:
            if not _is_cuda(a):
                raise TypeError("device-mode call needs CUDA/HIP torch tensors for every array argument")
            self.keep = a.detach().to(torch.float32).contiguous()
            self.ptr = C.c_void_p(self.keep.data_ptr())
        else:
            if torch is not None and isinstance(a, torch.Tensor):
                a = a.detach().cpu().numpy()
            self.keep = np.ascontiguousarray(a, dtype=np.float32)
            self.ptr = C.c_void_p(self.keep.ctypes.data)


class JmidEngine:
    """One predictor engine (weights resident on one GPU, one HIP stream)."""

    def __init__(self, weights: JMIDWeights, joint: bool, device_id: int = 0, hist_len: int = 6,
                 step: int = 50, schedule: Optional[VarianceSchedule] = None, lib_path: Optional[str] = None):
        self._lib = _lib.load_library(lib_path)      # lib_path: another build of the library (tests: both flavours in one process)
        self._h = _lib.Handle()
        self.dims = weights.dims
        self.joint = bool(joint)
        self.device_id = device_id
        self._caller_stream = 0          # NULL: the legacy default stream
        self.hist_len = hist_len
        rc = self._lib.jmid_create(C.byref(self._h), device_id, _lib.NET_JMID if joint else _lib.NET_IMID,
                                   self.dims.ctx_dim, self.dims.tf_layer, self.dims.nhead, hist_len)
        if rc != 0:
            msg = self._lib.jmid_last_error(None).decode()
            self._h = None
            raise JmidError(rc, msg)
        for name, t in weights.tensors.items():
            a = np.ascontiguousarray(t.numpy(), dtype=np.float32)
            self._check(self._lib.jmid_load_weight(self._h, name.encode(), C.c_void_p(a.ctypes.data), a.size))
        self._check(self._lib.jmid_finalize_weights(self._h))
        self.schedule = schedule or VarianceSchedule.linear()
        self.set_step(step)

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int) -> None:
        if rc == _lib.ERANGE:
            ERANGE_EVENTS.append((id(self), self._lib.jmid_last_error(self._h).decode()))
        if rc != 0:
            raise JmidError(rc, self._lib.jmid_last_error(self._h).decode())

    def _compute(self, fn, *args) -> None:
        """A compute entry of the C ABI.  JMID_ETIMEOUT is not an arithmetic condition: the library has switched this handle to the
        unfused kernels (same bits), so the call is repeated once, as it is, and the event recorded."""
        rc = fn(*args)
        if rc == _lib.ETIMEOUT:
            TIMEOUT_EVENTS.append((id(self), self._lib.jmid_last_error(self._h).decode()))
            rc = fn(*args)
        self._check(rc)

    def timeout_count(self) -> int:
        """Calls on this engine that ended with JMID_ETIMEOUT (at most one in practice: the first switches the handle for good)."""
        return int(self._lib.jmid_timeout_count(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.jmid_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def set_step(self, step: int, sampling: str = "ddim", flexibility: float = 0.0) -> None:
        """``step`` = the reference's ``step_size`` yaml key: number of reverse iterations out of 100
        (stride = int(100/step), MID/models/diffusion.py:507); ``sampling`` = "ddim" (what the predictor uses,
        MID/mid.py:333) or "ddpm" with ``flexibility`` (``get_sigmas``, diffusion.py:59-64)."""
        self.step, self.sampling = step, sampling
        if sampling == "ddim":
            tab = ddim_steps(self.schedule, step)
            cols = [np.array([getattr(s, k) for s in tab], dtype=np.float32) for k in ("beta", "c_e", "c_x", "n_x", "n_e")]
            self._check(self._lib.jmid_set_ddim_table(self._h, len(tab), *[C.c_void_p(c.ctypes.data) for c in cols]))
        elif sampling == "ddpm":
            tab = ddpm_steps(self.schedule, step, flexibility)
            cols = [np.array([getattr(s, k) for s in tab], dtype=np.float32) for k in ("beta", "c0", "c1", "sigma")]
            cols.append(np.array([int(s.noise) for s in tab], dtype=np.int32))
            self._check(self._lib.jmid_set_ddpm_table(self._h, len(tab), *[C.c_void_p(c.ctypes.data) for c in cols]))
        else:
            raise ValueError("sampling must be 'ddim' or 'ddpm'")
        self.n_steps = len(tab)

    def set_chunk_episodes(self, n: int) -> None:
        self._check(self._lib.jmid_set_chunk_episodes(self._h, int(n)))

    def set_tuning(self, key: str, value: int) -> None:
        self._check(self._lib.jmid_set_tuning(self._h, key.encode(), int(value)))

    def _mem(self, dev: bool) -> int:
        """Memory mode of a call; device-mode calls are ordered against torch's CURRENT stream (include/jmid_hip.h)."""
        if not dev:
            return _lib.MEM_HOST
        st = int(torch.cuda.current_stream(self.device_id).cuda_stream)
        if st != self._caller_stream:
            self._check(self._lib.jmid_set_caller_stream(self._h, C.c_void_p(st)))
            self._caller_stream = st
        return _lib.MEM_DEVICE

    def graph_replays(self) -> int:
        """Calls whose denoise loop ran as a replayed hipGraph (small one-chunk calls from their third repetition on)."""
        return int(self._lib.jmid_graph_replays(self._h))

    def erange_count(self) -> int:
        """Calls on this engine that ended with JMID_ERANGE (an activation left the fp16 range: the caller repeats in "f32")."""
        return int(self._lib.jmid_erange_count(self._h))

    def synchronize(self) -> None:
        self._check(self._lib.jmid_synchronize(self._h))

    # ------------------------------------------------------------------ compute
    def _first_index(self, first_index, n: int) -> np.ndarray:
        """The argument check of ``encode(first_index=)``: n values in 0..hist_len-2 -> contiguous int32 (no device is touched)."""
        if torch is not None and isinstance(first_index, torch.Tensor):
            first_index = first_index.detach().cpu().numpy()
        fi = np.asarray(first_index)
        if fi.shape != (n,) or not np.issubdtype(fi.dtype, np.integer):
            raise ValueError("first_index must hold one integer per row")
        if (fi < 0).any() or (fi > self.hist_len - 2).any():
            raise ValueError(f"first_index must lie in 0..hist_len-2 = 0..{self.hist_len - 2}: a row needs two history frames")
        return np.ascontiguousarray(fi, dtype=np.int32)

    def encode(self, x_st: ArrayLike, nbr_sum: ArrayLike, edge_mask: ArrayLike, first_index=None) -> ArrayLike:
        """x_st [n, hist, 6], nbr_sum [n, 2, hist, 6], edge_mask [n, 2] -> ctx [n, ctx_dim].  ``first_index`` [n] integers (a host array;
        ``jmid_encode_var``): row r was first seen at history frame first_index[r] and its LSTMs run over the frames from there on, from a
        zero state - the frames in front of it are not read and may hold NaN.  None: every row has the full window (``jmid_encode``)."""
        dev = _is_cuda(x_st)
        n = int(x_st.shape[0])
        if tuple(x_st.shape) != (n, self.hist_len, 6) or tuple(nbr_sum.shape) != (n, 2, self.hist_len, 6) \
                or tuple(edge_mask.shape) != (n, 2):
            raise ValueError("bad encoder input shapes")
        fi = None if first_index is None else self._first_index(first_index, n)
        a, b, c = _Buf(x_st, dev), _Buf(nbr_sum, dev), _Buf(edge_mask, dev)
        out = _out((n, self.dims.ctx_dim), device=x_st.device if dev else None)
        if fi is not None:
            self._check(self._lib.jmid_encode_var(self._h, n, a.ptr, b.ptr, c.ptr, _ptr(fi), _ptr(out), self._mem(dev)))
            return out
        self._check(self._lib.jmid_encode(self._h, n, a.ptr, b.ptr, c.ptr, _ptr(out), self._mem(dev)))
        return out

    def _shapes(self, x, ctx) -> Tuple[int, int, int, int]:
        if x.ndim != 4 or ctx.ndim != 3 or x.shape[0] != ctx.shape[0] or x.shape[-1] != 2:
            raise ValueError("expected x [E, K*A, T, 2] and ctx [E, A, ctx_dim]")
        E, KA, T, _ = (int(v) for v in x.shape)
        A = int(ctx.shape[1])
        if int(ctx.shape[2]) != self.dims.ctx_dim or KA % A != 0:
            raise ValueError("ctx width / row count mismatch")
        return E, A, KA // A, T

    def noise(self, seed: int, episode_ids, rows: int, T: int, draw: int = 0, device: bool = False, words: bool = False, n_agents=None,
              A: Optional[int] = None):
        """One draw of the library's counter generator (``jmid_noise_fill``; host twin ``noise.normal``): standard normals float32
        [E, rows, T, 2] for the episodes ``episode_ids`` - draw 0 is the x_T of a seeded call with rows = K * A, draw i + 1 the z of
        step-table entry i.  ``device=True``: a CUDA tensor.  ``words=True`` (diagnostics flavour): the raw Philox words, uint32.
        ``n_agents`` [E] (``jmid_noise_fill_padded``; host twin ``noise.fill_padded``): the draw of a padded batch, rows = K * A with A
        the largest count (or ``A``): episode e draws what it draws alone at rows = K * n_agents[e], its row s * n_e + a lands in row
        s * A + a, and the padded rows are NaN."""
        seed, ids = seeded_noise_args(None, seed, episode_ids)
        E = int(ids.size)
        if n_agents is not None:
            if words:
                raise ValueError("the raw words have no padded form")
            na = agent_counts(n_agents, E)
            A = int(na.max()) if A is None else int(A)
            if A < 1 or int(rows) % A != 0:
                raise ValueError(f"rows = {rows} is not K * A for A = {A}")
            out = _out((E, int(rows), int(T), 2), np.float32, f"cuda:{self.device_id}" if device else None)
            self._check(self._lib.jmid_noise_fill_padded(self._h, seed, E, A, int(rows) // A, int(T), _ptr(na), _ptr(ids), int(draw), _ptr(out),
                                                         self._mem(bool(device))))
            return out
        out = _out((E, int(rows), int(T), 2), np.uint32 if words else np.float32, f"cuda:{self.device_id}" if device else None)
        fn = self._lib.jmid_dbg_noise_words if words else self._lib.jmid_noise_fill
        self._check(fn(self._h, seed, E, int(rows), int(T), _ptr(ids), int(draw), _ptr(out), self._mem(bool(device))))
        return out

    def denoise(self, x_T: Optional[ArrayLike], ctx: ArrayLike, p0: Optional[ArrayLike] = None, dt: float = 0.25,
                precision: str = "f32", want_vel: bool = True, want_pos: bool = True, z: Optional[ArrayLike] = None,
                seed: Optional[int] = None, episode_ids=None, K: Optional[int] = None, T: Optional[int] = None, n_agents=None,
                guidance: Optional[Guidance] = None, want_guide: bool = False):
        """Batched reverse-denoising loop.  x_T [E, K*A, T, 2], ctx [E, A, ctx_dim], p0 [E, A, 2].
        ``guidance`` (a ``Guidance``; ``jmid_denoise_guided`` / ``_seeded``, DDIM, ``p0`` required): softplus collision steps between
        the denoise steps - explicit, seeded or padded (``n_agents``, with ``seed`` too: the padded draw).  ``want_guide=True``: a third
        value, guide [E, K, 2] = ``metrics.GUIDE_COLUMNS``.  Without it the call is the call it always was.
        ``n_agents`` [E] (``jmid_denoise_padded``, DDIM with an explicit x_T only): episode e has n_agents[e] <= A real agents, rows
        s*A + a with a >= n_agents[e] are padding - never read on the way in, NaN in vel and pos.
        ``z`` [n_steps, E, K*A, T, 2]: per-step normal draws, required when the DDPM table is installed.
        ``seed`` + ``episode_ids`` [E] (with ``x_T=None`` and the sample count ``K`` and horizon ``T``): the library draws x_T - and,
        under the DDPM table, every step's z - from its counter generator (``jmid_denoise_seeded``; ``noise.py``): the same bits as the
        explicit call fed ``noise(seed, episode_ids, K * A, T, draw)``, for every batch the episodes are part of.
        Returns (vel [E,K,A,T,2] or None, pos [E,K,A,T,2] or None)."""
        seeded = seeded_noise_args(x_T, seed, episode_ids)
        if guidance is None and want_guide:
            raise ValueError("want_guide needs guidance")
        if guidance is not None and z is not None:
            raise ValueError("a guided call is DDIM: no z")
        if n_agents is not None and ((seeded is not None and guidance is None) or z is not None):
            raise ValueError("a padded call (n_agents) is DDIM with an explicit x_T: no seed, no z")
        if seeded is not None:
            if z is not None:
                raise ValueError("z and seed are mutually exclusive: a seeded call draws z itself")
            if K is None or T is None or ctx.ndim != 3 or int(ctx.shape[2]) != self.dims.ctx_dim:
                raise ValueError("a seeded call needs K, T and ctx [E, A, ctx_dim]")
            dev = _is_cuda(ctx)
            E, A, K, T = int(ctx.shape[0]), int(ctx.shape[1]), int(K), int(T)
            seeded = seeded_noise_args(None, seed, episode_ids, E)
            x_like = ctx
        else:
            dev = _is_cuda(x_T)
            E, A, K, T = self._shapes(x_T, ctx)
            x_like = x_T
        want_pos = want_pos and p0 is not None
        bx, bc = (_Buf(x_T, dev) if seeded is None else None), _Buf(ctx, dev)
        bp = _Buf(p0, dev) if p0 is not None else None
        if z is not None and tuple(z.shape) != (self.n_steps, E, K * A, T, 2):
            raise ValueError("z must be [n_steps, E, K*A, T, 2]")
        where = x_like.device if dev else None
        vel = _out((E, K, A, T, 2), device=where) if want_vel else None
        pos = _out((E, K, A, T, 2), device=where) if want_pos else None
        tail = (bc.ptr, bp.ptr if bp else None, float(dt), _lib.PRECISIONS[precision], _ptr(vel), _ptr(pos), self._mem(dev))
        if guidance is not None:
            if p0 is None:
                raise ValueError("a guided call needs p0 (the guidance is defined on positions)")
            gargs, keep = self._guidance_args(guidance)
            guide = _out((E, K, 2), device=where) if want_guide else None
            na = agent_counts(n_agents, E) if n_agents is not None else None
            head = (self._h, E, A, K, T, _ptr(na))
            mid = (bc.ptr, bp.ptr, float(dt), _lib.PRECISIONS[precision]) + gargs + (_ptr(vel), _ptr(pos), _ptr(guide), self._mem(dev))
            if seeded is not None:
                self._compute(self._lib.jmid_denoise_guided_seeded, *head, seeded[0], _ptr(seeded[1]), *mid)
            else:
                self._compute(self._lib.jmid_denoise_guided, *head, bx.ptr, *mid)
            return (vel, pos, guide) if want_guide else (vel, pos)
        if seeded is not None:
            self._compute(self._lib.jmid_denoise_seeded, self._h, E, A, K, T, seeded[0], _ptr(seeded[1]), *tail)
        elif z is not None:
            bz = _Buf(z, dev)
            self._compute(self._lib.jmid_denoise_ddpm, self._h, E, A, K, T, bx.ptr, bz.ptr, *tail)
        elif n_agents is not None:
            na = agent_counts(n_agents, E)
            self._compute(self._lib.jmid_denoise_padded, self._h, E, A, K, T, _ptr(na), bx.ptr, *tail)
        else:
            self._compute(self._lib.jmid_denoise, self._h, E, A, K, T, bx.ptr, *tail)
        return vel, pos

    def _guidance_args(self, g: Guidance):
        """The arguments of a ``Guidance`` as the guided entries take them (threshold ... wall_radius) and the arrays they point into."""
        if g.weights is None:
            raise ValueError("guidance needs weights: one per step-table entry (schedule.guidance_weights)")
        w = np.ascontiguousarray(np.asarray(g.weights, dtype=np.float64).reshape(-1))
        if w.size != self.n_steps:
            raise ValueError(f"guidance.weights must hold one weight per step-table entry ({self.n_steps}), got {w.size}")
        if g.walls is None and g.wall_radius is not None:
            raise ValueError("wall_radius is given without walls")
        if g.walls is not None and g.wall_radius is None:
            raise ValueError("walls need wall_radius (the guidance knows no agent radius)")
        walls = wall_segments(g.walls)
        L = int(walls.shape[0])
        args = (float(g.threshold), float(g.margin), float(g.tau), _ptr(w), int(g.n_inner), L, _ptr(walls) if L else None,
                float(g.wall_radius) if g.wall_radius is not None else 0.0)
        return args, (w, walls)

    def guide_step(self, x: ArrayLike, p0: ArrayLike, dt: float = 0.25, threshold: float = 0.2, margin: float = 0.02, tau: float = 0.005,
                   weight: float = 0.02, n_inner: int = 4, n_agents=None, walls=None, wall_radius: Optional[float] = None, inplace: bool = False):
        """One guidance step on the device (``jmid_guide_step``; the rule stands in include/jmid_hip.h, its host twin is
        ``metrics.guide_step_host``): x [E, K*A, T, 2] velocities (row s*A + a), p0 [E, A, 2] -> (x_out, guide [E, K, 2] =
        ``metrics.GUIDE_COLUMNS``).  What a guided ``denoise`` runs behind one step-table entry with ``weight`` metres.  NumPy in ->
        NumPy out, CUDA tensors in -> CUDA tensors out; ``inplace=True`` (a contiguous float32 CUDA tensor): x itself is written and
        returned.  ``n_agents`` [E]: a padded block.  ``walls`` [L, 4] or [L, 2, 2] with ``wall_radius``: the wall terms too."""
        if walls is None and wall_radius is not None:
            raise ValueError("wall_radius is given without walls")
        if walls is not None and wall_radius is None:
            raise ValueError("walls need wall_radius (the guidance knows no agent radius)")
        if x.ndim != 4 or int(x.shape[-1]) != 2 or p0.ndim != 3 or int(p0.shape[0]) != int(x.shape[0]) or int(p0.shape[2]) != 2 \
                or int(x.shape[1]) % int(p0.shape[1]):
            raise ValueError("expected x [E, K*A, T, 2] and p0 [E, A, 2]")
        dev = _is_cuda(x)
        E, KA, T, _ = (int(v) for v in x.shape)
        A = int(p0.shape[1])
        K = KA // A
        bx, b0 = _Buf(x, dev), _Buf(p0, dev)
        where = x.device if dev else None
        if inplace:
            if not dev or bx.keep.data_ptr() != x.data_ptr():
                raise ValueError("inplace needs a contiguous float32 CUDA tensor")
            out = x
        else:
            out = _out((E, KA, T, 2), device=where)
        guide = _out((E, K, 2), device=where)
        na = agent_counts(n_agents, E) if n_agents is not None else None
        w = wall_segments(walls)
        L = int(w.shape[0])
        self._check(self._lib.jmid_guide_step(self._h, E, A, K, T, _ptr(na), bx.ptr, b0.ptr, float(dt), float(threshold), float(margin), float(tau),
                                              float(weight), int(n_inner), L, _ptr(w) if L else None,
                                              float(wall_radius) if wall_radius is not None else 0.0, _ptr(out), _ptr(guide), self._mem(dev)))
        return out, guide

    def denoise_padded_seeded(self, ctx: ArrayLike, p0: Optional[ArrayLike], n_agents, seed: int, episode_ids, K: int, T: int, dt: float = 0.25,
                              precision: str = "f32", want_vel: bool = True, want_pos: bool = True):
        """``denoise(n_agents=)`` with x_T drawn by the library (``jmid_denoise_padded_seeded``, DDIM only): the same bits as the padded
        call fed ``noise(seed, episode_ids, K * A, T, n_agents=n_agents)`` - every episode draws what it draws alone at its own count.
        ctx [E, A, ctx_dim], p0 [E, A, 2] -> (vel [E, K, A, T, 2] or None, pos or None), NaN in the padded rows."""
        if ctx.ndim != 3 or int(ctx.shape[2]) != self.dims.ctx_dim:
            raise ValueError("expected ctx [E, A, ctx_dim]")
        dev = _is_cuda(ctx)
        E, A, K, T = int(ctx.shape[0]), int(ctx.shape[1]), int(K), int(T)
        seed, ids = seeded_noise_args(None, seed, episode_ids, E)
        na = agent_counts(n_agents, E)
        want_pos = want_pos and p0 is not None
        bc, bp = _Buf(ctx, dev), (_Buf(p0, dev) if p0 is not None else None)
        where = ctx.device if dev else None
        vel = _out((E, K, A, T, 2), device=where) if want_vel else None
        pos = _out((E, K, A, T, 2), device=where) if want_pos else None
        self._compute(self._lib.jmid_denoise_padded_seeded, self._h, E, A, K, T, _ptr(na), seed, _ptr(ids), bc.ptr, bp.ptr if bp else None,
                      float(dt), _lib.PRECISIONS[precision], _ptr(vel), _ptr(pos), self._mem(dev))
        return vel, pos

    def denoise_reject(self, ctx: ArrayLike, p0: ArrayLike, seed: int, episode_ids, K: int, T: int, dt: float = 0.25, precision: str = "f32",
                       threshold: float = 0.2, max_rounds: int = 3, draw0: int = 0, want_vel: bool = True, want_pos: bool = True,
                       walls=None, wall_radius: Optional[float] = None, n_agents=None):
        """Collision-free sampling (``jmid_denoise_reject_seeded``; the rule stands in include/jmid_hip.h, its host twin is
        ``metrics.fill_slots``): the seeded ``denoise`` of draw number ``draw0``, then up to ``max_rounds`` reruns of the episodes that
        still hold a joint sample in which two agents come closer than ``threshold`` (the predicate of ``collision_statistics``) - an
        episode's K samples are redrawn together from draw ``draw0 + round`` and the acceptable candidates fill the bad slots in
        ascending order.  ctx [E, A, ctx_dim], p0 [E, A, 2] -> (vel [E, K, A, T, 2] or None, pos [E, K, A, T, 2] or None, slots [E, K, 3] int32 =
        (round, candidate, still colliding), episodes [E, 3] int32 = (colliding at round 0, fixed, last round rerun)).  DDIM only.
        NumPy in -> NumPy out, CUDA tensors in -> CUDA tensors out.  The accepted set stays resident for ``topk(None, ...)`` and the
        statistics entries.
        ``walls`` [L, 4] or [L, 2, 2] with ``wall_radius`` (``jmid_denoise_reject_walls_seeded``): a sample must also keep every agent's
        path, the step p0 -> pos[0] included, at least ``wall_radius`` away from every wall (the predicate of ``wall_statistics`` with
        this call's p0); a fifth value comes back, cause [E, 2] int32 = (slots whose round-0 sample fails the pedestrian predicate,
        the wall predicate).  Without ``walls`` the call, its route and its four values are what they were.
        ``n_agents`` [E] (``jmid_denoise_reject_padded_seeded``): ONE loop for a padded batch of mixed counts - episode e has n_agents[e] <= A
        real agents, the predicate is that of ``collision_statistics(n_agents=)`` / ``wall_statistics(n_agents=)``, round j draws by the
        padded rule at draw ``draw0 + j``, a rerun keeps the call's A as its row stride, and the padded rows of vel and pos are NaN.
        Always five values (cause [:, 1] is 0 without walls).  Without ``n_agents`` nothing changes."""
        if ctx.ndim != 3 or int(ctx.shape[2]) != self.dims.ctx_dim:
            raise ValueError("expected ctx [E, A, ctx_dim]")
        if (walls is None) != (wall_radius is None):
            raise ValueError("walls and wall_radius go together (the sampler knows no agent radius)")
        if self.sampling != "ddim":
            raise ValueError("collision-free sampling is DDIM only: under DDPM the draws 1.. are the steps' z")
        if p0 is None:
            raise ValueError("collision-free sampling needs p0: the predicate is defined on positions")
        dev = _is_cuda(ctx)
        E, A, K, T = int(ctx.shape[0]), int(ctx.shape[1]), int(K), int(T)
        if tuple(p0.shape) != (E, A, 2):
            raise ValueError("p0 must be [E, A, 2]")
        seed, ids = seeded_noise_args(None, seed, episode_ids, E)
        bc, bp = _Buf(ctx, dev), _Buf(p0, dev)
        where = ctx.device if dev else None
        vel = _out((E, K, A, T, 2), device=where) if want_vel else None
        pos = _out((E, K, A, T, 2), device=where) if want_pos else None
        slots, episodes = _out((E, K, 3), np.int32, where), _out((E, 3), np.int32, where)
        if n_agents is not None:
            na, cause = agent_counts(n_agents, E), _out((E, 2), np.int32, where)
            w = wall_segments(walls) if walls is not None else None
            L = int(w.shape[0]) if w is not None else 0
            self._compute(self._lib.jmid_denoise_reject_padded_seeded, self._h, E, A, K, T, _ptr(na), seed, _ptr(ids), int(draw0), bc.ptr, bp.ptr,
                          float(dt), _lib.PRECISIONS[precision], float(threshold), int(max_rounds), L, _ptr(w) if L else None,
                          float(wall_radius) if wall_radius is not None else 0.0, _ptr(vel), _ptr(pos), _ptr(slots), _ptr(episodes), _ptr(cause),
                          self._mem(dev))
            return vel, pos, slots, episodes, cause
        if walls is not None:
            w, cause = wall_segments(walls), _out((E, 2), np.int32, where)
            L = int(w.shape[0])
            self._compute(self._lib.jmid_denoise_reject_walls_seeded, self._h, E, A, K, T, seed, _ptr(ids), int(draw0), bc.ptr, bp.ptr, float(dt),
                          _lib.PRECISIONS[precision], float(threshold), int(max_rounds), L, _ptr(w) if L else None, float(wall_radius),
                          _ptr(vel), _ptr(pos), _ptr(slots), _ptr(episodes), _ptr(cause), self._mem(dev))
            return vel, pos, slots, episodes, cause
        self._compute(self._lib.jmid_denoise_reject_seeded, self._h, E, A, K, T, seed, _ptr(ids), int(draw0), bc.ptr, bp.ptr, float(dt),
                      _lib.PRECISIONS[precision], float(threshold), int(max_rounds), _ptr(vel), _ptr(pos), _ptr(slots), _ptr(episodes),
                      self._mem(dev))
        return vel, pos, slots, episodes

    def topk(self, pos: Optional[ArrayLike], k: int, dims: Optional[Tuple[int, int, int, int]] = None, n_agents=None):
        """Joint-KDE top-k on the device (``jmid_topk``; get_most_likely_samples, mid_sim_wrapper.py:14-169), batched over
        episodes.  pos [E, K, A, T, 2] -> (kept [E, A, k, T, 2], log-weights [E, A, k]) in ascending likelihood.
        ``pos=None`` with ``dims=(E, A, K, T)`` ranks the positions of the preceding ``denoise`` call, which are still in the
        engine's workspace (nothing but the k kept samples comes back to the host).
        ``n_agents`` [E] (``jmid_topk_padded``): episode e is ranked in 2 n_agents[e] dimensions over its real agents; kept samples
        and log-weights of the padded agents are NaN."""
        if pos is None:
            if dims is None:
                raise ValueError("pos=None needs dims=(E, A, K, T) of the preceding denoise call")
            E, A, K, T = (int(v) for v in dims)
            dev, bp = False, None
        else:
            dev = _is_cuda(pos)
            E, K, A, T, _ = (int(v) for v in pos.shape)
            bp = _Buf(pos, dev)
        na = agent_counts(n_agents, E) if n_agents is not None else None
        where = pos.device if dev else None
        bw = kde_bandwidths(T).to(pos.device) if dev else kde_bandwidths(T)
        sel, lw = _out((E, A, k, T, 2), device=where), _out((E, A, k), device=where)
        tail = (bp.ptr if bp is not None else None, _ptr(bw), _ptr(sel), _ptr(lw), self._mem(dev))
        if na is not None:
            self._check(self._lib.jmid_topk_padded(self._h, E, A, K, T, int(k), _ptr(na), *tail))
        else:
            self._check(self._lib.jmid_topk(self._h, E, A, K, T, int(k), *tail))
        return sel, lw

    def predict_padded(self, x_st: np.ndarray, nbr_sum: np.ndarray, edge_mask: np.ndarray, x_T: np.ndarray, p0: np.ndarray, k: int,
                       n_agents, dt: float = 0.25, precision: str = "f32", constraints: Optional[ChainConstraints] = None):
        """``predict`` for episodes of different agent counts in one call (``jmid_predict_padded``): the same arrays with A = the
        largest count as the row stride (``scene.pad_rows`` / ``scene.pad_samples`` make them) and ``n_agents`` [E].  The padded
        agents' rows of every output are NaN.  ``constraints``: as ``predict``."""
        return self._predict(n_agents, x_st, nbr_sum, edge_mask, x_T, p0, k, dt, precision, constraints)

    def predict(self, x_st: np.ndarray, nbr_sum: np.ndarray, edge_mask: np.ndarray, x_T: np.ndarray, p0: np.ndarray, k: int,
                dt: float = 0.25, precision: str = "f32", constraints: Optional[ChainConstraints] = None):
        """One predictor call end to end (``jmid_predict``): encoder -> denoise loop -> integrator -> joint-KDE top-k, host arrays in
        and out, one upload, one download, nothing in between.  x_st [E*A, hist, 6], nbr_sum [E*A, 2, hist, 6], edge_mask [E*A, 2],
        x_T [E, K*A, T, 2], p0 [E, A, 2].  k < K -> (kept [E, A, k, T, 2], log-weights [E, A, k]); k == K -> (pos [E, K, A, T, 2], None).
        ``constraints`` (a ``ChainConstraints``; ``jmid_predict_constrained``): guided sampling and / or collision repair inside the same
        one call - the bits of the staged ``encode`` -> ``denoise(guidance=)`` -> ``repair_collisions(None, ...)`` -> ``topk(None, ...)`` -
        and a third value, the ``ChainReport``.  Without it the call is the call it always was."""
        return self._predict(None, x_st, nbr_sum, edge_mask, x_T, p0, k, dt, precision, constraints)

    def _constrained(self, constraints: ChainConstraints, E: int, K: int):
        """The ``<constraints>`` arguments of a constrained chain as ctypes takes them, the four report arrays behind its outputs (None
        where the mechanism is off), and what the pointers point into."""
        a = chain_constraint_arguments(constraints, self.n_steps)
        weights, L, walls, repair, r_walls = a[1], a[12], a[13], a[6], a[11]
        args = a[:1] + (_ptr(weights),) + a[2:13] + (_ptr(walls) if L else None, a[14])
        report = ChainReport(_out((E, K, 2)) if weights is not None else None, _out((E, K, 4)) if repair else None,
                             _out((E, 3), np.int32) if repair else None, _out((E, K, 2)) if r_walls else None)
        return args, report, (weights, walls)

    def _predict(self, n_agents, x_st, nbr_sum, edge_mask, x_T, p0, k, dt, precision, constraints=None):
        E, KA, T, _ = (int(v) for v in x_T.shape)
        A = int(p0.shape[1])
        K = KA // A
        if tuple(x_st.shape) != (E * A, self.hist_len, 6) or tuple(nbr_sum.shape) != (E * A, 2, self.hist_len, 6) \
                or tuple(edge_mask.shape) != (E * A, 2) or KA != K * A or tuple(p0.shape) != (E, A, 2):
            raise ValueError("bad predict() input shapes")
        b = [_Buf(a, False) for a in (x_st, nbr_sum, edge_mask, x_T, p0)]
        na = agent_counts(n_agents, E) if n_agents is not None else None
        if constraints is not None:
            fn, head = self._lib.jmid_predict_constrained, (self._h, E, A, K, T, int(k), _ptr(na))
        elif na is not None:
            fn, head = self._lib.jmid_predict_padded, (self._h, E, A, K, T, int(k), _ptr(na))
        else:
            fn, head = self._lib.jmid_predict, (self._h, E, A, K, T, int(k))
        return self._ranked_or_all(fn, (*head, *[x.ptr for x in b], float(dt), _lib.PRECISIONS[precision]), E, A, K, T, k, constraints)

    def _ranked_or_all(self, fn, args, E: int, A: int, K: int, T: int, k: int, constraints: Optional[ChainConstraints] = None):
        """The output half of a chained predictor entry (``args`` = everything in front of it): k < K -> the joint-KDE top-k, (kept
        [E, A, k, T, 2], log-weights [E, A, k]); k == K -> every sample, (pos [E, K, A, T, 2], None).  ``constraints`` (``fn`` is then the
        constrained entry): its arguments go between bw and the outputs, its report arrays behind them, and the ``ChainReport`` is the
        third value."""
        mid, tail, report = (), (), None
        if constraints is not None:
            mid, report, _keep = self._constrained(constraints, E, K)
            tail = tuple(_ptr(r) for r in report)
        more = () if report is None else (report,)
        if k < K:
            bw, sel, lw = kde_bandwidths(T), _out((E, A, k, T, 2)), _out((E, A, k))
            self._compute(fn, *args, _ptr(bw), *mid, _ptr(sel), _ptr(lw), None, *tail)
            return (sel, lw) + more
        pos = _out((E, K, A, T, 2))
        self._compute(fn, *args, None, *mid, None, None, _ptr(pos), *tail)
        return (pos, None) + more

    def build_scene(self, human_xy: np.ndarray, robot_xy: np.ndarray, time_step: float, horizon: Optional[int] = None,
                    force_all_in_cluster: bool = False, first_frame=None, allow_absent: bool = False) -> Dict[str, np.ndarray]:
        """The scene batch on the device (``jmid_build_scene``; the device twin of ``scene.build_scenes_batched``): human_xy [E, F, N, 2]
        and robot_xy [E, F, 2] float64 on the ``time_step`` grid, oldest first - or [F, N, 2] and [F, 2] for one scene, whose results
        then come without the episode axis.  The encoder inputs stay on the device (``scene_arrays`` copies them out, ``predict_scene``
        runs the predictor on them); returned are ``in_cluster`` [E, N] bool, ``robot_in_cluster`` [E] bool, ``n_in`` [E] int32 and
        ``cv`` [E, N, horizon, 2] float64 (None without ``horizon``).
        ``first_frame`` [E, N + 1] integers, robot first (``jmid_build_scene_var``; ``scene.build_scenes_batched(first_frame=)`` is the
        host twin): node j is present on frames first_frame[j] .. F-1 and its earlier positions are never read.  A pedestrian with a single
        frame is no ego row (``in_cluster`` False, not counted in ``n_in``).  ``scene_arrays`` then returns ``first_index`` as well and
        ``predict_scene`` / ``forecast_scene`` encode every row from its own first frame.
        ``allow_absent=True`` (``jmid_build_scene_absent``; ``scene.build_scenes_batched(allow_absent=True)`` is the host twin): a
        pedestrian's ``first_frame`` may be -1 - he is not in the scene of that episode: never read, ``in_cluster`` False, NaN rows in
        ``scene_arrays``, ``cv`` and the forecasts, ``first_index`` -1, and everybody else as if his column were removed."""
        hum = np.ascontiguousarray(human_xy, dtype=np.float64)
        rob = np.ascontiguousarray(robot_xy, dtype=np.float64)
        single = hum.ndim == 3
        if single:
            hum, rob = hum[None], rob[None]
        if hum.ndim != 4 or hum.shape[-1] != 2 or rob.shape != (hum.shape[0], hum.shape[1], 2):
            raise ValueError("expected human_xy [E, F, N, 2] and robot_xy [E, F, 2] (or one scene without the episode axis)")
        E, F, N, _ = (int(v) for v in hum.shape)
        inc = np.empty((E, N), dtype=np.uint8)
        rin = np.empty(E, dtype=np.uint8)
        n_in = np.empty(E, dtype=np.int32)
        cv = np.empty((E, N, int(horizon), 2), dtype=np.float64) if horizon is not None else None
        tail = (float(time_step), int(horizon) if horizon is not None else 0, int(bool(force_all_in_cluster)),
                C.c_void_p(inc.ctypes.data), C.c_void_p(rin.ctypes.data), C.c_void_p(n_in.ctypes.data),
                C.c_void_p(cv.ctypes.data) if cv is not None else None, _lib.MEM_HOST)
        if first_frame is not None:
            ff = np.asarray(first_frame)
            if not np.issubdtype(ff.dtype, np.integer) or ff.shape != ((N + 1,) if single else (E, N + 1)):
                raise ValueError("first_frame must hold N + 1 integers per episode, robot first")
            ff = np.ascontiguousarray(ff.reshape(E, N + 1), dtype=np.int32)
            entry = self._lib.jmid_build_scene_absent if allow_absent else self._lib.jmid_build_scene_var
            self._check(entry(self._h, E, N, F, C.c_void_p(hum.ctypes.data), C.c_void_p(rob.ctypes.data), C.c_void_p(ff.ctypes.data), *tail))
        elif allow_absent:
            raise ValueError("allow_absent needs first_frame")
        else:
            self._check(self._lib.jmid_build_scene(self._h, E, N, F, C.c_void_p(hum.ctypes.data), C.c_void_p(rob.ctypes.data), *tail))
        self._scene_shape, self._scene_n_in = (E, N, F, single), n_in
        out = {"in_cluster": inc.astype(bool), "robot_in_cluster": rin.astype(bool), "n_in": n_in, "cv": cv}
        return {k: (v[0] if single and v is not None else v) for k, v in out.items()}

    def scene_arrays(self) -> Dict[str, np.ndarray]:
        """The arrays the preceding ``build_scene`` left on the device, under the keys of ``scene.build_scenes_batched``: x, x_st
        [E, N, F, 6], nbr_sum [E, N, 2, F, 6], edge_mask [E, N, 2], p0 [E, N, 2] float32 (``jmid_scene_get``; every pedestrian has a row)
        and first_index [E, N] int32 (``jmid_scene_get_first_index``; zeros unless the scene was built with ``first_frame``).
        After a one-scene ``build_scene`` the episode axis is absent."""
        shape = getattr(self, "_scene_shape", None)
        E, N, F, single = shape if shape is not None else (0, 0, self.hist_len, False)      # (no build: the library says so)
        out = {"x": np.empty((E, N, F, 6), np.float32), "x_st": np.empty((E, N, F, 6), np.float32),
               "nbr_sum": np.empty((E, N, 2, F, 6), np.float32), "edge_mask": np.empty((E, N, 2), np.float32),
               "p0": np.empty((E, N, 2), np.float32)}
        self._check(self._lib.jmid_scene_get(self._h, *[C.c_void_p(a.ctypes.data) for a in out.values()], _lib.MEM_HOST))
        out["first_index"] = np.empty((E, N), np.int32)
        self._check(self._lib.jmid_scene_get_first_index(self._h, C.c_void_p(out["first_index"].ctypes.data), _lib.MEM_HOST))
        return {k: v[0] for k, v in out.items()} if single else out

    def _scene_noise(self, x_T, seed, episode_ids, K, T, padded=False):
        """What predict_scene / forecast_scene and their padded forms share: (E, A, K, T, the library entry's name suffix, its noise
        arguments, and the array those point into - the caller keeps it alive over the call)."""
        # A = the first episode's count (the library refuses the call when another episode's differs, or when nothing is resident);
        # padded: the largest count
        n_in = getattr(self, "_scene_n_in", None)
        A = int(n_in.max() if padded else n_in[0]) if n_in is not None and len(n_in) else 0
        A = max(A, 1)
        seeded = seeded_noise_args(x_T, seed, episode_ids)
        if seeded is not None:
            if K is None or T is None:
                raise ValueError("a seeded call needs K and T")
            return int(seeded[1].size), A, int(K), int(T), "_seeded", (seeded[0], C.c_void_p(seeded[1].ctypes.data)), seeded[1]
        x_T = np.asarray(x_T)
        if x_T.ndim != 4 or x_T.shape[-1] != 2:
            raise ValueError("expected x_T [E, K*A, T, 2]")
        E, KA, T, _ = (int(v) for v in x_T.shape)
        if KA % A != 0:
            raise ValueError(f"x_T has {KA} rows per episode: not a multiple of the scene's {A} in-cluster pedestrians")
        bx = _Buf(x_T, False)
        return E, A, KA // A, T, "", (bx.ptr,), bx

    @staticmethod
    def _constrained_noise(sfx, nz):
        """The noise arguments of a constrained scene chain (x_T, seed, episode_ids) from ``_scene_noise``'s: x_T NULL selects the seeded form."""
        return (None, *nz) if sfx else (*nz, 0, None)

    def predict_scene(self, x_T: Optional[np.ndarray], k: int, dt: float = 0.25, precision: str = "f32", seed: Optional[int] = None,
                      episode_ids=None, K: Optional[int] = None, T: Optional[int] = None, constraints: Optional[ChainConstraints] = None):
        """``predict`` on the scene the preceding ``build_scene`` left on the device (``jmid_predict_scene``): x_T [E, K*A, T, 2] with A the
        in-cluster count of EVERY episode (``n_in``) and ``k`` kept futures of the K.  k < K -> (kept [E, A, k, T, 2], log-weights
        [E, A, k]); k == K -> (pos [E, K, A, T, 2], None).  The same bits as ``predict`` fed the in-cluster rows of ``scene_arrays``.
        ``seed`` + ``episode_ids`` [E] with ``x_T=None``, ``K`` and ``T``: x_T is drawn on the device (``jmid_predict_scene_seeded``).
        ``constraints`` (``jmid_predict_scene_constrained``): as ``predict`` - guidance and repair inside the one call, a third value."""
        return self._predict_scene(False, x_T, k, dt, precision, seed, episode_ids, K, T, constraints)

    def _predict_scene(self, padded, x_T, k, dt, precision, seed, episode_ids, K, T, constraints):
        E, A, K, T, sfx, nz, _keep = self._scene_noise(x_T, seed, episode_ids, K, T, padded)
        k = int(k)
        if constraints is not None:
            head = (self._h, E, A, K, T, k, int(padded), *self._constrained_noise(sfx, nz))
            return self._ranked_or_all(self._lib.jmid_predict_scene_constrained, (*head, float(dt), _lib.PRECISIONS[precision]), E, A, K, T, k,
                                       constraints)
        fn = getattr(self._lib, ("jmid_predict_scene_padded" if padded else "jmid_predict_scene") + sfx)
        return self._ranked_or_all(fn, (self._h, E, A, K, T, k, *nz, float(dt), _lib.PRECISIONS[precision]), E, A, K, T, k)

    def predict_scene_padded(self, x_T: Optional[np.ndarray], k: int, dt: float = 0.25, precision: str = "f32", seed: Optional[int] = None,
                             episode_ids=None, K: Optional[int] = None, T: Optional[int] = None,
                             constraints: Optional[ChainConstraints] = None):
        """``predict_scene`` for a resident scene of MIXED in-cluster counts, in one call (``jmid_predict_scene_padded``): A = the largest
        ``n_in``, x_T [E, K*A, T, 2] in the padded layout (row s*A + a real iff a < n_in[e]; the others are never read), the results of
        ``predict_padded`` fed the gathered rows of ``scene_arrays`` - NaN in the padded rows.  Every ``n_in`` must be at least 1.
        ``seed`` + ``episode_ids`` [E] with ``x_T=None``, ``K`` and ``T`` (``jmid_predict_scene_padded_seeded``): every episode draws what it
        draws alone at its own count, ``noise(seed, episode_ids, K * A, T, n_agents=n_in)``.  ``constraints``: as ``predict_scene``."""
        return self._predict_scene(True, x_T, k, dt, precision, seed, episode_ids, K, T, constraints)

    def forecast_scene_padded(self, x_T: Optional[np.ndarray], k: int, dt: float = 0.25, precision: str = "f32", seed: Optional[int] = None,
                              episode_ids=None, K: Optional[int] = None, T: Optional[int] = None,
                              constraints: Optional[ChainConstraints] = None):
        """``forecast_scene`` for a resident scene of mixed in-cluster counts (``jmid_forecast_scene_padded`` /
        ``jmid_forecast_scene_padded_seeded``): the arguments of ``predict_scene_padded``, the results of ``forecast_scene`` - no NaN: an
        in-cluster pedestrian reads its own row, everybody else the constant-velocity row.  ``constraints``: as ``forecast_scene``."""
        return self._forecast_scene("jmid_forecast_scene_padded", True, x_T, k, dt, precision, seed, episode_ids, K, T, constraints)

    def build_scene_stamped(self, stamps: np.ndarray, human_xy: np.ndarray, robot_xy: np.ndarray, time_step: float,
                            horizon: Optional[int] = None, force_all_in_cluster: bool = False,
                            n_frames: Optional[np.ndarray] = None, tracks: bool = False,
                            max_coast: Optional[int] = None) -> Dict[str, np.ndarray]:
        """``build_scene`` from raw stamped frames (``jmid_build_scene_stamped``; the frame table is the device twin of
        ``scene.frame_table_frames_batched``): stamps [E, R], human_xy [E, R, N, 2], robot_xy [E, R, 2] float64, oldest-pushed first, the
        first ``n_frames[e]`` of each episode valid (None: all R) - or [R], [R, N, 2], [R, 2] for one scene, whose results then come without
        the episode axis.  Returns what ``build_scene`` returns plus ``n_grid`` [E] int32.  Raises ``scene.HistoryTooShortError`` when an
        episode has fewer than ``hist_len`` frames on the grid (JMID_EHISTORY; a scene built before stays resident).
        ``tracks=True`` (``jmid_build_scene_stamped_var``; the device twin of ``scene.frame_table_tracks_batched``): a history window per
        track - a NaN human coordinate means "not seen in this frame" and drops nothing, a window of 2 .. hist_len-1 grid frames is built
        like ``build_scene(first_frame=)`` - and ``first_frame`` [E, N + 1] int32 (robot first) is returned as well.
        ``HistoryTooShortError`` then means fewer than 2 grid frames; a pedestrian who is not seen in the newest kept frame raises
        ``scene.TrackAbsentError(episode, track)`` (leave the track out; a scene built before stays resident).
        ``max_coast`` = 0 .. hist_len-2 (with ``tracks=True``; ``jmid_build_scene_stamped_coast``, the device twin of
        ``scene.frame_table_tracks_batched(max_coast=)``): such a pedestrian is coasted to the anchor frame over at most ``max_coast`` bins,
        or left out of the scene (``first_frame`` -1, NaN rows) - nothing is raised for him, and ``coast`` [E, N] int32 is returned as
        well (0 seen, b > 0 coasted over b bins, -1 left out).  An episode with nobody left raises ``JmidError`` (JMID_EINVAL)."""
        from .scene import HistoryTooShortError, TrackAbsentError
        if max_coast is not None and not tracks:
            raise ValueError("max_coast needs tracks=True")
        st = np.ascontiguousarray(stamps, dtype=np.float64)
        hum = np.ascontiguousarray(human_xy, dtype=np.float64)
        rob = np.ascontiguousarray(robot_xy, dtype=np.float64)
        single = hum.ndim == 3
        if single:
            st, hum, rob = st[None], hum[None], rob[None]
        if hum.ndim != 4 or hum.shape[-1] != 2 or rob.shape != (hum.shape[0], hum.shape[1], 2) or st.shape != hum.shape[:2]:
            raise ValueError("expected stamps [E, R], human_xy [E, R, N, 2] and robot_xy [E, R, 2] (or one scene without the episode axis)")
        E, R, N, _ = (int(v) for v in hum.shape)
        nf = None
        if n_frames is not None:
            nf = np.ascontiguousarray(np.atleast_1d(n_frames), dtype=np.int32)
            if nf.shape != (E,):
                raise ValueError("n_frames must hold one count per episode")
        inc = np.empty((E, N), dtype=np.uint8)
        rin = np.empty(E, dtype=np.uint8)
        n_in = np.empty(E, dtype=np.int32)
        n_grid = np.zeros(E, dtype=np.int32)         # (zeros: a refusal in front of the kernel leaves them, and is then no absent-now one)
        cv = np.empty((E, N, int(horizon), 2), dtype=np.float64) if horizon is not None else None
        head = (self._h, E, N, R, C.c_void_p(st.ctypes.data), C.c_void_p(hum.ctypes.data), C.c_void_p(rob.ctypes.data),
                C.c_void_p(nf.ctypes.data) if nf is not None else None, float(time_step),
                int(horizon) if horizon is not None else 0, int(bool(force_all_in_cluster)),
                C.c_void_p(inc.ctypes.data), C.c_void_p(rin.ctypes.data), C.c_void_p(n_in.ctypes.data),
                C.c_void_p(n_grid.ctypes.data), C.c_void_p(cv.ctypes.data) if cv is not None else None)
        first = coast = None
        if max_coast is not None:
            first, coast = np.zeros((E, N + 1), dtype=np.int32), np.zeros((E, N), dtype=np.int32)
            rc = self._lib.jmid_build_scene_stamped_coast(*head, C.c_void_p(first.ctypes.data), int(max_coast), C.c_void_p(coast.ctypes.data),
                                                          _lib.MEM_HOST)
        elif tracks:
            first = np.zeros((E, N + 1), dtype=np.int32)
            rc = self._lib.jmid_build_scene_stamped_var(*head, C.c_void_p(first.ctypes.data), _lib.MEM_HOST)
        else:
            rc = self._lib.jmid_build_scene_stamped(*head, _lib.MEM_HOST)
        if rc == _lib.EHISTORY:
            err = HistoryTooShortError(self._lib.jmid_last_error(self._h).decode())
            err.n_grid = n_grid[0] if single else n_grid
            raise err
        if tracks and coast is None and rc == _lib.EINVAL and (n_grid >= 2).all() and (first < 0).any():     # the absent-now refusal: both arrays were filled
            e, j = (int(v[0]) for v in np.nonzero(first < 0))
            err = TrackAbsentError(e, j - 1, f"JMID_EINVAL: {self._lib.jmid_last_error(self._h).decode()}")
            err.first_frame = first[0] if single else first
            raise err
        self._check(rc)
        self._scene_shape, self._scene_n_in = (E, N, self.hist_len, single), n_in
        out = {"in_cluster": inc.astype(bool), "robot_in_cluster": rin.astype(bool), "n_in": n_in, "n_grid": n_grid, "cv": cv}
        if tracks:
            out["first_frame"] = first
        if coast is not None:
            out["coast"] = coast
        return {k: (v[0] if single and v is not None else v) for k, v in out.items()}

    def scene_frames(self) -> Dict[str, np.ndarray]:
        """The grid the resident scene was built from and its current pose (``jmid_scene_get_frames``): ``human_xy`` [E, F, N, 2],
        ``robot_xy`` [E, F, 2], ``pose_now`` [E, N, 2] float64 - after ``build_scene_stamped`` the frame table of ``scene.frame_table``,
        after ``build_scene`` its own input and the last frame.  After a one-scene build the episode axis is absent."""
        shape = getattr(self, "_scene_shape", None)
        E, N, F, single = shape if shape is not None else (0, 0, self.hist_len, False)      # (no build: the library says so)
        out = {"human_xy": np.empty((E, F, N, 2), np.float64), "robot_xy": np.empty((E, F, 2), np.float64),
               "pose_now": np.empty((E, N, 2), np.float64)}
        self._check(self._lib.jmid_scene_get_frames(self._h, *[C.c_void_p(a.ctypes.data) for a in out.values()], _lib.MEM_HOST))
        return {k: v[0] for k, v in out.items()} if single else out

    def forecast_scene(self, x_T: Optional[np.ndarray], k: int, dt: float = 0.25, precision: str = "f32", seed: Optional[int] = None,
                       episode_ids=None, K: Optional[int] = None, T: Optional[int] = None, constraints: Optional[ChainConstraints] = None):
        """``predict_scene`` followed by the result assembly on the device (``jmid_forecast_scene``; the twin of
        ``scene.assemble_forecasts``): x_T [E, K*A, T, 2] -> (forecasts [E, N, k, T+1, 2], log-weights [E, N, k]) float64, per episode
        exactly what ``predict_ret_best()`` returns.  The resident scene must have been built with ``horizon`` = T.  After a one-scene
        build the episode axis of the results is absent.  ``seed`` + ``episode_ids`` [E] with ``x_T=None``, ``K`` and ``T``: x_T is
        drawn on the device (``jmid_forecast_scene_seeded``).  ``constraints`` (``jmid_forecast_scene_constrained``): guidance and repair
        inside the one call - the ranking and the assembly read the guided, repaired set - and a third value, the ``ChainReport``."""
        return self._forecast_scene("jmid_forecast_scene", False, x_T, k, dt, precision, seed, episode_ids, K, T, constraints)

    def _forecast_scene(self, entry, padded, x_T, k, dt, precision, seed, episode_ids, K, T, constraints=None):
        E, A, K, T, sfx, nz, _keep = self._scene_noise(x_T, seed, episode_ids, K, T, padded)
        k = int(k)
        shape = getattr(self, "_scene_shape", None)
        N, single = (shape[1], shape[3]) if shape is not None else (1, False)
        bw = kde_bandwidths(T) if k < K else None
        fc, lw = _out((E, N, max(k, 0), T + 1, 2), np.float64), _out((E, N, max(k, 0)), np.float64)
        if constraints is not None:
            mid, report, _keep2 = self._constrained(constraints, E, K)
            self._compute(self._lib.jmid_forecast_scene_constrained, self._h, E, A, K, T, k, int(padded), *self._constrained_noise(sfx, nz),
                          float(dt), _lib.PRECISIONS[precision], _ptr(bw), *mid, _ptr(fc), _ptr(lw), *[_ptr(r) for r in report])
            return (fc[0], lw[0], report) if single else (fc, lw, report)
        fn = getattr(self._lib, entry + sfx)
        self._compute(fn, self._h, E, A, K, T, k, *nz, float(dt), _lib.PRECISIONS[precision], _ptr(bw), _ptr(fc), _ptr(lw))
        return (fc[0], lw[0]) if single else (fc, lw)

    def net_eval(self, x: ArrayLike, ctx: ArrayLike, step_idx: int = 0, precision: str = "f32", n_agents=None):
        """One evaluation of e_theta for DDIM table entry ``step_idx``; x [E, K*A, T, 2] -> e same shape.  ``n_agents`` [E]
        (``jmid_net_eval_padded``): rows of agents a >= n_agents[e] are padding, NaN in e."""
        dev = _is_cuda(x)
        E, A, K, T = self._shapes(x, ctx)
        bx, bc = _Buf(x, dev), _Buf(ctx, dev)
        out = _out(tuple(x.shape), device=x.device if dev else None)
        if n_agents is not None:
            na = agent_counts(n_agents, E)
            self._compute(self._lib.jmid_net_eval_padded, self._h, E, A, K, T, _ptr(na), int(step_idx), bx.ptr, bc.ptr,
                          _lib.PRECISIONS[precision], _ptr(out), self._mem(dev))
            return out
        self._compute(self._lib.jmid_net_eval, self._h, E, A, K, T, int(step_idx), bx.ptr, bc.ptr, _lib.PRECISIONS[precision], _ptr(out),
                      self._mem(dev))
        return out

    def set_loss_schedule(self, schedule: Optional[VarianceSchedule] = None) -> None:
        """Install the forward process per timestep (``jmid_set_loss_schedule``; ``schedule.loss_tables``) - ``loss`` does it from
        ``self.schedule`` on first use.  Independent of ``set_step``."""
        tabs = loss_tables(schedule or self.schedule)
        self._check(self._lib.jmid_set_loss_schedule(self._h, len(tabs[0]), *[C.c_void_p(c.ctypes.data) for c in tabs]))
        self._loss_schedule = True

    def loss(self, x0: ArrayLike, ctx: ArrayLike, t, e: Optional[ArrayLike] = None, seed: Optional[int] = None, episode_ids=None,
             n_agents=None, precision: str = "f32", want_rows: bool = False, want_e_theta: bool = False) -> "LossResult":
        """The reference's denoising loss (``jmid_loss``; ``DiffusionTraj.get_loss``, MID/models/diffusion.py:448-476): one net
        evaluation with every agent row at its own timestep.  x0 [E, A, T, 2] (the recorded futures), ctx [E, A, ctx_dim], t int [E, A]
        in 1..num_steps (always a host array), and exactly one of ``e`` [E, A, T, 2] (the noise) or ``seed`` + ``episode_ids`` [E]
        (``jmid_loss_seeded``: e is ``noise(seed, episode_ids, A, T, 0)``).  ``n_agents`` [E]: a padded batch - the rows of agents
        a >= n_agents[e] are masked as attention keys and dropped from the loss (NaN in ``rows`` and ``e_theta``).
        -> ``LossResult``: ``loss`` (mean squared error over the real rows' T * 2 components), ``count`` (their number), ``rows`` [E, A]
        float64 sum of squared errors per row (``want_rows``), ``e_theta`` [E, A, T, 2] (``want_e_theta``).  NumPy in -> NumPy out (and
        ``loss`` a float, ``count`` an int); CUDA tensors in -> CUDA tensors out (``loss`` and ``count`` 0-d float64 tensors)."""
        if (e is None) == (seed is None):
            raise ValueError("exactly one of e and seed must be given")
        dev = _is_cuda(x0)
        if x0.ndim != 4 or ctx.ndim != 3:
            raise ValueError("expected x0 [E, A, T, 2] and ctx [E, A, ctx_dim]")
        E, A, K, T = self._shapes(x0, ctx)
        if K != 1:
            raise ValueError("x0 must hold one row per agent: [E, A, T, 2]")
        tt = np.ascontiguousarray(np.asarray(t.cpu() if torch is not None and torch.is_tensor(t) else t), dtype=np.int32)
        if tt.size != E * A:
            raise ValueError(f"t must hold one timestep per agent row ({E * A}), got {tt.size}")
        seeded = seeded_noise_args(None, seed, episode_ids, E) if seed is not None else None
        if e is not None and (_is_cuda(e) != dev or tuple(e.shape) != tuple(x0.shape)):
            raise ValueError("e must have x0's shape and live where x0 lives")
        if not getattr(self, "_loss_schedule", False):
            self.set_loss_schedule()
        bx, bc = _Buf(x0, dev), _Buf(ctx, dev)
        be = _Buf(e, dev) if e is not None else None
        na = agent_counts(n_agents, E) if n_agents is not None else None
        where = x0.device if dev else None
        out = _out((2,), np.float64, where)
        rows = _out((E, A), np.float64, where) if want_rows else None
        eth = _out((E, A, T, 2), device=where) if want_e_theta else None
        head = (self._h, E, A, T, _ptr(na), _ptr(tt), bx.ptr)
        tail = (bc.ptr, _lib.PRECISIONS[precision], _ptr(out), _ptr(rows), _ptr(eth), self._mem(dev))
        if seeded is not None:
            self._compute(self._lib.jmid_loss_seeded, *head, seeded[0], _ptr(seeded[1]), *tail)
        else:
            self._compute(self._lib.jmid_loss, *head, be.ptr, *tail)
        if dev:
            return LossResult(out[0], out[1], rows, eth)
        return LossResult(float(out[0]), int(out[1]), rows, eth)

    def episode_metrics(self, pos: ArrayLike, gt: ArrayLike) -> ArrayLike:
        """pos [E,K,A,T,2], gt [E,A,T,2] -> [E,4] = (mean ADE, joint min ADE, mean FDE, joint min FDE)."""
        dev = _is_cuda(pos)
        E, K, A, T, _ = (int(v) for v in pos.shape)
        if tuple(gt.shape) != (E, A, T, 2):
            raise ValueError("gt must be [E, A, T, 2]")
        bp, bg = _Buf(pos, dev), _Buf(gt, dev)
        out = _out((E, 4), device=pos.device if dev else None)
        self._check(self._lib.jmid_episode_metrics(self._h, E, A, K, T, bp.ptr, bg.ptr, _ptr(out), self._mem(dev)))
        return out

    def eval_statistics(self, pos: Optional[ArrayLike], gt: ArrayLike, dims: Optional[Tuple[int, int, int, int]] = None):
        """The reference's evaluation statistics on the device (``jmid_eval_statistics``; compute_batch_statistics,
        MID/evaluation/evaluation.py:456-739).  pos [E, K, A, T, 2], gt [E, A, T, 2] -> (agent [E, A, 10], scene [E, 6]) with the
        columns ``metrics.STAT_AGENT_COLUMNS`` / ``metrics.STAT_SCENE_COLUMNS``; NumPy in -> NumPy out, CUDA tensors in -> CUDA tensors
        out.  ``pos=None`` with ``dims=(E, A, K, T)`` scores the positions of the preceding ``denoise`` call, which are still in the
        engine's workspace (``gt`` then decides where the outputs live).  2 <= K <= 1024, T <= 24: ``metrics.eval_statistics_host``
        beyond."""
        dev = _is_cuda(gt)
        if pos is None:
            if dims is None:
                raise ValueError("pos=None needs dims=(E, A, K, T) of the preceding denoise call")
            E, A, K, T = (int(v) for v in dims)
            bp = None
        else:
            if _is_cuda(pos) != dev:
                raise TypeError("pos and gt must both be CUDA/HIP tensors or both host arrays")
            E, K, A, T, _ = (int(v) for v in pos.shape)
            bp = _Buf(pos, dev)
        if tuple(gt.shape) != (E, A, T, 2):
            raise ValueError("gt must be [E, A, T, 2]")
        bg = _Buf(gt, dev)
        where = gt.device if dev else None
        agent, scene = _out((E, A, 10), device=where), _out((E, 6), device=where)
        self._check(self._lib.jmid_eval_statistics(self._h, E, A, K, T, bp.ptr if bp is not None else None, bg.ptr, _ptr(agent), _ptr(scene),
                                                   self._mem(dev)))
        return agent, scene

    def eval_statistics_masked(self, pos: Optional[ArrayLike], gt: ArrayLike, interp_future: ArrayLike,
                               interp_history: Optional[ArrayLike] = None, cutoffs=(2, 5, 8),
                               dims: Optional[Tuple[int, int, int, int]] = None):
        """The masked form of ``eval_statistics`` (``jmid_eval_statistics_masked``; the ``is_eval_hst`` branch of
        compute_batch_statistics, MID/evaluation/evaluation.py:540-715): pos [E, K, A, T, 2] (or None with ``dims``, as there),
        gt [E, A, T, 2], interp_future [E, A, T] bool (True = the step's ground truth is not real: not scored), interp_history
        [E, A, F] bool or None (an agent whose history is all True is left out) -> (agent [E, A, 12], cut [E, A, len(cutoffs), 5],
        scene [E, 6]) with the columns ``metrics.STAT_MASKED_AGENT_COLUMNS`` / ``STAT_CUTOFF_COLUMNS`` / ``STAT_SCENE_COLUMNS``.
        NumPy in -> NumPy out, CUDA tensors in -> CUDA tensors out (the masks follow ``gt``).  At most 4 cut-off steps, each in
        [0, T); 2 <= K <= 1024, T <= 24: ``metrics.eval_statistics_masked_host`` beyond."""
        dev = _is_cuda(gt)
        if pos is None:
            if dims is None:
                raise ValueError("pos=None needs dims=(E, A, K, T) of the preceding denoise call")
            E, A, K, T = (int(v) for v in dims)
            bp = None
        else:
            if _is_cuda(pos) != dev:
                raise TypeError("pos and gt must both be CUDA/HIP tensors or both host arrays")
            E, K, A, T, _ = (int(v) for v in pos.shape)
            bp = _Buf(pos, dev)
        if tuple(gt.shape) != (E, A, T, 2):
            raise ValueError("gt must be [E, A, T, 2]")
        if tuple(interp_future.shape) != (E, A, T):
            raise ValueError("interp_future must be [E, A, T]")
        if interp_history is not None and tuple(interp_history.shape[:2]) != (E, A):
            raise ValueError("interp_history must be [E, A, F]")
        if _is_cuda(interp_future) != dev or (interp_history is not None and _is_cuda(interp_history) != dev):
            raise TypeError("the masks must live where gt lives")
        cuts = (C.c_int * max(len(cutoffs), 1))(*[int(c) for c in cutoffs])
        n_cut = len(cutoffs)
        bg = _Buf(gt, dev)
        if dev:
            fut = (interp_future != 0).to(torch.uint8).contiguous()
            skip = (interp_history != 0).reshape(E, A, -1).all(dim=-1).to(torch.uint8).contiguous() if interp_history is not None else None
        else:
            to_np = lambda m: m.detach().cpu().numpy() if torch is not None and isinstance(m, torch.Tensor) else np.asarray(m)
            fut = np.ascontiguousarray(to_np(interp_future) != 0, dtype=np.uint8)
            skip = (np.ascontiguousarray((to_np(interp_history) != 0).reshape(E, A, -1).all(axis=-1), dtype=np.uint8)
                    if interp_history is not None else None)
        where = gt.device if dev else None
        agent, cut, scene = _out((E, A, 12), device=where), _out((E, A, n_cut, 5), device=where), _out((E, 6), device=where)
        ptr = lambda t: _ptr(t) if t is not None and (t.numel() if dev else t.size) else None      # (an empty array goes as NULL)
        self._check(self._lib.jmid_eval_statistics_masked(self._h, E, A, K, T, bp.ptr if bp is not None else None, bg.ptr, ptr(fut),
                                                          ptr(skip), n_cut, cuts, ptr(agent), ptr(cut), ptr(scene), self._mem(dev)))
        return agent, cut, scene

    def collision_statistics(self, pos: Optional[ArrayLike], threshold: float = 0.2,
                             dims: Optional[Tuple[int, int, int, int]] = None, pairs: bool = False, agents: bool = True, n_agents=None):
        """Collision statistics of joint samples on the device (``jmid_collision_statistics``; calc_min_dists and
        get_agents_in_collision, MID/models/collision_check_utils.py:58-97).  pos [E, K, A, T, 2] -> (pair [E, K, P] or None,
        agent [E, K, A] uint8 or None, sample [E, K, 4], scene [E, 5]) with the columns ``metrics.COLLISION_SAMPLE_COLUMNS`` /
        ``metrics.COLLISION_SCENE_COLUMNS``; ``pairs`` / ``agents`` choose whether the first two are computed.  NumPy in -> NumPy out,
        CUDA tensors in -> CUDA tensors out.  ``pos=None`` with ``dims=(E, A, K, T)`` takes the positions of the preceding ``denoise``
        call, which are still in the engine's workspace (host arrays out).  Ground-truth futures: ``gt[:, None]`` (K = 1).
        K <= 1024, 2 <= T <= 24, A <= 64: ``metrics.collision_statistics_host`` beyond.
        ``n_agents`` [E] (``jmid_collision_statistics_padded``): episode e has n_agents[e] <= A real agents; every value of the episode is
        what the plain call gives for its compacted block, a pair with a padded agent is NaN at its index at A and counts nowhere, a padded
        agent's byte is 0, agent_collision_rate divides by K * n_agents[e].  Padded rows of pos are never read."""
        if pos is None:
            if dims is None:
                raise ValueError("pos=None needs dims=(E, A, K, T) of the preceding denoise call")
            E, A, K, T = (int(v) for v in dims)
            dev, bp = False, None
        else:
            dev = _is_cuda(pos)
            E, K, A, T, _ = (int(v) for v in pos.shape)
            bp = _Buf(pos, dev)
        shapes = (((E, K, A * (A - 1) // 2), np.float32) if pairs else None, ((E, K, A), np.uint8) if agents else None,
                  ((E, K, 4), np.float32), ((E, 5), np.float32))
        outs = [_out(*s, pos.device if dev else None) if s else None for s in shapes]
        if n_agents is not None:
            na = agent_counts(n_agents, E)
            self._check(self._lib.jmid_collision_statistics_padded(self._h, E, A, K, T, _ptr(na), bp.ptr if bp is not None else None,
                                                                   float(threshold), *[_ptr(o) for o in outs], self._mem(dev)))
            return tuple(outs)
        self._check(self._lib.jmid_collision_statistics(self._h, E, A, K, T, bp.ptr if bp is not None else None, float(threshold),
                                                        *[_ptr(o) for o in outs], self._mem(dev)))
        return tuple(outs)

    def repair_collisions(self, pos: Optional[ArrayLike], threshold: float = 0.2, margin: float = 0.02, tau: float = 0.005, step: float = 0.02,
                          max_iter: int = 32, p0: Optional[ArrayLike] = None, dt: float = 0.25, vel: Optional[ArrayLike] = None,
                          dims: Optional[Tuple[int, int, int, int]] = None, n_agents=None, want_pos: Optional[bool] = None, walls=None,
                          wall_radius: Optional[float] = None):
        """Collision repair on the device (``jmid_repair_collisions``; the rule stands in include/jmid_hip.h, its host twin is
        ``metrics.repair_collisions_host``): every joint sample of pos [E, K, A, T, 2] in which ``collision_statistics`` counts a colliding
        agent at ``threshold`` is pushed apart under a softplus penalty until the predicate holds - a small fp64 optimisation on the
        finished samples, no net evaluation, no redraw, no download - and comes back either repaired (acceptable) or bit for bit as it
        went in.  -> (pos_out [E, K, A, T, 2] or None, vel_out or None, sample [E, K, 4] = ``metrics.REPAIR_SAMPLE_COLUMNS``,
        episode [E, 3] int32 = ``metrics.REPAIR_EPISODE_COLUMNS``).  NumPy in -> NumPy out, CUDA tensors in -> CUDA tensors out.
        ``vel`` [E, K, A, T, 2] with ``p0`` [E, A, 2] and ``dt``: the samples' velocities; a copy comes back in which the rows of the
        repaired samples are (x[t] - x[t - 1]) / dt, x[-1] = p0.
        ``pos=None`` with ``dims=(E, A, K, T)``: the set the preceding ``denoise`` / ``denoise_reject`` call left in the engine's workspace is
        repaired IN PLACE (with ``p0``, the accepted block's velocities too where it holds them): ``topk(None, ...)`` and the statistics
        entries then see the repaired set; pos_out is None unless ``want_pos=True`` (``p0`` / ``vel`` decide where the outputs live; host
        arrays without them).  ``n_agents`` [E]: a padded batch - padded agents take part in nothing and their rows pass through.
        ``walls`` [L, 4] or [L, 2, 2] (a host array, as for ``wall_statistics``) with ``wall_radius`` (``jmid_repair_collisions_walls``): the
        wall terms join the objective and the wall predicate at (walls, wall_radius, p0) joins both gates - a sample that hits a wall is a
        candidate too, a single agent included, and is kept only when both predicates accept it; ``p0`` is then the fixed first point of
        every path.  A fifth value comes back: wall [E, K, 2] = ``metrics.REPAIR_WALL_COLUMNS``.  No walls (L = 0): the four values above,
        bit for bit, and +inf in the fifth."""
        if walls is None and wall_radius is not None:
            raise ValueError("wall_radius is given without walls")
        if walls is not None and wall_radius is None:
            raise ValueError("walls need wall_radius (the repair knows no agent radius)")
        if pos is None:
            if dims is None:
                raise ValueError("pos=None needs dims=(E, A, K, T) of the preceding denoise call")
            E, A, K, T = (int(v) for v in dims)
            like = vel if vel is not None else p0
            dev, bp = like is not None and _is_cuda(like), None
            want_pos = bool(want_pos)
        else:
            dev, like = _is_cuda(pos), pos
            E, K, A, T, _ = (int(v) for v in pos.shape)
            bp = _Buf(pos, dev)
            want_pos = True if want_pos is None else bool(want_pos)
        if vel is not None and p0 is None:
            raise ValueError("vel needs p0 (a velocity's first step starts at the present position)")
        if p0 is not None and tuple(p0.shape) != (E, A, 2):
            raise ValueError("p0 must be [E, A, 2]")
        if vel is not None and tuple(vel.shape) != (E, K, A, T, 2):
            raise ValueError("vel must be [E, K, A, T, 2]")
        b0 = _Buf(p0, dev) if p0 is not None else None
        where = like.device if dev else None
        vel_out = None
        if vel is not None:      # in and out: the library rewrites the rows of the repaired samples in this copy
            bv = _Buf(vel, dev)
            vel_out = bv.keep.clone() if dev else np.array(bv.keep, dtype=np.float32, copy=True)
        pos_out = _out((E, K, A, T, 2), device=where) if want_pos else None
        sample, episode = _out((E, K, 4), device=where), _out((E, 3), np.int32, where)
        na = agent_counts(n_agents, E) if n_agents is not None else None
        if walls is not None:
            w = wall_segments(walls)
            wall = _out((E, K, 2), device=where)
            self._check(self._lib.jmid_repair_collisions_walls(self._h, E, A, K, T, _ptr(na), bp.ptr if bp is not None else None,
                                                               b0.ptr if b0 is not None else None, float(dt), float(threshold), float(margin),
                                                               float(tau), float(step), int(max_iter), int(w.shape[0]),
                                                               _ptr(w) if w.shape[0] else None, float(wall_radius), _ptr(pos_out), _ptr(vel_out),
                                                               _ptr(sample), _ptr(episode), _ptr(wall), self._mem(dev)))
            return pos_out, vel_out, sample, episode, wall
        self._check(self._lib.jmid_repair_collisions(self._h, E, A, K, T, _ptr(na), bp.ptr if bp is not None else None,
                                                     b0.ptr if b0 is not None else None, float(dt), float(threshold), float(margin), float(tau),
                                                     float(step), int(max_iter), _ptr(pos_out), _ptr(vel_out), _ptr(sample), _ptr(episode),
                                                     self._mem(dev)))
        return pos_out, vel_out, sample, episode

    def wall_statistics(self, pos: Optional[ArrayLike], walls, radius: float, p0: Optional[ArrayLike] = None,
                        dims: Optional[Tuple[int, int, int, int]] = None, n_agents=None):
        """Wall statistics of joint samples on the device (``jmid_wall_statistics``; the reference simulator's
        closest_distance_between_line_segments(wall, step) - radius < 0, include/jmid_hip.h states the definitions).  pos [E, K, A, T, 2],
        walls [L, 4] or [L, 2, 2] (a host array, ``crowd_env.static_obstacles(rule)[0]``), p0 [E, A, 2] or None (the step from the present
        position into the forecast is then walked too) -> (dist [E, K, A, L], agent [E, K, A] uint8, sample [E, K, 3], scene [E, 5]) with
        the columns ``metrics.WALL_SAMPLE_COLUMNS`` / ``metrics.WALL_SCENE_COLUMNS``.  NumPy in -> NumPy out, CUDA tensors in -> CUDA
        tensors out.  ``pos=None`` with ``dims=(E, A, K, T)`` takes the positions of the preceding ``denoise`` / ``denoise_reject`` call,
        which are still in the engine's workspace (``p0`` then decides where the outputs live; host arrays without it).
        K <= 1024, 2 <= T <= 24, A <= 64, L <= 64: ``metrics.wall_statistics_host`` beyond.
        ``n_agents`` [E] (``jmid_wall_statistics_padded``): the padded agents' rows of dist are NaN, their bytes 0, they count nowhere and
        agent_wall_hit_rate divides by K * n_agents[e]; padded rows of pos and p0 are never read."""
        w = wall_segments(walls)
        L = int(w.shape[0])
        if pos is None:
            if dims is None:
                raise ValueError("pos=None needs dims=(E, A, K, T) of the preceding denoise call")
            E, A, K, T = (int(v) for v in dims)
            dev, bp = p0 is not None and _is_cuda(p0), None
        else:
            dev = _is_cuda(pos)
            E, K, A, T, _ = (int(v) for v in pos.shape)
            bp = _Buf(pos, dev)
        if p0 is not None and tuple(p0.shape) != (E, A, 2):
            raise ValueError("p0 must be [E, A, 2]")
        b0 = _Buf(p0, dev) if p0 is not None else None
        where = (pos if pos is not None else p0).device if dev else None
        outs = [_out((E, K, A, L), np.float32, where), _out((E, K, A), np.uint8, where), _out((E, K, 3), np.float32, where),
                _out((E, 5), np.float32, where)]
        if n_agents is not None:
            na = agent_counts(n_agents, E)
            self._check(self._lib.jmid_wall_statistics_padded(self._h, E, A, K, T, _ptr(na), bp.ptr if bp is not None else None,
                                                              b0.ptr if b0 is not None else None, L, _ptr(w) if L else None, float(radius),
                                                              *[_ptr(o) for o in outs], self._mem(dev)))
            return tuple(outs)
        self._check(self._lib.jmid_wall_statistics(self._h, E, A, K, T, bp.ptr if bp is not None else None, b0.ptr if b0 is not None else None,
                                                   L, _ptr(w) if L else None, float(radius), *[_ptr(o) for o in outs], self._mem(dev)))
        return tuple(outs)

    # ------------------------------------------------------------------ measurement
    def kernel_classes(self):
        return [self._lib.jmid_kernel_class_name(i).decode() for i in range(self._lib.jmid_kernel_class_count())]

    def profile_enable(self, classes=None) -> None:
        names = self.kernel_classes()
        mask = 0
        for i, n in enumerate(names):
            if classes is None or n in classes:
                mask |= 1 << i
        self._check(self._lib.jmid_profile_enable(self._h, mask))

    def profile_disable(self) -> None:
        self._check(self._lib.jmid_profile_enable(self._h, 0))

    def profile_reset(self) -> None:
        self._check(self._lib.jmid_profile_reset(self._h))

    def profile_get(self) -> Dict[str, Tuple[int, float]]:
        out = {}
        for i, n in enumerate(self.kernel_classes()):
            cnt, ms = C.c_int64(0), C.c_double(0.0)
            self._check(self._lib.jmid_profile_get(self._h, i, C.byref(cnt), C.byref(ms)))
            out[n] = (int(cnt.value), float(ms.value))
        return out

    # ------------------------------------------------------------------ diagnostics (unit tests)
    def dbg_gemm(self, A: np.ndarray, Wt: np.ndarray, bias: Optional[np.ndarray], relu: bool = False,
                 precision: str = "f32") -> np.ndarray:
        A = np.ascontiguousarray(A, np.float32)
        Wt = np.ascontiguousarray(Wt, np.float32)
        M, K = A.shape
        N = Wt.shape[0]
        out = np.empty((M, N), np.float32)
        b = np.ascontiguousarray(bias, np.float32) if bias is not None else None
        self._check(self._lib.jmid_dbg_gemm(self._h, M, N, K, C.c_void_p(A.ctypes.data), C.c_void_p(Wt.ctypes.data),
                                            C.c_void_p(b.ctypes.data) if b is not None else None, int(relu),
                                            _lib.PRECISIONS[precision], C.c_void_p(out.ctypes.data)))
        return out

    def dbg_attention(self, qkv: np.ndarray, nseq: int, S: int, precision: str = "f32") -> np.ndarray:
        qkv = np.ascontiguousarray(qkv, np.float32)
        d = 2 * self.dims.ctx_dim
        assert qkv.shape == (nseq * S, 3 * d)
        out = np.empty((nseq * S, d), np.float32)
        self._check(self._lib.jmid_dbg_attention(self._h, nseq, S, C.c_void_p(qkv.ctypes.data),
                                                 _lib.PRECISIONS[precision], C.c_void_p(out.ctypes.data)))
        return out

    def dbg_gemm_ln_mx(self, A: np.ndarray, Wt: np.ndarray, bias, gamma, beta, X: np.ndarray, fused) -> np.ndarray:
        """LayerNorm(X + A Wt^T + bias) with the F16MX second-generation kernels (d_model 512): fused = 1 the row-complete kernel,
        0 the GEMM + add_ln2 pair, 3 the small-launch GEMM whose workgroups exchange the row statistics and normalise their own
        columns (gemm_small.hpp, OUT_LNX)."""
        A = np.ascontiguousarray(A, np.float32)
        Wt = np.ascontiguousarray(Wt, np.float32)
        X = np.array(X, np.float32, order="C", copy=True)
        v = [np.ascontiguousarray(t, np.float32) for t in (bias, gamma, beta)]
        M, K = A.shape
        assert Wt.shape == (512, K) and X.shape == (M, 512)
        self._check(self._lib.jmid_dbg_gemm_ln_mx(self._h, M, K, C.c_void_p(A.ctypes.data), C.c_void_p(Wt.ctypes.data),
                                                  *[C.c_void_p(t.ctypes.data) for t in v], C.c_void_p(X.ctypes.data),
                                                  int(fused)))
        return X

    def dbg_add_layernorm(self, X: np.ndarray, Y: np.ndarray, gamma: np.ndarray, beta: np.ndarray) -> np.ndarray:
        X = np.array(X, np.float32, order="C", copy=True)
        Y = np.ascontiguousarray(Y, np.float32)
        g = np.ascontiguousarray(gamma, np.float32)
        b = np.ascontiguousarray(beta, np.float32)
        M, d = X.shape
        self._check(self._lib.jmid_dbg_add_layernorm(self._h, M, d, C.c_void_p(X.ctypes.data),
                                                     C.c_void_p(Y.ctypes.data), C.c_void_p(g.ctypes.data),
                                                     C.c_void_p(b.ctypes.data)))
        return X

    def dbg_qkv0(self, x: np.ndarray, hyp: np.ndarray, step: int, dims: Tuple[int, int, int, int], precision: str = "f16mx"):
        """Layer 0's Q, K, V of one denoise step as the step's kernels leave them for the attention kernel (``jmid_dbg_qkv0``; the
        "qkv0" knob decides how they are made): x [M, 2], hyp [E * A, hyper width] -> (qkv [M, 3 d] float32, the time part of the
        hyper nets at step-table entry ``step`` [hyper width])."""
        E, A, K, T = (int(v) for v in dims)
        x = np.ascontiguousarray(x, np.float32)
        hyp = np.ascontiguousarray(hyp, np.float32)
        M, d = E * K * A * T, 2 * self.dims.ctx_dim
        width = self.hyper_width()
        if x.shape != (M, 2) or hyp.shape != (E * A, width):
            raise ValueError(f"expected x [{M}, 2] and hyp [{E * A}, {width}]")
        out = np.empty((M, 3 * d), np.float32)
        thyp = np.empty((width,), np.float32)
        self._check(self._lib.jmid_dbg_qkv0(self._h, E, A, K, T, C.c_void_p(x.ctypes.data), C.c_void_p(hyp.ctypes.data), width, int(step),
                                            _lib.PRECISIONS[precision], C.c_void_p(out.ctypes.data), C.c_void_p(thyp.ctypes.data)))
        return out, thyp

    def dbg_tail(self, X: np.ndarray, hyp: np.ndarray, step: int, dims: Tuple[int, int, int, int], precision: str = "f16mx"):
        """The tail of one denoise step alone (``jmid_dbg_tail``; the "tail_fold" knob decides how it runs): X [M, d] stands for the
        last LayerNorm's output, hyp [E * A, hyper width] -> (e [M, 2] float32, the time part of the hyper nets at step-table entry
        ``step`` [hyper width]).  "f32": the two fp32 GEMMs + the output kernel."""
        E, A, K, T = (int(v) for v in dims)
        X = np.ascontiguousarray(X, np.float32)
        hyp = np.ascontiguousarray(hyp, np.float32)
        M, d = E * K * A * T, 2 * self.dims.ctx_dim
        width = self.hyper_width()
        if X.shape != (M, d) or hyp.shape != (E * A, width):
            raise ValueError(f"expected X [{M}, {d}] and hyp [{E * A}, {width}]")
        out = np.empty((M, 2), np.float32)
        thyp = np.empty((width,), np.float32)
        self._check(self._lib.jmid_dbg_tail(self._h, E, A, K, T, C.c_void_p(X.ctypes.data), C.c_void_p(hyp.ctypes.data), width, int(step),
                                            _lib.PRECISIONS[precision], C.c_void_p(out.ctypes.data), C.c_void_p(thyp.ctypes.data)))
        return out, thyp

    SEAM_PLAN_FIELDS = ("kernel", "out_tpw", "rep", "ddpm", "embedded", "tail_fold", "range_flag")
    SEAM_KERNELS = ("out_ddim", "out_ddim_traj", "tail_fold", "tail_fold_traj", "embed")
    SEAM_REPS = ("f32", "pair", "hi_bf8")
    SEAM_COEF_FIELDS = ("c_e", "c_x", "n_x", "n_e", "c0", "c1", "sigma", "noise")

    def dbg_seam(self, X, x: np.ndarray, dims: Tuple[int, int, int, int], step: int, next_step: int = -1, precision: str = "f16mx",
                 z=None, ctx=None, hyp=None, embed_only: bool = False):
        """The seam between e_theta of step-table entry ``step`` and the residual stream of entry ``next_step`` as a step of a
        one-chunk call of shape ``dims`` = (E, A, K, T) runs it (``jmid_dbg_seam``; the "tail_fold" and "out_traj" knobs and
        ``set_step``'s sampling decide how): the tail on X [M, d_model], the sampler update of x [M, 2] with the draw z [M, 2] (or None),
        the embedding of the updated x for ``next_step`` (-1: the loop's last step, none).  Exactly one of ctx [E A, ctx_dim] (the
        call's own hyper GEMM) and hyp [E A, hyper width].  ``embed_only``: the first step's embedding kernel alone on x at ``step``.
        Returns a dict: x_next [M, 2]; hi, lo [M, d_model] (the embedding's buffers as the mode stores them, as float32; before the
        launch they hold X as split where the tail reads them, else the fill byte 0x3c: 1.05859375 in an fp16 plane, 1.0 in the bf8
        one); hyp [E A, width] as the kernels read it; thyp [2, width], the time rows of ``step`` and ``next_step``; coef, the
        handle's float32 coefficients of ``step`` by name; plan by ``SEAM_PLAN_FIELDS`` (kernel and rep as names)."""
        E, A, K, T = (int(v) for v in dims)
        M, d, width = E * K * A * T, self.dims.d_model, self.hyper_width()
        x = np.ascontiguousarray(x, np.float32)
        if x.shape != (M, 2):
            raise ValueError(f"expected x [{M}, 2]")
        if (ctx is None) == (hyp is None):
            raise ValueError("exactly one of ctx and hyp")

        def arr(a, shape, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float32)
            if a.shape != shape:
                raise ValueError(f"expected {what} {list(shape)}")
            return a
        X = arr(X, (M, d), "X")
        if X is None and not embed_only:
            raise ValueError("X is needed unless embed_only")
        z = arr(z, (M, 2), "z")
        ctx = arr(ctx, (E * A, self.dims.ctx_dim), "ctx")
        hyp = arr(hyp, (E * A, width), "hyp")
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        x_next, hi, lo = np.empty((M, 2), np.float32), np.empty((M, d), np.float32), np.empty((M, d), np.float32)
        hyp_out, thyp, coef = np.empty((E * A, width), np.float32), np.empty((2, width), np.float32), np.empty((len(self.SEAM_COEF_FIELDS),), np.float32)
        plan = (C.c_int * len(self.SEAM_PLAN_FIELDS))()
        self._check(self._lib.jmid_dbg_seam(self._h, E, A, K, T, ptr(X), ptr(x), ptr(z), ptr(ctx), ptr(hyp), width, int(step), int(next_step),
                                            _lib.PRECISIONS[precision], int(bool(embed_only)), ptr(x_next), ptr(hi), ptr(lo), ptr(hyp_out),
                                            ptr(thyp), ptr(coef), plan))
        plan = dict(zip(self.SEAM_PLAN_FIELDS, (int(v) for v in plan)))
        plan["kernel"], plan["rep"] = self.SEAM_KERNELS[plan["kernel"]], self.SEAM_REPS[plan["rep"]]
        return dict(x_next=x_next, hi=hi, lo=lo, hyp=hyp_out, thyp=thyp, coef=dict(zip(self.SEAM_COEF_FIELDS, coef)), plan=plan)

    LAYER_PLAN_FIELDS = ("stages", "in_proj_mode", "in_proj_shape", "in_proj_flags", "linear1_mode", "linear1_shape", "linear1_flags",
                         "out_proj_path", "out_proj_ln_rows", "out_proj_gemm_shape", "linear2_path", "linear2_ln_rows", "linear2_gemm_shape",
                         "vt_direct", "k8", "q8l", "attn_nsplit", "masked", "merge", "byte_lo", "attn_dma", "range_flag", "out_proj_mode", "linear2_mode", "attn_pack")

    def dbg_layer(self, X: np.ndarray, layer: int, dims: Tuple[int, int, int, int], precision: str = "f16mx", n_agents=None, last: bool = False):
        """Encoder layer ``layer`` of one net evaluation as a step of a one-chunk call of shape ``dims`` = (E, A, K, T) runs it
        (``jmid_dbg_layer``), every stage copied out in between: X [M, d_model] float32 -> (stages, plan).  ``stages[s]`` is the pair
        (hi plane, lo plane) of stage s as float32 arrays - 0: X as split, 1: Q | K | V as the attention kernel reads them [M, 3 d],
        2: the attention output, 3: X after norm1, 4: linear1 + ReLU [M, d_ff], 5: X after norm2 - or None where the stage does not
        exist (stage 2 when the out-projection's launch merges the split-KV partials).  ``plan``: the launch plan it ran, by
        ``LAYER_PLAN_FIELDS``.  ``n_agents`` [E]: a padded call; ``last``: the encoder's last layer."""
        E, A, K, T = (int(v) for v in dims)
        X = np.ascontiguousarray(X, np.float32)
        M, d, ff = E * K * A * T, self.dims.d_model, self.dims.d_ff
        if X.shape != (M, d):
            raise ValueError(f"expected X [{M}, {d}]")
        nag = None
        if n_agents is not None:
            nag = np.ascontiguousarray(n_agents, np.int32)
            if nag.shape != (E,):
                raise ValueError(f"expected n_agents [{E}]")
        widths = (d, 3 * d, d, d, ff, d)
        total = sum(widths)
        hi, lo = np.empty((M * total,), np.float32), np.empty((M * total,), np.float32)
        plan = (C.c_int * len(self.LAYER_PLAN_FIELDS))()
        self._check(self._lib.jmid_dbg_layer(self._h, E, A, K, T, int(layer), _lib.PRECISIONS[precision], C.c_void_p(X.ctypes.data),
                                             C.c_void_p(nag.ctypes.data) if nag is not None else None, int(bool(last)),
                                             C.c_void_p(hi.ctypes.data), C.c_void_p(lo.ctypes.data), plan))
        plan = dict(zip(self.LAYER_PLAN_FIELDS, (int(v) for v in plan)))
        stages, at = [], 0
        for s, w in enumerate(widths):
            pair = (hi[M * at:M * (at + w)].reshape(M, w), lo[M * at:M * (at + w)].reshape(M, w))
            stages.append(pair if plan["stages"] >> s & 1 else None)
            at += w
        return stages, plan

    def hyper_width(self) -> int:
        """Row length of the ConcatSquash hyper vectors, gate1 | bias1 | gate3 | bias3 | gate4 | bias4 | gateO | biasO (the library
        checks it: ``jmid_dbg_qkv0`` refuses any other)."""
        return 2 * self.dims.d_model + 2 * self.dims.d_mid + 2 * self.dims.d_low + 4
