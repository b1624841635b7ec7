"""Which engine entries a configuration of ``predict_ret_best()`` / ``predict_batch()`` calls, and in which order: the GPU tests
compare results only, so a change that silently sends ``device_frames=True`` down the staged path would pass them and lose the
latency the option exists for.  A recording stand-in replaces ``JmidEngine``: no library, no device, zero arrays of the right shape."""
import os
import types
import warnings

import numpy as np
import pytest
import torch

from safe_interactive_crowdnav_amd import _lib, forecaster as FC, scene as SC
from safe_interactive_crowdnav_amd.weights import NetDims

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERANGE = next(code for code, name in _lib.ERR_NAMES.items() if name == "JMID_ERANGE")
WEIGHTS = types.SimpleNamespace(dims=NetDims(ctx_dim=32), checksum=lambda: "fake")
TIMING_KEYS = {"scene_ms", "device_ms", "topk_ms", "assemble_ms", "total_ms"}


class FakeEngine:
    """``JmidEngine``'s call surface as far as forecaster.py uses it.  Every entry appends its name to ``trace`` - with the precision
    where it takes one, ``(nopos)`` for want_pos=False, ``(resident)`` for topk / repair_collisions(pos=None), ``(seeded)`` for the seed
    forms, ``(ff)`` / ``(fi)`` for first_frame / first_index, ``(padded)`` for n_agents, ``(walls)`` for walls, ``(p0)`` for the repair's p0 -
    and an entry named in ``erange`` raises JMID_ERANGE in every precision but "f32".  ``draws``: the draw0 of every ``denoise_reject``."""

    def __init__(self, weights, joint=True, device_id=0, hist_len=6, step=2, lib_path=None):
        self.dims, self.device_id, self.hist_len, self.step, self.sampling = weights.dims, device_id, hist_len, step, "ddim"
        self.trace, self.erange, self.draws = [], set(), []
        self.schedule = types.SimpleNamespace(num_steps=100)
        self.set_step(step)

    def _log(self, name, precision=None):
        self.trace.append(name if precision is None else f"{name}[{precision}]")
        if precision not in (None, "f32") and name in self.erange:
            raise _lib.JmidError(ERANGE, "an activation left the fp16 range (stand-in)")

    @staticmethod
    def _ranked(E, A, K, T, k):
        if k < K:
            return np.zeros((E, A, k, T, 2), np.float32), np.zeros((E, A, k), np.float32)
        return np.zeros((E, K, A, T, 2), np.float32), None

    def set_step(self, step, sampling="ddim", flexibility=0.0):
        self.step, self.sampling, self.n_steps = step, sampling, len(range(100, 0, -int(100 / step)))

    def noise(self, seed, episode_ids, rows, T, draw=0):
        self._log("noise")
        return np.zeros((len(episode_ids), rows, T, 2), np.float32)

    def encode(self, x_st, nbr_sum, edge_mask, first_index=None):
        self._log("encode" + ("(fi)" if first_index is not None else ""))
        return np.zeros((x_st.shape[0], self.dims.ctx_dim), np.float32)

    def denoise(self, x_T, ctx, p0, dt=0.25, precision="f32", want_vel=True, want_pos=True, z=None, seed=None, episode_ids=None, K=None,
                T=None):
        self._log("denoise" + ("(seeded)" if seed is not None else "") + ("" if want_pos else "(nopos)"), precision)
        E, A = ctx.shape[:2]
        K, T = (K, T) if x_T is None else (x_T.shape[1] // A, x_T.shape[2])
        return None, (np.zeros((E, K, A, T, 2), np.float32) if want_pos else None)

    def denoise_reject(self, ctx, p0, seed, episode_ids, K, T, dt=0.25, precision="f32", threshold=0.2, max_rounds=3, draw0=0, want_vel=True,
                       want_pos=True, walls=None, wall_radius=None, n_agents=None):
        self.draws.append(int(draw0))
        self._log("denoise_reject" + ("(padded)" if n_agents is not None else "") + ("(walls)" if walls is not None else "")
                  + ("" if want_pos else "(nopos)"), precision)
        n, a = ctx.shape[:2]
        if n_agents is not None:
            assert len(n_agents) == n and max(n_agents) == a and min(n_agents) >= 1 and draw0 == 0
        out = (None, np.zeros((n, K, a, T, 2), np.float32) if want_pos else None, np.zeros((n, K, 3), np.int32), np.zeros((n, 3), np.int32))
        return out + ((np.zeros((n, 2), np.int32),) if walls is not None or n_agents is not None else ())

    def repair_collisions(self, pos, threshold=0.2, margin=0.02, tau=0.005, step=0.02, max_iter=32, p0=None, dt=0.25, vel=None, dims=None,
                          n_agents=None, want_pos=None, walls=None, wall_radius=None):
        self._log("repair" + ("(resident)" if pos is None else "") + ("(padded)" if n_agents is not None else "")
                  + ("(walls)" if walls is not None else "") + ("(p0)" if p0 is not None else ""))
        E, A, K, T = dims if pos is None else (pos.shape[0], pos.shape[2], pos.shape[1], pos.shape[3])
        out = (None if pos is None else np.zeros((E, K, A, T, 2), np.float32), None, np.zeros((E, K, 4), np.float32), np.zeros((E, 3), np.int32))
        return out + ((np.zeros((E, K, 2), np.float32),) if walls is not None else ())

    def topk(self, pos, k, dims=None, n_agents=None):
        self._log("topk" + ("(resident)" if pos is None else "") + ("(padded)" if n_agents is not None else ""))
        E, A, K, T = dims if pos is None else (pos.shape[0], pos.shape[2], pos.shape[1], pos.shape[3])
        return self._ranked(E, A, K + 1, T, k)

    def predict(self, x_st, nbr_sum, edge_mask, x_T, p0, k, dt=0.25, precision="f32", name="predict"):
        self._log(name, precision)
        E, A = p0.shape[:2]
        return self._ranked(E, A, x_T.shape[1] // A, x_T.shape[2], k)

    def predict_padded(self, x_st, nbr_sum, edge_mask, x_T, p0, k, n_agents, dt=0.25, precision="f32"):
        return self.predict(x_st, nbr_sum, edge_mask, x_T, p0, k, dt, precision, name="predict_padded")

    def _resident(self, hum, rob, time_step, horizon, first_frame=None, pose_now=None):
        self.single = hum.ndim == 3
        if self.single:
            hum, rob, first_frame = hum[None], rob[None], None if first_frame is None else np.asarray(first_frame)[None]
        self.batch = SC.build_scenes_batched(hum, rob, time_step, horizon=horizon, first_frame=first_frame)
        self.frames = dict(human_xy=hum, robot_xy=rob, pose_now=hum[:, -1] if pose_now is None else pose_now[None])
        inc = self.batch["in_cluster"]
        return self._squeeze(dict(in_cluster=inc, robot_in_cluster=self.batch["robot_in_cluster"], n_in=inc.sum(axis=1).astype(np.int32),
                                  cv=self.batch["cv"]))

    def _squeeze(self, arrays):
        return {key: v[0] for key, v in arrays.items()} if self.single else dict(arrays)

    def build_scene(self, human_xy, robot_xy, time_step, horizon=None, force_all_in_cluster=False, first_frame=None):
        self._log("build_scene" + ("(ff)" if first_frame is not None else ""))
        return self._resident(np.asarray(human_xy), np.asarray(robot_xy), time_step, horizon, first_frame)

    def build_scene_stamped(self, stamps, human_xy, robot_xy, time_step, horizon=None):
        self._log("build_scene_stamped")
        hum, rob, pose_now = SC.frame_table_frames(stamps, human_xy, robot_xy, time_step, self.hist_len)
        if len(hum) < self.hist_len:
            raise SC.HistoryTooShortError(f"{len(hum)} history frames available, {self.hist_len} needed")
        return self._resident(hum, rob, time_step, horizon, pose_now=pose_now)

    def scene_arrays(self):
        self._log("scene_arrays")
        return self._squeeze({key: self.batch[key] for key in ("x", "x_st", "nbr_sum", "edge_mask", "p0", "first_index")})

    def scene_frames(self):
        self._log("scene_frames")
        return self._squeeze(self.frames)

    def _scene_dims(self, x_T, K, T):
        inc = self.batch["in_cluster"]
        A = int(inc[0].sum())
        return (inc.shape[0], inc.shape[1], A) + ((K, T) if x_T is None else (x_T.shape[1] // A, x_T.shape[2]))

    def predict_scene(self, x_T, k, dt=0.25, precision="f32", seed=None, episode_ids=None, K=None, T=None):
        self._log("predict_scene" + ("(seeded)" if seed is not None else ""), precision)
        E, _, A, K, T = self._scene_dims(x_T, K, T)
        return self._ranked(E, A, K, T, k)

    def forecast_scene(self, x_T, k, dt=0.25, precision="f32", seed=None, episode_ids=None, K=None, T=None):
        self._log("forecast_scene" + ("(seeded)" if seed is not None else ""), precision)
        E, N, _, _, T = self._scene_dims(x_T, K, T)
        fc, lw = np.zeros((E, N, k, T + 1, 2)), np.zeros((E, N, k))
        return (fc[0], lw[0]) if self.single else (fc, lw)


class State:
    def __init__(self, p):
        self.position = (float(p[0]), float(p[1]))


@pytest.fixture
def make(monkeypatch, tmp_path):
    """-> make(k, frames=None, erange=(), **flags): a fresh forecaster on a fresh stand-in engine, fed the fixture's first ``frames``
    stamped frames (None: all 7)."""
    z = np.load(os.path.join(GOLDEN, "wrapper_jmid_w32_spread50.npz"))
    monkeypatch.setattr(FC, "JmidEngine", FakeEngine)

    def make(k, frames=None, erange=(), **flags):
        monkeypatch.setattr(FC, "_ENGINE_CACHE", {})
        env, ypath = FC.write_configs(str(tmp_path / f"k{k}"), joint=True, ctx_dim=32, N=int(z["N"]), K=int(z["K"]), k_ret=k,
                                      H=int(z["H"]), step=2)
        # (rng_compat: what "auto" resolves to on a host without a GPU, by name so that the test reads the same on one with)
        f = FC.HumanTrajectoryForecasterSim(env, ypath, weights=WEIGHTS, **{"precision": "f16mx", "rng_compat": "cpu", **flags})
        assert isinstance(f.engine, FakeEngine)
        f.engine.erange = set(erange)
        for r, h, t in list(zip(z["robot_xy"], z["human_xy"], z["stamps"]))[:frames]:
            f.update_state_hists(State(r), [State(p) for p in h], float(t))
        return f
    return make


def call(f):
    """One ``predict_ret_best()`` -> what it traced."""
    f.engine.trace.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # (the once-per-instance JMID_ERANGE warning)
        fc, lw = f.predict_ret_best()
    assert fc.shape == (f.num_hums, f.num_ret_samples, f.predict_horizon + 1, 2) and lw.shape == fc.shape[:2]
    assert fc.dtype == lw.dtype == np.float64 and set(f.timings) == TIMING_KEYS
    return " ".join(f.engine.trace)


STAGED_CHECK = "encode denoise[f16mx] denoise[f16x3]"
SINGLE = [     # (flags, k, first call, second call)
    (dict(self_check=True), 4, STAGED_CHECK + " topk", "predict[f16mx]"),
    (dict(self_check=True), 10, STAGED_CHECK, "predict[f16mx]"),
    (dict(self_check=False), 4, "predict[f16mx]", None),
    (dict(self_check=False), 10, "predict[f16mx]", None),
    (dict(precision="f32", self_check=True), 4, "predict[f32]", None),
    (dict(self_check=False, device_topk=False), 4, "encode denoise[f16mx]", None),
    (dict(self_check=False, device_topk=False), 10, "predict[f16mx]", None),
    (dict(self_check=True, device_scene=True), 4, "build_scene scene_arrays " + STAGED_CHECK + " topk", "build_scene predict_scene[f16mx]"),
    (dict(self_check=False, device_scene=True), 10, "build_scene predict_scene[f16mx]", None),
    (dict(self_check=True, device_frames=True), 10, "build_scene_stamped scene_arrays scene_frames " + STAGED_CHECK,
     "build_scene_stamped forecast_scene[f16mx]"),
    (dict(self_check=False, device_frames=True), 10, "build_scene_stamped forecast_scene[f16mx]", None),
    (dict(self_check=False, device_frames=True, device_topk=False), 4,
     "build_scene_stamped scene_arrays scene_frames encode denoise[f16mx]", None),
    (dict(self_check=False, rng_compat="device"), 10, "noise predict[f16mx]", None),
    (dict(self_check=False, rng_compat="device", device_frames=True), 10, "build_scene_stamped noise forecast_scene[f16mx]", None),
    (dict(frames=3, short_history=True), 4, "encode(fi) denoise(nopos)[f16mx] topk(resident)", None),
    (dict(frames=3, short_history=True), 10, "encode(fi) denoise[f16mx]", None),
    (dict(frames=3, short_history=True, device_scene=True), 10, "build_scene(ff) predict_scene[f16mx]", None),
    (dict(frames=3, short_history=True, device_frames=True), 10, "build_scene(ff) predict_scene[f16mx]", None),
]


@pytest.mark.parametrize("flags,k,first,second", SINGLE)
def test_single_call_routes(make, flags, k, first, second):
    f = make(k, **{"self_check": False, **flags})
    assert call(f) == first
    assert call(f) == (first if second is None else second)
    assert f.erange_fallbacks == 0


ERANGE_ROWS = [     # (flags, k, entries that raise, trace of every call)
    (dict(), 4, ("predict", "denoise", "denoise(nopos)"), "predict[f16mx] encode denoise(nopos)[f16mx] denoise(nopos)[f32] topk(resident)"),
    (dict(), 10, ("predict", "denoise", "denoise(nopos)"), "predict[f16mx] encode denoise[f16mx] denoise[f32]"),
    (dict(device_frames=True), 10, ("forecast_scene", "denoise"),
     "build_scene_stamped forecast_scene[f16mx] scene_arrays scene_frames encode denoise[f16mx] denoise[f32]"),
]


@pytest.mark.parametrize("flags,k,erange,trace", ERANGE_ROWS)
def test_single_call_erange_goes_to_the_staged_path_in_fp32(make, flags, k, erange, trace):
    f = make(k, erange=erange, self_check=False, **flags)
    for n in (1, 2):
        before = FC.ERANGE_FALLBACKS
        assert call(f) == trace
        assert f.erange_fallbacks == n and FC.ERANGE_FALLBACKS == before + 1


@pytest.mark.parametrize("flags,frames,trace", [(dict(), 3, ""), (dict(device_frames=True), 3, "build_scene_stamped"),
                                                (dict(short_history=True), 1, ""), (dict(rng_compat="device"), 3, "")])
def test_a_too_short_history_draws_nothing(make, flags, frames, trace):
    f = make(10, frames=frames, self_check=False, **flags)
    for _ in range(2):
        f.engine.trace.clear()
        rng = torch.get_rng_state()
        with pytest.raises(SC.HistoryTooShortError):
            f.predict_ret_best()
        assert " ".join(f.engine.trace) == trace
        assert torch.equal(torch.get_rng_state(), rng) and f._noise_draw == 0


# ------------------------------------------------------------------------------------------------------------- predict_batch
def batch_inputs(seed=17):
    """The histories of tests/test_gpu_forecaster.py::test_predict_batch_with_natural_clusters..., six episodes of them: six pedestrians
    around a robot at (0, -3).  Seed 17: two count groups; ``THREE_COUNTS_SEED``: three."""
    E, F, N, dt = 6, 6, 6, 0.25
    rng = np.random.default_rng(seed)
    pos0 = rng.uniform(-5.0, 5.0, (E, N, 2))
    vel = rng.uniform(-1.0, 1.0, (E, N, 2))
    t = np.arange(F) * dt
    hum = pos0[:, None] + vel[:, None] * t[None, :, None, None] + 0.01 * rng.standard_normal((E, F, N, 2))
    rob = np.array([0.0, -3.0])[None, None] + 0.02 * rng.standard_normal((E, F, 2))
    return hum, rob


THREE_COUNTS_SEED = 0      # in-cluster counts (1, 2, 4, 2, 2, 2) on the host scene: asserted where it is used
PLAIN, FULL = "encode denoise(nopos)[f16mx] topk(resident)", "encode denoise[f16mx]"
BATCH = [     # (keywords, k, trace); K = 8, two count groups
    (dict(), 3, [PLAIN] * 2),
    (dict(), 8, [FULL] * 2),
    (dict(device_scene=True), 3, ["build_scene scene_arrays"] + [PLAIN] * 2),
    (dict(device_frames=True), 3, ["build_scene"] + ["build_scene forecast_scene[f16mx]"] * 2),
    (dict(device_frames=True), 8, ["build_scene"] + ["build_scene forecast_scene[f16mx]"] * 2),
    (dict(padded=True), 3, ["predict_padded[f16mx]"]),
    (dict(padded=True), 8, ["predict_padded[f16mx]"]),
    (dict(device_topk=False), 3, [FULL] * 2),
    (dict(device_topk=False, device_frames=True), 3, ["build_scene build_scene scene_arrays"] + [FULL] * 2),
    (dict(device_topk=False, padded=True), 3, [FULL] * 2),
    (dict(noise="device", seed=5), 3, ["encode denoise(seeded)(nopos)[f16mx] topk(resident)"] * 2),
    (dict(noise="device", seed=5, device_frames=True), 3, ["build_scene"] + ["build_scene forecast_scene(seeded)[f16mx]"] * 2),
    (dict(padded=True, erange=("predict_padded",)), 3, ["predict_padded[f16mx] predict_padded[f32]"]),
    (dict(device_frames=True, erange=("forecast_scene",)), 3,
     ["build_scene"] + ["build_scene forecast_scene[f16mx] forecast_scene[f32]"] * 2),
    (dict(erange=("denoise(nopos)",)), 3, ["encode denoise(nopos)[f16mx] denoise(nopos)[f32] topk(resident)"] * 2),
    (dict(last=3, short_history=True), 3, ["encode(fi) denoise(nopos)[f16mx] topk(resident)"] * 2),
    (dict(last=3, short_history=True, device_frames=True), 3, ["build_scene(ff)"] + ["build_scene(ff) forecast_scene[f16mx]"] * 2),
]


@pytest.mark.parametrize("kw,k,trace", BATCH)
def test_predict_batch_routes(kw, k, trace):
    kw = dict(kw)
    erange, last = set(kw.pop("erange", ())), kw.pop("last", 6)
    hum, rob = batch_inputs()
    E, N, K, H = 6, 6, 8, 6
    eng = FakeEngine(WEIGHTS)
    eng.erange = erange
    before = FC.ERANGE_FALLBACKS
    fc, lw, inc = FC.predict_batch(eng, hum[:, -last:], rob[:, -last:], range(E), num_samples=K, num_ret_samples=k, horizon=H,
                                   time_step=0.25, precision="f16mx", **kw)
    assert sorted(set(inc.sum(axis=1).tolist())) == [1, 2]          # two count groups
    assert fc.shape == (E, N, k, H + 1, 2) and lw.shape == (E, N, k) and fc.dtype == lw.dtype == np.float64
    assert " ".join(eng.trace) == " ".join(trace)
    assert FC.ERANGE_FALLBACKS == before + (sum(t.count("[f32]") for t in trace) if erange else 0)


# ------------------------------------------------------------------------------------------------------------- constraint routes
# recorded at the commit in front of the constraints record and the one staged run: the entries, their order and the draw numbers of
# every constraint keyword on the three callers (the GPU tests compare results against twins; these compare the calls)
WALLS = np.array([[0.5, -3.0, 0.5, 3.0], [-2.0, 1.0, 2.0, 1.2]])
WALLED = dict(static_obstacles=WALLS, wall_radius=0.3, constraint_type="opt_softplus_walls")
SOFT, REDRAW = dict(constraint_type="opt_softplus"), dict(rng_compat="device", collision_free_rounds=2)
REPAIR_4, REPAIR_K = "encode denoise(nopos)[f16mx] repair(resident) topk(resident)", "encode denoise[f16mx] repair"
REDRAW_4, REDRAW_K = "encode denoise_reject(nopos)[f16mx] topk(resident)", "encode denoise_reject[f16mx]"
REDRAW_CHECK = "encode denoise_reject[f16mx] denoise_reject[f16x3]"
CONSTRAINED = [     # (flags, k, first call, second call, draw0 of the first call's loops, of the second call's)
    (SOFT, 4, REPAIR_4, REPAIR_4, [], []),
    (SOFT, 10, REPAIR_K, REPAIR_K, [], []),
    (dict(SOFT, self_check=True), 4, STAGED_CHECK + " repair topk", REPAIR_4, [], []),
    (dict(SOFT, self_check=True), 10, STAGED_CHECK + " repair", REPAIR_K, [], []),
    (REDRAW, 4, REDRAW_4, REDRAW_4, [0], [3]),
    (REDRAW, 10, REDRAW_K, REDRAW_K, [0], [3]),
    (dict(REDRAW, self_check=True), 4, REDRAW_CHECK + " topk", REDRAW_4, [0, 0], [3]),      # (the check's loop starts from the same draw0)
    (dict(REDRAW, self_check=True), 10, REDRAW_CHECK, REDRAW_K, [0, 0], [3]),
    (dict(REDRAW, **WALLED), 4, "encode denoise_reject(walls)(nopos)[f16mx] repair(resident)(walls)(p0) topk(resident)", None, [0], [3]),
    (dict(REDRAW, **WALLED), 10, "encode denoise_reject(walls)[f16mx] repair(walls)(p0)", None, [0], [3]),
    (dict(WALLED, device_frames=True), 4,
     "build_scene_stamped scene_arrays scene_frames encode denoise(nopos)[f16mx] repair(resident)(walls)(p0) topk(resident)", None, [], []),
]
REPAIR_CAUSE_KEYS = {"pedestrians", "walls", "both", "pedestrians_repaired", "walls_repaired", "both_repaired", "candidates", "repaired",
                     "reverted"}


@pytest.mark.parametrize("flags,k,first,second,draws_first,draws_second", CONSTRAINED)
def test_constraint_routes(make, flags, k, first, second, draws_first, draws_second):
    f = make(k, **{"self_check": False, **flags})
    for trace, draws in ((first, draws_first), (first if second is None else second, draws_second)):
        f.engine.draws.clear()
        assert call(f) == trace
        assert f.engine.draws == draws
        walls, rounds, fix = "static_obstacles" in flags, "collision_free_rounds" in flags, "constraint_type" in flags
        assert (f.rejection is None) if not rounds else len(f.rejection) == (5 if walls else 3)
        assert (f.repair is None) if not fix else len(f.repair) == 4
        assert (f.repair_causes is None) if not (fix and walls) else set(f.repair_causes) == REPAIR_CAUSE_KEYS
    assert f.erange_fallbacks == 0 and f.precision == "f16mx"


def test_erange_in_the_redraw_loop_repeats_the_whole_loop_in_fp32(make):
    """JMID_ERANGE from ``denoise_reject``: the loop again in exact fp32 from the same draw0, counted once per call, warned about once
    per instance."""
    f = make(4, erange=("denoise_reject(nopos)",), self_check=False, **REDRAW)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for n, draw0 in ((1, 0), (2, 3)):
            f.engine.trace.clear()
            f.engine.draws.clear()
            before = FC.ERANGE_FALLBACKS
            f.predict_ret_best()
            assert " ".join(f.engine.trace) == "encode denoise_reject(nopos)[f16mx] denoise_reject(nopos)[f32] topk(resident)"
            assert f.engine.draws == [draw0, draw0]
            assert f.erange_fallbacks == n and FC.ERANGE_FALLBACKS == before + 1 and len(f.rejection) == 3
    assert [str(w.message).startswith("JMID_ERANGE") for w in caught if issubclass(w.category, RuntimeWarning)] == [True]


GROUP_WALLED = "encode denoise_reject(walls)(nopos)[f16mx] repair(resident)(walls)(p0) topk(resident)"
DEVICE_NOISE = dict(noise="device", seed=5, collision_free_rounds=2)
BATCH_CONSTRAINED = [     # (keywords, k, trace, keys of stats); K = 8, three count groups
    (SOFT, 3, [REPAIR_4] * 3, ["repair"]),
    (dict(DEVICE_NOISE, **WALLED), 3, [GROUP_WALLED] * 3, ["cause", "episodes", "repair", "repair_causes", "slots"]),
    (dict(DEVICE_NOISE, collision_free_padded=True, **SOFT), 3,
     ["encode denoise_reject(padded)(nopos)[f16mx] repair(resident)(padded) topk(resident)(padded)"], ["cause", "episodes", "repair", "slots"]),
    (dict(DEVICE_NOISE, erange=("denoise_reject(nopos)",)), 3,
     ["encode denoise_reject(nopos)[f16mx] denoise_reject(nopos)[f32] topk(resident)"] * 3, ["episodes", "slots"]),
    # the padded branch beyond the device top-k: ranked on the host over every episode's real agents, no topk entry
    (dict(DEVICE_NOISE, collision_free_padded=True, device_topk=False, **SOFT), 3, ["encode denoise_reject(padded)[f16mx] repair(padded)"],
     ["cause", "episodes", "repair", "slots"]),
]


@pytest.mark.parametrize("kw,k,trace,keys", BATCH_CONSTRAINED)
def test_predict_batch_constraint_routes(kw, k, trace, keys):
    kw = dict(kw)
    erange = set(kw.pop("erange", ()))
    hum, rob = batch_inputs(THREE_COUNTS_SEED)
    E, N, K, H = 6, 6, 8, 6
    eng, stats = FakeEngine(WEIGHTS), {}
    eng.erange = erange
    before = FC.ERANGE_FALLBACKS
    fc, lw, inc = FC.predict_batch(eng, hum, rob, range(E), num_samples=K, num_ret_samples=k, horizon=H, time_step=0.25, precision="f16mx",
                                   stats=stats, **kw)
    assert inc.sum(axis=1).tolist() == [1, 2, 4, 2, 2, 2]          # three count groups, nobody's cluster empty
    assert fc.shape == (E, N, k, H + 1, 2) and lw.shape == (E, N, k) and fc.dtype == lw.dtype == np.float64
    assert " ".join(eng.trace) == " ".join(trace)
    assert sorted(stats) == keys and not any(eng.draws)           # (every loop of a batch starts at draw 0)
    assert FC.ERANGE_FALLBACKS == before + (sum(t.count("[f32]") for t in trace) if erange else 0)
    if "repair" in stats:
        assert stats["repair"].shape == (E, 3)
    if "repair_causes" in stats:
        assert set(stats["repair_causes"]) == REPAIR_CAUSE_KEYS
    if "episodes" in stats:
        assert stats["episodes"].shape == (E, 3) and stats["slots"].shape == (E, K, 3)
    if "cause" in stats:
        assert stats["cause"].shape == (E, 2)


OFFLINE = [     # (keywords of offline.generate, trace): offline the repair REPLACES the redraws, in the forecaster it follows them
    (dict(with_constraints=True, seed=3, sampling="ddim"), "denoise_reject[f32]"),
    (dict(with_constraints=True, seed=3, sampling="ddim", static_obstacles=WALLS, wall_radius=0.3), "denoise_reject(walls)[f32]"),
    (dict(with_constraints=True, **SOFT), "denoise[f32] repair"),
    (dict(with_constraints=True, seed=3, sampling="ddim", **SOFT), "denoise(seeded)[f32] repair"),
    (dict(with_constraints=True, **WALLED), "denoise[f32] repair(walls)(p0)"),
    (dict(with_constraints=True, seed=3, sampling="ddim", **WALLED), "denoise(seeded)[f32] repair(walls)(p0)"),
]


@pytest.mark.parametrize("kw,trace", OFFLINE)
def test_offline_generate_constraint_routes(kw, trace):
    from safe_interactive_crowdnav_amd import offline
    B, T, n = 3, 6, 5
    eng = FakeEngine(WEIGHTS)
    rng = torch.get_rng_state()
    pos, steps, a, b, c = offline.generate(eng, np.zeros((B, 32), np.float32), np.zeros((B, 2), np.float32), 0.25, T, n, True, step=2, **kw)
    assert " ".join(eng.trace) == trace
    assert ("constraint_type" in kw) == ("repair" in trace) == ("denoise_reject" not in trace)
    assert pos.shape == (n, B, T, 2) and pos.dtype == np.float32 and steps == n * 3 and (a, b, c) == (0, 0, 0)
    assert torch.equal(torch.get_rng_state(), rng) == ("seed" in kw)      # a seeded call draws nothing on the host
