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
    where it takes one, ``(nopos)`` for want_pos=False, ``(resident)`` for topk(pos=None), ``(seeded)`` for the seed forms, ``(ff)`` /
    ``(fi)`` for first_frame / first_index - and an entry named in ``erange`` raises JMID_ERANGE in every precision but "f32"."""

    def __init__(self, weights, joint=True, device_id=0, hist_len=6, step=2, lib_path=None):
        self.dims, self.device_id, self.hist_len, self.step, self.sampling = weights.dims, device_id, hist_len, step, "ddim"
        self.trace, self.erange = [], set()

    def _log(self, name, precision=None):
        self.trace.append(name if precision is None else f"{name}[{precision}]")
        if precision not in (None, "f32") and name in self.erange:
            raise _lib.JmidError(ERANGE, "an activation left the fp16 range (stand-in)")

    @staticmethod
    def _ranked(E, A, K, T, k):
        if k < K:
            return np.zeros((E, A, k, T, 2), np.float32), np.zeros((E, A, k), np.float32)
        return np.zeros((E, K, A, T, 2), np.float32), None

    def set_step(self, step, sampling="ddim"):
        self.step, self.sampling = step, sampling

    def noise(self, seed, episode_ids, rows, T, draw=0):
        self._log("noise")
        return np.zeros((len(episode_ids), rows, T, 2), np.float32)

    def encode(self, x_st, nbr_sum, edge_mask, first_index=None):
        self._log("encode" + ("(fi)" if first_index is not None else ""))
        return np.zeros((x_st.shape[0], self.dims.ctx_dim), np.float32)

    def denoise(self, x_T, ctx, p0, dt=0.25, precision="f32", want_vel=True, want_pos=True, seed=None, episode_ids=None, K=None, T=None):
        self._log("denoise" + ("(seeded)" if seed is not None else "") + ("" if want_pos else "(nopos)"), precision)
        E, A = ctx.shape[:2]
        K, T = (K, T) if x_T is None else (x_T.shape[1] // A, x_T.shape[2])
        return None, (np.zeros((E, K, A, T, 2), np.float32) if want_pos else None)

    def topk(self, pos, k, dims=None):
        self._log("topk" + ("(resident)" if pos is None else ""))
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
def batch_inputs():
    """The histories of tests/test_gpu_forecaster.py::test_predict_batch_with_natural_clusters..., six episodes of them."""
    E, F, N, dt = 6, 6, 6, 0.25
    rng = np.random.default_rng(17)
    pos0 = rng.uniform(-5.0, 5.0, (E, N, 2))
    vel = rng.uniform(-1.0, 1.0, (E, N, 2))
    t = np.arange(F) * dt
    hum = pos0[:, None] + vel[:, None] * t[None, :, None, None] + 0.01 * rng.standard_normal((E, F, N, 2))
    rob = np.array([0.0, -3.0])[None, None] + 0.02 * rng.standard_normal((E, F, 2))
    return hum, rob


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
