"""Stamped frames in, predict_ret_best arrays out, on the device (jmid_build_scene_stamped / jmid_scene_get_frames /
jmid_forecast_scene, csrc/frames.hpp) against the host twins (scene.frame_table, frame_table_frames_batched, assemble_forecasts), bit
for bit: the frame table is selections plus one fp64 interpolation formula without FMA contraction, the assembly is copies and exact
widenings.  tests/test_frames_host.py pins the twins to scene.frame_table and holds the batched inputs to the cluster margin."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from safe_interactive_crowdnav_amd import _lib
from safe_interactive_crowdnav_amd import scene as SC
from safe_interactive_crowdnav_amd.engine import JmidEngine, JmidError
from safe_interactive_crowdnav_amd.forecaster import HumanTrajectoryForecasterSim, predict_batch, write_configs
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims
from tests.test_frames_host import RAW_SETS, as_lists, bits_equal, capture_frames, raw_batch
from tests.test_scene_device_inputs import DT, F, random_positions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_ENGINES = {}


def engine_for(ctx_dim=32, joint=True, wseed=5, step=2):
    key = (ctx_dim, joint, wseed, step)
    if key not in _ENGINES:
        _ENGINES[key] = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=ctx_dim), wseed), joint=joint, hist_len=6, step=step)
    return _ENGINES[key]


class State:
    def __init__(self, p):
        self.position = (float(p[0]), float(p[1]))


def logw_matches(got, want, k, K):
    """k < K: bit-equal.  k == K: the library's host log(1.0 / K) against np.log(1 / K) - two libms, each within 1 ulp of the true value."""
    if k < K:
        return bits_equal(got, want)
    ref = np.log(1.0 / K)
    return got.shape == want.shape and float(np.abs(got - ref).max()) <= 2 * np.spacing(abs(ref))


# ------------------------------------------------------------------------------------------------ 1. the captures, raw
@pytest.mark.parametrize("case", ["wrapper_jmid_jitter.npz", "wrapper_jmid_gap.npz", "wrapper_jmid_together.npz"])
def test_stamped_build_equals_the_frame_table_and_the_reference_batch_tensors(case):
    z, st, hum, rob = capture_frames(case)
    dt, past = float(z["time_step"]), int(z["past"])
    want = SC.frame_table(*as_lists(st, hum, rob), dt, past)
    eng = engine_for()
    out = eng.build_scene_stamped(st, hum, rob, dt, horizon=int(z["H"]))
    assert int(out["n_grid"]) == past
    fr = eng.scene_frames()
    for key, w in zip(("human_xy", "robot_xy", "pose_now"), want):
        assert fr[key].dtype == np.float64 and bits_equal(fr[key], w), f"{case}: {key} differs from scene.frame_table"
    ids = np.nonzero(out["in_cluster"])[0]
    np.testing.assert_array_equal(ids, z["node_ids"])
    arr = eng.scene_arrays()
    for key in ("x_st", "nbr_sum", "edge_mask"):
        assert np.array_equal(arr[key][ids], z[key]), f"{case}: {key} differs from the reference's"
    sb = SC.build_scene(want[0], want[1], dt, int(z["H"]), past)
    for i in sb.ids_out:
        np.testing.assert_array_equal(out["cv"][int(i)], sb.cv_forecasts[int(i)])


# ------------------------------------------------------------------------------------------------ 2. batched raw sets
@pytest.mark.parametrize("name", sorted(RAW_SETS))
def test_batched_stamped_build_equals_the_host_twin(name):
    E, R, N, seed = RAW_SETS[name]
    stamps, hum, rob, n_frames = raw_batch(E, R, N, seed)
    ref = SC.frame_table_frames_batched(stamps, hum, rob, n_frames, DT, F)
    eng = engine_for()
    out = eng.build_scene_stamped(stamps, hum, rob, DT, horizon=12, n_frames=n_frames)
    np.testing.assert_array_equal(out["n_grid"], ref["n_grid"])
    fr = eng.scene_frames()
    for key in ("human_xy", "robot_xy", "pose_now"):
        assert fr[key].shape == ref[key].shape and bits_equal(fr[key], ref[key]), f"{name}: {key} differs from the host twin"
    # ... and the scene on that grid is jmid_build_scene's
    sc = SC.build_scenes_batched(ref["human_xy"], ref["robot_xy"], DT, horizon=12)
    np.testing.assert_array_equal(out["in_cluster"], sc["in_cluster"])
    assert bits_equal(out["cv"], sc["cv"])
    arr = eng.scene_arrays()
    for key in ("x", "x_st", "nbr_sum", "edge_mask", "p0"):
        assert np.array_equal(arr[key].view(np.uint32), sc[key].view(np.uint32)), f"{name}: {key}"
    # a plain build leaves its own input as the grid and the last frame as pose_now
    eng.build_scene(ref["human_xy"], ref["robot_xy"], DT)
    fr = eng.scene_frames()
    assert bits_equal(fr["human_xy"], ref["human_xy"]) and bits_equal(fr["robot_xy"], ref["robot_xy"])
    assert bits_equal(fr["pose_now"], ref["human_xy"][:, -1])


# ------------------------------------------------------------------------------------------------ 3. forecast_scene
@pytest.mark.parametrize("case", ["wrapper_jmid_topk.npz", "wrapper_jmid_together.npz", "wrapper_jmid_spread.npz",
                                  "wrapper_jmid_one_human.npz", "wrapper_imid_together.npz"])
def test_forecast_scene_equals_predict_scene_and_the_host_assembly(case):
    z, st, hum, rob = capture_frames(case)
    K, k, H, dt, N = int(z["K"]), int(z["k_ret"]), int(z["H"]), float(z["time_step"]), int(z["N"])
    eng = engine_for(ctx_dim=32, joint=bool(z["joint"]), wseed=int(z["wseed"]), step=2)
    out = eng.build_scene_stamped(st, hum, rob, dt, horizon=H)
    A = int(out["n_in"])
    assert (k < K) == ("topk" in case) and (A < N) == ("spread" in case)
    pose_now = eng.scene_frames()["pose_now"]
    x_T = torch.randn([1, K * A, H, 2], generator=torch.Generator().manual_seed(int(z["dseed"]))).numpy()
    for precision in ("f32", "f16mx"):
        rows, lw = eng.predict_scene(x_T, k, dt=dt, precision=precision)
        want = SC.assemble_forecasts(out["in_cluster"], rows[0], None if lw is None else lw[0], out["cv"], pose_now, k, K)
        got = eng.forecast_scene(x_T, k, dt=dt, precision=precision)
        assert got[0].shape == (N, k, H + 1, 2) and got[1].shape == (N, k) and got[0].dtype == got[1].dtype == np.float64
        assert bits_equal(got[0], want[0]), f"{case} {precision}: forecasts"
        assert logw_matches(got[1], want[1], k, K), f"{case} {precision}: logw"
        assert bits_equal(eng.forecast_scene(x_T, k, dt=dt, precision=precision)[0], want[0])      # the scene stays resident


def test_batched_forecast_scene_equals_the_host_assembly():
    """E > 1 with rows outside the cluster and more than one block of assemble_kernel (E * N * k > 256); predict_batch's switch."""
    E, N, K, k, H = 16, 6, 16, 5, 8
    hum, rob = random_positions(E, N, 67, half_width=5.0)
    eng = engine_for()
    b = eng.build_scene(hum, rob, DT, horizon=H)
    A = int(np.bincount(b["n_in"]).argmax())
    eps = np.nonzero(b["n_in"] == A)[0]
    assert len(eps) >= 2 and A < N
    x_T = torch.randn([len(eps), K * A, H, 2], generator=torch.Generator().manual_seed(3)).numpy()
    for kk in (k, K):
        g = eng.build_scene(hum[eps], rob[eps], DT, horizon=H)
        rows, lw = eng.predict_scene(x_T, kk, dt=DT, precision="f16mx")
        want = SC.assemble_forecasts(g["in_cluster"], rows, lw, g["cv"], hum[eps][:, -1], kk, K)
        got = eng.forecast_scene(x_T, kk, dt=DT, precision="f16mx")
        assert bits_equal(got[0], want[0]) and logw_matches(got[1], want[1], kk, K)
    seeds = [300 + e for e in range(E)]
    kw = dict(num_samples=K, num_ret_samples=k, horizon=H, time_step=DT, precision="f16mx")
    fc0, lw0, inc0 = predict_batch(eng, hum, rob, seeds, **kw)
    fc1, lw1, inc1 = predict_batch(eng, hum, rob, seeds, device_frames=True, **kw)
    assert len(np.unique(inc0.sum(axis=1))) >= 3
    assert np.array_equal(inc0, inc1) and bits_equal(fc0, fc1) and bits_equal(lw0, lw1)


# ------------------------------------------------------------------------------------------------ 4. the forecaster
def run_forecaster(z, tmp, ctx_dim, device_frames, calls=2, **kw):
    N, K, k_ret, H = int(z["N"]), int(z["K"]), int(z["k_ret"]), int(z["H"])
    env, ypath = write_configs(str(tmp), joint=bool(z["joint"]), ctx_dim=ctx_dim, N=N, K=K, k_ret=k_ret, H=H,
                               step=2 if ctx_dim == 32 else int(z["step"]), time_step=float(z["time_step"]))
    f = HumanTrajectoryForecasterSim(env, ypath, weights=JMIDWeights.from_seed(NetDims(ctx_dim=ctx_dim), int(z["wseed"])),
                                     device_frames=device_frames, **kw)
    assert f.device_frames is device_frames
    for r, h, t in zip(z["robot_xy"], z["human_xy"], z["stamps"]):
        f.update_state_hists(State(r), [State(p) for p in h], float(t))
    torch.manual_seed(int(z["dseed"]))
    torch.cuda.manual_seed(int(z["dseed"]))
    results = [f.predict_ret_best() for _ in range(calls)]
    assert set(f.timings) == {"scene_ms", "device_ms", "topk_ms", "assemble_ms", "total_ms"}
    return results, torch.get_rng_state(), torch.cuda.get_rng_state(0)


@pytest.mark.parametrize("case", ["wrapper_jmid_together.npz", "wrapper_jmid_jitter.npz", "wrapper_jmid_gap.npz",
                                  "wrapper_jmid_spread.npz", "wrapper_jmid_topk.npz"])
def test_forecaster_with_device_frames_equals_the_host_path(case, tmp_path):
    z = np.load(os.path.join(GOLDEN, case))
    N, K, k_ret, H = int(z["N"]), int(z["K"]), int(z["k_ret"]), int(z["H"])
    # the first call of a shape is the self check on the staged path (scene_arrays / scene_frames, host assembly), the second the
    # one-entry path (jmid_forecast_scene)
    off = run_forecaster(z, tmp_path / "off", 32, False)
    on = run_forecaster(z, tmp_path / "on", 32, True)
    for a, b in zip(off[0], on[0]):
        assert b[0].shape == (N, k_ret, H + 1, 2) and b[0].dtype == np.float64 and b[1].shape == (N, k_ret) and b[1].dtype == np.float64
        assert bits_equal(a[0], b[0]), f"{case}: forecasts"
        assert logw_matches(b[1], a[1], k_ret, K), f"{case}: logw"
    assert torch.equal(off[1], on[1]) and torch.equal(off[2], on[2])


@pytest.mark.parametrize("case", ["wrapper_jmid_jitter.npz", "wrapper_jmid_gap.npz"])
def test_forecaster_with_device_frames_holds_the_reference_gate(case, tmp_path):
    z = np.load(os.path.join(GOLDEN, case))
    assert int(z["ctx_dim"]) == 256 and int(z["k_ret"]) >= int(z["K"])
    (got,), _, _ = run_forecaster(z, tmp_path, 256, True, calls=1, rng_compat="cpu", precision="f16x3")     # (no self check: the one-entry path)
    forecasts, logw = got
    ade = np.linalg.norm(forecasts - z["forecasts"], axis=-1).mean()
    print(f"{case}: mean ADE(forecasts) vs reference = {ade:.3e}")
    assert ade <= 1e-4
    np.testing.assert_allclose(logw, z["logw"], rtol=0, atol=1e-3)


def test_hand_edited_histories_take_the_host_frame_table(tmp_path):
    z = np.load(os.path.join(GOLDEN, "wrapper_jmid_together.npz"))
    N, K, k_ret, H = int(z["N"]), int(z["K"]), int(z["k_ret"]), int(z["H"])
    env, ypath = write_configs(str(tmp_path), joint=True, ctx_dim=32, N=N, K=K, k_ret=k_ret, H=H, step=2, time_step=float(z["time_step"]))
    w = JMIDWeights.from_seed(NetDims(ctx_dim=32), int(z["wseed"]))
    res = []
    for flag in (False, True):
        f = HumanTrajectoryForecasterSim(env, ypath, weights=w, device_frames=flag, precision="f32")
        for r, h, t in zip(z["robot_xy"], z["human_xy"], z["stamps"]):
            f.update_state_hists(State(r), [State(p) for p in h], float(t))
        f.prev_states[1][2][2] += 1e-3               # one human's stamp no longer matches the others': the join drops that frame
        torch.manual_seed(1)
        res.append(f.predict_ret_best())
    assert bits_equal(res[0][0], res[1][0]) and bits_equal(res[0][1], res[1][1])


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_keep_the_resident_scene():
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=32), 5), joint=True, hist_len=6, step=2)
    E, R, N, seed = RAW_SETS["spread"]
    stamps, hum, rob, n_frames = raw_batch(E, R, N, seed)
    x4 = np.zeros((1, 4, 4, 2), np.float32)

    def einval(fn, *args, **kw):
        with pytest.raises(JmidError) as ei:
            fn(*args, **kw)
        assert ei.value.code == -1, ei.value

    einval(eng.scene_frames)                                         # nothing resident yet
    einval(eng.forecast_scene, x4, 4, dt=DT)                         # forecast_scene without a scene
    eng.build_scene_stamped(stamps, hum, rob, DT, horizon=4, n_frames=n_frames)
    resident = eng.scene_arrays()["x_st"].copy()
    grid = eng.scene_frames()["human_xy"].copy()

    def still_resident():
        return np.array_equal(eng.scene_arrays()["x_st"], resident) and bits_equal(eng.scene_frames()["human_xy"], grid)

    # too short a history: JMID_EHISTORY, n_grid_out filled
    short = n_frames.copy()
    short[3] = 4
    with pytest.raises(SC.HistoryTooShortError) as ei:
        eng.build_scene_stamped(stamps, hum, rob, DT, horizon=4, n_frames=short)
    want = SC.frame_table_frames_batched(stamps, hum, rob, short, DT, F)["n_grid"]
    assert want[3] < F and np.array_equal(ei.value.n_grid, want) and "episode 3" in str(ei.value)
    inc = np.empty((E, N), np.uint8); rin = np.empty(E, np.uint8); n_in = np.empty(E, np.int32); ng = np.full(E, -9, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    call = lambda R_, nf, dt: eng._lib.jmid_build_scene_stamped(eng._h, E, N, R_, ptr(stamps), ptr(hum), ptr(rob), ptr(nf) if nf is not None else None,
                                                                dt, 0, 0, ptr(inc), ptr(rin), ptr(n_in), ptr(ng), None, _lib.MEM_HOST)
    assert call(R, short, DT) == -7 and np.array_equal(ng, want) and still_resident()
    assert call(0, None, DT) == -1 and call(65, None, DT) == -1                                     # R = 0, R = 65
    for bad in (0, R + 1, -1):                                                                       # n_frames outside 1..R
        nf = n_frames.copy()
        nf[E - 1] = bad
        assert call(R, nf, DT) == -1
    for bad_dt in (float("nan"), float("inf"), 0.0, -0.25, 0.004):                                   # round(0.4) = 0
        assert call(R, n_frames, bad_dt) == -1
    assert still_resident()
    # forecast_scene: T must be the build's horizon; a scene built without cv has none
    A = int(eng._scene_n_in[0])
    one = np.nonzero(eng._scene_n_in == A)[0][:1]
    eng.build_scene_stamped(stamps[one], hum[one], rob[one], DT, horizon=4, n_frames=n_frames[one])
    xa = torch.randn([1, 4 * A, 4, 2], generator=torch.Generator().manual_seed(1)).numpy()
    einval(eng.forecast_scene, np.zeros((1, 4 * A, 5, 2), np.float32), 4, dt=DT)
    fc, lw = eng.forecast_scene(xa, 4, dt=DT)                        # ... and the handle still forecasts
    assert fc.shape == (1, N, 4, 5, 2) and np.isfinite(fc).all()
    eng.build_scene_stamped(stamps[one], hum[one], rob[one], DT, n_frames=n_frames[one])
    einval(eng.forecast_scene, xa, 4, dt=DT)
    assert np.isfinite(eng.predict_scene(xa, 4, dt=DT)[0]).all()      # (predict_scene needs no cv)
    eng.close()
