"""Pedestrians who are not seen now, on the device: left out of the scene (jmid_build_scene_absent, csrc/scene.hpp) or coasted to the
anchor frame (jmid_build_scene_stamped_coast, csrc/frames.hpp: track_frames_coast_kernel), against the host twins
(scene.frame_table_tracks(max_coast=), scene.build_scenes_batched(allow_absent=True); pinned by tests/test_absent_tracks_host.py),
today's builds with the left-out columns removed, and the forecaster's host route - bit for bit: selections plus one fp64 multiply-add
without FMA contraction."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from safe_interactive_crowdnav_amd import _lib
from safe_interactive_crowdnav_amd import scene as SC
from safe_interactive_crowdnav_amd.engine import JmidEngine, JmidError
from safe_interactive_crowdnav_amd.forecaster import HumanTrajectoryForecasterSim, predict_batch, write_configs
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

E, N, R, F, H, K, k, DT = 4, 4, 9, 6, 4, 3, 2, 0.25
SEED = 31
_ENGINE, _BUILT = [], {}


def engine():
    if not _ENGINE:
        _ENGINE.append(JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=32), 5), joint=True, hist_len=F, step=2))     # 2 DDIM steps
    return _ENGINE[0]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class State:
    def __init__(self, p):
        self.position = (float(p[0]), float(p[1]))


def walk(stamps, seed, far=None):
    """Four pedestrians and the robot within one attention radius at the given stamps (``far``: that pedestrian 8 m away)."""
    rng = np.random.default_rng(seed)
    base = np.array([[0.1, 0.2], [-0.9, 0.6], [0.8, 0.9], [-0.3, -0.7]])
    vel = rng.uniform(-0.3, 0.3, (N, 2))
    t = np.asarray(stamps)[:, None, None] - stamps[-1]
    hum = base[None] + vel[None] * t + 0.01 * rng.standard_normal((len(stamps), N, 2))
    if far is not None:
        hum[:, far] += 8.0
    rob = np.array([0.2, -1.0])[None] + np.array([0.0, 0.2])[None] * t[:, 0] + 0.01 * rng.standard_normal((len(stamps), 2))
    return hum, rob


def episodes():
    """stamps [E, R], human_xy [E, R, N, 2], robot_xy [E, R, 2], nine frames on the grid each:
      0  a full window, nobody absent, pedestrian 3 outside the cluster
      1  pedestrian 1 not seen on the two newest frames (b_new = 2, six filled bins behind): coasted at max_coast 2, left out at 1
      2  pedestrian 0 seen once, at bin 1 (step 0: a two-row ego that stands still); pedestrian 2 with b_new = 1 and a hole at bin 2 (the
         step comes from the interpolated row)
      3  pedestrian 3 - the one nearest the robot - never seen, pedestrian 0 with b_new = 4: both left out; pedestrian 2 far away"""
    st = np.stack([5.0 + 2.0 * e + DT * np.arange(R) for e in range(E)])
    parts = [walk(st[e], 60 + e, far={0: 3, 3: 2}.get(e)) for e in range(E)]
    hum, rob = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    hum[1, 7:, 1] = np.nan
    hum[2, :7, 0] = np.nan
    hum[2, 8, 0, 1] = np.nan                                  # (one coordinate is enough)
    hum[2, 8, 2] = np.nan
    hum[2, 6, 2, 0] = np.nan
    hum[3, :, 3] = np.nan
    hum[3, 5:, 0] = np.nan
    return st, hum, rob


COAST = [[0, 0, 0, 0], [0, 2, 0, 0], [1, 0, 1, 0], [-1, 0, 0, -1]]
FIRST = [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 4, 0, 0, 0], [0, -1, 0, 0, -1]]
N_IN = [3, 4, 4, 1]
ARRAYS = ("x", "x_st", "nbr_sum", "edge_mask", "p0", "first_index")


def scene_state(eng, out):
    """Everything a build leaves: the resident arrays and frames, and what it returned."""
    got = dict(eng.scene_arrays())
    got.update(eng.scene_frames())
    got.update({key: out[key] for key in ("in_cluster", "robot_in_cluster", "n_in", "cv")})
    return got


def assert_same_state(got, want, what):
    assert set(got) == set(want)
    for key in want:
        assert same(got[key], want[key]), f"{what}: {key}"


def built():
    """The four episodes built once with max_coast = 2: (twin, what the build returned, the state it left) - read-only."""
    if not _BUILT:
        st, hum, rob = episodes()
        ref = SC.frame_table_tracks_batched(st, hum, rob, None, DT, F, max_coast=2)
        eng = engine()
        out = eng.build_scene_stamped(st, hum, rob, DT, horizon=H, tracks=True, max_coast=2)
        _BUILT.update(ref=ref, out=out, state=scene_state(eng, out))
    return _BUILT["ref"], _BUILT["out"], _BUILT["state"]


# ------------------------------------------------------------------------------------------------ 1, 3. the build
def test_coast_build_equals_the_host_twin_and_the_absent_build_on_its_grid():
    ref, out, got = built()
    assert ref["coast"].tolist() == COAST and ref["first_frame"].tolist() == FIRST and ref["n_grid"].tolist() == [F] * E
    for key in ("n_grid", "first_frame", "coast"):
        assert out[key].dtype == np.int32 and same(out[key], ref[key]), f"{key} differs from the host twin"
    for key in ("human_xy", "robot_xy", "pose_now"):
        assert got[key].dtype == np.float64 and same(got[key], ref[key]), f"{key} differs from the host twin"
    assert out["n_in"].tolist() == N_IN and same(got["first_index"], ref["first_frame"][:, 1:])
    # the coasted ones are nodes like any other; pose_now = the last grid row for everybody here
    assert out["in_cluster"][1, 1] and out["in_cluster"][2, 0] and out["in_cluster"][2, 2] and not out["in_cluster"][3, [0, 3]].any()
    assert same(got["pose_now"], ref["human_xy"][:, F - 1])
    assert same(got["x"][2, 0, 4:, 2:], np.zeros((2, 4), np.float32))                           # seen once: no velocity, no acceleration
    eng = engine()
    want = scene_state(eng, eng.build_scene(ref["human_xy"], ref["robot_xy"], DT, horizon=H, first_frame=ref["first_frame"], allow_absent=True))
    assert_same_state(got, want, "against build_scene(first_frame=, allow_absent=True)")
    # ... and the host scene twin
    sc = SC.build_scenes_batched(ref["human_xy"], ref["robot_xy"], DT, horizon=H, first_frame=ref["first_frame"], allow_absent=True)
    for key in ARRAYS + ("in_cluster", "robot_in_cluster", "cv"):
        assert same(got[key], sc[key]), f"{key} differs from scene.build_scenes_batched(allow_absent=True)"
    # max_coast = 1: pedestrian 1 of episode 1 is left out, everybody else's grid as before
    st, hum, rob = episodes()
    ref1 = SC.frame_table_tracks_batched(st, hum, rob, None, DT, F, max_coast=1)
    out1 = eng.build_scene_stamped(st, hum, rob, DT, horizon=H, tracks=True, max_coast=1)
    assert ref1["coast"][1].tolist() == [0, -1, 0, 0] and same(out1["coast"], ref1["coast"]) and same(out1["first_frame"], ref1["first_frame"])
    fr = eng.scene_frames()
    assert all(same(fr[key], ref1[key]) for key in ("human_xy", "robot_xy", "pose_now")) and out1["n_in"].tolist() == [3, 3, 4, 1]


def test_device_memory_mode_equals_host_memory_mode():
    ref, out, want = built()
    st, hum, rob = episodes()
    eng = engine()
    eng.build_scene(np.zeros((1, F, 1, 2)), np.ones((1, F, 2)), DT)                      # (something else resident in between)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ds, dh, dr = dev(st), dev(hum), dev(rob)
    inc, rin = torch.zeros((E, N), dtype=torch.uint8, device="cuda"), torch.zeros(E, dtype=torch.uint8, device="cuda")
    n_in, n_grid = torch.zeros(E, dtype=torch.int32, device="cuda"), torch.zeros(E, dtype=torch.int32, device="cuda")
    first, coast = torch.full((E, N + 1), -9, dtype=torch.int32, device="cuda"), torch.full((E, N), -9, dtype=torch.int32, device="cuda")
    cv = torch.zeros((E, N, H, 2), dtype=torch.float64, device="cuda")
    eng._check(eng._lib.jmid_build_scene_stamped_coast(eng._h, E, N, R, ptr(ds), ptr(dh), ptr(dr), None, DT, H, 0, ptr(inc), ptr(rin), ptr(n_in),
                                                       ptr(n_grid), ptr(cv), ptr(first), 2, ptr(coast), eng._mem(True)))
    torch.cuda.synchronize()
    eng._scene_shape, eng._scene_n_in = (E, N, F, False), n_in.cpu().numpy()             # what the engine's own build notes
    got = dict(eng.scene_arrays())
    got.update(eng.scene_frames())
    got.update(in_cluster=inc.cpu().numpy().astype(bool), robot_in_cluster=rin.cpu().numpy().astype(bool), n_in=n_in.cpu().numpy(), cv=cv.cpu().numpy())
    assert_same_state(got, want, "JMID_MEM_DEVICE against JMID_MEM_HOST")
    assert n_grid.cpu().tolist() == [F] * E and same(first.cpu().numpy(), out["first_frame"]) and same(coast.cpu().numpy(), out["coast"])
    # the grid-level entry: device grids, first_frame a host array in both modes
    dg, dgr = dev(ref["human_xy"]), dev(ref["robot_xy"])
    ff = np.ascontiguousarray(ref["first_frame"])
    eng._check(eng._lib.jmid_build_scene_absent(eng._h, E, N, F, ptr(dg), ptr(dgr), C.c_void_p(ff.ctypes.data), DT, H, 0, ptr(inc), ptr(rin), ptr(n_in),
                                                ptr(cv), eng._mem(True)))
    torch.cuda.synchronize()
    got = dict(eng.scene_arrays())
    got.update(eng.scene_frames())
    got.update(in_cluster=inc.cpu().numpy().astype(bool), robot_in_cluster=rin.cpu().numpy().astype(bool), n_in=n_in.cpu().numpy(), cv=cv.cpu().numpy())
    assert_same_state(got, want, "jmid_build_scene_absent, JMID_MEM_DEVICE")


# ------------------------------------------------------------------------------------------------ 2. nobody absent: today's build
def test_nobody_absent_is_todays_tracks_build():
    s0 = 5.0 + DT * np.arange(R)
    s1 = 3.0 + np.cumsum([0.0, 0.26, 0.25, 0.0, 0.12, 0.6, 0.25, 0.05, 0.25])     # jitter, a duplicate, an empty bin
    st = np.stack([s0, s1])
    parts = [walk(s0, 50, far=3), walk(s1, 51)]
    hum, rob = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    hum[1, :4, 1] = np.nan                                    # a late pedestrian and a hole: per-track windows, everybody seen now
    hum[1, 6, 2] = np.nan
    eng = engine()
    x_T = torch.randn([2, K * N, H, 2], generator=torch.Generator().manual_seed(12)).numpy()
    states, forecasts = [], []
    for c in (None, 2):
        out = eng.build_scene_stamped(st, hum, rob, DT, horizon=H, tracks=True, max_coast=c)
        assert out["n_grid"].tolist() == [F, F] and out["n_in"].tolist() == [3, 4] and (out["first_frame"] >= 0).all()
        assert ("coast" in out) == (c is not None) and (c is None or not out["coast"].any())
        states.append((scene_state(eng, out), out["n_grid"], out["first_frame"]))
        forecasts.append([eng.forecast_scene_padded(x_T, k, dt=DT, precision=p) for p in ("f32", "f16mx")])
    assert states[0][2][1].tolist() != [0] * (N + 1)
    assert_same_state(states[1][0], states[0][0], "max_coast=2 against today's tracks build")
    assert same(states[1][1], states[0][1]) and same(states[1][2], states[0][2])
    for (fc0, lw0), (fc1, lw1) in zip(*forecasts):
        assert np.isfinite(fc0).all() and same(fc0, fc1) and same(lw0, lw1)
    # ... and the grid-level entry without a -1: the bytes of jmid_build_scene_var
    ref = SC.frame_table_tracks_batched(st, hum, rob, None, DT, F)
    a = scene_state(eng, eng.build_scene(ref["human_xy"], ref["robot_xy"], DT, horizon=H, first_frame=ref["first_frame"]))
    b = scene_state(eng, eng.build_scene(ref["human_xy"], ref["robot_xy"], DT, horizon=H, first_frame=ref["first_frame"], allow_absent=True))
    assert_same_state(b, a, "allow_absent=True without a -1")


# ------------------------------------------------------------------------------------------------ 4. left out = not there
def test_present_tracks_equal_the_episode_built_alone_without_the_left_out_columns():
    ref, out, got = built()
    st, hum, rob = episodes()
    eng = engine()
    for e in range(E):
        keep = ref["first_frame"][e, 1:] >= 0
        ids = dict(seed=SEED, episode_ids=np.array([100 + e]), K=K, T=H)
        o1 = eng.build_scene_stamped(st[e], hum[e], rob[e], DT, horizon=H, tracks=True, max_coast=2)
        fc, lw = eng.forecast_scene(None, k, dt=DT, precision="f32", **ids)
        assert fc.shape == (N, k, H + 1, 2) and lw.shape == (N, k) and o1["n_in"] == N_IN[e]
        alone = eng.build_scene(ref["human_xy"][e][:, keep], ref["robot_xy"][e], DT, horizon=H, first_frame=ref["first_frame"][e][np.r_[True, keep]])
        arrays = eng.scene_arrays()
        want_fc, want_lw = eng.forecast_scene(None, k, dt=DT, precision="f32", **ids)
        assert np.isfinite(want_fc).all() and same(fc[keep], want_fc) and same(lw[keep], want_lw), f"episode {e}: forecasts"
        assert np.isnan(fc[~keep]).all() and np.isnan(lw[~keep]).all()
        for key in ARRAYS:                                    # the resident rows of the batch of four
            assert same(got[key][e][keep], arrays[key]), f"episode {e}: {key}"
        assert same(got["in_cluster"][e][keep], alone["in_cluster"]) and same(got["cv"][e][keep], alone["cv"])
        assert got["robot_in_cluster"][e] == alone["robot_in_cluster"] and got["n_in"][e] == alone["n_in"]
        for key in ("x", "x_st", "nbr_sum", "edge_mask", "p0"):
            assert np.isnan(got[key][e][~keep]).all()
        assert np.isnan(got["cv"][e][~keep]).all() and not got["in_cluster"][e][~keep].any() and (got["first_index"][e][~keep] == -1).all()
    assert (ref["first_frame"][3, 1:] < 0).sum() == 2


# ------------------------------------------------------------------------------------------------ 5, 6. the padded chain
@pytest.mark.parametrize("precision", ["f32", "f16mx"])
def test_padded_forecasts_equal_the_absent_build_on_the_twins_grid(precision):
    ref, _, _ = built()
    st, hum, rob = episodes()
    eng = engine()
    x_T = torch.randn([E, K * max(N_IN), H, 2], generator=torch.Generator().manual_seed(11)).numpy()
    eng.build_scene_stamped(st, hum, rob, DT, horizon=H, tracks=True, max_coast=2)
    fc, lw = eng.forecast_scene_padded(x_T, k, dt=DT, precision=precision)
    eng.build_scene(ref["human_xy"], ref["robot_xy"], DT, horizon=H, first_frame=ref["first_frame"], allow_absent=True)
    want_fc, want_lw = eng.forecast_scene_padded(x_T, k, dt=DT, precision=precision)
    assert fc.shape == (E, N, k, H + 1, 2) and lw.shape == (E, N, k) and same(fc, want_fc) and same(lw, want_lw)
    gone = ref["first_frame"][:, 1:] < 0
    assert gone.sum() == 2 and np.isnan(fc[gone]).all() and np.isnan(lw[gone]).all() and np.isfinite(fc[~gone]).all() and np.isfinite(lw[~gone]).all()
    assert same(fc[~gone][:, :, 0], np.repeat(ref["pose_now"][~gone][:, None], k, axis=1))      # the coasted pose is the one prepended


def test_predict_batch_with_first_frame():
    ref, _, _ = built()
    eng = engine()
    hum, rob, ff = ref["human_xy"], ref["robot_xy"], ref["first_frame"]
    seeds = 100 + np.arange(E)
    kw = dict(num_samples=K, num_ret_samples=k, horizon=H, time_step=DT, precision="f32", noise="device", seed=SEED, first_frame=ff)
    host = predict_batch(eng, hum, rob, seeds, **kw)
    grouped = predict_batch(eng, hum, rob, seeds, device_frames=True, **kw)
    resident = predict_batch(eng, hum, rob, seeds, padded="resident", **kw)
    gone = ff[:, 1:] < 0
    for fc, lw, inc in (host, grouped, resident):
        assert fc.shape == (E, N, k, H + 1, 2) and np.isnan(fc[gone]).all() and np.isnan(lw[gone]).all() and not inc[gone].any()
        assert np.isfinite(fc[~gone]).all() and np.isfinite(lw[~gone]).all() and inc.sum(axis=1).tolist() == N_IN
    assert all(same(a, b) for a, b in zip(host, grouped))   # (head_dim 16, f32, device noise: the same bits staged and chained)
    # one padded call: an episode without padding has the grouped call's bits, and so has every constant-velocity row
    full = np.nonzero(np.asarray(N_IN) == max(N_IN))[0]
    assert same(resident[2], grouped[2]) and same(resident[0][full], grouped[0][full]) and same(resident[1][full], grouped[1][full])
    assert same(resident[0][~grouped[2] & ~gone], grouped[0][~grouped[2] & ~gone])
    # per episode: the batch without him
    for e in range(E):
        keep = ~gone[e]
        one = predict_batch(eng, hum[e:e + 1][:, :, keep], rob[e:e + 1], seeds[e:e + 1], **{**kw, "first_frame": ff[e:e + 1][:, np.r_[True, keep]]})
        assert same(host[0][e][keep], one[0][0]) and same(host[1][e][keep], one[1][0]) and same(host[2][e][keep], one[2][0])
    with pytest.raises(ValueError):
        predict_batch(eng, hum, rob, seeds, padded=True, **{**kw, "noise": "torch"})


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_keep_the_resident_scene():
    st, hum, rob = episodes()
    ref = SC.frame_table_tracks_batched(st, hum, rob, None, DT, F, max_coast=2)
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=32), 5), joint=True, hist_len=F, step=2)
    resident = scene_state(eng, eng.build_scene_stamped(st, hum, rob, DT, horizon=H, tracks=True, max_coast=2))
    kept = {key: resident[key].copy() for key in ARRAYS + ("human_xy", "robot_xy", "pose_now")}

    def still_resident():
        now = dict(eng.scene_arrays())
        now.update(eng.scene_frames())
        return all(same(now[key], kept[key]) for key in kept)

    inc, rin, n_in = np.empty((E, N), np.uint8), np.empty(E, np.uint8), np.empty(E, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)

    def raw_call(hum_, nf_, c):
        ng, first, coast = np.full(E, -9, np.int32), np.full((E, N + 1), -9, np.int32), np.full((E, N), -9, np.int32)
        rc = eng._lib.jmid_build_scene_stamped_coast(eng._h, E, N, R, ptr(st), ptr(hum_), ptr(rob), None if nf_ is None else ptr(nf_), DT, 0, 0, ptr(inc),
                                                     ptr(rin), ptr(n_in), ptr(ng), None, ptr(first), c, ptr(coast), _lib.MEM_HOST)
        return rc, ng, first, coast, eng._lib.jmid_last_error(eng._h).decode()

    # max_coast outside 0..F-2: before anything runs
    for c in (-1, F - 1):
        rc, ng, first, coast, msg = raw_call(hum, None, c)
        assert rc == _lib.EINVAL and "max_coast" in msg and (ng == -9).all() and (coast == -9).all()
        with pytest.raises(JmidError):
            eng.build_scene_stamped(st, hum, rob, DT, horizon=H, tracks=True, max_coast=c)
        assert still_resident()
    with pytest.raises(ValueError):
        eng.build_scene_stamped(st, hum, rob, DT, horizon=H, max_coast=1)
    # fewer than 2 grid frames: JMID_EHISTORY, the outputs filled
    short = np.array([R, 1, R, R], dtype=np.int32)
    want = SC.frame_table_tracks_batched(st, hum, rob, short, DT, F, max_coast=2)
    rc, ng, first, coast, msg = raw_call(hum, short, 2)
    assert rc == _lib.EHISTORY and ng.tolist() == [F, 1, F, F] and "episode 1" in msg and same(first, want["first_frame"]) and same(coast, want["coast"])
    with pytest.raises(SC.HistoryTooShortError):
        eng.build_scene_stamped(st, hum, rob, DT, horizon=H, n_frames=short, tracks=True, max_coast=2)
    assert still_resident()
    # an episode with nobody left: JMID_EINVAL names it, the outputs filled
    empty = hum.copy()
    empty[3, 4:, 1:3] = np.nan                               # the two who were left are last seen at bin 5
    want = SC.frame_table_tracks_batched(st, empty, rob, None, DT, F, max_coast=2)
    assert (want["first_frame"][3, 1:] == -1).all()
    rc, ng, first, coast, msg = raw_call(empty, None, 2)
    assert rc == _lib.EINVAL and "episode 3" in msg and same(ng, want["n_grid"]) and same(first, want["first_frame"]) and same(coast, want["coast"])
    with pytest.raises(JmidError) as ei:
        eng.build_scene_stamped(st, empty, rob, DT, horizon=H, tracks=True, max_coast=2)
    assert ei.value.code == _lib.EINVAL and still_resident()
    # the grid-level entry: everybody -1, the robot -1, below -1
    grid = (ref["human_xy"], ref["robot_xy"], DT)
    for e, j, v, word in ((1, slice(1, None), -1, "episode 1"), (0, 0, -1, "first_frame[0, 0]"), (2, 3, -2, "first_frame[2, 3]")):
        bad = ref["first_frame"].copy()
        bad[e, j] = v
        with pytest.raises(JmidError) as ei:
            eng.build_scene(*grid, horizon=H, first_frame=bad, allow_absent=True)
        assert ei.value.code == _lib.EINVAL and word in str(ei.value) and still_resident()
    # today's entries keep their refusals
    with pytest.raises(JmidError) as ei:
        eng.build_scene(*grid, horizon=H, first_frame=ref["first_frame"])
    assert ei.value.code == _lib.EINVAL and still_resident()
    with pytest.raises(SC.TrackAbsentError):
        eng.build_scene_stamped(st, hum, rob, DT, horizon=H, tracks=True)
    assert still_resident()
    # ... and the handle still forecasts on the resident scene
    x_T = torch.randn([E, K * max(N_IN), H, 2], generator=torch.Generator().manual_seed(13)).numpy()
    fc = eng.forecast_scene_padded(x_T, k, dt=DT)[0]
    assert np.isfinite(fc[ref["first_frame"][:, 1:] >= 0]).all()
    eng.close()


# ------------------------------------------------------------------------------------------------ 9. the forecaster
def feed(i):
    """Frame i of four pedestrians and the robot: pedestrian 2 is occluded at frames 3 and 4 and gone for good from frame 6 on."""
    t = 1.0 + DT * i
    hum = np.array([[0.1 + 0.3 * t, 0.2 + 0.05 * t * t], [-0.9 - 0.2 * t, 0.6 + 0.3 * t], [0.8 + 0.1 * t * t, 0.9 - 0.4 * t], [-0.4 + 0.1 * t, -0.6]])
    if i in (3, 4) or i >= 6:
        hum[2] = np.nan
    return np.array([0.2, -1.4 + 0.2 * t]), hum, t


def forecaster(tmp, n, **kw):
    env, ypath = write_configs(str(tmp), joint=True, ctx_dim=32, N=n, K=K, k_ret=k, H=H, step=2, time_step=DT)
    return HumanTrajectoryForecasterSim(env, ypath, weights=JMIDWeights.from_seed(NetDims(ctx_dim=32), 7), precision="f32", **kw)


def predict(f, seed):
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    try:
        return f.predict_ret_best()
    except SC.HistoryTooShortError as e:
        return e


def test_forecaster_with_coast_frames(tmp_path, monkeypatch):
    kw = dict(track_presence=True, short_history=True, coast_frames=2)
    host = forecaster(tmp_path / "host", N, **kw)
    dev = forecaster(tmp_path / "dev", N, device_frames=True, **kw)
    res = forecaster(tmp_path / "res", N, device_scene=True, **kw)          # the twin's grid, built on the device with its -1
    off = forecaster(tmp_path / "off", N, track_presence=True, short_history=True)
    assert dev.coast_frames == 2 and off.coast_frames == 0
    for bad in (dict(coast_frames=1), dict(track_presence=True, short_history=True, coast_frames=F - 1)):
        with pytest.raises(ValueError):
            forecaster(tmp_path / "bad", N, **bad)
    trace, eng = [], dev.engine
    assert host.engine is eng
    for name in ("build_scene_stamped", "build_scene", "forecast_scene", "predict_scene", "predict", "encode", "denoise"):
        monkeypatch.setattr(eng, name, lambda *a, _call=getattr(eng, name), _name=name, **kw: (trace.append((_name, kw.get("max_coast"), a[1].shape[1] if _name == "build_scene_stamped" else None)), _call(*a, **kw))[1])
    coasted = {3: 1, 4: 2, 6: 1, 7: 2}
    for i in range(9):
        r, h, t = feed(i)
        for f in (host, dev, res, off):
            f.update_state_hists(State(r), [State(p) for p in h], t)
        a, c, d = predict(host, 200 + i), predict(off, 200 + i), predict(res, 200 + i)
        trace.clear()
        b = predict(dev, 200 + i)
        # the device route: ONE build from the raw frames of all N tracks and ONE chain
        assert trace == [("build_scene_stamped", 2, N)] + [("forecast_scene", None, None)] * (i > 0)
        if i == 0:                                           # one frame
            assert all(isinstance(v, SC.HistoryTooShortError) for v in (a, b, c, d))
            continue
        assert same(a[0], d[0]) and same(a[1], d[1]), f"frame {i}: device_scene differs from the host route"
        assert a[0].shape == (N, k, H + 1, 2) and a[1].shape == (N, k) and a[0].dtype == a[1].dtype == np.float64
        assert same(a[0], b[0]) and same(a[1], b[1]), f"frame {i}: device_frames differs from the host route"
        others = [0, 1, 3]
        assert np.isfinite(a[0][others]).all() and np.isfinite(a[1][others]).all()
        assert same(a[0][others][:, :, 0], np.repeat(h[others][:, None], k, axis=1))
        if i in coasted:                                     # finite, from his coasted pose on; without coasting his rows are NaN
            assert np.isfinite(a[0][2]).all() and np.isfinite(a[1][2]).all() and np.isnan(c[0][2]).all()
            twin = SC.frame_table_tracks(*SC.histories_as_frames(host.prev_states, host.prev_robot_states, joined=False), DT, F, max_coast=2)
            assert twin[5].tolist() == [0, 0, coasted[i], 0] and same(a[0][2, :, 0], np.repeat(twin[2][2][None], k, axis=0))
            if i < 5:                                        # his last step, repeated (from frame 6 on it comes from an interpolated row)
                seen = feed(i - coasted[i])[1][2]
                step = seen - feed(i - coasted[i] - 1)[1][2]
                assert same(twin[2][2], seen + float(coasted[i]) * step)
        elif i == 8:                                         # last seen three bins ago: left out
            assert np.isnan(a[0][2]).all() and np.isnan(a[1][2]).all()
            assert same(a[0][others], c[0][others]) and same(a[1][others], c[1][others])     # = the host filter's forecasts for the others
        else:
            assert np.isfinite(a[0][2]).all() and same(a[0], c[0]) and same(a[1], c[1])         # everybody seen: today's forecaster
