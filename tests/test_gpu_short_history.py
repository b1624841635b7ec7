"""Short histories on the device: jmid_encode_var (csrc/encoder.hpp: the LSTMs from first_index on), jmid_build_scene_var +
jmid_scene_get_first_index (csrc/scene.hpp: first_frame per node), the chained entries on such a scene, the forecaster's ``short_history``
and ``offline.get_loss(first_history_index=)`` - against the reference's captures (tests/golden/shorthist_*.npz), the host twin
(scene.build_scenes_batched, pinned to those captures by tests/test_short_history_host.py) and engines of a shorter hist_len."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tests.test_gpu_parity as P      # its engines (one per width and seed), ade() and tolerances
import tests.width_cases as WC
from safe_interactive_crowdnav_amd import _lib, offline
from safe_interactive_crowdnav_amd import scene as SC
from safe_interactive_crowdnav_amd.engine import JmidEngine, JmidError
from safe_interactive_crowdnav_amd.forecaster import HumanTrajectoryForecasterSim, predict_batch, write_configs
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims
from tests.test_short_history_host import CASES, DT, F, H, mixed_batch, same_bits

GOLDEN = P.GOLDEN
_ENGINES = {}


def engine_for(ctx_dim=32, hist_len=F, wseed=5, step=2):
    key = (ctx_dim, hist_len, wseed, step)
    if key not in _ENGINES:
        _ENGINES[key] = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=ctx_dim), wseed), joint=True, hist_len=hist_len, step=step)
    return _ENGINES[key]


class State:
    def __init__(self, p):
        self.position = (float(p[0]), float(p[1]))


# ------------------------------------------------------------------------------------------------ 1. the encoder
@pytest.mark.parametrize("ctx_dim", WC.OLD_CTX_DIMS)      # (every hidden size against float64, first_index included: tests/test_gpu_encoder.py)
def test_row_equals_the_slice_on_an_engine_of_that_history_length(ctx_dim):
    """Row r with first_index f is, bit for bit, the row of an engine created with hist_len = F - f fed frames f ..: the same LSTM steps
    from the same zero state.  What stands in front of f - NaN here, in x_st AND nbr_sum - reaches no output."""
    n, fi = 7, np.array([0, 1, 2, 3, 4, 4, 0], dtype=np.int32)
    rng = np.random.default_rng(11 + ctx_dim)
    x_st = rng.standard_normal((n, F, 6)).astype(np.float32)
    nbr = rng.standard_normal((n, 2, F, 6)).astype(np.float32)
    em = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    full = (x_st.copy(), nbr.copy(), em)
    for r, f in enumerate(fi):
        x_st[r, :f] = np.nan
        nbr[r, :, :f] = np.nan
    eng = engine_for(ctx_dim)
    ctx = eng.encode(x_st, nbr, em, first_index=fi)
    assert ctx.shape == (n, ctx_dim) and ctx.dtype == np.float32 and np.isfinite(ctx).all()
    for r, f in enumerate(fi):
        short = engine_for(ctx_dim, hist_len=F - int(f))
        want = short.encode(np.ascontiguousarray(x_st[r:r + 1, f:]), np.ascontiguousarray(nbr[r:r + 1, :, f:]), em[r:r + 1])
        same_bits(ctx[r], want[0])
    # device memory mode: the same bits (first_index stays a host array)
    dev = eng.encode(torch.from_numpy(x_st).cuda(), torch.from_numpy(nbr).cuda(), torch.from_numpy(em).cuda(), first_index=fi)
    same_bits(dev.cpu().numpy(), ctx)
    # None and all zero: the existing jmid_encode
    base = np.empty((n, ctx_dim), np.float32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    eng._check(eng._lib.jmid_encode(eng._h, n, ptr(full[0]), ptr(full[1]), ptr(full[2]), ptr(base), _lib.MEM_HOST))
    same_bits(eng.encode(*full), base)
    same_bits(eng.encode(*full, first_index=None), base)
    same_bits(eng.encode(*full, first_index=np.zeros(n, dtype=np.int64)), base)
    assert not np.array_equal(ctx[1], base[1]) and np.array_equal(ctx[0], base[0])      # a later start is another encoding


def test_encode_var_refuses_on_the_host_and_leaves_the_handle_usable():
    eng = engine_for(32)
    n = 2
    x_st, nbr, em = np.zeros((n, F, 6), np.float32), np.zeros((n, 2, F, 6), np.float32), np.zeros((n, 2), np.float32)
    out = np.empty((n, 32), np.float32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    for bad in ([0, F - 1], [-1, 0]):
        fi = np.asarray(bad, dtype=np.int32)
        rc = eng._lib.jmid_encode_var(eng._h, n, ptr(x_st), ptr(nbr), ptr(em), ptr(fi), ptr(out), _lib.MEM_HOST)
        assert rc == -1 and b"first_index" in eng._lib.jmid_last_error(eng._h)
    assert eng._lib.jmid_encode_var(eng._h, n, ptr(x_st), ptr(nbr), ptr(em), None, ptr(out), _lib.MEM_HOST) == -1
    with pytest.raises(ValueError):
        eng.encode(x_st, nbr, em, first_index=[0, F - 1])
    same_bits(eng.encode(x_st, nbr, em, first_index=np.array([0, F - 2])), eng.encode(x_st, nbr, em, first_index=[0, F - 2]))


def fixture_rows():
    """(name, arrays) of every reference capture that holds encoder inputs and the get_latent output, the loss fixture's rows included."""
    out = list(sorted(CASES.items()))
    z = np.load(os.path.join(GOLDEN, "shorthist_loss_jmid_w32_e2a3t6.npz"))
    d = {k: z[k] for k in z.files}
    d["ctx"] = d["ctx"].reshape(-1, int(z["ctx_dim"]))
    out.append(("loss_jmid_w32_e2a3t6", d))
    return out


@pytest.mark.parametrize("name,z", fixture_rows(), ids=[n for n, _ in fixture_rows()])
def test_context_matches_the_reference_get_latent(name, z):
    """The bound tests/test_gpu_parity.py::test_context_encoder_matches_reference_golden applies to full-length rows."""
    eng, w = P.get_engine(int(z["ctx_dim"]), int(z["wseed"]), True)
    assert w.checksum() == str(z["wsum"])
    assert np.isnan(z["x_st"]).any() or (z["first_hist"] == 0).all()
    ctx = eng.encode(z["x_st"], z["nbr_sum"], z["edge_mask"], first_index=z["first_hist"])
    print(f"{name}: max |ctx - reference| = {np.abs(ctx - z['ctx']).max():.3e}")
    np.testing.assert_allclose(ctx, z["ctx"], rtol=0, atol=5e-6)


# ------------------------------------------------------------------------------------------------ 2. the scene
def check_device_scene(eng, hum, rob, ff, force=False):
    ref = SC.build_scenes_batched(hum, rob, DT, force_all_in_cluster=force, horizon=H, first_frame=ff)
    out = eng.build_scene(hum, rob, DT, horizon=H, force_all_in_cluster=force, first_frame=ff)
    arr = eng.scene_arrays()
    np.testing.assert_array_equal(out["in_cluster"], ref["in_cluster"])
    np.testing.assert_array_equal(out["robot_in_cluster"], ref["robot_in_cluster"])
    np.testing.assert_array_equal(out["n_in"], ref["in_cluster"].sum(axis=1))
    same_bits(out["cv"], ref["cv"])
    for key in ("x", "x_st", "nbr_sum", "edge_mask", "p0"):
        same_bits(arr[key], ref[key])
    assert arr["first_index"].dtype == np.int32
    np.testing.assert_array_equal(arr["first_index"], ref["first_index"])
    return out, arr, ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_scene_equals_the_host_twin_on_every_fixture(name):
    z = CASES[name]
    eng = engine_for()
    out, arr, _ = check_device_scene(eng, z["human_xy"][None], z["robot_xy"][None], z["first_frame"][None])
    rows = np.nonzero(out["in_cluster"][0])[0]
    np.testing.assert_array_equal(rows, z["node_ids"])
    same_bits(arr["nbr_sum"][0, rows], z["nbr_sum"])      # ... and therefore the reference's
    # one scene without the episode axis
    one = eng.build_scene(z["human_xy"], z["robot_xy"], DT, horizon=H, first_frame=z["first_frame"])
    assert one["in_cluster"].shape == (z["human_xy"].shape[1],)
    np.testing.assert_array_equal(eng.scene_arrays()["first_index"], z["first_frame"][1:])


def test_device_scene_on_a_batch_of_full_and_short_episodes():
    hum, rob, ff = mixed_batch()
    out, _, _ = check_device_scene(engine_for(), hum, rob, ff)
    assert list(out["n_in"]) == [3, 4, 3]
    check_device_scene(engine_for(), hum, rob, ff, force=True)
    # junk in front of first_frame is never read
    eng = engine_for()
    junk_h, junk_r = np.where(np.isnan(hum), 1e30, hum), np.where(np.isnan(rob), -7.0, rob)
    eng.build_scene(hum, rob, DT, horizon=H, first_frame=ff)
    want = eng.scene_arrays()
    eng.build_scene(junk_h, junk_r, DT, horizon=H, first_frame=ff)
    got = eng.scene_arrays()
    for key in want:
        np.testing.assert_array_equal(got[key].view(np.uint32), want[key].view(np.uint32))


def test_null_first_frame_is_jmid_build_scene_and_refusals_keep_the_resident_scene():
    hum, rob, ff = mixed_batch()
    hum0, rob0 = hum[:1], rob[:1]                          # the full-history episode
    E, _, N, _ = hum0.shape
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=32), 5), joint=True, hist_len=F, step=2)
    want_out = eng.build_scene(hum0, rob0, DT, horizon=H)
    want = eng.scene_arrays()
    assert (want["first_index"] == 0).all()
    inc, rin, n_in = np.empty((E, N), np.uint8), np.empty(E, np.uint8), np.empty(E, np.int32)
    cv = np.empty((E, N, H, 2))
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    eng._check(eng._lib.jmid_build_scene_var(eng._h, E, N, F, ptr(hum0), ptr(rob0), None, DT, H, 0, ptr(inc), ptr(rin), ptr(n_in), ptr(cv),
                                             _lib.MEM_HOST))
    got = eng.scene_arrays()
    for key in want:
        np.testing.assert_array_equal(got[key].view(np.uint32), want[key].view(np.uint32))
    np.testing.assert_array_equal(inc.astype(bool), want_out["in_cluster"])
    same_bits(cv, want_out["cv"])
    zero = eng.build_scene(hum0, rob0, DT, horizon=H, first_frame=np.zeros((E, N + 1), np.int32))
    np.testing.assert_array_equal(zero["in_cluster"], want_out["in_cluster"])
    for key in want:
        np.testing.assert_array_equal(eng.scene_arrays()[key].view(np.uint32), want[key].view(np.uint32))
    # refusals, all on the host: the resident scene stays
    eng.build_scene(hum, rob, DT, horizon=H, first_frame=ff)
    resident = eng.scene_arrays()
    for bad in (np.where(ff == 4, F, ff), np.where(ff == 4, -1, ff), np.concatenate([np.full((3, 1), F - 1), ff[:, 1:]], axis=1)):
        with pytest.raises(JmidError) as ei:
            eng.build_scene(hum, rob, DT, horizon=H, first_frame=bad.astype(np.int32))
        assert ei.value.code == -1
        now = eng.scene_arrays()
        for key in resident:
            np.testing.assert_array_equal(now[key].view(np.uint32), resident[key].view(np.uint32))
    with pytest.raises(ValueError):
        eng.build_scene(hum, rob, DT, first_frame=ff[:, :4])
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. the chain
@pytest.mark.parametrize("precision", ["f32", "f16mx"])
def test_predict_scene_on_a_var_scene_equals_the_staged_calls(precision):
    z = CASES["oneframe_n4"]                               # ego rows 0, 2, 3 with first_index 0, 1, 2; pedestrian 1 a one-frame neighbour
    A, K, k = 3, 4, 2
    eng = engine_for()
    out = eng.build_scene(z["human_xy"], z["robot_xy"], DT, horizon=H, first_frame=z["first_frame"])
    assert int(out["n_in"]) == A
    arr = eng.scene_arrays()
    rows = np.nonzero(out["in_cluster"])[0]
    x_T = torch.randn([1, K * A, H, 2], generator=torch.Generator().manual_seed(21)).numpy()
    sel, lw = eng.predict_scene(x_T, k, dt=DT, precision=precision)
    pos_all, _ = eng.predict_scene(x_T, K, dt=DT, precision=precision)
    fc, fclw = eng.forecast_scene(x_T, k, dt=DT, precision=precision)
    ctx = eng.encode(arr["x_st"][rows], arr["nbr_sum"][rows], arr["edge_mask"][rows], first_index=arr["first_index"][rows])
    _, pos = eng.denoise(x_T, ctx[None], arr["p0"][rows][None], dt=DT, precision=precision)
    want_sel, want_lw = eng.topk(None, k, dims=(1, A, K, H))
    assert np.isfinite(pos).all()
    same_bits(pos_all, pos)
    same_bits(sel, want_sel)
    same_bits(lw, want_lw)
    want_fc, want_fclw = SC.assemble_forecasts(out["in_cluster"], want_sel[0], want_lw[0], out["cv"], z["human_xy"][-1], k, K)
    same_bits(fc, want_fc)
    same_bits(fclw, want_fclw)
    same_bits(fc[1, 0, 1:], np.repeat(z["human_xy"][-1, 1][None], H, axis=0))           # the one-frame pedestrian stands still
    # the full-window encoding of the same rows is another one: first_index did reach the chained encoder
    full = eng.encode(np.nan_to_num(arr["x_st"][rows]), arr["nbr_sum"][rows], arr["edge_mask"][rows])
    assert not np.array_equal(full[1:], ctx[1:])


# ------------------------------------------------------------------------------------------------ 4. the forecaster
def walk(i):
    """Frame i of three pedestrians and the robot, all within one attention radius."""
    t = DT * i
    hum = np.array([[0.1 + 0.3 * t, 0.2 + 0.05 * t * t], [-0.9 - 0.2 * t, 0.6 + 0.3 * t], [0.8 + 0.1 * t * t, 0.9 - 0.4 * t]])
    return np.array([0.2, -1.4 + 0.2 * t]), hum, t


def test_forecaster_predicts_from_two_frames_on(tmp_path):
    N, K, k, Hh = 3, 6, 3, 6
    env, ypath = write_configs(str(tmp_path), joint=True, ctx_dim=32, N=N, K=K, k_ret=k, H=Hh, step=2, time_step=DT)
    w = JMIDWeights.from_seed(NetDims(ctx_dim=32), 7)
    mk = lambda **kw: HumanTrajectoryForecasterSim(env, ypath, weights=w, precision="f32", **kw)
    short, short_dev, plain = mk(short_history=True), mk(short_history=True, device_scene=True), mk()
    assert plain.short_history is False and short.short_history is True
    eng = short.engine
    raw_h, raw_r = [], []
    for i in range(1, 8):
        r, h, t = walk(i - 1)
        raw_h.append(h)
        raw_r.append(r)
        res = {}
        for name, f in (("short", short), ("short_dev", short_dev), ("plain", plain)):
            f.update_state_hists(State(r), [State(p) for p in h], t)
            torch.manual_seed(100 + i)
            torch.cuda.manual_seed(100 + i)
            try:
                res[name] = f.predict_ret_best()
            except SC.HistoryTooShortError as e:
                res[name] = e
        if i < F:
            assert isinstance(res["plain"], SC.HistoryTooShortError)                 # the default: today's refusal
        if i == 1:
            assert isinstance(res["short"], SC.HistoryTooShortError) and isinstance(res["short_dev"], SC.HistoryTooShortError)
            continue
        fc, lw = res["short"]
        assert fc.shape == (N, k, Hh + 1, 2) and lw.shape == (N, k) and fc.dtype == np.float64 and lw.dtype == np.float64
        assert np.isfinite(fc).all() and np.isfinite(lw).all()
        np.testing.assert_array_equal(fc[:, :, 0], np.repeat(h[:, None], k, axis=1))  # step 0: the current pose
        same_bits(res["short_dev"][0], fc)
        same_bits(res["short_dev"][1], lw)
        if i >= F:
            same_bits(res["plain"][0], fc)
            same_bits(res["plain"][1], lw)
            continue
        # the engine-level chain on the same x_T
        hum, rob, ff = SC.pad_short_window(np.stack(raw_h), np.stack(raw_r), F)
        assert list(ff) == [F - i] * (N + 1)
        b = SC.build_scenes_batched(hum[None], rob[None], DT, horizon=Hh, first_frame=ff[None])
        rows = np.nonzero(b["in_cluster"][0])[0]
        A = len(rows)
        assert A == N
        torch.manual_seed(100 + i)
        x_T = torch.randn([K * A, Hh, 2]).numpy()[None]
        ctx = eng.encode(b["x_st"][0, rows], b["nbr_sum"][0, rows], b["edge_mask"][0, rows], first_index=b["first_index"][0, rows])
        eng.denoise(x_T, ctx[None], b["p0"][:, rows], dt=DT, precision="f32", want_vel=False, want_pos=False)
        sel, slw = eng.topk(None, k, dims=(1, A, K, Hh))
        want_fc, want_lw = SC.assemble_forecasts(b["in_cluster"][0], sel[0], slw[0], b["cv"][0], h, k, K)
        same_bits(fc, want_fc)
        same_bits(lw, want_lw)


def test_predict_batch_takes_short_windows():
    hum = np.stack([np.stack([walk(i)[1] for i in range(3)]), np.stack([walk(i)[1] + 0.05 for i in range(2, 5)])])      # [2, L = 3, 3, 2]
    rob = np.stack([np.stack([walk(i)[0] for i in range(3)]), np.stack([walk(i)[0] for i in range(2, 5)])])
    eng = engine_for()
    kw = dict(num_samples=4, num_ret_samples=2, horizon=H, time_step=DT, precision="f32", short_history=True)
    fc0, lw0, inc0 = predict_batch(eng, hum, rob, [5, 6], **kw)
    fc1, lw1, inc1 = predict_batch(eng, hum, rob, [5, 6], device_scene=True, **kw)
    assert fc0.shape == (2, 3, 2, H + 1, 2) and np.isfinite(fc0).all() and inc0.all()
    same_bits(fc0, fc1)
    same_bits(lw0, lw1)
    np.testing.assert_array_equal(inc0, inc1)


# ------------------------------------------------------------------------------------------------ 5. the loss
@pytest.mark.parametrize("precision", P.PRECISIONS)
def test_get_loss_with_first_history_index_matches_the_reference(precision):
    """The checks of tests/test_gpu_loss.py::test_loss_matches_the_reference_get_loss: e_theta per episode within the mode's tolerance and
    |loss - loss_ref| <= 2 sqrt(loss_ref) rms(d) + rms(d)^2 + 1e-6 loss_ref with d = returned - reference e_theta."""
    z = np.load(os.path.join(GOLDEN, "shorthist_loss_jmid_w32_e2a3t6.npz"))
    eng, w = P.get_engine(int(z["ctx_dim"]), int(z["wseed"]), True)
    assert w.checksum() == str(z["wsum"]) and sorted(set(z["first_hist"].tolist())) == [0, 1, 4]
    E, A, T = z["x0"].shape[:3]
    torch.manual_seed(int(z["dseed"]))
    assert np.array_equal(torch.randn([E * A, T, 2]).numpy().reshape(E, A, T, 2), z["e"])      # the draw get_loss is about to make
    torch.manual_seed(int(z["dseed"]))
    r = offline.get_loss(eng, z["x_st"], z["nbr_sum"], z["edge_mask"], z["x0"].reshape(E * A, T, 2), batch_size=E, t=z["t"],
                         precision=precision, want_rows=True, want_e_theta=True, first_history_index=z["first_hist"])
    for ep in range(E):
        d = P.ade(r.e_theta[ep], z["e_theta"][ep])
        print(f"[{precision}] episode {ep}: e_theta {d:.3e}")
        assert d <= P.E_THETA_TOL[precision], d
    delta = (r.e_theta.astype(np.float64) - z["e_theta"].astype(np.float64)).reshape(-1)
    rms, ref = float(np.sqrt(np.mean(delta ** 2))), float(z["loss"])
    bound = 2.0 * np.sqrt(ref) * rms + rms ** 2 + 1e-6 * ref
    print(f"[{precision}] loss {r.loss:.9f}  reference {ref:.9f}  rms(delta) {rms:.3e}  bound/ref {bound / ref:.3e}")
    assert abs(r.loss - ref) <= bound, (r.loss, ref, bound)
    # validation() passes the keyword through
    torch.manual_seed(int(z["dseed"]))
    v = offline.validation(eng, [dict(x_st=z["x_st"], nbr_sum=z["nbr_sum"], edge_mask=z["edge_mask"], y_t=z["x0"].reshape(E * A, T, 2),
                                      batch_size=E, t=z["t"], first_history_index=z["first_hist"])], precision=precision)
    assert v == float(r.loss)
