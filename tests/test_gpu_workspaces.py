"""The handle's grow-on-demand buffers (csrc/host_mem.hpp): every entry point shares the code that grows a workspace, so each case here
grows one on purpose - small shape, large shape, the small one again - and looks at what was resident before, or at the small call's
bits.  Nothing here is a tolerance: a call that reads a stale address, a slot of the wrong size or a buffer freed under it gives other
bits (or faults).  The smallest engine of the suite, f32 and one split mode; a fresh engine for every case and memory mode, so that
each of them starts from empty workspaces and grows them itself."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from safe_interactive_crowdnav_amd import noise as NZ
from safe_interactive_crowdnav_amd import scene as SC
from safe_interactive_crowdnav_amd.engine import JmidEngine
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims
from tests.test_frames_host import bits_equal, raw_batch
from tests.test_scene_device_inputs import DT, F, random_positions

PRECISIONS = ["f32", "f16mx"]
MODES = [False, True]       # device-mode call (CUDA tensors in and out)?
SMALL, LARGE = (1, 2, 4, 4), (4, 5, 20, 12)       # E, A, K, T


_WEIGHTS = JMIDWeights.from_seed(NetDims(ctx_dim=32), 5)


@pytest.fixture
def fresh():
    """-> a function that makes a new engine (nothing allocated yet); all of them are checked and closed after the test"""
    made = []

    def make():
        made.append(JmidEngine(_WEIGHTS, joint=True, hist_len=6, step=2))
        return made[-1]
    yield make
    for e in made:
        assert e.erange_count() == 0 and e.timeout_count() == 0
        e.close()


def host(a):
    return None if a is None else a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def same(a, b):
    """array_equal, NaN rows (padded agents) included"""
    a, b = host(a), host(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def put(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if device else a


def denoise_inputs(E, A, K, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn([E, K * A, T, 2], generator=g).numpy(), torch.randn([E, A, 32], generator=g).numpy(),
            torch.randn([E, A, 2], generator=g).numpy(), torch.randn([E, A, T, 2], generator=g).numpy())


def encoder_inputs(E, A, K, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn([E * A, F, 6], generator=g).numpy(), torch.randn([E * A, 2, F, 6], generator=g).numpy(),
            torch.rand([E * A, 2], generator=g).numpy(), torch.randn([E, K * A, T, 2], generator=g).numpy(),
            torch.randn([E, A, 2], generator=g).numpy())


# ------------------------------------------------------------------------------------------------ 1. the second workspace
@pytest.mark.parametrize("precision", PRECISIONS)
def test_second_workspace_grows_and_the_resident_positions_survive(fresh, precision):
    E, A, K, T = SMALL
    x_T, ctx, p0, gt = denoise_inputs(E, A, K, T, 11)
    E2, A2, K2, T2 = 8, 5, 64, 12
    g = torch.Generator().manual_seed(12)
    pos2, gt2 = torch.randn([E2, K2, A2, T2, 2], generator=g).numpy(), torch.randn([E2, A2, T2, 2], generator=g).numpy()
    per_mode = []
    for device in MODES:
        eng = fresh()
        _, pos = eng.denoise(put(x_T, device), put(ctx, device), put(p0, device), dt=DT, precision=precision, want_vel=False)

        def resident():
            return [host(a) for a in (*eng.eval_statistics(None, put(gt, device), dims=SMALL),
                                      *eng.collision_statistics(None, dims=SMALL, pairs=True), *eng.topk(None, 2, dims=SMALL))]
        before = resident()
        # the same statistics of the positions the call copied out: pos = NULL read those, not something else
        for got, want in zip(before, [*eng.eval_statistics(pos, put(gt, device)), *eng.collision_statistics(pos, pairs=True), *eng.topk(pos, 2)]):
            assert same(got, want)
        big = eng.eval_statistics(pos2, gt2)        # host mode, explicit arrays: the second workspace is reallocated
        after = resident()
        assert all(same(a, b) for a, b in zip(before, after)), "the resident positions did not survive the second workspace's growth"
        # ... and the large call itself, in the other memory mode (its slots are then the caller's arrays)
        assert all(same(a, b) for a, b in zip(big, eng.eval_statistics(put(pos2, True), put(gt2, True))))
        per_mode.append([host(pos)] + before)
    assert all(same(a, b) for a, b in zip(*per_mode)), "host- and device-mode results differ"


# ------------------------------------------------------------------------------------------------ 2. the chained entries
def staged(eng, x_st, nbr, em, x_T, p0, k, precision):
    """jmid_predict's stages as three calls (tests/test_gpu_api.py::test_predict_entry_equals_the_staged_calls)"""
    E, A = p0.shape[:2]
    _, pos = eng.denoise(x_T, eng.encode(x_st, nbr, em).reshape(E, A, -1), p0, dt=DT, precision=precision, want_vel=False)
    return eng.topk(pos, k)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_predict_small_large_small(fresh, precision):
    """(1, 2, 4, 4) -> (4, 5, 20, 12) -> the first again: the pinned and the device staging block of the chain move in between"""
    small, large = encoder_inputs(*SMALL, 21), encoder_inputs(*LARGE, 22)
    eng = fresh()
    first = eng.predict(*small, 2, dt=DT, precision=precision)
    big = eng.predict(*large, 5, dt=DT, precision=precision)
    third = eng.predict(*small, 2, dt=DT, precision=precision)
    assert same(first[0], third[0]) and same(first[1], third[1])
    for got, want in ((big, staged(eng, *large, 5, precision)), (first, staged(eng, *small, 2, precision))):
        assert same(got[0], want[0]) and same(got[1], want[1])


def build_scene_in(eng, device, hum, rob, horizon, stamps=None, n_frames=None):
    """eng.build_scene / eng.build_scene_stamped (host mode), or the same entries in JMID_MEM_DEVICE: every array a device buffer, as
    tests/test_gpu_scene_device.py::test_device_memory_mode_equals_host_memory_mode calls them -> the engine's dict, as host arrays"""
    if not device:
        if stamps is None:
            return eng.build_scene(hum, rob, DT, horizon=horizon, force_all_in_cluster=True)
        return eng.build_scene_stamped(stamps, hum, rob, DT, horizon=horizon, force_all_in_cluster=True, n_frames=n_frames)
    E, N = hum.shape[0], hum.shape[2]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    dh, dr = torch.from_numpy(hum).cuda(), torch.from_numpy(rob).cuda()
    inc, rin = torch.zeros((E, N), dtype=torch.uint8, device="cuda"), torch.zeros(E, dtype=torch.uint8, device="cuda")
    n_in, n_grid = torch.zeros(E, dtype=torch.int32, device="cuda"), torch.zeros(E, dtype=torch.int32, device="cuda")
    cv = torch.zeros((E, N, horizon, 2), dtype=torch.float64, device="cuda")
    if stamps is None:
        eng._check(eng._lib.jmid_build_scene(eng._h, E, N, hum.shape[1], ptr(dh), ptr(dr), DT, horizon, 1, ptr(inc), ptr(rin), ptr(n_in), ptr(cv),
                                             eng._mem(True)))
    else:
        ds, dn = torch.from_numpy(stamps).cuda(), torch.from_numpy(np.ascontiguousarray(n_frames, dtype=np.int32)).cuda()
        eng._check(eng._lib.jmid_build_scene_stamped(eng._h, E, N, hum.shape[1], ptr(ds), ptr(dh), ptr(dr), ptr(dn), DT, horizon, 1, ptr(inc),
                                                     ptr(rin), ptr(n_in), ptr(n_grid), ptr(cv), eng._mem(True)))
    torch.cuda.synchronize()
    eng._scene_shape, eng._scene_n_in = (E, N, F, False), host(n_in)      # what the engine's own build_scene notes for predict_scene
    return {"in_cluster": host(inc).astype(bool), "robot_in_cluster": host(rin).astype(bool), "n_in": host(n_in), "n_grid": host(n_grid),
            "cv": host(cv)}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_scene_chain_small_large_small(fresh, precision):
    """build_scene E = 1, N = 2 -> build_scene_stamped E = 4, N = 8, R = 16 (the scene and the frames workspace move, and the pinned
    staging) -> the first again, with host arrays and with device buffers (no raw-frame slots then, and other sources of the grid)"""
    K, k, T = 4, 2, 4
    hum, rob = random_positions(1, 2, 7, half_width=2.0)
    x1 = torch.randn([1, K * 2, T, 2], generator=torch.Generator().manual_seed(31)).numpy()
    E, N, R, K2, k2, T2 = 4, 8, 16, 6, 3, 12
    stamps, hum2, rob2, n_frames = raw_batch(E, R, N, 17)
    x2 = torch.randn([E, K2 * N, T2, 2], generator=torch.Generator().manual_seed(32)).numpy()
    # the large one against the host twins, as tests/test_gpu_frames_device.py and tests/test_gpu_scene_device.py compare them
    ref = SC.frame_table_frames_batched(stamps, hum2, rob2, n_frames, DT, F)
    sc = SC.build_scenes_batched(ref["human_xy"], ref["robot_xy"], DT, force_all_in_cluster=True, horizon=T2)
    per_mode = []
    for device in MODES:
        eng = fresh()

        def small():
            out = build_scene_in(eng, device, hum, rob, T)
            return [out["in_cluster"], out["cv"], *eng.predict_scene(x1, k, dt=DT, precision=precision),
                    *eng.forecast_scene(x1, k, dt=DT, precision=precision)]
        first = small()
        out = build_scene_in(eng, device, hum2, rob2, T2, stamps, n_frames)
        np.testing.assert_array_equal(out["n_grid"], ref["n_grid"])
        assert out["n_in"].tolist() == [N] * E
        fr = eng.scene_frames()
        for key in ("human_xy", "robot_xy", "pose_now"):
            assert bits_equal(fr[key], ref[key]), f"{key} differs from the host twin"
        assert bits_equal(out["cv"], sc["cv"])
        arr = eng.scene_arrays()
        for key in ("x", "x_st", "nbr_sum", "edge_mask", "p0"):
            assert np.array_equal(arr[key].view(np.uint32), sc[key].view(np.uint32)), key
        got = eng.predict_scene(x2, k2, dt=DT, precision=precision)
        fc, lw = eng.forecast_scene(x2, k2, dt=DT, precision=precision)
        want = staged(eng, arr["x_st"].reshape(E * N, F, 6), arr["nbr_sum"].reshape(E * N, 2, F, 6), arr["edge_mask"].reshape(E * N, 2), x2,
                      arr["p0"], k2, precision)
        assert same(got[0], want[0]) and same(got[1], want[1])
        for e in range(E):
            w = SC.assemble_forecasts(out["in_cluster"][e], got[0][e], got[1][e], out["cv"][e], fr["pose_now"][e], k2, K2)
            assert bits_equal(fc[e], w[0]) and bits_equal(lw[e], w[1])
        third = small()
        assert all(same(a, b) for a, b in zip(first, third))
        per_mode.append(first + [out["in_cluster"], out["n_in"], out["n_grid"], out["cv"], *fr.values(), *arr.values(), *got, fc, lw])
    assert all(same(a, b) for a, b in zip(*per_mode)), "host- and device-mode results differ"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_chain_kinds_in_sequence_equal_fresh_handles(fresh, precision):
    """predict on host arrays -> build_scene(first_frame=) + forecast_scene_padded(seed=) -> build_scene + predict_scene on the episodes
    of equal count -> predict on host arrays again, on ONE handle: every kind of chain lays the same pinned and device block out its own
    way (with and without the host inputs, the assembled arrays, sel / logw, first_index), and each result must be what the same call
    gives on a handle that has run nothing else."""
    E, N, K, T, k = 3, 4, 6, 3, 2
    host_in = encoder_inputs(E, N, K, T, 61)
    hum, rob = random_positions(E, N, 7, half_width=2.0)
    # every pedestrian in the cluster but those seen on the last frame alone: counts 3, 2, 3
    first = np.array([[0, 0, 2, 1, F - 1], [1, F - 1, 0, F - 1, 3], [0, 1, 0, F - 1, 0]], np.int32)
    ids, pick = [9, 4, 70], [0, 2]
    x_s = torch.randn([len(pick), K * N, T, 2], generator=torch.Generator().manual_seed(62)).numpy()

    def host_chain(eng):
        return eng.predict(*host_in, k, dt=DT, precision=precision)

    def padded_forecast(eng):
        out = eng.build_scene(hum, rob, DT, horizon=T, force_all_in_cluster=True, first_frame=first)
        assert out["n_in"].tolist() == [3, 2, 3]
        return eng.forecast_scene_padded(None, k, dt=DT, precision=precision, seed=5, episode_ids=ids, K=K, T=T)

    def scene_chain(eng):
        out = eng.build_scene(hum[pick], rob[pick], DT, force_all_in_cluster=True)
        assert out["n_in"].tolist() == [N] * len(pick)
        return eng.predict_scene(x_s, k, dt=DT, precision=precision)

    steps = (host_chain, padded_forecast, scene_chain, host_chain)
    one = fresh()
    for i, step in enumerate(steps):
        got, want = step(one), step(fresh())
        assert all(same(a, b) for a, b in zip(got, want)), f"call {i + 1} ({step.__name__}) depends on what ran before it on the handle"


# ------------------------------------------------------------------------------------------------ 3. the id and count buffers
@pytest.mark.parametrize("precision", PRECISIONS)
def test_episode_ids_pass_their_capacity(fresh, precision):
    """E = 2 -> 70 -> 2 seeded: the id buffer (64 at first) is reallocated in between; an episode's samples do not depend on the batch"""
    _, A, K, T = SMALL
    _, ctx, p0, _ = denoise_inputs(70, A, K, T, 41)
    ids = np.arange(100, 170)
    pick = [7, 3]
    per_mode = []
    for device in MODES:
        eng = fresh()

        def run(sel):
            return eng.denoise(None, put(ctx[sel], device), put(p0[sel], device), dt=DT, precision=precision, seed=5, episode_ids=ids[sel], K=K, T=T)
        first, whole, third = run(pick), run(np.arange(70)), run(pick)
        for j in (0, 1):
            assert same(first[j], third[j]) and same(host(whole[j])[pick], first[j])
        per_mode.append([host(a) for a in whole])
    assert all(same(a, b) for a, b in zip(*per_mode)), "host- and device-mode results differ"


def test_noise_of_seventy_episodes_equals_the_host_twin(fresh):
    """as tests/test_gpu_noise.py::test_normals_equal_the_host_twin holds it: one fp32 ulp where the fp64 value lies on a rounding
    boundary, at most one value in 2^16 (none at all of these 2 240)"""
    ids, rows, T = np.arange(70)[::-1].copy(), 4, 4
    got = []
    for device in MODES:
        eng = fresh()
        first, whole, third = (host(eng.noise(9, i, rows, T, draw=1, device=device)) for i in (ids[:2], ids, ids[:2]))      # 2 -> 70 -> 2
        assert same(first, third) and same(first, whole[:2])
        got.append(whole)
    assert same(got[0], got[1])
    want = NZ.normal(9, ids, rows, T, 1)
    assert got[0].shape == want.shape and got[0].dtype == np.float32
    assert int((got[0].view(np.uint32) != want.view(np.uint32)).sum()) * (1 << 16) <= got[0].size
    np.testing.assert_array_equal(host(eng.noise(9, ids, rows, T, draw=1, words=True)), NZ.words(9, ids, rows, T, 1))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_agent_counts_pass_their_capacity(fresh, precision):
    """E = 2 -> 70 -> 2 padded: the count buffer likewise; every episode of the large call against the same episode run alone (the same
    row stride A and count: the same arithmetic, whatever the batch)"""
    _, A, K, T = 1, 3, 4, 4
    x_T, ctx, p0, _ = denoise_inputs(70, A, K, T, 51)
    n = (np.arange(70) % A + 1).astype(np.int32)
    pick = [7, 3]
    per_mode = []
    for device in MODES:
        eng = fresh()

        def run(sel):
            return eng.denoise(put(x_T[sel], device), put(ctx[sel], device), put(p0[sel], device), dt=DT, precision=precision, n_agents=n[sel])
        first, whole, third = run(pick), run(np.arange(70)), run(pick)
        for j in (0, 1):
            assert same(first[j], third[j]) and same(host(whole[j])[pick], first[j])
        if not device:
            for e in range(70):
                alone = run([e])
                assert same(alone[0], whole[0][e:e + 1]) and same(alone[1], whole[1][e:e + 1]), f"episode {e}"
            assert np.isnan(whole[1][1, :, 2:]).all() and np.isfinite(whole[1][1, :, :2]).all()       # n[1] = 2 of A = 3
        per_mode.append([host(a) for a in whole])
    assert all(same(a, b) for a, b in zip(*per_mode)), "host- and device-mode results differ"
