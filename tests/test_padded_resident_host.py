"""Padded resident scenes, the host side: the noise decision (``noise.fill_padded``: an episode of a padded batch draws exactly what it
draws alone, at its own count), the route of ``predict_batch(padded="resident")`` and the refusals ``padded=True`` keeps."""
import numpy as np
import pytest

from safe_interactive_crowdnav_amd import forecaster as FC, noise as NZ
from safe_interactive_crowdnav_amd.forecaster import Route, plan_route
from tests.test_forecaster_routes import WEIGHTS, FakeEngine, batch_inputs


def test_fill_padded_is_every_episodes_own_draw_scattered():
    seed, ids, n, A, K, T = 0x1234_5678_9ABC, np.array([7, 0, 41], np.uint32), [1, 3, 2], 3, 5, 3
    # n_e = 1: 30 elements - the last Philox block is half used, and a block of four compact elements lies in two padded rows
    assert (K * 1 * T * 2) % 4 == 2 and (T * 2) % 4 != 0
    for draw in (0, 2):
        got = NZ.fill_padded(seed, ids, n, A, K, T, draw)
        assert got.shape == (3, K * A, T, 2) and got.dtype == np.float32
        g = got.reshape(3, K, A, T, 2)
        for e, ne in enumerate(n):
            alone = NZ.normal(seed, ids[e:e + 1], K * ne, T, draw)[0].reshape(K, ne, T, 2)
            assert g[e, :, :ne].tobytes() == alone.tobytes()
            assert np.isnan(g[e, :, ne:]).all() and g[e, :, ne:].size == K * (A - ne) * T * 2
    # an episode that fills the stride is the plain draw at rows = K * A
    assert NZ.fill_padded(seed, ids[1:2], [3], A, K, T).tobytes() == NZ.normal(seed, ids[1:2], K * A, T).tobytes()
    for bad in ([0, 3, 2], [1, 4, 2], [1, 3]):
        with pytest.raises(ValueError):
            NZ.fill_padded(seed, ids, bad, A, K, T)


RESIDENT = [     # (keywords, k, route); the groups' A = 2, K = 8, H = 6 of tests/test_forecaster_route_table.py
    (dict(resident=True), 3, Route("resident", "chain", "device_resident")),
    (dict(resident=True), 8, Route("resident", "chain", "none")),
    (dict(resident=True, short=True), 3, Route("resident", "chain", "device_resident")),
    (dict(resident=True, device_topk=False), 3, Route("resident", "staged", "host")),           # -> the grouped device path
    (dict(resident=True, device_topk=False), 8, Route("resident", "chain", "none")),
]


@pytest.mark.parametrize("kw,k,route", RESIDENT)
def test_resident_padded_route(kw, k, route):
    assert plan_route(k=k, K=8, A=2, H=6, batch=True, **kw) == route
    assert FC.scene_source(False, False, batch=True, resident=True) == "resident"
    assert FC.scene_source(False, False, batch=True) == "host"


class PaddedSceneEngine(FakeEngine):
    """the recording stand-in of tests/test_forecaster_routes.py plus the entry this path calls"""

    def forecast_scene_padded(self, x_T, k, dt=0.25, precision="f32", seed=None, episode_ids=None, K=None, T=None):
        self._log("forecast_scene_padded" + ("(seeded)" if seed is not None else ""), precision)
        inc = self.batch["in_cluster"]
        E, N = inc.shape
        A = int(inc.sum(axis=1).max())
        if x_T is None:
            assert len(episode_ids) == E
        else:
            assert x_T.shape[0] == E and x_T.shape[1] == K_FAKE * A
            T = x_T.shape[2]
        return np.zeros((E, N, k, T + 1, 2)), np.zeros((E, N, k))


K_FAKE = 8
TRACES = [     # (keywords, k, trace)
    (dict(), 3, "build_scene forecast_scene_padded[f16mx]"),
    (dict(), 8, "build_scene forecast_scene_padded[f16mx]"),
    (dict(noise="device", seed=5), 3, "build_scene forecast_scene_padded(seeded)[f16mx]"),
    (dict(last=3, short_history=True), 3, "build_scene(ff) forecast_scene_padded[f16mx]"),
    (dict(erange=("forecast_scene_padded",)), 3, "build_scene forecast_scene_padded[f16mx] forecast_scene_padded[f32]"),
    # a ranking the device top-k does not take: the grouped device path, staged
    (dict(device_topk=False), 3, "build_scene build_scene scene_arrays encode denoise[f16mx] encode denoise[f16mx]"),
]


@pytest.mark.parametrize("kw,k,trace", TRACES)
def test_predict_batch_resident_padded_is_one_build_and_one_call(kw, k, trace):
    kw = dict(kw)
    erange, last = set(kw.pop("erange", ())), kw.pop("last", 6)
    hum, rob = batch_inputs()
    E, N, H = 6, 6, 6
    eng = PaddedSceneEngine(WEIGHTS)
    eng.erange = erange
    fc, lw, inc = FC.predict_batch(eng, hum[:, -last:], rob[:, -last:], range(E), num_samples=K_FAKE, num_ret_samples=k, horizon=H,
                                   time_step=0.25, precision="f16mx", padded="resident", **kw)
    assert sorted(set(inc.sum(axis=1).tolist())) == [1, 2]          # mixed counts
    assert fc.shape == (E, N, k, H + 1, 2) and lw.shape == (E, N, k) and fc.dtype == lw.dtype == np.float64
    assert " ".join(eng.trace) == trace


def test_padded_true_keeps_its_refusals():
    hum, rob = batch_inputs()
    eng = PaddedSceneEngine(WEIGHTS)
    kw = dict(num_samples=8, num_ret_samples=8, horizon=6, time_step=0.25, padded=True)
    for bad in (dict(device_scene=True), dict(device_frames=True), dict(noise="device")):
        with pytest.raises(ValueError, match="padded"):
            FC.predict_batch(eng, hum, rob, list(range(6)), **kw, **bad)
    with pytest.raises(ValueError, match="first_index"):
        FC.predict_batch(eng, hum[:, -3:], rob[:, -3:], list(range(6)), short_history=True, **kw)
    with pytest.raises(ValueError, match="padded"):
        FC.predict_batch(eng, hum, rob, list(range(6)), **dict(kw, padded="device"))
    assert eng.trace == []
