"""``forecaster.plan_route`` on its own - no engine, no arrays: the route record of every configuration whose engine trace
tests/test_forecaster_routes.py pins (single calls: A = 3 of N = 6, K = 10, H = 12; batch groups: A = 2, K = 8, H = 6)."""
import pytest

from safe_interactive_crowdnav_amd.forecaster import TOPK_MAX_AGENTS, Route, plan_route, topk_fits_device

SINGLE = [     # (keywords, k, route)
    (dict(check=True), 4, Route("host", "staged", "device")),
    (dict(check=True), 10, Route("host", "staged", "none")),
    (dict(), 4, Route("host", "chain", "device_resident")),
    (dict(), 10, Route("host", "chain", "none")),
    (dict(device_topk=False), 4, Route("host", "staged", "host")),
    (dict(device_topk=False), 10, Route("host", "chain", "none")),
    (dict(device_scene=True, check=True), 4, Route("resident", "staged", "device")),
    (dict(device_scene=True), 10, Route("resident", "chain", "none")),
    (dict(device_frames=True, check=True), 10, Route("stamped", "staged", "none")),
    (dict(device_frames=True), 10, Route("stamped", "chain", "none")),
    (dict(device_frames=True, device_topk=False), 4, Route("stamped", "staged", "host")),
    (dict(device_frames=True, frames=False), 10, Route("host", "chain", "none")),          # hand-edited histories: the host frame table
    (dict(device_frames=True, device_scene=True, frames=False), 4, Route("resident", "chain", "device_resident")),
    (dict(short=True), 4, Route("host", "staged", "device_resident")),                      # jmid_predict has no first_index
    (dict(short=True), 10, Route("host", "staged", "none")),
    (dict(short=True, device_scene=True), 10, Route("resident", "chain", "none")),
    (dict(short=True, device_frames=True), 10, Route("resident", "chain", "none")),
]
BATCH = [
    (dict(), 3, Route("host", "staged", "device_resident")),
    (dict(), 8, Route("host", "staged", "none")),
    (dict(device_scene=True), 3, Route("resident", "staged", "device_resident")),
    (dict(device_frames=True), 3, Route("resident", "chain", "device_resident")),
    (dict(device_frames=True), 8, Route("resident", "chain", "none")),
    (dict(padded=True), 3, Route("host", "chain", "device_resident")),
    (dict(padded=True), 8, Route("host", "chain", "none")),
    (dict(device_topk=False), 3, Route("host", "staged", "host")),
    (dict(device_topk=False, device_frames=True), 3, Route("resident", "staged", "host")),
    (dict(device_topk=False, padded=True), 3, Route("host", "staged", "host")),               # -> the grouped path
    (dict(short=True), 3, Route("host", "staged", "device_resident")),
    (dict(short=True, device_frames=True), 3, Route("resident", "chain", "device_resident")),
]


@pytest.mark.parametrize("kw,k,route", SINGLE)
def test_single_call_route(kw, k, route):
    assert plan_route(k=k, K=10, A=3, H=12, **kw) == route


@pytest.mark.parametrize("kw,k,route", BATCH)
def test_batch_group_route(kw, k, route):
    assert plan_route(k=k, K=8, A=2, H=6, batch=True, **kw) == route


def test_beyond_the_device_top_k_limits_the_host_ranks():
    """A ranking the device kernel does not take (jmid_topk: A <= 32, K <= 1024, H <= 24) is staged and ranked by the host twin, in
    every form; k == K needs no ranking and stays chained."""
    A = TOPK_MAX_AGENTS + 1
    assert topk_fits_device(A - 1, 1024, 24) and not topk_fits_device(A, 1024, 24)
    assert not topk_fits_device(1, 1025, 24) and not topk_fits_device(1, 1024, 25)
    for kw in (dict(), dict(device_scene=True), dict(device_frames=True), dict(batch=True, device_frames=True), dict(batch=True, padded=True)):
        assert plan_route(k=4, K=10, A=A, H=12, **kw)[1:] == ("staged", "host"), kw
        assert plan_route(k=10, K=10, A=A, H=12, **kw).rank == "none"
    assert plan_route(k=10, K=10, A=A, H=12, device_frames=True) == Route("stamped", "chain", "none")
