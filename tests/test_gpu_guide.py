"""One guidance step on the device (csrc/guide.hpp; jmid_guide_step) against its NumPy twin (``metrics.guide_step_host``;
tests/test_guide_host.py pins the twin itself): x_out and guide_out bit for bit, on every shape at which the kernel takes another path -
the strided point ownership, the padded counts, the wall instance, the LDS limit, T = 1, both iteration counts, in place."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from safe_interactive_crowdnav_amd import _lib, metrics
from safe_interactive_crowdnav_amd.engine import JmidError
from tests.guide_cases import DT, THRESHOLD, guide_cases, same_bits
from tests.test_gpu_noise import engine_for

_TWIN = {}
WEIGHT = 0.02


def case(name):
    """(x, p0, keywords, the twin's two outputs), the twin computed once per input."""
    if name not in _TWIN:
        x, p0, kw = guide_cases()[name]
        _TWIN[name] = (x, p0, kw, metrics.guide_step_host(x, p0, DT, THRESHOLD, weight=WEIGHT, **kw))
    return _TWIN[name]


# what has to happen in a case for it to cover what it is there for: (samples that iterate at least, samples that do not at least)
EXPECT = {"e2a3k4t8": (1, 0), "a1k2t4l2": (1, 0), "a12k2t24": (1, 0), "e3a4k3t6": (1, 3), "e3a4k3t6l3": (1, 0), "a64t24l64": (1, 0),
          "t1": (0, 8), "t1l2": (1, 0), "n_inner1": (1, 0), "e2a3k4t8l4": (1, 0)}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(EXPECT))
def test_equals_the_twin(name, device):
    eng = engine_for()
    x, p0, kw, (want, want_rows) = case(name)
    moved = int(want_rows[..., 0].sum())
    assert moved >= EXPECT[name][0] and want_rows[..., 0].size - moved >= EXPECT[name][1]
    args = [torch.from_numpy(a).cuda() for a in (x, p0)] if device else [x, p0]
    out, rows = eng.guide_step(args[0], args[1], DT, THRESHOLD, weight=WEIGHT, **kw)
    out, rows = (a.cpu().numpy() if device else a for a in (out, rows))
    differ = int((out.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{name}: {moved} of {want_rows[..., 0].size} samples iterate, iterations {int(want_rows[..., 1].sum())}, {differ} of {out.size} values "
          f"differ from the twin")
    assert np.array_equal(rows, want_rows.astype(np.float32))
    assert same_bits(out, want)
    if name == "n_inner1":
        assert rows[..., 1].max() == 1 and not np.array_equal(rows, case("e2a3k4t8")[3][1].astype(np.float32))


def test_in_place_and_zero_weight():
    eng = engine_for()
    x, p0, kw, (want, want_rows) = case("e2a3k4t8l4")
    xd, pd = torch.from_numpy(x).cuda(), torch.from_numpy(p0).cuda()
    keep = xd.clone()
    out, rows = eng.guide_step(xd, pd, DT, THRESHOLD, weight=WEIGHT, inplace=True, **kw)
    assert out is xd and same_bits(xd, want) and np.array_equal(rows.cpu().numpy(), want_rows.astype(np.float32))
    # out of place, the input stays; weight 0 copies and reports nothing
    out, rows = eng.guide_step(keep, pd, DT, THRESHOLD, weight=WEIGHT, **kw)
    assert same_bits(out, want) and same_bits(keep, x)
    for arrays in ((keep, pd), (x, p0)):
        out, rows = eng.guide_step(*arrays, DT, THRESHOLD, weight=0.0, **kw)
        assert same_bits(out, x) and not np.asarray(rows.cpu() if torch.is_tensor(rows) else rows).any()


def test_padded_rows_are_neither_read_nor_written():
    eng = engine_for()
    x, p0, kw, (want, want_rows) = case("e3a4k3t6")
    E, A, K, T = 3, 4, 3, 6
    xn, pn = x.copy(), p0.copy()
    for e, n in enumerate(kw["n_agents"]):
        xn.reshape(E, K, A, T, 2)[e, :, n:] = np.nan
        pn[e, n:] = np.nan
    out, rows = eng.guide_step(xn, pn, DT, THRESHOLD, weight=WEIGHT, **kw)
    real = ~np.isnan(xn)
    assert np.array_equal(rows, want_rows.astype(np.float32)) and same_bits(out[real], want[real]) and np.isnan(out[~real]).all()


def test_guide_has_a_profile_class_of_its_own():
    eng = engine_for()
    x, p0, kw, _ = case("e2a3k4t8")
    assert "guide" in eng.kernel_classes()
    eng.profile_reset()
    eng.profile_enable(["guide"])
    try:
        eng.guide_step(x, p0, DT, THRESHOLD, weight=WEIGHT)
        eng.guide_step(x, p0, DT, THRESHOLD, weight=0.0)      # no launch
        n, ms = eng.profile_get()["guide"]
    finally:
        eng.profile_disable()
    assert n == 1 and ms > 0


def test_refusals_of_the_raw_entry():
    eng = engine_for()
    x, p0, _, _ = case("e2a3k4t8")
    E, A, K, T = 2, 3, 4, 8
    out, rows = np.empty_like(x), np.empty((E, K, 2), dtype=np.float32)
    walls = np.array([[0.0, 0.0, 1.0, 0.0]])
    ok = dict(E=E, A=A, K=K, T=T, n_agents=None, x=x, p0=p0, dt=DT, threshold=0.2, margin=0.02, tau=0.005, weight=0.02, n_inner=4, L=0,
              walls=None, wall_radius=0.0)

    def call(**kw):
        a = {**ok, **kw}
        ptr = lambda v: None if v is None else C.c_void_p(v.ctypes.data)
        na = None if a["n_agents"] is None else np.asarray(a["n_agents"], dtype=np.int32)
        return eng._lib.jmid_guide_step(eng._h, a["E"], a["A"], a["K"], a["T"], ptr(na), ptr(a["x"]), ptr(a["p0"]), a["dt"], a["threshold"],
                                        a["margin"], a["tau"], a["weight"], a["n_inner"], a["L"], ptr(a["walls"]), a["wall_radius"], ptr(out),
                                        ptr(rows), _lib.MEM_HOST)

    assert call() == 0
    bad = [dict(threshold=-0.1), dict(threshold=np.nan), dict(margin=-1.0), dict(margin=np.inf), dict(tau=0.0), dict(tau=np.nan),
           dict(L=65, walls=np.zeros((65, 4))), dict(L=-1), dict(L=1), dict(L=1, walls=np.full((1, 4), np.inf), wall_radius=0.3),
           dict(L=1, walls=walls, wall_radius=-0.1), dict(L=1, walls=walls, wall_radius=np.nan), dict(p0=None), dict(dt=0.0), dict(dt=np.inf),
           dict(dt=np.nan), dict(weight=-0.01), dict(weight=np.inf), dict(weight=np.nan), dict(n_inner=0), dict(n_inner=65), dict(x=None),
           dict(T=25), dict(A=65), dict(K=1025), dict(E=0), dict(n_agents=[3, 4]), dict(n_agents=[0, 3])]
    for kw in bad:
        assert call(**kw) == _lib.EINVAL, kw
    assert call() == 0      # the handle stays usable
    with pytest.raises(ValueError):
        eng.guide_step(x, p0, DT, walls=walls)
    with pytest.raises(ValueError):
        eng.guide_step(x, p0[:1], DT)
    with pytest.raises(JmidError):
        eng.guide_step(x, p0, DT, n_inner=0)
