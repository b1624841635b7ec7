"""Guided sampling in the denoise loop (jmid_denoise_guided, jmid_denoise_guided_seeded; include/jmid_hip.h states the rule): what the
guided call must equal bit for bit - the unguided call where nothing iterates, the chain of one-entry calls with jmid_guide_step between
them (where in the loop the kernel sits, and that the next step embeds the guided state), the explicit call on the seeded noise, itself
under every split of the batch - and what the entries refuse."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from safe_interactive_crowdnav_amd import _lib
from safe_interactive_crowdnav_amd.engine import Guidance, JmidError
from safe_interactive_crowdnav_amd.schedule import ddim_steps
from tests.guide_cases import integrate64
from tests.test_gpu_noise import engine_for, install_ddpm, same_bits

DT = 0.25
MODES = ["f32", "f16mx"]
E, A, K, T = 2, 2, 3, 4
THRESHOLD = 2.0      # metres: the seeded random-init net gives velocities of ~10 m/s, so sampled paths lie 0.3-3 m apart; the tests assert that the guidance fires
WEIGHTS = np.array([0.01, 0.02])      # one per entry of engine_for()'s two-entry DDIM table


def inputs(E, A, seed=3, spread=0.05):
    """ctx [E, A, 32], p0 [E, A, 2] (the agents of an episode start ``spread`` apart: their sampled paths cross), x_T [E, K*A, T, 2]."""
    g = torch.Generator().manual_seed(seed)
    ctx = torch.randn([E, A, 32], generator=g).numpy()
    p0 = (spread * torch.randn([E, A, 2], generator=g)).numpy()
    return ctx, p0, torch.randn([E, K * A, T, 2], generator=g).numpy()


def guidance(weights=WEIGHTS, **kw):
    return Guidance(THRESHOLD, weights=weights, **kw)


class one_entry:
    """The engine under a one-entry DDIM table that holds entry ``i`` of its two-entry one; the two-entry table comes back on exit."""

    def __init__(self, eng, i):
        self.eng, self.i = eng, i

    def __enter__(self):
        s = ddim_steps(self.eng.schedule, 2)[self.i]
        cols = [np.array([getattr(s, k)], dtype=np.float32) for k in ("beta", "c_e", "c_x", "n_x", "n_e")]
        self.eng._check(self.eng._lib.jmid_set_ddim_table(self.eng._h, 1, *[C.c_void_p(c.ctypes.data) for c in cols]))
        self.eng.n_steps = 1
        return self.eng

    def __exit__(self, *exc):
        self.eng.set_step(2)


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("joint", [True, False], ids=["jmid", "imid"])
def test_all_zero_table_is_the_unguided_call(joint, precision):
    eng = engine_for(joint)
    ctx, p0, x_T = inputs(E, A)
    want = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision)
    vel, pos, guide = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision, guidance=guidance(np.zeros(2)), want_guide=True)
    assert same_bits(vel, want[0]) and same_bits(pos, want[1]) and not guide.any()


@pytest.mark.parametrize("precision", MODES)
def test_far_apart_scene_is_the_unguided_call(precision):
    eng = engine_for()
    ctx, p0, x_T = inputs(E, A)
    p0 = p0 + 1000.0 * np.arange(A, dtype=np.float32)[None, :, None]
    want = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision)
    vel, pos, guide = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision, guidance=guidance(), want_guide=True)
    assert same_bits(vel, want[0]) and same_bits(pos, want[1]) and not guide.any()


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_guided_call_equals_the_chain_of_one_entry_calls(device, precision):
    eng = engine_for()
    ctx, p0, x_T = inputs(E, A)
    if device:
        ctx, p0, x_T = (torch.from_numpy(a).cuda() for a in (ctx, p0, x_T))
    g = guidance()
    vel, pos, guide = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision, guidance=g, want_guide=True)
    unguided = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision)
    step = dict(dt=DT, threshold=THRESHOLD, n_inner=g.n_inner)
    flat = lambda v: v.reshape(E, K * A, T, 2)
    with one_entry(eng, 0):
        v0, _ = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision)
    g0, r0 = eng.guide_step(flat(v0), p0, weight=WEIGHTS[0], **step)
    with one_entry(eng, 1):
        v1, _ = eng.denoise(g0, ctx, p0, dt=DT, precision=precision)
        last = eng.denoise(g0, ctx, p0, dt=DT, precision=precision, guidance=guidance(WEIGHTS[1:]), want_guide=True)
    g1, r1 = eng.guide_step(flat(v1), p0, weight=WEIGHTS[1], **step)
    to_np = lambda a: a.cpu().numpy() if torch.is_tensor(a) else a
    guide, r0, r1 = to_np(guide), to_np(r0), to_np(r1)
    print(f"[{precision}] samples that iterate behind entry 0 / 1: {int(r0[..., 0].sum())} / {int(r1[..., 0].sum())} of {E * K}")
    assert r0[..., 0].sum() >= 1 and r1[..., 0].sum() >= 1      # the guidance fires behind both entries, or the test shows nothing
    assert not same_bits(vel, unguided[0])
    assert same_bits(flat(vel), g1) and np.array_equal(guide, r0 + r1)
    # the one-entry guided call is the one-entry call + guide_step, and its integrator is the call's
    assert same_bits(last[0], vel) and same_bits(last[1], pos) and np.array_equal(to_np(last[2]), r1)
    want = integrate64(to_np(flat(vel)), to_np(p0), DT)
    assert np.abs(to_np(pos) - want).max() <= T * 2.0 ** -23 * max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("precision", MODES)
def test_seeded_equals_explicit(precision):
    eng = engine_for()
    ctx, p0, _ = inputs(3, A)
    seed, ids = (1 << 33) + 5, [7, 2, 4000000000]
    x_T = eng.noise(seed, ids, K * A, T, draw=0)
    want = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision, guidance=guidance(), want_guide=True)
    got = eng.denoise(None, ctx, p0, dt=DT, precision=precision, seed=seed, episode_ids=ids, K=K, T=T, guidance=guidance(), want_guide=True)
    assert want[2].any()
    assert all(same_bits(a, b) for a, b in zip(got, want))
    # the guided positions are what stays resident
    sel, lw = eng.topk(None, 2, dims=(3, A, K, T))
    sel_w, lw_w = eng.topk(got[1], 2)
    assert same_bits(sel, sel_w) and same_bits(lw, lw_w)


@pytest.mark.parametrize("precision", MODES)
def test_padded_call(precision):
    """Episodes without padding keep the bits of the call without counts (what the padded denoise tests claim of a padded call); the
    padded rows are NaN in both outputs; an episode with one real agent never iterates; seeded equals explicit on the padded draw."""
    eng = engine_for()
    ctx, p0, x_T = inputs(3, A)
    n = np.array([2, 1, 2], dtype=np.int32)
    plain = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision, guidance=guidance(), want_guide=True)
    vel, pos, guide = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision, guidance=guidance(), want_guide=True, n_agents=n)
    assert guide[[0, 2]].any() and not guide[1].any()
    for e in (0, 2):
        assert same_bits(vel[e], plain[0][e]) and same_bits(pos[e], plain[1][e]) and np.array_equal(guide[e], plain[2][e])
    assert np.isnan(vel[1, :, 1:]).all() and np.isnan(pos[1, :, 1:]).all() and np.isfinite(vel[1, :, :1]).all() and np.isfinite(pos[[0, 2]]).all()
    seed, ids = 11, [3, 4, 5]
    x_pad = eng.noise(seed, ids, K * A, T, n_agents=n)
    want = eng.denoise(x_pad, ctx, p0, dt=DT, precision=precision, guidance=guidance(), want_guide=True, n_agents=n)
    got = eng.denoise(None, ctx, p0, dt=DT, precision=precision, seed=seed, episode_ids=ids, K=K, T=T, guidance=guidance(), want_guide=True,
                      n_agents=n)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want))
    # walls in a padded call: the single agent of episode 1 can iterate now
    walls = np.array([[-2.0, 0.1, 2.0, 0.1], [-2.0, -0.1, 2.0, -0.1]])
    gw = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision, guidance=guidance(walls=walls, wall_radius=0.3), want_guide=True, n_agents=n)[2]
    assert gw[1].any()


@pytest.mark.parametrize("precision", MODES)
def test_batch_split_and_chunk_plan_do_not_change_a_bit(precision):
    eng = engine_for()
    ctx, p0, x_T = inputs(4, A)
    whole = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision, guidance=guidance(), want_guide=True)
    assert whole[2].any()
    for lo, hi in ((0, 2), (2, 4)):
        part = eng.denoise(x_T[lo:hi], ctx[lo:hi], p0[lo:hi], dt=DT, precision=precision, guidance=guidance(), want_guide=True)
        assert all(same_bits(a, b[lo:hi]) for a, b in zip(part, whole))
    try:
        for chunk in (1, 2, 3):      # four, two, and a ragged pair of chunks, two at a time on their own streams
            eng.set_chunk_episodes(chunk)
            got = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision, guidance=guidance(), want_guide=True)
            assert all(same_bits(a, b) for a, b in zip(got, whole)), chunk
    finally:
        eng.set_chunk_episodes(0)


def test_profile_class_counts_one_launch_per_guided_entry_and_chunk():
    eng = engine_for()
    ctx, p0, x_T = inputs(E, A)
    eng.profile_reset()
    eng.profile_enable(["guide"])
    try:
        eng.set_chunk_episodes(1)
        eng.denoise(x_T, ctx, p0, dt=DT, guidance=guidance())                           # 2 entries x 2 chunks
        eng.denoise(x_T, ctx, p0, dt=DT, guidance=guidance(np.array([0.0, 0.02])))      # 1 entry x 2 chunks
        n, _ = eng.profile_get()["guide"]
    finally:
        eng.profile_disable()
        eng.set_chunk_episodes(0)
    assert n == 6


def test_refusals():
    eng = engine_for()
    ctx, p0, x_T = inputs(E, A)
    vel = np.empty((E, K, A, T, 2), dtype=np.float32)
    w = np.ascontiguousarray(WEIGHTS)
    walls = np.array([[0.0, 0.0, 1.0, 0.0]])
    ok = dict(n_agents=None, x_T=x_T, ctx=ctx, p0=p0, dt=DT, threshold=0.2, margin=0.02, tau=0.005, weights=w, n_inner=4, L=0, walls=None,
              wall_radius=0.0)
    ptr = lambda v: None if v is None else C.c_void_p(v.ctypes.data)

    def call(**kw):
        a = {**ok, **kw}
        na = None if a["n_agents"] is None else np.asarray(a["n_agents"], dtype=np.int32)
        return eng._lib.jmid_denoise_guided(eng._h, E, A, K, T, ptr(na), ptr(a["x_T"]), ptr(a["ctx"]), ptr(a["p0"]), a["dt"], _lib.PRECISIONS["f32"],
                                            a["threshold"], a["margin"], a["tau"], ptr(a["weights"]), a["n_inner"], a["L"], ptr(a["walls"]),
                                            a["wall_radius"], ptr(vel), None, None, _lib.MEM_HOST)

    assert call() == 0
    bad = [dict(threshold=-0.1), dict(threshold=np.inf), dict(margin=-1.0), dict(margin=np.nan), dict(tau=0.0), dict(tau=np.inf), dict(L=65),
           dict(L=1), dict(L=1, walls=np.full((1, 4), np.nan), wall_radius=0.3), dict(L=1, walls=walls, wall_radius=-1.0), dict(p0=None),
           dict(dt=0.0), dict(dt=-0.25), dict(dt=np.nan), dict(weights=None), dict(weights=np.array([0.01, -0.01])),
           dict(weights=np.array([np.nan, 0.01])), dict(weights=np.array([0.01, np.inf])), dict(n_inner=0), dict(n_inner=65), dict(x_T=None),
           dict(ctx=None), dict(n_agents=[3, 1]), dict(n_agents=[0, 1])]
    for kw in bad:
        assert call(**kw) == _lib.EINVAL, kw
    ids = np.array([0, 1], dtype=np.uint32)
    seeded = lambda ids_ptr: eng._lib.jmid_denoise_guided_seeded(eng._h, E, A, K, T, None, 5, ids_ptr, ptr(ctx), ptr(p0), DT, _lib.PRECISIONS["f32"], 0.2,
                                                                 0.02, 0.005, ptr(w), 4, 0, None, 0.0, ptr(vel), None, None, _lib.MEM_HOST)
    assert seeded(ptr(ids)) == 0 and seeded(None) == _lib.EINVAL
    try:      # a handle with the DDPM table set
        install_ddpm(eng, 2)
        assert call() == _lib.EINVAL and b"DDIM" in eng._lib.jmid_last_error(eng._h)
        assert seeded(ptr(ids)) == _lib.EINVAL
    finally:
        eng.set_step(2)
    assert call() == 0      # the handle stays usable, and the unguided entries are what they were
    with pytest.raises(ValueError):
        eng.denoise(x_T, ctx, p0, dt=DT, guidance=Guidance(0.2, weights=[0.01]))                 # not one per entry
    with pytest.raises(ValueError):
        eng.denoise(x_T, ctx, p0, dt=DT, guidance=Guidance(0.2))                                  # no table
    with pytest.raises(ValueError):
        eng.denoise(x_T, ctx, None, dt=DT, guidance=guidance())
    with pytest.raises(ValueError):
        eng.denoise(x_T, ctx, p0, dt=DT, guidance=guidance(walls=walls))
    with pytest.raises(JmidError):
        eng.denoise(x_T, ctx, p0, dt=DT, guidance=guidance(n_inner=0))
