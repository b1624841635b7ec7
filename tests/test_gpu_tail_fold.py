"""The tail of a denoise step (concat3 -> concat4 -> output layer) as one 2 x d_model map per (episode, agent) row and step
(csrc/tail_fold.hpp) against the two GEMMs + output kernel it replaces (jmid_set_tuning "tail_fold" = 1): accuracy against float64,
the whole denoise loop against the reference goldens, bit invariance under chunking / lanes / kernel form / table form /
repetition, and the range report."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tests.width_cases as WC
from oracle import jmid_oracle as O
from safe_interactive_crowdnav_amd.engine import JmidEngine, JmidError
from safe_interactive_crowdnav_amd.schedule import ddim_steps
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ADE_GATE = 1e-4
SPLIT_MODES = ["f16x3", "f16x2", "f16mx"]

_ENGINES = {}


def get_engine(ctx_dim, wseed, joint=True):
    key = (ctx_dim, wseed, joint)
    if key not in _ENGINES:
        w = JMIDWeights.from_seed(NetDims(ctx_dim=ctx_dim, nhead=WC.nhead_of(ctx_dim)), wseed)      # (the tail does not read the head count)
        _ENGINES[key] = (JmidEngine(w, joint=joint), w)
    return _ENGINES[key]


def ade(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64), axis=-1).mean())


def within_the_gemm_paths_error(precision, fold, gemm):
    """(max, mean) of |e - float64| on the folded path against the GEMM path's on the same inputs.  f16x2 / f16mx: both paths share
    the fp16 rounding of X_hi and the GEMM path adds Y3's, so the folded mean may not exceed the GEMM path's, and the maximum - a
    sample maximum of two error sums that share their dominant term - may exceed it by a quarter at most.  f16x3: fp32-class sums of
    the same terms in different orders, a factor two either way."""
    if precision == "f16x3":
        return fold[0] <= 2.0 * gemm[0] and fold[1] <= 2.0 * gemm[1]
    return fold[0] <= 1.25 * gemm[0] and fold[1] <= gemm[1]


# ---- 1. the kernels against float64 ----
_REF = {}
STEP = 3


def sigmoid8(v):
    return 1.0 / (1.0 + np.exp(-v))


def tail_case(ctx_dim, shape):
    """Inputs of one case and the staged tail in float64 from the fp32 weights, the hyper rows and the handle's time row, on the X
    that is passed in; made once per (width, shape) and shared by the modes, knobs and kernel forms."""
    key = (ctx_dim, shape)
    if key not in _REF:
        eng, w = get_engine(ctx_dim, 5)
        eng.set_step(10)
        E, A, K, T = shape
        d, dmid, dlow = 2 * ctx_dim, ctx_dim, ctx_dim // 2
        width = eng.hyper_width()
        M = E * K * A * T
        g = torch.Generator().manual_seed(2000 * ctx_dim + M)
        X = torch.randn([M, d], generator=g)
        X = ((X - X.mean(1, keepdim=True)) / X.std(1, keepdim=True)).numpy()          # LayerNorm-like rows
        hyp = torch.randn([E * A, width], generator=g).numpy()
        _, thyp = eng.dbg_tail(X, hyp, STEP, shape, "f16x3")
        f8 = lambda name: w.tensors[name].numpy().astype(np.float64)
        # the time row is an input of both paths (the handle's fp32 table): the reference takes the row the handle holds, after
        # checking the tail's part of it against its definition, w0 beta + w1 sin(beta) + w2 cos(beta), in float64
        beta = float(ddim_steps(eng.schedule, 10)[STEP].beta)
        tcol = np.array([beta, np.sin(beta), np.cos(beta)])
        tw = [f8(f"{n}._hyper_{k}.weight")[:, :3] for n in ("concat3", "concat4", "linear") for k in ("gate", "bias")]
        t_def = np.concatenate([m @ tcol for m in tw])
        np.testing.assert_allclose(thyp[2 * d:], t_def, rtol=0, atol=4e-7 * max(np.abs(m).sum(1).max() for m in tw) + 1e-7)
        m = np.arange(M)
        r = m // T
        ea = (r // (K * A)) * A + r % A
        h8, t8 = hyp.astype(np.float64), thyp.astype(np.float64)
        y, o = X.astype(np.float64), 2 * d
        for name, n in (("concat3", dmid), ("concat4", dlow), ("linear", 2)):
            gate = sigmoid8(h8[ea, o:o + n] + t8[None, o:o + n])
            bias = h8[ea, o + n:o + 2 * n] + t8[None, o + n:o + 2 * n]
            y = (y @ f8(f"{name}._layer.weight").T + f8(f"{name}._layer.bias")) * gate + bias
            o += 2 * n
        _REF[key] = (X, hyp, y)
    return _REF[key]


@pytest.mark.parametrize("precision", SPLIT_MODES)
@pytest.mark.parametrize("ctx_dim", WC.OLD_CTX_DIMS)
@pytest.mark.parametrize("shape", [(2, 2, 3, 4), (3, 3, 5, 7), (1, 5, 20, 12)])
def test_folded_tail_is_no_further_from_float64_than_the_gemms(shape, ctx_dim, precision):
    """48 tokens (several rows of the table in a wave's neighbourhood), T odd (trajectories straddle the 128-row panel boundaries) and
    one scene, at d_model 64 (eight lanes of a wave hold columns) and 512, per token ("out_traj" = 0 at these sizes) and per trajectory
    (= 1).  The table built per step ("tail_fold" = 2) and the two kernel forms give the bits of the default."""
    folded_against_the_gemms(shape, ctx_dim, precision)


GEMM_TOL = {"f16x3": 4e-5, "f16x2": 2e-3, "f16mx": 2e-3}      # TOL of tests/test_gpu_kernels.py: max |err| relative to max(1, max |ref|)


@pytest.mark.parametrize("precision", SPLIT_MODES)
@pytest.mark.parametrize("ctx_dim", [c for c in WC.CTX_DIMS if c not in WC.OLD_CTX_DIMS])
def test_tail_at_every_other_accepted_width(ctx_dim, precision):
    """d_model 128 (concat3's N = 64 on the GEMM path), 192, 256 - and 1024, beyond tail_fold.hpp's kTailMaxD: nothing is folded there,
    the plan takes the two EPI_CSL GEMMs + the output kernel under every value of the knob, so the three runs must be the same bits (the
    seam test asserts the plan's word; this one that the knob is inert).  At every width the GEMM path also holds the project's
    tolerance for a GEMM of its mode against float64, so a width at which both paths are wrong together cannot pass."""
    err, got = folded_against_the_gemms((2, 2, 3, 4), ctx_dim, precision)
    ref_max = max(1.0, float(np.abs(tail_case(ctx_dim, (2, 2, 3, 4))[2]).max()))
    for traj in (0, 1):
        assert err[traj, 1][0] <= GEMM_TOL[precision] * ref_max, (traj, err)
        if not WC.tail_folds(ctx_dim):
            np.testing.assert_array_equal(got[traj, 0], got[traj, 1], err_msg="no fold is planned at this width: the knob selects nothing")


def folded_against_the_gemms(shape, ctx_dim, precision):
    """one (shape, width, mode): every value of "tail_fold" x "out_traj" against float64; returns ((max, mean) errors, outputs) by (out_traj, tail_fold)"""
    eng, _ = get_engine(ctx_dim, 5)
    eng.set_step(10)
    X, hyp, ref = tail_case(ctx_dim, shape)
    err, got = {}, {}
    try:
        for traj in (0, 1):
            eng.set_tuning("out_traj", traj)
            for knob in (0, 1, 2):
                eng.set_tuning("tail_fold", knob)
                e, _ = eng.dbg_tail(X, hyp, STEP, shape, precision)
                assert np.isfinite(e).all()
                a = np.abs(e.astype(np.float64) - ref)
                err[traj, knob] = (float(a.max()), float(a.mean()))
                got[traj, knob] = e
    finally:
        eng.set_tuning("tail_fold", 0)
        eng.set_tuning("out_traj", 0)
    for traj in (0, 1):
        print(f"tail {shape} d={2 * ctx_dim} [{precision}] out_traj={traj} |e - float64|: folded max {err[traj, 0][0]:.3e} mean {err[traj, 0][1]:.3e}; "
              f"gemm max {err[traj, 1][0]:.3e} mean {err[traj, 1][1]:.3e}; |ref| max {np.abs(ref).max():.3e}")
    for traj in (0, 1):
        np.testing.assert_array_equal(got[traj, 2], got[traj, 0], err_msg=f"one-step table, out_traj {traj}")
        assert within_the_gemm_paths_error(precision, err[traj, 0], err[traj, 1]), (traj, err)
    np.testing.assert_array_equal(got[1, 0], got[0, 0], err_msg="per trajectory against per token")
    return err, got


# ---- 2. the whole loop ----
LOOP_CASES = ["net_jmid_w256_a2k3t4_s2.npz", "net_jmid_w32_a5k20t12_s50.npz", "net_jmid_w256_a5k20t12_s50.npz",
              "net_imid_w32_a2k3t4_s2.npz", "net_imid_w256_a5k20t12_s50.npz", "ddpm_jmid_w32_a2k3t4_s10.npz"]


@pytest.mark.parametrize("case", LOOP_CASES)
def test_denoise_loop_holds_the_gate_on_both_paths(case):
    """JMID and iMID, DDIM and DDPM: both paths pass the 1e-4 m gate against the reference capture in every split-fp16 mode, and the
    folded path's mean ADE does not exceed the GEMM path's by more than the difference between the f16x2 and the f16mx call on the
    same fixture (two roundings of the same net)."""
    z = np.load(os.path.join(GOLDEN, case))
    eng, w = get_engine(int(z["ctx_dim"]), int(z["wseed"]), bool(z["joint"]))
    assert w.checksum() == str(z["wsum"])
    ddpm = case.startswith("ddpm")
    eng.set_step(int(z["step"]), "ddpm" if ddpm else "ddim")
    ctx, x_T = z["ctx"][None], z["x_T"][None]
    kw = {"z": z["z"][:, None]} if ddpm else {}
    a = {}
    try:
        for knob in (0, 1):
            eng.set_tuning("tail_fold", knob)
            for precision in SPLIT_MODES:
                vel, _ = eng.denoise(x_T, ctx, precision=precision, want_pos=False, **kw)
                a[knob, precision] = ade(vel[0], z["vel"])
    finally:
        eng.set_tuning("tail_fold", 0)
        eng.set_step(int(z["step"]), "ddim")
    modes = abs(a[1, "f16x2"] - a[1, "f16mx"])
    print(f"{case} mean ADE(vel) vs reference: f16mx folded {a[0, 'f16mx']:.4e} gemm {a[1, 'f16mx']:.4e}; "
          f"f16x2 folded {a[0, 'f16x2']:.4e} gemm {a[1, 'f16x2']:.4e}; f16x3 folded {a[0, 'f16x3']:.4e} gemm {a[1, 'f16x3']:.4e}; "
          f"|f16x2 - f16mx| (gemm) {modes:.4e}")
    for precision in SPLIT_MODES:
        assert a[0, precision] <= ADE_GATE and a[1, precision] <= ADE_GATE, (precision, a)
    for precision in ("f16mx", "f16x2"):
        assert a[0, precision] <= a[1, precision] + modes, (precision, a)


_E64 = {}


def e_theta_float64():
    """One evaluation of the net on the one-scene fixture in float64 (the oracle on double weights), shared by the modes."""
    if not _E64:
        z = np.load(os.path.join(GOLDEN, "net_jmid_w256_a5k20t12_s50.npz"))
        eng, w = get_engine(int(z["ctx_dim"]), int(z["wseed"]), True)
        K, step = int(z["K"]), int(z["step"])
        w8 = {k: v.double() for k, v in w.tensors.items()}
        beta = float(ddim_steps(eng.schedule, step)[0].beta)
        ctx8 = torch.from_numpy(z["ctx"]).double().repeat(K, 1)
        x8 = torch.from_numpy(z["x_T"]).double()
        with torch.no_grad():
            e = O.net_forward(w8, x8, ctx8, torch.full([x8.shape[0]], beta, dtype=torch.float64), joint=True)
        _E64.update(z=z, e=e.numpy())
    return _E64["z"], _E64["e"]


@pytest.mark.parametrize("precision", SPLIT_MODES)
def test_net_eval_is_within_the_gemm_paths_error(precision):
    """jmid_net_eval (always the one-step table): e_theta of one scene on both paths against the float64 net, under the bound of the
    kernel test."""
    z, ref = e_theta_float64()
    eng, _ = get_engine(int(z["ctx_dim"]), int(z["wseed"]), True)
    eng.set_step(int(z["step"]))
    err = {}
    try:
        for knob in (0, 1):
            eng.set_tuning("tail_fold", knob)
            e = eng.net_eval(z["x_T"][None], z["ctx"][None], step_idx=0, precision=precision)[0]
            a = np.abs(e.astype(np.float64) - ref)
            err[knob] = (float(a.max()), float(a.mean()))
    finally:
        eng.set_tuning("tail_fold", 0)
    print(f"net_eval [{precision}] |e - float64|: folded max {err[0][0]:.3e} mean {err[0][1]:.3e}; gemm max {err[1][0]:.3e} mean {err[1][1]:.3e}")
    assert within_the_gemm_paths_error(precision, err[0], err[1]), err


# ---- 3. bits ----
@pytest.mark.parametrize("precision", ["f16mx", "f16x3"])
def test_bits_do_not_depend_on_chunks_lanes_kernel_form_table_form_or_repetition(precision):
    """4 episodes of the one-scene shape (5 agents, 20 samples, 12 steps ahead), 50 denoise steps: the table is built per chunk, or
    per step, and the step kernel runs per trajectory piece or per token, and none of it may change a bit."""
    eng, _ = get_engine(256, 5)
    eng.set_step(50)
    E, A, K, T = 4, 5, 20, 12
    g = torch.Generator().manual_seed(17)
    ctx = torch.randn([E, A, 256], generator=g).numpy()
    x_T = torch.randn([E, K * A, T, 2], generator=g).numpy()
    run = lambda: eng.denoise(x_T, ctx, precision=precision, want_pos=False)[0]
    try:
        eng.set_chunk_episodes(4)
        eng.set_tuning("lanes", 1)
        ref = run()
        assert np.isfinite(ref).all()
        np.testing.assert_array_equal(run(), ref)               # two consecutive calls on one handle
        for chunk in (1, 2, 4):
            for lanes in (1, 2):
                eng.set_chunk_episodes(chunk)
                eng.set_tuning("lanes", lanes)
                np.testing.assert_array_equal(run(), ref, err_msg=f"chunk {chunk} lanes {lanes}")
        eng.set_chunk_episodes(0)
        eng.set_tuning("lanes", 2)
        np.testing.assert_array_equal(run(), ref, err_msg="default plan")
        for traj in (1, 2, 0):
            eng.set_tuning("out_traj", traj)
            np.testing.assert_array_equal(run(), ref, err_msg=f"out_traj {traj}")
        eng.set_tuning("tail_fold", 2)
        np.testing.assert_array_equal(run(), ref, err_msg="tail_fold 2")
    finally:
        eng.set_tuning("tail_fold", 0)
        eng.set_tuning("out_traj", 0)
        eng.set_tuning("lanes", 2)
        eng.set_chunk_episodes(0)


# ---- 4. range ----
@pytest.mark.expects_erange
@pytest.mark.parametrize("knob", [0, 1])
def test_scaled_tail_weights_report_erange(knob):
    """concat3 and concat4 scaled by 2048 (their split planes stay inside the fp16 range, so the handle accepts the weights) and the
    output layer by 1e36: |Weff| of the unscaled net is about 1e-3, so the map leaves fp32 (about 6e39) while every factor on the way
    to it - v, q, u - stays finite.  The folded path says so (JMID_ERANGE) as the GEMM path does, where e overflows and the next
    step's planes meet a non-finite x - never finite garbage.  On the folded path the flag has to come from the table's build: the tail
    is first run alone (jmid_dbg_tail) on the same handle, where nothing runs after it."""
    w = JMIDWeights.from_seed(NetDims(ctx_dim=256), 5)
    t = dict(w.tensors)
    for name, s in (("concat3._layer.weight", 2048.0), ("concat4._layer.weight", 2048.0), ("linear._layer.weight", 1e36)):
        t[name] = t[name] * s
    eng = JmidEngine(JMIDWeights(w.dims, t), joint=True, step=2)
    try:
        eng.set_tuning("tail_fold", knob)
        g = torch.Generator().manual_seed(3)
        ctx = torch.randn([1, 5, 256], generator=g).numpy()
        x_T = torch.randn([1, 100, 12, 2], generator=g).numpy()
        if knob == 0:
            hyp = torch.randn([5, eng.hyper_width()], generator=g).numpy()
            X = torch.randn([1200, 512], generator=g).numpy()
            with pytest.raises(JmidError) as ei:
                eng.dbg_tail(X, hyp, 0, (1, 5, 20, 12), "f16mx")
            assert ei.value.code == -5, ei.value
        with pytest.raises(JmidError) as ei:
            eng.denoise(x_T, ctx, precision="f16mx", want_pos=False)
        assert ei.value.code == -5, ei.value
    finally:
        eng.close()
