"""Layer 0's Q / K / V^T operand planes expanded from per-(row, step) coefficient tables (csrc/qkv0.hpp) against the in_proj GEMM
they replace (jmid_set_tuning "qkv0" = 1): accuracy against float64, the whole denoise loop against the reference goldens, bit
invariance under chunking / lanes / repetition, and the fp16-range report."""
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
GEMM_TOL = {"f16x3": 4e-5, "f16x2": 2e-3, "f16mx": 2e-3}      # TOL of tests/test_gpu_kernels.py: max |err| relative to max(1, max |ref|)

_ENGINES = {}


def get_engine(ctx_dim, wseed, nhead=4):
    key = (ctx_dim, wseed) if nhead == 4 else (ctx_dim, wseed, nhead)
    if key not in _ENGINES:
        w = JMIDWeights.from_seed(NetDims(ctx_dim=ctx_dim, nhead=nhead), wseed)
        _ENGINES[key] = (JmidEngine(w, joint=True), w)
    return _ENGINES[key]


def ade(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64), axis=-1).mean())


# ---- 1. the kernel against float64 ----
_REF = {}


def qkv0_case(ctx_dim, shape, nhead=4):
    """Inputs of one case and in_proj(embed(x)) of layer 0 in float64 from the same fp32 weights, hyper rows and time row; made once
    per (width, shape) and shared by the three modes."""
    key = (ctx_dim, shape) if nhead == 4 else (ctx_dim, shape, nhead)
    if key not in _REF:
        eng, w = get_engine(ctx_dim, 5, nhead)
        eng.set_step(10)
        E, A, K, T = shape
        d = 2 * ctx_dim
        width = eng.hyper_width()             # gate1 | bias1 | gate3 | bias3 | gate4 | bias4 | gateO | biasO; the library refuses any other
        M = E * K * A * T
        g = torch.Generator().manual_seed(1000 * ctx_dim + M)
        x = torch.randn([M, 2], generator=g).numpy()
        hyp = torch.randn([E * A, width], generator=g).numpy()
        step = 3
        _, thyp = eng.dbg_qkv0(x, hyp, step, shape, "f16x3")
        f8 = lambda name: w.tensors[name].numpy().astype(np.float64)
        # The time row is an INPUT of the kernels under test (both paths read the handle's fp32 table), so the reference takes the
        # row the handle holds - after checking it against its definition, w0 beta + w1 sin(beta) + w2 cos(beta) over the three time
        # columns of concat1's hyper nets, evaluated here in float64 from the step table's fp32 beta.
        beta = float(ddim_steps(eng.schedule, 10)[step].beta)
        tcol = np.array([beta, np.sin(beta), np.cos(beta)])
        t_def = np.concatenate([f8("concat1._hyper_gate.weight")[:, :3] @ tcol, f8("concat1._hyper_bias.weight")[:, :3] @ tcol])
        np.testing.assert_allclose(thyp[:2 * d], t_def, rtol=0, atol=4e-7 * np.abs(f8("concat1._hyper_gate.weight")[:, :3]).sum(1).max() + 1e-7)
        W1, b1 = f8("concat1._layer.weight"), f8("concat1._layer.bias")
        Win, b_in = f8("transformer_encoder.layers.0.self_attn.in_proj_weight"), f8("transformer_encoder.layers.0.self_attn.in_proj_bias")
        pe = O.positional_encoding(24, d)[:, 0, :].numpy().astype(np.float64)
        m = np.arange(M)
        r, t = m // T, m % T
        ea = (r // (K * A)) * A + r % A
        h8, t8 = hyp.astype(np.float64), thyp.astype(np.float64)
        gate = 1.0 / (1.0 + np.exp(-(h8[ea, :d] + t8[None, :d])))
        bias = h8[ea, d:2 * d] + t8[None, d:2 * d]
        X0 = (x.astype(np.float64) @ W1.T + b1) * gate + bias + pe[t]
        _REF[key] = (x, hyp, step, X0 @ Win.T + b_in)
    return _REF[key]


@pytest.mark.parametrize("precision", SPLIT_MODES)
@pytest.mark.parametrize("ctx_dim", WC.OLD_CTX_DIMS)
@pytest.mark.parametrize("shape", [(2, 2, 3, 4), (3, 3, 5, 7), (1, 5, 20, 12)])
def test_expanded_planes_are_no_further_from_float64_than_the_gemm(shape, ctx_dim, precision, nhead=4):
    """S = 24 (rows and samples vary inside a sequence), S = 105 (S % 4 != 0: the V^T layout that needed the transpose kernel) and
    S = 1200 (one scene: ragged 128-row tile, panel boundaries), at d_model 64 (head_dim 16: no bf8 images) and 512 (K / Q_lo images in
    f16mx).  The expansion drops the fp16 rounding of the embedding in front of the GEMM, so its max and mean absolute error against
    float64 are bounded by the GEMM path's on the same inputs, without a margin."""
    eng, _ = get_engine(ctx_dim, 5, nhead)
    eng.set_step(10)
    x, hyp, step, ref = qkv0_case(ctx_dim, shape, nhead)
    err = {}
    try:
        for knob in (0, 1, 2):                # 2: the expansion with the table's GEMM as one running sum (printed, not bounded)
            eng.set_tuning("qkv0", knob)
            got, _ = eng.dbg_qkv0(x, hyp, step, shape, precision)
            assert np.isfinite(got).all()
            e = np.abs(got.astype(np.float64) - ref)
            err[knob] = (float(e.max()), float(e.mean()))
    finally:
        eng.set_tuning("qkv0", 0)
    print(f"qkv0 {shape} d={2 * ctx_dim} [{precision}] |err| vs float64: expanded max {err[0][0]:.3e} mean {err[0][1]:.3e}; "
          f"gemm max {err[1][0]:.3e} mean {err[1][1]:.3e}; expanded without per-tile sums max {err[2][0]:.3e} mean {err[2][1]:.3e}; "
          f"|ref| max {np.abs(ref).max():.3e}")
    assert err[0][0] <= err[1][0], err
    assert err[0][1] <= err[1][1], err
    # ... and the yardstick itself cannot drift: the GEMM path holds the project's tolerance for a GEMM of its mode (test_gpu_kernels.py)
    assert err[1][0] <= GEMM_TOL[precision] * max(1.0, float(np.abs(ref).max())), err


@pytest.mark.parametrize("precision", SPLIT_MODES)
@pytest.mark.parametrize("net", WC.NEW_NETS, ids=WC.net_id)
def test_expanded_planes_at_every_other_accepted_width_and_head_size(net, precision):
    """The same comparison at the other rows of tests/width_cases.py, at S = 24: head sizes 32 and 64 (the planes' head-major V^T
    layout), d_model 192 (in_proj's N = 576 and K = 192 are no multiples of 128: the GEMM path it is compared with runs F16X2's kernel in
    an f16mx call), d_model 1024 with the bf8 images."""
    test_expanded_planes_are_no_further_from_float64_than_the_gemm((2, 2, 3, 4), net[0], precision, net[1])


# ---- 2. the whole loop ----
@pytest.mark.parametrize("case", ["net_jmid_w256_a2k3t4_s2.npz", "net_jmid_w32_a5k20t12_s50.npz", "net_jmid_w256_a5k20t12_s50.npz"])
def test_denoise_loop_holds_the_gate_on_both_paths(case):
    """Both paths pass the 1e-4 m gate against the reference capture in every split-fp16 mode (all three take the new path), and the
    default path's mean ADE does not exceed the GEMM path's by more than the difference between the f16x2 and the f16mx call on the
    same fixture (two roundings of the same net)."""
    z = np.load(os.path.join(GOLDEN, case))
    eng, w = get_engine(int(z["ctx_dim"]), int(z["wseed"]))
    assert w.checksum() == str(z["wsum"])
    eng.set_step(int(z["step"]))
    ctx, x_T = z["ctx"][None], z["x_T"][None]
    a = {}
    try:
        for knob in (0, 1):
            eng.set_tuning("qkv0", knob)
            for precision in SPLIT_MODES:
                vel, _ = eng.denoise(x_T, ctx, precision=precision, want_pos=False)
                a[knob, precision] = ade(vel[0], z["vel"])
    finally:
        eng.set_tuning("qkv0", 0)
    modes = abs(a[1, "f16x2"] - a[1, "f16mx"])
    print(f"{case} mean ADE(vel) vs reference: f16mx expanded {a[0, 'f16mx']:.4e} gemm {a[1, 'f16mx']:.4e}; "
          f"f16x2 expanded {a[0, 'f16x2']:.4e} gemm {a[1, 'f16x2']:.4e}; f16x3 expanded {a[0, 'f16x3']:.4e} gemm {a[1, 'f16x3']:.4e}; "
          f"|f16x2 - f16mx| (gemm) {modes:.4e}")
    for precision in SPLIT_MODES:
        assert a[0, precision] <= ADE_GATE and a[1, precision] <= ADE_GATE, (precision, a)
    for precision in ("f16mx", "f16x2"):      # (f16x3 is fp32-class on both paths: its distance to an fp32 capture is the capture's own rounding)
        assert a[0, precision] <= a[1, precision] + modes, (precision, a)


# ---- 3. bits ----
def test_bits_do_not_depend_on_chunks_lanes_transpose_knob_or_repetition():
    """4 episodes of the one-scene shape (5 agents, 20 samples, 12 steps ahead), 50 denoise steps, f16mx: the tables are built per chunk
    and the expansion picks its launch shape per chunk, and neither may change a bit."""
    eng, _ = get_engine(256, 5)
    eng.set_step(50)
    E, A, K, T = 4, 5, 20, 12
    g = torch.Generator().manual_seed(11)
    ctx = torch.randn([E, A, 256], generator=g).numpy()
    x_T = torch.randn([E, K * A, T, 2], generator=g).numpy()
    run = lambda: eng.denoise(x_T, ctx, precision="f16mx", want_pos=False)[0]
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
        for novt in (1, 0):
            eng.set_tuning("no_vt_direct", novt)
            np.testing.assert_array_equal(run(), ref, err_msg=f"no_vt_direct {novt}")
    finally:
        eng.set_tuning("no_vt_direct", 0)
        eng.set_tuning("lanes", 2)
        eng.set_chunk_episodes(0)


# ---- 4. range ----
@pytest.mark.expects_erange
@pytest.mark.parametrize("knob", [0, 1])
def test_scaled_layer0_weights_report_erange(knob):
    """concat1 and layer 0's in_proj scaled by 64: Q / K / V leave the fp16 range, and the call says so (JMID_ERANGE) on the expanded
    path as it does on the GEMM path - never finite garbage.  The scale is the given one; the input is chosen so that the planes do
    leave the range: at unit-normal x the unscaled |QKV0| peaks near 3.5 (the float64 test prints it), so 64 x 64 alone gives 1.4e4,
    under the 6e4 limit on either path; x = 32 N(0, 1) puts the planes at several 1e5 while the embedding itself (64 x 0.7 x |x| of a
    few thousand at most) stays in range - the planes are where the flag has to come from.  The flag of a whole call could also come
    from a later kernel that meets the poisoned planes, so the layer-0 kernels are first run alone (jmid_dbg_qkv0: embedding + the
    planes, nothing after them) on the same scaled handle and input: they must raise it themselves."""
    w = JMIDWeights.from_seed(NetDims(ctx_dim=256), 5)
    t = dict(w.tensors)
    for name in ("concat1._layer.weight", "concat1._layer.bias", "transformer_encoder.layers.0.self_attn.in_proj_weight"):
        t[name] = t[name] * 64.0
    eng = JmidEngine(JMIDWeights(w.dims, t), joint=True, step=2)
    try:
        eng.set_tuning("qkv0", knob)
        g = torch.Generator().manual_seed(3)
        ctx = torch.randn([1, 5, 256], generator=g).numpy()
        x_T = (32.0 * torch.randn([1, 100, 12, 2], generator=g)).numpy()
        hyp = torch.randn([5, eng.hyper_width()], generator=g).numpy()
        with pytest.raises(JmidError) as ei:
            eng.dbg_qkv0(x_T.reshape(-1, 2), hyp, 0, (1, 5, 20, 12), "f16mx")
        assert ei.value.code == -5, ei.value
        with pytest.raises(JmidError) as ei:
            eng.denoise(x_T, ctx, precision="f16mx", want_pos=False)
        assert ei.value.code == -5, ei.value
    finally:
        eng.close()
