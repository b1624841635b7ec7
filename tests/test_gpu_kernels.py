"""Single-kernel checks of the HIP library against float64 numpy/torch references (GPU box only)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tests.width_cases as WC
from safe_interactive_crowdnav_amd.engine import JmidEngine
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

PRECISIONS = ["f32", "f16x3", "f16x2", "f16mx"]
# max abs error allowed relative to max|ref| per precision mode
# (f16x2: the activation operand is its fp16 hi plane, 2^-12 relative per element)
TOL = {"f32": 2e-5, "f16x3": 4e-5, "f16x2": 2e-3, "f16mx": 2e-3, "f16": 2e-2}


@pytest.fixture(scope="module", params=WC.OLD_CTX_DIMS)
def engine(request):
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=request.param), 1), joint=True)
    yield eng
    eng.close()


# head sizes 32 and 64 (attn_f16x3_kernel<32 | 64>, attn_f32_kernel<32 | 64>; 64 also at d_model 512): for the attention test only - the
# GEMM tests do not depend on the handle's width
@pytest.fixture(scope="module", params=[(64, 4), (128, 4), (256, 8)], ids=WC.net_id)
def head_engine(request):
    assert request.param in WC.NEW_NETS
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=request.param[0], nhead=request.param[1]), 1), joint=True)
    yield eng
    eng.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("M,N,K,relu", [(1200, 1536, 512, False), (77, 16, 32, False), (300, 192, 64, True),
                                        (129, 130, 96, False), (2500, 512, 1024, True), (5, 1796, 256, False),
                                        (40000, 512, 512, False)])
def test_gemm_matches_float64(engine, M, N, K, relu, precision):
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    # asymmetric data (transpose-detecting): scale rows / cols differently
    A *= np.linspace(0.5, 1.5, M, dtype=np.float32)[:, None]
    W *= np.linspace(1.5, 0.5, N, dtype=np.float32)[:, None]
    ref = A.astype(np.float64) @ W.astype(np.float64).T + b
    if relu:
        ref = np.maximum(ref, 0)
    out = engine.dbg_gemm(A, W, b, relu=relu, precision=precision)
    err = np.abs(out - ref).max()
    assert err <= TOL[precision] * max(1.0, np.abs(ref).max()), err


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("M,N,K,relu", [(16800, 576, 192, False), (16800, 192, 192, False), (16800, 384, 192, True), (16800, 192, 384, False)])
def test_gemm_matches_float64_at_the_batch_shapes_of_d_model_192(engine, M, N, K, relu, precision):
    """in_proj, out_proj, linear1 and linear2 of d_model 192 (tests/width_cases.py) at 16 800 rows = 131 row tiles of 128 + 32 rows: enough
    tiles for the 128 x 128 shape (launch_plan.hpp large_gemm_shape), whose last column tile is cut at N = 576 and N = 192 - a shape the
    net's GEMMs at d_model 64 and 512 never take (tests/test_host_logic.py pins the plan)."""
    test_gemm_matches_float64(engine, M, N, K, relu, precision)


ATTN_SHAPES = [(2, 1200), (7, 12), (3, 48), (2, 33), (1, 129), (5, 1), (2, 24)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nseq,S", ATTN_SHAPES)
def test_attention_matches_float64_at_head_sizes_32_and_64(head_engine, nseq, S, precision):
    test_attention_matches_float64(head_engine, nseq, S, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nseq,S", ATTN_SHAPES)
def test_attention_matches_float64(engine, nseq, S, precision):
    d = 2 * engine.dims.ctx_dim
    nh = engine.dims.nhead
    hd = d // nh
    rng = np.random.default_rng(nseq * 1000 + S)
    qkv = rng.standard_normal((nseq * S, 3 * d)).astype(np.float32)
    qkv[:, :d] *= 1.7  # sharper softmax
    out = engine.dbg_attention(qkv, nseq, S, precision=precision)
    t = torch.from_numpy(qkv).double().view(nseq, S, 3, nh, hd)
    q, k, v = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(nseq * S, d).numpy()
    assert np.abs(out - ref).max() <= TOL[precision] * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_attention_online_softmax_rescale_branch_at_head_sizes_32_and_64(head_engine, precision):
    test_attention_online_softmax_rescale_branch(head_engine, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_attention_online_softmax_rescale_branch(engine, precision):
    """A key whose score dwarfs everything seen so far must rescale the running state correctly, in every mode's kernel (the default
    precision of dbg_attention is the exact-fp32 kernel alone): spike one key late in the sequence (cdna guide rule: force the rare
    branch), and a smaller one in an earlier tile that is not the first - query 17's reference maximum moves twice, by 3 sqrt(hd) and by
    another 3 sqrt(hd) nats (17 log2 units at head 16: past the lazy rule's 8; 49 at head 128: past the threshold rule's 14)."""
    d = 2 * engine.dims.ctx_dim
    nh = engine.dims.nhead
    hd = d // nh
    S = 200
    rng = np.random.default_rng(0)
    qkv = rng.standard_normal((S, 3 * d)).astype(np.float32)
    qkv[150, d:2 * d] = 6.0 * qkv[17, :d]  # key 150 aligned with query 17 -> huge score in a late tile
    qkv[70, d:2 * d] = 3.0 * qkv[17, :d]   # ... and half of it in tile 2
    out = engine.dbg_attention(qkv, 1, S, precision=precision)
    t = torch.from_numpy(qkv).double().view(1, S, 3, nh, hd)
    q, k, v = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(S, d).numpy()
    err = np.abs(out - ref).max()
    print(f"rescale branch d={d} head {hd} [{precision}]: |err| {err:.3e} (allowed {TOL[precision] * max(1.0, np.abs(ref).max()):.3e})")
    assert err <= TOL[precision] * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("M", [1, 5, 1200])
def test_add_layernorm_matches_torch(engine, M):
    d = 2 * engine.dims.ctx_dim
    rng = np.random.default_rng(M)
    X = rng.standard_normal((M, d)).astype(np.float32)
    Y = rng.standard_normal((M, d)).astype(np.float32)
    g = rng.standard_normal(d).astype(np.float32)
    b = rng.standard_normal(d).astype(np.float32)
    out = engine.dbg_add_layernorm(X, Y, g, b)
    ref = torch.nn.functional.layer_norm(torch.from_numpy(X + Y).double(), (d,), torch.from_numpy(g).double(),
                                         torch.from_numpy(b).double(), 1e-5).numpy()
    assert np.abs(out - ref).max() <= 1e-5


@pytest.mark.parametrize("precision", ["f16x3", "f16x2", "f16mx"])
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("M,N,K", [(700, 512, 512), (513, 256, 64), (1025, 1536, 512)])
def test_f16x3_gemm_variants_agree_bitwise(engine, variant, M, N, K, precision):
    """Every tile configuration of the split-fp16 GEMM accumulates k in the same order with the same three MFMAs per
    step (two in f16x2; f16mx: four fp16 steps, then the fp8 correction of the k64 block): the kernels are interchangeable
    bit for bit (tile selection by size must not change a result).  The register-staged kernels (variants 1, 2) have no
    fp8-correction K loop: forced in f16mx they compute the f16x2 products (correction term in fp16), bit for bit what the
    f16x2 GEMM's own choice of kernel computes."""
    ref_precision = "f16x2" if precision == "f16mx" and variant in (1, 2) else precision
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    try:
        engine.set_tuning("gemm_h_variant", 0)
        ref = engine.dbg_gemm(A, W, b, precision=ref_precision)
        engine.set_tuning("gemm_h_variant", variant)
        out = engine.dbg_gemm(A, W, b, precision=precision)
    finally:
        engine.set_tuning("gemm_h_variant", 0)
    np.testing.assert_array_equal(out, ref)
    exact = A.astype(np.float64) @ W.astype(np.float64).T + b
    assert np.abs(out - exact).max() <= TOL[precision] * max(1.0, np.abs(exact).max())


@pytest.mark.parametrize("rows", [64, 128])
@pytest.mark.parametrize("M,K", [(64, 512), (300, 512), (7200, 1024), (1000, 64)])
def test_f16mx_fused_gemm_layernorm_gen2_matches_float64_and_its_unfused_pair(M, K, rows):
    """gemm_ln2_mx_kernel (JMID_PREC_F16MX, d_model 512: transposed product, row statistics in the accumulators, byte lo
    plane of the residual stream) against float64, and bit for bit against the GEMM + add_ln2 pair small launches use -
    nn.TransformerEncoderLayer's x = norm(x + sublayer(x)) as built at MID/models/diffusion.py:161-166."""
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=256), 1), joint=True)
    try:
        rng = np.random.default_rng(M + K)
        A = rng.standard_normal((M, K)).astype(np.float32) * np.linspace(0.5, 1.5, M, dtype=np.float32)[:, None]
        W = (rng.standard_normal((512, K)) / np.sqrt(K)).astype(np.float32) * np.linspace(1.5, 0.5, 512, dtype=np.float32)[:, None]
        b, g, t = (rng.standard_normal(512).astype(np.float32) for _ in range(3))
        X = rng.standard_normal((M, 512)).astype(np.float32) * 2.0
        eng.set_tuning("ln_rows", rows)          # both tile shapes of the fused kernel (128 rows x 8 waves, 64 rows x 4 waves)
        fused = eng.dbg_gemm_ln_mx(A, W, b, g, t, X, fused=True)
        pair = eng.dbg_gemm_ln_mx(A, W, b, g, t, X, fused=False)
    finally:
        eng.close()
    v = X.astype(np.float64) + A.astype(np.float64) @ W.astype(np.float64).T + b
    ref = (v - v.mean(1, keepdims=True)) / np.sqrt(v.var(1, keepdims=True) + 1e-5) * g + t
    bad = np.argwhere(np.abs(fused - ref) > 2e-2)
    assert len(bad) == 0, (len(bad), bad[:10], np.unique(bad[:, 1] % 128)[:40])
    # inputs enter as fp16 (A_hi, X as hi + bf8(lo)): 2^-11 relative per operand, outputs leave as hi + bf8(lo)
    assert np.abs(fused - ref).max() <= 6e-3 * max(1.0, np.abs(ref).max())
    np.testing.assert_array_equal(fused, pair)




@pytest.mark.parametrize("M,K", [(64, 512), (300, 512), (1200, 512), (1200, 1024), (2048, 1024), (1999, 128), (1, 512),
                                 (2049, 512), (2400, 512), (2400, 1024), (4096, 1024), (4001, 128)])      # (> 2048 rows: two workgroups per CU)
def test_small_launch_gemm_with_statistics_exchange_equals_its_unfused_pair(M, K):
    """gemm_small_kernel<.., OUT_LNX> (one scene in F16MX: out_proj / linear2 + residual + LayerNorm in ONE launch - the eight
    workgroups of a 64-row tile exchange the row statistics as {value, launch tag} granules and normalise their own 64 columns)
    against float64 and bit for bit against the GEMM + add_ln2 pair and the row-complete batch kernel; repeated, so that a stale granule (the buffer is reused
    launch after launch, only the tag moves) or an unlucky arrival order would show - every word is compared."""
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=256), 1), joint=True)
    try:
        rng = np.random.default_rng(M + K)
        A = rng.standard_normal((M, K)).astype(np.float32) * np.linspace(0.5, 1.5, M, dtype=np.float32)[:, None]
        W = (rng.standard_normal((512, K)) / np.sqrt(K)).astype(np.float32) * np.linspace(1.5, 0.5, 512, dtype=np.float32)[:, None]
        b, g, t = (rng.standard_normal(512).astype(np.float32) for _ in range(3))
        X = rng.standard_normal((M, 512)).astype(np.float32) * 2.0
        pair = eng.dbg_gemm_ln_mx(A, W, b, g, t, X, fused=0)
        row_complete = eng.dbg_gemm_ln_mx(A, W, b, g, t, X, fused=1)
        np.testing.assert_array_equal(row_complete, pair)
        eng.set_tuning("small_lnx", 0)           # what ships: two exchanges (sums, then squared deviations from the row mean), the canonical order
        for _ in range(8):
            fused = eng.dbg_gemm_ln_mx(A, W, b, g, t, X, fused=3)
            np.testing.assert_array_equal(fused, pair)
        eng.set_tuning("small_lnx", 1)           # diagnostics: ONE exchange, the variance merged from the blocks' (mean, M2) pairs -
        one = [eng.dbg_gemm_ln_mx(A, W, b, g, t, X, fused=3) for _ in range(8)]      # deterministic, but another summation order:
        for o in one[1:]:
            np.testing.assert_array_equal(o, one[0])
        # ... a last-bit difference of a row statistic can move an output across an fp16 rounding boundary of its hi plane; hi + bf8(lo)
        # then differ by at most one step of the lo image (2^-14 of the value)
        assert np.abs(one[0] - pair).max() <= 2.5e-4 * max(1.0, np.abs(pair).max())
        assert (one[0] != pair).mean() <= 0.02
    finally:
        eng.close()
    v = X.astype(np.float64) + A.astype(np.float64) @ W.astype(np.float64).T + b
    ref = (v - v.mean(1, keepdims=True)) / np.sqrt(v.var(1, keepdims=True) + 1e-5) * g + t
    bad = np.argwhere(np.abs(fused - ref) > 2e-2)
    assert len(bad) == 0, (len(bad), bad[:10], np.unique(bad[:, 1] % 128)[:40])
    assert np.abs(fused - ref).max() <= 6e-3 * max(1.0, np.abs(ref).max())

