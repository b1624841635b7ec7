"""Float64 references of the seam between e_theta of denoise step i and the residual stream of step i + 1, and componentwise error
bounds made of named roundings (the style of tests/layer_reference.py, whose constants and helpers are reused).

The seam: the ctx part of the hyper nets (once per call), the sampler update of x, the next step's embedding (ConcatSquash 2 -> d plus
the positional row) as the mode stores it.  Every stage function returns ``(ref, bound)``:

* ``ref``: the stage in float64 on the operands the device read - fp32 arrays taken as exact.
* ``bound``: same shape, |device - ref| <= bound for a correct kernel.  Each constant counts roundings of the line named next to it
  (paths relative to safe-interactive-crowdnav_amd/csrc); there is no empirical factor.

Token m of a call of shape (E, A, K, T) is ((e K + k) A + a) T + t; its hyper row is e A + a (common.hpp RowMap).
"""
import math

import numpy as np

import width_cases as WC
from layer_reference import BF8, LAMBDA, PAIR, U32, abs_matmul, bf8, gemm_core, out_term, split16  # noqa: F401  (re-exported for the tests)

G32 = U32 / (1.0 - 16 * U32)      # one fp32 rounding with the products of up to 16 of them folded in (Higham's gamma_n / n)
U_EXP = 2.0 ** -22                # expf: within 1 ulp (layer_reference.attention_stage's u_exp)
U_DIV = 2.0 ** -23                # fp32 division: within 1 ulp (correctly rounded under hipcc's default; 1 ulp also covers a reciprocal + fix-up)
PE_MAX_LEN = 24
FILL_F16 = float(np.array([0x3c3c], np.uint16).view(np.float16)[0])      # an fp16 plane of JMID_DBG_SEAM_FILL bytes
FILL_BF8 = 1.0                                                           # the bf8 byte 0x3c


# ---- the handle's tables, rebuilt from their definitions ----
def hyper_layout(d, dmid, dlow):
    """offsets of gate1 | bias1 | gate3 | bias3 | gate4 | bias4 | gateO | biasO in a hyper row (jmid_weights.hip)"""
    o, out = 0, {}
    for name, n in (("1", d), ("3", dmid), ("4", dlow), ("o", 2)):
        out["g" + name], out["b" + name] = o, o + n
        o += 2 * n
    out["total"] = o
    return out


def hyper_weights(tensors, d, dmid, dlow):
    """(Whyp [width, ctx_dim], bhyp [width], time columns [width, 3]) in float64: the ctx part of the four hyper nets as the handle
    packs it (jmid_weights.hip:217-246) - column 0..2 of a hyper layer's weight is the time embedding, the rest ctx"""
    L = hyper_layout(d, dmid, dlow)
    g8 = lambda n: tensors[n].detach().cpu().numpy().astype(np.float64)
    C = g8("concat1._hyper_gate.weight").shape[1] - 3
    W, b, tw = np.zeros((L["total"], C)), np.zeros(L["total"]), np.zeros((L["total"], 3))
    for prefix, key, n in (("concat1", "1", d), ("concat3", "3", dmid), ("concat4", "4", dlow), ("linear", "o", 2)):
        wg, bg, wb = g8(f"{prefix}._hyper_gate.weight"), g8(f"{prefix}._hyper_gate.bias"), g8(f"{prefix}._hyper_bias.weight")
        go, bo = L["g" + key], L["b" + key]
        W[go:go + n], W[bo:bo + n] = wg[:, 3:], wb[:, 3:]
        b[go:go + n] = bg
        tw[go:go + n], tw[bo:bo + n] = wg[:, :3], wb[:, :3]
    return W, b, tw


def positional_table(d):
    """the handle's fp32 table [24, d] by its own recipe (jmid_weights.hip:191-201): fp32 products, libm exp / sin / cos in double
    (Python's math module calls the same libm), each rounded to fp32"""
    f = np.float32
    coef = f(-math.log(10000.0) / d)
    pe = np.zeros((PE_MAX_LEN, d), np.float32)
    for i in range(0, d, 2):
        div = f(math.exp(float(f(i) * coef)))
        for pos in range(PE_MAX_LEN):
            arg = float(f(pos) * div)
            pe[pos, i] = f(math.sin(arg))
            if i + 1 < d:
                pe[pos, i + 1] = f(math.cos(arg))
    return pe


def time_row_check(thyp, tw, beta):
    """(definition of a time row in float64: w0 beta + w1 sin(beta) + w2 cos(beta), tolerance of the handle's fp32 evaluation of it):
    three fp32 products and two sums of terms of at most sum |w| each, sinf / cosf within 2 ulp of values <= 1 (jmid_weights.hip:69-72)"""
    b = float(beta)
    ref = tw @ np.array([b, math.sin(b), math.cos(b)])
    tol = 9 * U32 * np.abs(tw).sum(1) + 1e-30
    return ref, tol


def row_of(shape):
    """(hyper row ea [M], position t [M]) of every token"""
    E, A, K, T = shape
    m = np.arange(E * A * K * T)
    r = m // T
    return (r // (K * A)) * A + r % A, m % T


# ---- the cases (shared by the host and the GPU test) ----
NETS = WC.NETS                                       # (ctx_dim, nhead): every row of tests/width_cases.py
WIDTHS = WC.CTX_DIMS                                 # their ctx_dim: nothing of the seam reads the head count (dims_of)
OLD_WIDTHS = WC.OLD_CTX_DIMS                         # d_model 64 and 512: every shape below; the other rows: NEW_SHAPES
MODES = ["f32", "f16x3", "f16x2", "f16mx"]
# (E, A, K, T): M = 1; 48 tokens, several hyper rows in a wave's neighbourhood; T odd, 315 tokens across 128-row panels; with
# "out_traj" = 1 a wave takes 12 tokens + 1; T at the positional table's limit, two full blocks
SHAPES = [(1, 1, 1, 1), (2, 2, 3, 4), (3, 3, 5, 7), (1, 2, 3, 13), (2, 1, 2, 24)]
# 49 152 tokens: plan_step picks 12 tokens per wave by itself, half the pieces start at t0 = 12 (d_model 64, "out_traj" = 0)
BIG_SHAPE, BIG_TPW = (8, 4, 64, 24), 12
# the rows beyond the two old widths: one token; T odd across 128-row panels; T at the positional table's limit
NEW_SHAPES = [(1, 1, 1, 1), (3, 3, 5, 7), (2, 1, 2, 24)]
tail_folds, per_trajectory = WC.tail_folds, WC.per_trajectory      # what the plan does beyond tail_fold.hpp's limits (d_model 1024)


def rep_of(precision, d):
    """how the mode stores the residual stream (jmid_planner.hip byte_lo_plane, embed_args)"""
    return "f32" if precision == "f32" else "hi_bf8" if (precision == "f16mx" and d == 512) else "pair"


def dims_of(ctx_dim, nhead=None):
    """d_model, d_mid, d_low (weights.NetDims); with nhead also the head size - which no stage of the seam reads"""
    dims = (2 * ctx_dim, ctx_dim, ctx_dim // 2)
    return dims if nhead is None else dims + (2 * ctx_dim // nhead,)


def seam_inputs(ctx_dim, shape):
    """x ~ N(0, 1) with one row in sixteen x 8 and one in sixteen / 64 (at least one row x 8), z ~ N(0, 1), X with LayerNorm-like rows,
    ctx ~ N(0, 1), hyper rows given directly ~ N(0, 1) (their gates saturate more than ctx-made rows do), and an e ~ N(0, 1) for the
    host test, which has no tail"""
    E, A, K, T = shape
    M, (d, dmid, dlow) = E * A * K * T, dims_of(ctx_dim)
    rng = np.random.default_rng(3000 * ctx_dim + 7 * M + T)
    x = rng.standard_normal((M, 2))
    rows = rng.permutation(M)
    n = max(1, M // 16)
    x[rows[:n]] *= 8.0
    x[rows[n:2 * n]] /= 64.0
    z = rng.standard_normal((M, 2))
    X = rng.standard_normal((M, d))
    X = (X - X.mean(1, keepdims=True)) / X.std(1, keepdims=True)
    ctx = rng.standard_normal((E * A, ctx_dim))
    hyp = rng.standard_normal((E * A, hyper_layout(d, dmid, dlow)["total"]))
    e = rng.standard_normal((M, 2))
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(x=f(x), z=f(z), X=f(X), ctx=f(ctx), hyp=f(hyp), e=f(e))


# ---- stages ----
def hyper_stage(ctx, W, b):
    """ctx @ Whyp^T + bhyp (jmid_planner.hip fill_workspace: run_gemm<EPI_BIAS>, gemm_f32.hpp): layer_reference's F32 GEMM bound"""
    ref, bound, _ = gemm_core(np.asarray(ctx, np.float64), np.zeros_like(ctx, dtype=np.float64), W, b, "f32")
    return ref, bound


def contraction_term(e, hyp_rows, thyp, L, folded):
    """|e of the updating instance - e of the e_out instance| if the compiler contracted the output expression differently in the two.
    GEMM path (elementwise.hpp:220-221 / :326-327): e = fl(fl(fl(p) + hb) + tb), p = (s + bo) g; contracted, fl(fma(s + bo, g, hb)) loses
    the rounding of p: the two differ by at most U32 |p| + U32 (|fl(p) + hb| + |p + hb|), and the last add rounds each once more:
    2 U32 |e|.  With |p| <= |e| + |hb| + |tb| and |p + hb| <= |e| + |tb|:  U32 (5 |e| + |hb| + 3 |tb|).
    Folded path (tail_fold.hpp:232-241): explicit fmaf, then sums only - nothing to contract: zero.
    (The build passes -ffp-contract=off, so on the shipped library the term is slack; it is kept for a build without the flag.)"""
    e = np.abs(np.asarray(e, np.float64))
    if folded:
        return np.zeros_like(e)
    hb = np.abs(hyp_rows[:, L["bo"]:L["bo"] + 2].astype(np.float64))
    tb = np.abs(thyp[L["bo"]:L["bo"] + 2].astype(np.float64))[None, :]
    return G32 * (5 * e + hb + 3 * tb)


def update_stage(x, z, e, coef, ddpm, de):
    """The sampler update in float64 on fp32 x, z, e and the handle's fp32 coefficients; ``de``: contraction_term.
    DDIM (elementwise.hpp:233-235, :341-343; tail_fold.hpp:250-252):  t1 = e c_e, t2 = x - t1, p = t2 / c_x, t3 = n_x p, t4 = n_e e,
    x' = t3 + t4 - one rounding each (the division within an ulp), each carried to x' by the factors behind it.
    DDPM (elementwise.hpp:230-231, :338-339; tail_fold.hpp:247-248):  t1 = c1 e, t2 = x - t1, t3 = c0 t2, t4 = sigma z, x' = t3 + t4;
    z None, or an entry that takes no draw: t4 is absent."""
    x, e = np.asarray(x, np.float64), np.asarray(e, np.float64)
    c = {k: float(v) for k, v in coef.items()}
    if ddpm:
        zz = np.asarray(z, np.float64) if (z is not None and c["noise"]) else np.zeros_like(x)
        t1 = c["c1"] * e
        t2 = x - t1
        t3 = c["c0"] * t2
        t4 = c["sigma"] * zz
        ref = t3 + t4
        bound = G32 * (abs(c["c0"]) * (np.abs(t1) + np.abs(t2)) + np.abs(t3) + np.abs(t4) + np.abs(ref))
        bound = bound + abs(c["c0"] * c["c1"]) * de
    else:
        t1 = e * c["c_e"]
        t2 = x - t1
        p = t2 / c["c_x"]
        t3 = c["n_x"] * p
        t4 = c["n_e"] * e
        ref = t3 + t4
        f = abs(c["n_x"] / c["c_x"])
        bound = G32 * (f * (np.abs(t1) + np.abs(t2)) + np.abs(t3) + np.abs(t4) + np.abs(ref)) + U_DIV * np.abs(t3)
        bound = bound + abs(c["n_e"] - c["n_x"] * c["c_e"] / c["c_x"]) * de
    return ref, bound


def embed_stage(x_next, hyp, thyp_row, W1, b1, pe, shape, rep, t0_of=None):
    """ConcatSquash(2 -> d) + positional row in float64 on the device's x_next [M, 2], the device's hyper rows [E A, width] and the
    handle's time row, stored as ``rep`` ("f32" | "pair" | "hi_bf8").  W1 [d, 2], b1 [d] float64, pe [24, d] fp32.
    elementwise.hpp embed_cols:40-41 and embed_store_cols:48-49:
        a = h_g + t_g (1 rounding), E = expf(-a) (1 ulp), gate = 1 / (1 + E) (1 rounding, division 1 ulp)
              -> |d gate| <= gate ((1 - gate) (U_EXP + U32 |a|) + U32 + U_DIV)                       [E / (1 + E) = 1 - gate]
        bias = h_b + t_b (1)
        lin = w0 x0 + w1 x1 + b1: two products, two sums (4)
        o = lin gate + bias + pe: one product, two sums (3)
    then out_term(ref, rep)."""
    E, A, K, T = shape
    d = W1.shape[0]
    ea, t = row_of(shape)
    x = np.asarray(x_next, np.float64)
    h8, t8 = np.asarray(hyp, np.float64), np.asarray(thyp_row, np.float64)
    a = h8[ea, 0:d] + t8[None, 0:d]
    gate = 1.0 / (1.0 + np.exp(-a))
    bias = h8[ea, d:2 * d] + t8[None, d:2 * d]
    p0, p1 = x[:, 0:1] * W1[None, :, 0], x[:, 1:2] * W1[None, :, 1]
    lin = p0 + p1 + b1[None, :]
    m = lin * gate
    n = m + bias
    ref = n + np.asarray(pe, np.float64)[t]
    d_gate = gate * ((1.0 - gate) * (U_EXP + G32 * np.abs(a)) + G32 + U_DIV)
    d_bias = G32 * np.abs(bias)
    d_lin = G32 * (np.abs(p0) + np.abs(p1) + np.abs(p0 + p1) + np.abs(lin))
    d_m = gate * d_lin + np.abs(lin) * d_gate + G32 * np.abs(m)
    bound = d_m + d_bias + G32 * np.abs(n) + G32 * np.abs(ref)
    return ref, bound + out_term(ref, rep)


def stored(hi, lo):
    """the value the planes hold, float64"""
    return np.asarray(hi, np.float64) + np.asarray(lo, np.float64)


def untouched_planes(X, precision, rep):
    """(hi, lo) of the embedding's buffers as jmid_dbg_seam leaves them before the launch: X as split where the tail reads the plane,
    the fill byte elsewhere"""
    X = np.asarray(X, np.float32)
    if precision == "f32":
        return X, np.zeros_like(X)
    hi, lo = split16(X)
    if precision == "f16x3":
        return hi, lo
    return hi, np.full_like(X, FILL_BF8 if rep == "hi_bf8" else FILL_F16)
