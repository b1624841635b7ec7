"""Float64 references of the stages of one transformer encoder layer, and componentwise error bounds made of named roundings.

Every function takes the planes (hi, lo: fp32 arrays of fp16 / bf8 values, as ``JmidEngine.dbg_layer`` returns them) of the stage
before it and the fp32 weights of the layer, and returns ``(ref, bound, plain)``:

* ``ref``: the stage in float64 ON THE OPERANDS THE MODE DEFINES - the A operand of a GEMM is its hi plane alone in F16X2 / F16MX
  kernels, hi + lo in F16X3, the fp32 value in F32; the residual is the planes the kernel reads; attention reads Q, K, V as
  delivered.  The 2^-11 an fp16 activation costs never enters it.
* ``bound``: same shape, |device - ref| <= bound for a correct kernel.  Each constant below counts roundings of the kernel named
  next to it (paths relative to safe-interactive-crowdnav_amd/csrc); there is no empirical factor.
* ``plain``: the stage in float64 on hi + lo of every input (what the tests of test_gpu_kernels.py compare against).

Arithmetic of a GEMM, by the GemmMode of its launch plan: "x3", "x2", "mx" (launch_plan.hpp: GM_X3, GM_X2, GM_MX), or "f32".
"""
import numpy as np

U16 = 2.0 ** -11          # fp16, round to nearest: relative error of one conversion (11 significand bits)
U32 = 2.0 ** -24          # fp32, round to nearest
PAIR = 2.0 ** -22         # hi + lo fp16 pair: lo = fp16(v - hi) rounds a residual of at most 2^-11 |v| (gemm_f16x3.hpp split_f32)
BF8 = 2.0 ** -3           # bf8 (e5m2), nearest by adding 0x80 below the top byte (gemm_f16x3.hpp bf8_of_f16): 3 significand bits
F16_FLOOR = 2.0 ** -25    # half the fp16 subnormal step: absolute error of a conversion below 2^-14
F16_FLOOR_RTZ = 2.0 ** -24
BF8_FLOOR = 2.0 ** -17    # half the bf8 subnormal step (2^-16)
LAMBDA = 8.0              # Higham-Mary: a sum of n roundings stays below LAMBDA sqrt(n) u with probability 1 - 2 exp(-LAMBDA^2 / 2)
KW = 256.0                # gemm_f16x3.hpp kWScale: weights are split as 256 W
LOG2E = 1.4426950408889634
EPS = 1e-5

GEMM_MODES = {-1: "f32", 0: "x3", 1: "x2", 2: "mx"}      # GemmMode words of dbg_layer's plan


# ---- the number formats (numpy twins of split_f32 / bf8_of_f16; used by the reference's callers and the host emulation) ----
def f16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def split16(x):
    """hi = fp16(x), lo = fp16(x - hi): gemm_f16x3.hpp split_f32"""
    x = np.asarray(x, np.float32)
    hi = f16(x)
    return hi, f16(x - hi)


def bf8(x):
    """the bf8 image of fp16(x), decoded: gemm_f16x3.hpp bf8_of_f16 (top byte after adding 0x80)"""
    bits = np.asarray(x, np.float32).astype(np.float16).view(np.uint16).astype(np.uint32)
    top = ((bits + 0x80) >> 8).astype(np.uint16) << 8
    return top.astype(np.uint16).view(np.float16).astype(np.float32)


def f16_rtz(x):
    """v_cvt_pkrtz_f16_f32: toward zero"""
    x = np.asarray(x, np.float32)
    h = x.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x)
    h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float32)


def layer_weights(tensors, layer):
    """the fp32 tensors of encoder layer ``layer`` as float64 arrays"""
    p = f"transformer_encoder.layers.{layer}."
    g = lambda n: tensors[p + n].detach().cpu().numpy().astype(np.float64)
    return dict(in_w=g("self_attn.in_proj_weight"), in_b=g("self_attn.in_proj_bias"), out_w=g("self_attn.out_proj.weight"),
                out_b=g("self_attn.out_proj.bias"), l1_w=g("linear1.weight"), l1_b=g("linear1.bias"), l2_w=g("linear2.weight"),
                l2_b=g("linear2.bias"), n1_g=g("norm1.weight"), n1_b=g("norm1.bias"), n2_g=g("norm2.weight"), n2_b=g("norm2.bias"))


def key_valid(n_agents, E, A, K, T):
    """[E, S] bool: key j of episode e is valid iff (j // T) % A < n[e] (scene.key_mask_words); n_agents None: all"""
    S = K * A * T
    if n_agents is None:
        return np.ones((E, S), bool)
    j = np.arange(S)
    return ((j // T) % A)[None, :] < np.asarray(n_agents).reshape(-1, 1)


def real_rows(n_agents, E, A, K, T):
    """[M] bool: token rows of real agents (the query rows of padded agents are garbage by design)"""
    return key_valid(n_agents, E, A, K, T).reshape(-1)


def layer_input(shape, n_agents, d):
    """X [M, d] fp32 of a case: standard normal, row scales a fixed permutation of linspace(0.25, 4, M) (large and small rows share
    tiles); the rows of padded agents are 6 x a real row of the same episode - their keys then score high and their values are large, so
    a padded key that gets through carries softmax weight of order 1, not 1 / S."""
    E, A, K, T = shape
    M = E * A * K * T
    rng = np.random.default_rng(1000 * d + M)
    X = rng.standard_normal((M, d)) * np.linspace(0.25, 4.0, M)[rng.permutation(M)][:, None]
    if n_agents is not None:
        real = real_rows(n_agents, E, A, K, T)
        S = K * A * T
        for e in range(E):
            rows = np.arange(e * S, (e + 1) * S)
            src = rows[real[rows]]
            pad = rows[~real[rows]]
            X[pad] = 6.0 * X[src[np.arange(len(pad)) % len(src)]]
    return X.astype(np.float32)


# ---- output representations ----
def out_term(ref, rep, scale=1.0):
    """The rounding of a result into the planes it is stored in.  ``scale``: the planes hold scale x the value (Q's pre-scale)."""
    a = np.abs(ref)
    if rep == "f32":
        return U32 * a
    if rep == "pair":          # hi + lo fp16
        return PAIR * a + F16_FLOOR / scale
    if rep == "hi":            # hi alone: the lo plane is not written (F16X2 / F16MX consumers take A_hi only)
        return U16 * a + F16_FLOOR / scale
    if rep == "hi_bf8":        # hi + bf8(lo): |lo| <= 2^-11 |v|, one bf8 rounding of it, after its own fp16 rounding
        return (PAIR + BF8 * U16) * a + BF8_FLOOR / scale
    raise ValueError(rep)


def abs_matmul(A, W):
    """|A| . |W|^T for a bound: fp32 arithmetic is plenty, widened by its own rounding"""
    return (np.abs(A).astype(np.float32) @ np.abs(W).astype(np.float32).T).astype(np.float64) * (1.0 + 1e-5)


# ---- GEMM-type stages ----
def weight_error(arith):
    """(u_w, absolute floor per weight, absolute floor per activation in units of |W|): the relative error of A . W as the mode
    represents the weight, read from the kernels' K loops."""
    if arith == "f32":         # gemm_f32.hpp: fp32 MFMA on the fp32 operands
        return 0.0, 0.0, 0.0
    pair_w, floor_w = PAIR, F16_FLOOR / KW                     # W_hi + W_lo of 256 W (split_planes_blocked_kernel)
    if arith == "x2":          # gemm_f16x3.hpp:10  acc += Ahi.Whi ; acc += Ahi.Wlo
        return pair_w, floor_w, 0.0
    if arith == "x3":          # gemm_f16x3.hpp:7   + Alo.Whi; the Alo.Wlo term (|Alo| <= 2^-11 |Ahi|, |Wlo| <= 2^-11 |Whi|) is dropped
        return pair_w + U16 * U16, floor_w, 0.0
    if arith == "mx":          # gemm_f16x3.hpp:1146-1147  acc += Ahi.Whi ; acc += bf8(Ahi) . bf8(Wlo)
        # |Wlo| <= 2^-11 |W|: bf8(Wlo) is off by BF8 |Wlo| (w8_image_kernel), bf8(Ahi) by BF8 |Ahi| against a factor of at most (1 + BF8) |Wlo|
        return pair_w + U16 * (BF8 + BF8 * (1.0 + BF8)), floor_w + BF8_FLOOR / KW, BF8_FLOOR * U16 * (1.0 + BF8)
    raise ValueError(arith)


def gemm_operand(hi, lo, arith):
    hi = np.asarray(hi, np.float64)
    return hi + np.asarray(lo, np.float64) if arith in ("x3", "f32") else hi


def gemm_core(A_hi, A_lo, W, b, arith):
    """(A . W^T + b in float64 on the mode's A operand, its bound before the output is stored, the same product on hi + lo)"""
    A = gemm_operand(A_hi, A_lo, arith)
    K = A.shape[1]
    ref = A @ W.T + b
    plain = ref
    if arith in ("x2", "mx") and np.any(A_lo):
        plain = (A + np.asarray(A_lo, np.float64)) @ W.T + b
    u_w, floor_w, floor_a = weight_error(arith)
    terms = {"f32": 1, "x3": 3, "x2": 2, "mx": 2}[arith]      # MFMA terms that go into the one fp32 accumulator per k
    mag = abs_matmul(A, W) + np.abs(b)
    bound = (u_w + LAMBDA * np.sqrt(terms * K) * U32) * mag
    bound = bound + floor_w * np.abs(A).sum(1, keepdims=True) + floor_a * np.abs(W).sum(1)[None, :]
    bound = bound + 2 * U32 * np.abs(ref)                     # the epilogue: acc x 2^-8 is exact, + bias rounds once; one more for the accumulator's last add
    return ref, bound, plain


def gemm_stage(A_hi, A_lo, W, b, arith, relu, out_rep):
    """linear1 + ReLU (gemm_f16x3.hpp epilogue OUT_SPLIT; gemm_f32.hpp): ReLU is 1-Lipschitz, the bound passes through it"""
    ref, bound, plain = gemm_core(A_hi, A_lo, W, b, arith)
    if relu:
        ref, plain = np.maximum(ref, 0.0), np.maximum(plain, 0.0)
    return ref, bound + out_term(ref, out_rep), plain


def qkv_stage(X_hi, X_lo, W, b, arith, reps, qscale):
    """in_proj as the attention kernel reads it (OUT_QKV epilogue: gemm_f16x3.hpp:255-270, the staged rows :793-870; OUT_F32 for iMID
    and F32).  reps = (Q, K, V) output representations; Q is stored as planes of q x qscale and read back / qscale (qkv0.hpp
    qkv_planes_read_kernel): two fp32 roundings around the planes' own."""
    ref, bound, plain = gemm_core(X_hi, X_lo, W, b, arith)
    d = ref.shape[1] // 3
    for part, rep in enumerate(reps):
        sl = slice(part * d, (part + 1) * d)
        scale = qscale if part == 0 and rep != "f32" else 1.0
        bound[:, sl] += out_term(ref[:, sl], rep, scale)
        if part == 0 and rep != "f32":
            bound[:, sl] += 3 * U32 * np.abs(ref[:, sl])      # x qscale, the read-back's hi + lo and / qscale
    return ref, bound, plain


# ---- LayerNorm stages ----
def ln_stage(X_hi, X_lo, A_hi, A_lo, W, b, gamma, beta, arith, out_rep, A_err=None, A_plain=None):
    """X <- LayerNorm(X + A . W^T + b) gamma + beta.  v in float64 on the planes the kernel reads (residual: X_hi + X_lo; A: the mode's
    operand); the GEMM bound delta propagated to first order through y = (v - mu) / sigma gamma + beta; the fp32 statistics' own
    roundings (elementwise.hpp add_ln_kernel:138-159, gemm_ln2_mx.hpp add_ln2_kernel:494-520: two-pass variance, rsqrtf, the fma chain
    of the output); the output term.
    A_err (with A_hi a float64 reference of A and A_lo zero): A never left the device - the out-projection merged the split-KV partials
    itself (gemm_small.hpp lnx_combine) -, the operand the kernel formed lies within A_err of A_hi: that enters delta as A_err . |W|^T.
    A_plain: the plain reference of such an A."""
    X = np.asarray(X_hi, np.float64) + np.asarray(X_lo, np.float64)
    y_ref, delta, y_plain = gemm_core(A_hi, A_lo, W, b, arith)
    if A_err is not None:
        delta = delta * (1.0 + U16) + abs_matmul(A_err, W)
        y_plain = np.asarray(A_plain, np.float64) @ W.T + b
    d = X.shape[1]
    v, v_plain = X + y_ref, X + y_plain
    # hi + lo of the residual is one fp32 add, + Y another (Y itself was stored as fp32 on the unfused path: a third)
    delta = delta + 3 * U32 * (np.abs(X) + np.abs(y_ref))

    def norm(v):
        mu = v.mean(1, keepdims=True)
        sig = np.sqrt(((v - mu) ** 2).mean(1, keepdims=True) + EPS)
        return mu, sig, (v - mu) / sig * gamma + beta

    mu, sig, ref = norm(v)
    dev = np.abs(v - mu)
    ag = np.abs(gamma)[None, :] / sig
    prop = ag * (delta + delta.mean(1, keepdims=True) + dev / sig ** 2 * (dev * delta).mean(1, keepdims=True))
    n_sum = LAMBDA * np.sqrt(d) * U32                          # a sum of d fp32 values (wave_sum / the 8-block merge)
    mean_err = n_sum * np.abs(v).mean(1, keepdims=True)        # mu
    sig_rel = 0.5 * (n_sum + 4 * U32) + 2 * U32                # var: v - mu and its square round once each, the sum, / d + eps; sigma is half of it; rsqrtf 1 ulp
    stats = ag * (mean_err + dev * sig_rel + 2 * U32 * (np.abs(v) + np.abs(mu)))      # (v - mu) rstd [or fma(v, rstd, -mu rstd)]: two roundings at |v| + |mu|
    stats = stats + 2 * U32 * (np.abs(ref) + np.abs(beta)[None, :])                   # x gamma, + beta
    return ref, prop + stats + out_term(ref, out_rep), norm(v_plain)[2]


# ---- attention ----
def logit_error(kind):
    """relative error of q . k as the kernel forms it from the planes delivered, on |q| . |k| (attn_f16x3.hpp)."""
    if kind == "f32":          # attn_f32.hpp: fp32 products of the fp32 values
        return 0.0, 1
    if kind == "f16":          # :188-190 / :667-669  Kh.Qh + Kh.Ql + Kl.Qh: the Kl.Ql term is dropped
        return U16 * U16, 3
    if kind == "bf8":          # :633, :650-651  Kh.Qh + bf8(Kh).bf8(Ql) + bf8(Kl).bf8(Qh) on the images delivered (Ql, Kl ARE bf8 values):
        # bf8(Kh) is off by BF8 |Kh| against |Ql| <= (1 + BF8) 2^-11 |Qh|, the same with Q and K exchanged, and Kl.Ql is dropped
        return 2 * BF8 * (1 + BF8) * U16 + ((1 + BF8) * U16) ** 2, 3
    raise ValueError(kind)


def attention_stage(qkv_hi, qkv_lo, nseq, S, nhead, valid, logits, p_rep, v_lo_used, out_rep, nsplit=1):
    """softmax(q k^T / sqrt(hd)) v per head on Q, K, V as stage 1 delivered them (hi + lo; V's lo plane only where the kernel reads
    it).  valid [nseq, S]: the key mask.  logits: "f32" | "f16" | "bf8" (logit_error); p_rep: how P enters P . V - "p1" one fp16 plane
    rounded to nearest (attn_f16x3.hpp:702-711), "split" hi + lo by truncation (split8, :41-51; the P_lo . V_lo term is dropped when V has
    a lo plane), "f32"."""
    M, d3 = qkv_hi.shape
    d = d3 // 3
    hd = d // nhead
    full = np.asarray(qkv_hi, np.float64) + np.asarray(qkv_lo, np.float64)
    q = full[:, :d].reshape(nseq, S, nhead, hd).transpose(0, 2, 1, 3)
    k = full[:, d:2 * d].reshape(nseq, S, nhead, hd).transpose(0, 2, 1, 3)
    v_src = full[:, 2 * d:] if v_lo_used else np.asarray(qkv_hi[:, 2 * d:], np.float64)
    v = v_src.reshape(nseq, S, nhead, hd).transpose(0, 2, 1, 3)
    scale = 1.0 / np.sqrt(hd)
    s = (q @ k.swapaxes(-1, -2)) * scale                                        # nats
    a = (np.abs(q).astype(np.float32) @ np.abs(k).astype(np.float32).swapaxes(-1, -2)).astype(np.float64) * scale * (1 + 1e-5)
    mask = valid[:, None, None, :]
    s = np.where(mask, s, -np.inf)
    a = np.where(mask, a, 0.0)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ref = p @ v
    pav = p @ np.abs(v)
    # Delta_i: the bound on a query's logits, in nats (the kernels work in log2 units on Q pre-scaled by log2(e) / sqrt(hd): the same
    # relative errors).  The accumulator starts at minus the reference maximum (:314), |m| <= max_j |s_j| <= max_j a_j
    u_qk, terms = logit_error(logits)
    amax = a.max(-1, keepdims=True)
    Delta = (u_qk + 2 * U32) * a                                                # + the read-back's / qscale and the kernel's own x scale
    Delta = Delta + LAMBDA * np.sqrt(terms * hd) * U32 * (a + amax)             # fp32 accumulation of terms x hd products onto -m
    Delta = Delta + 2 * U32 * amax                                              # s - m, and - delta on the slow path (:700)
    Delta_i = Delta.max(-1, keepdims=True)
    u_exp = 2.0 ** -22                                                          # v_exp_f32 / expf: within 1 ulp, doubled
    if p_rep == "p1":
        u_p, p_floor = U16, F16_FLOOR
    elif p_rep == "split":
        u_p = 2.0 ** -20 + (2.0 ** -10 * U16 if v_lo_used else 0.0)           # two truncations; P_lo . V_lo dropped
        p_floor = F16_FLOOR_RTZ
    else:
        u_p, p_floor = 0.0, 0.0
    n_acc = LAMBDA * np.sqrt(S * (1 if p_rep != "split" else 3)) * U32         # P . V and the row sum l, each a sum over the keys
    rel = np.expm1(2 * Delta_i) + u_exp + u_p + 2 * n_acc
    rel = rel + 3 * U32                                                          # 1 / l and O x inv (:900-911)
    if nsplit > 1:                                                               # attn_combine_kernel :950-990 / gemm_small.hpp lnx_combine:
        rel = rel + u_exp + 5 * U32                                              # w_i = 2^(m_i - M), w_i O_i, w_i l_i, their sums, the division
    bound = rel * pav
    # P below 2^-14 of its reference maximum is an fp16 subnormal: absolute error p_floor, against a row maximum of P that is >= 1 when formed
    # (in units of the normalised P: p_floor x the row's largest weight, on every valid key's |v|)
    bound = bound + p_floor * p.max(-1, keepdims=True) * np.einsum("nk,nhkc->nhc", valid.astype(np.float64), np.abs(v))[:, :, None, :]
    ref = ref.transpose(0, 2, 1, 3).reshape(M, d)
    bound = bound.transpose(0, 2, 1, 3).reshape(M, d)
    bound = bound + out_term(ref, out_rep)
    plain = ref
    if not v_lo_used and np.any(qkv_lo[:, 2 * d:]):
        vp = full[:, 2 * d:].reshape(nseq, S, nhead, hd).transpose(0, 2, 1, 3)
        plain = (p @ vp).transpose(0, 2, 1, 3).reshape(M, d)
    return ref, bound, plain


# ---- what a mode's layer does, from dbg_layer's plan ----
def stage_specs(precision, joint, plan, last):
    """The arithmetic and the representations of the five computed stages of a layer in ``precision`` on a JMID (joint) or iMID net,
    as the launch plan of jmid_dbg_layer says (jmid_planner.hip net_step / residual_block)."""
    if precision == "f32":
        return dict(in_proj="f32", qkv_reps=("f32",) * 3, logits="f32", p_rep="f32", v_lo=True, attn_out="f32",
                    out_proj="f32", x_rep="f32", linear1="f32", h1_rep="f32", linear2="f32", x_last_rep="f32")
    x2 = precision in ("f16x2", "f16mx")
    m = lambda key: GEMM_MODES[plan[key]]
    if joint:
        q_rep = "hi_bf8" if plan["q8l"] else "pair"
        k_rep = "hi_bf8" if plan["k8"] else "pair"
        v_rep = "hi" if x2 else "pair"                         # F16X2: the V^T lo plane is not written (attn_f16x3.hpp:489)
        logits = "bf8" if plan["k8"] else "f16"
        p_rep = "p1" if (x2 and plan["attn_dma"]) else "split"   # one plane of P in the LDS-DMA kernel's two-term modes
        attn_out = "hi" if x2 else "pair"
        v_lo = not x2
        qkv_reps = (q_rep, k_rep, v_rep)
    else:                      # iMID: in_proj to fp32, the exact-fp32 attention kernel, its output as hi + lo planes (attn_f32.hpp:161-172)
        qkv_reps, logits, p_rep, attn_out, v_lo = ("f32",) * 3, "f32", "f32", "pair", True
    x_rep = "hi_bf8" if plan["byte_lo"] else "pair"
    x_last = x_rep if not (last and x2) else "hi"
    return dict(in_proj=m("in_proj_mode"), qkv_reps=qkv_reps, logits=logits, p_rep=p_rep, v_lo=v_lo, attn_out=attn_out,
                out_proj=m("out_proj_mode"), x_rep=x_rep, linear1=m("linear1_mode"), h1_rep="hi" if x2 else "pair",
                linear2=m("linear2_mode"), x_last_rep=x_last)
