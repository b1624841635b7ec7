"""The bounds of tests/seam_reference.py are neither impossible nor toothless (no GPU needed): a NumPy fp32 twin of the seam - the
hyper GEMM, the sampler update, the next step's embedding stored as the mode stores it -, with every mul-add both contracted into an
fma and not, stays inside every bound on the inputs of every case of tests/test_gpu_seam.py; and eleven emulated WRONG kernels each
leave the bound of their own stage wherever the fault can be expressed.

Every listed mutation leaves a derived bound at every case where it changes anything.  Where it does not, it is not a fault: the
hyper row "r // K" is the right row with one agent per episode; the tb offsets only exist from the second 12-token block of a wave's
piece on (T > 12 per trajectory); a piece starts mid-trajectory only where plan_step cuts trajectories (the 49 152-token case); the
lo-plane faults need a lo plane, the bf8 one the byte plane (f16mx at d_model 512).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_reference as R  # noqa: E402
import seam_reference as S  # noqa: E402
from test_layer_bounds_host import emu_gemm, store  # noqa: E402
from safe_interactive_crowdnav_amd.schedule import VarianceSchedule, ddim_steps, ddpm_steps
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

f32, f64 = np.float32, np.float64
CASES = [(s, c, m, 0) for s in S.SHAPES for c in S.OLD_WIDTHS for m in S.MODES] + [(S.BIG_SHAPE, 32, m, S.BIG_TPW) for m in ("f16mx", "f32")]
# ... and the other widths of tests/width_cases.py at the shapes the GPU test runs them at
CASES += [(s, c, m, 0) for s in S.NEW_SHAPES for c in S.WIDTHS if c not in S.OLD_WIDTHS for m in S.MODES]
DDIM_STEP, DDPM_STEP, DDPM_LAST, FLEX = 3, 40, 99, 0.5
_W = {}


def net(ctx_dim):
    if ctx_dim not in _W:
        t = JMIDWeights.from_seed(NetDims(ctx_dim=ctx_dim), 5).tensors
        d, dmid, dlow = S.dims_of(ctx_dim)
        W, b, tw = S.hyper_weights(t, d, dmid, dlow)
        g8 = lambda n: t[n].detach().cpu().numpy().astype(f64)
        sched = VarianceSchedule.linear()
        _W[ctx_dim] = dict(W=W, b=b, tw=tw, W1=g8("concat1._layer.weight"), b1=g8("concat1._layer.bias"), pe=S.positional_table(d),
                           L=S.hyper_layout(d, dmid, dlow), ddim=ddim_steps(sched, 10), ddpm=ddpm_steps(sched, 100, FLEX))
    return _W[ctx_dim]


def thyp_row(n, beta):
    """the handle's fp32 time row (jmid_weights.hip:69-72)"""
    b = f32(beta)
    tw = n["tw"].astype(f32)
    return tw[:, 0] * b + tw[:, 1] * f32(np.sin(b)) + tw[:, 2] * f32(np.cos(b))


def coef_of(n, kind, step):
    if kind == "ddim":
        s = n["ddim"][step]
        return dict(c_e=s.c_e, c_x=s.c_x, n_x=s.n_x, n_e=s.n_e, c0=f32(0), c1=f32(0), sigma=f32(0), noise=f32(0))
    s = n["ddpm"][step]
    return dict(c_e=f32(0), c_x=f32(1), n_x=f32(1), n_e=f32(0), c0=s.c0, c1=s.c1, sigma=s.sigma, noise=f32(s.noise))


# ------------------------------------------------------------------------------------------------ the twin
def fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def block_maps(shape, tpw):
    """per token: (t0 of its wave's piece, tb of its 12-token block inside the piece); tpw 0: one wave per token"""
    _, t = S.row_of(shape)
    if not tpw:
        return t, np.zeros_like(t)
    t0 = (t // tpw) * tpw
    return t0, ((t - t0) // 12) * 12


def twin_update(x, z, e, c, ddpm, contract, shape, tpw, mut=None):
    x, e = np.asarray(x, f32), np.asarray(e, f32)
    _, tb = block_maps(shape, tpw)
    src = np.arange(len(x)) - (tb if mut == "lane_no_tb" else 0)
    x = x[src]
    if ddpm:
        use = (z is not None and bool(c["noise"])) or (mut == "ddpm_last_adds_noise" and z is not None)
        if mut == "ddpm_mid_drops_noise":
            use = False
        zz = np.asarray(z, f32)[src] if use else np.zeros_like(x)
        if contract:
            return fma(c["c0"], fma(-c["c1"], e, x), c["sigma"] * zz)
        return c["c0"] * (x - c["c1"] * e) + c["sigma"] * zz
    if contract:
        return fma(c["n_x"], fma(-e, c["c_e"], x) / c["c_x"], c["n_e"] * e)
    return c["n_x"] * ((x - e * c["c_e"]) / c["c_x"]) + c["n_e"] * e


def twin_embed(xn, hyp, trow, n, shape, rep, contract, tpw, mut=None):
    E, A, K, T = shape
    d = n["W1"].shape[0]
    ea, t = S.row_of(shape)
    t0, tb = block_maps(shape, tpw)
    if mut == "ea_r_div_K":
        ea = (np.arange(len(t)) // T) // K
    if mut == "pe_no_tb":
        t = t - tb
    if mut == "t0_zero":
        t = t - t0
    W1, b1 = n["W1"].astype(f32), n["b1"].astype(f32)
    hyp, trow = np.asarray(hyp, f32), np.asarray(trow, f32)
    a = hyp[ea, :d] + (0 if mut == "gate_no_time" else trow[None, :d])
    gate = f32(1) / (f32(1) + np.exp(-a, dtype=f32))
    bias = hyp[ea, d:2 * d] + trow[None, d:2 * d]
    x0, x1 = np.asarray(xn, f32)[:, 0:1], np.asarray(xn, f32)[:, 1:2]
    if contract:
        lin = fma(W1[None, :, 1], x1, W1[None, :, 0] * x0) + b1[None, :]
        o = fma(lin, gate, bias) + n["pe"][t]
    else:
        lin = W1[None, :, 0] * x0 + W1[None, :, 1] * x1 + b1[None, :]
        o = lin * gate + bias + n["pe"][t]
    assert o.dtype == f32
    hi, lo = store(o, rep)
    if mut == "lo_zero":
        lo = np.zeros_like(lo)
    if mut == "bf8_trunc":
        l16 = R.split16(o)[1].astype(np.float16).view(np.uint16)
        lo = (l16 & 0xff00).view(np.float16).astype(f32)
    return hi, lo


def outside(dev, ref, bound):
    return int((np.abs(np.asarray(dev, f64) - ref) > bound).sum())


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("ctx_dim", S.WIDTHS)
@pytest.mark.parametrize("EA", [1, 4, 25])
def test_hyper_twin_is_inside_its_bound(EA, ctx_dim):
    n = net(ctx_dim)
    ctx = np.random.default_rng(EA + ctx_dim).standard_normal((EA, ctx_dim)).astype(f32)
    ref, bound = S.hyper_stage(ctx, n["W"], n["b"])
    dev = emu_gemm(ctx, np.zeros_like(ctx), n["W"], n["b"], "f32")
    assert outside(dev, ref, bound) == 0
    # a row of another (episode, agent) is far outside: the bound separates hyper rows
    if EA > 1:
        assert outside(np.roll(dev, 1, 0), ref, bound) > 0


@pytest.mark.parametrize("shape,ctx_dim,precision,tpw", CASES)
def test_twin_is_inside_and_every_wrong_kernel_is_outside(shape, ctx_dim, precision, tpw):
    E, A, K, T = shape
    d = S.dims_of(ctx_dim)[0]
    n, rep, inp = net(ctx_dim), S.rep_of(precision, d), S.seam_inputs(ctx_dim, shape)
    hyp = emu_gemm(inp["ctx"], np.zeros_like(inp["ctx"]), n["W"], n["b"], "f32")
    x, z, e = inp["x"], inp["z"], inp["e"]
    scen = {"ddim": ("ddim", DDIM_STEP, DDIM_STEP + 1, None), "ddpm": ("ddpm", DDPM_STEP, DDPM_STEP + 1, z), "last": ("ddpm", DDPM_LAST, -1, None)}
    forms = [tpw] if tpw else [0, T]                 # one wave per token and per trajectory ("out_traj" = 0 / 1); the big case: plan_step's own pieces

    def stages(name, form, contract, mut=None, z_in="scenario"):
        kind, step, nxt, zs = scen[name]
        zs = zs if isinstance(z_in, str) else z_in
        c = coef_of(n, kind, step)
        if mut == "ddim_coef_next":
            c = coef_of(n, kind, step + 1)
        beta = lambda i: (n["ddim"] if kind == "ddim" else n["ddpm"])[i].beta
        th, th_n = thyp_row(n, beta(step)), thyp_row(n, beta(max(nxt, 0)))
        de = S.contraction_term(e, hyp[S.row_of(shape)[0]], th, n["L"], folded=False)
        xn = twin_update(x, zs, e, c, kind == "ddpm", contract, shape, form, mut)
        u_ref, u_bound = S.update_stage(x, zs, e, coef_of(n, kind, step), kind == "ddpm", de)
        out = dict(update=outside(xn, u_ref, u_bound))
        if nxt >= 0:
            hi, lo = twin_embed(xn, hyp, th if mut == "time_row_i" else th_n, n, shape, rep, contract, form, mut)
            e_ref, e_bound = S.embed_stage(xn, hyp, th_n, n["W1"], n["b1"], n["pe"], shape, rep)
            out["embed"] = outside(S.stored(hi, lo), e_ref, e_bound)
        return out

    # 1. the correct twin, contracted and not, in both kernel forms
    for name in scen:
        for form in forms:
            for contract in (False, True):
                assert not any(stages(name, form, contract).values()), (name, form, contract)
    # the last DDPM entry takes no draw: a z that is passed is not read
    assert not any(stages("last", forms[-1], False, z_in=z).values())

    # 2. the wrong kernels, each against the bound of its own stage
    traj = forms[-1]
    hit = {}
    hit["time_row_i"] = stages("ddim", traj, False, "time_row_i")["embed"]
    hit["gate_no_time"] = stages("ddim", traj, False, "gate_no_time")["embed"]
    hit["ddpm_last_adds_noise"] = stages("last", traj, False, "ddpm_last_adds_noise", z_in=z)["update"]
    hit["ddpm_mid_drops_noise"] = stages("ddpm", traj, False, "ddpm_mid_drops_noise")["update"]
    hit["ddim_coef_next"] = stages("ddim", traj, False, "ddim_coef_next")["update"]
    if rep != "f32":
        hit["lo_zero"] = stages("ddim", traj, False, "lo_zero")["embed"]
    if A > 1:                                        # (one agent: r // K is the episode, the right row)
        hit["ea_r_div_K"] = stages("ddpm", traj, False, "ea_r_div_K")["embed"]
    if traj > 12:                                    # a second 12-token block inside a wave's piece
        hit["pe_no_tb"] = stages("ddim", traj, False, "pe_no_tb")["embed"]
        hit["lane_no_tb"] = min(stages(s, traj, False, "lane_no_tb")["update"] for s in ("ddim", "ddpm"))
    if tpw and tpw < T:                              # pieces that start mid-trajectory
        hit["t0_zero"] = stages("ddim", tpw, False, "t0_zero")["embed"]
    if rep == "hi_bf8":
        hit["bf8_trunc"] = stages("ddim", traj, False, "bf8_trunc")["embed"]
    print(f"seam host {shape} d={d} [{precision}] elements outside the bound per wrong kernel: {hit}")
    assert all(v > 0 for v in hit.values()), hit
