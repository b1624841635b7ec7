#!/usr/bin/env python3
"""Generate tests/golden/padded_*.npz by RUNNING THE REFERENCE's masked branch (build container only, as make_golden.py):

    python tests/golden/make_golden_padded.py

JointPredictionTransformerConcatLinear.forward(..., mask=attn_mask) (MID/models/diffusion.py:186-195) is how the reference puts scenes of
different agent counts through one joint sequence.  The mask here is generate_mask's (MID/dataset/preprocessing.py:36-89) for rows
(e, s, a) of a padded batch [E, K * A] - 0 where two tokens belong to real rows of the same episode, 0 on the diagonal, -inf elsewhere -
and the token order is that branch's own: token (row, t) at row * T + t.

Per fixture: x [E, K*A, T, 2] and ctx [E, A, ctx_dim] (zeros in the padded agents' rows), n_agents [E], the reference's
e = net([x, ctx rows], beta_100, mask=M) and the velocities of a 4-step DDIM loop (diffusion.py:524-528) driven by that masked net.
The script asserts that the real rows agree with the reference's UNMASKED branch on each episode compacted to A = n_agents[e] to 1e-5
(measured: the `compact_err` stored in the file), which is what the padded entry points promise.  Stored: dims, seed, weight checksum, data.
"""
import os

import numpy as np

from make_golden import REPO, build_ref_sampler, install_shims, np32  # noqa: F401  (install_shims runs on import)

import torch  # noqa: E402

from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
STEP = 4          # DDIM steps of the loop: t = 100, 75, 50, 25


def row_mask(n_agents, A, K, T):
    """attn_mask [E K A T, E K A T] for rows (e, s, a), tokens (row, t)."""
    E = len(n_agents)
    ep = np.repeat(np.arange(E), K * A * T)
    real = np.concatenate([np.tile(np.repeat(np.arange(A) < n, T), K) for n in n_agents])
    ok = (ep[:, None] == ep[None, :]) & real[:, None] & real[None, :]
    ok |= np.eye(ok.shape[0], dtype=bool)
    m = torch.zeros(ok.shape, dtype=torch.float32)
    m[torch.from_numpy(~ok)] = float("-inf")
    return m


def ddim_loop(net_eval, x_T, var_sched):
    """diffusion.py:508-531 with sampling="ddim", the net call abstracted."""
    stride = 100 // STEP
    x = x_T
    for t in range(100, 0, -stride):
        ab, ab_next = var_sched.alpha_bars[t], var_sched.alpha_bars[t - stride]
        e = net_eval(x, t)
        x0 = (x - e * (1 - ab).sqrt()) / ab.sqrt()
        x = ab_next.sqrt() * x0 + (1 - ab_next).sqrt() * e
    return x


def gen(tag, ctx_dim, A, K, T, n_agents, wseed, dseed):
    weights = JMIDWeights.from_seed(NetDims(ctx_dim=ctx_dim), wseed)
    sampler = build_ref_sampler(weights, True)
    net, vs = sampler.net, sampler.var_sched
    E = len(n_agents)
    g = torch.Generator().manual_seed(dseed)
    x = torch.randn([E, K * A, T, 2], generator=g)
    ctx = torch.randn([E, A, ctx_dim], generator=g)
    real = torch.tensor([[a < n for a in range(A)] for n in n_agents])                 # [E, A]
    ctx = ctx * real[:, :, None]
    x = (x.view(E, K, A, T, 2) * real[:, None, :, None, None]).reshape(E, K * A, T, 2)
    M = row_mask(n_agents, A, K, T)
    ctx_rows = ctx[:, None].expand(E, K, A, ctx_dim).reshape(E * K * A, ctx_dim)

    def masked(xx, t):
        return net([xx.reshape(E * K * A, T, 2), ctx_rows], beta=vs.betas[[t] * (E * K * A)], mask=M).reshape(E, K * A, T, 2)

    with torch.no_grad():
        e = masked(x, 100)
        vel = ddim_loop(masked, x, vs)
        assert torch.isfinite(e).all() and torch.isfinite(vel).all()
        err = 0.0
        for ep, n in enumerate(n_agents):
            xc = x[ep].view(K, A, T, 2)[:, :n].reshape(K * n, T, 2)
            cc = ctx[ep, :n].repeat(K, 1)

            def compact(xx, t):
                return net([xx, cc], beta=vs.betas[[t] * (K * n)])

            for ours, theirs in ((e[ep], compact(xc, 100)), (vel[ep], ddim_loop(compact, xc, vs))):
                err = max(err, float((ours.view(K, A, T, 2)[:, :n] - theirs.view(K, n, T, 2)).abs().max()))
    assert err <= 1e-5, err
    name = f"padded_{tag}.npz"
    np.savez_compressed(os.path.join(HERE, name), ctx_dim=ctx_dim, A=A, K=K, T=T, step=STEP, wseed=wseed, dseed=dseed, wsum=weights.checksum(),
                        n_agents=np.asarray(n_agents, np.int32), x=np32(x), ctx=np32(ctx), e=np32(e), vel=np32(vel.view(E, K, A, T, 2)),
                        compact_err=err)
    print(f"wrote {name}: {os.path.getsize(os.path.join(HERE, name)) / 1024:.1f} KB, masked vs compact {err:.2e}")


def main():
    for ctx_dim, w in ((32, "w32"), (256, "w256")):
        # S = 384, 12 key tiles: episode 1 has all-zero words 2, 5, 8, 11, episode 0 all-ones words throughout, the rest partial
        gen(f"{w}_e3a4k8t12", ctx_dim, 4, 8, 12, [4, 1, 3], 61 + (ctx_dim == 256), 701)
        # S = 90: the last tile is also cut by S
        gen(f"{w}_e3a3k5t6", ctx_dim, 3, 5, 6, [2, 3, 1], 63 + (ctx_dim == 256), 702)


if __name__ == "__main__":
    main()
