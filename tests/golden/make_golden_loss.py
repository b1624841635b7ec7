#!/usr/bin/env python3
"""Generate tests/golden/loss_*.npz by RUNNING THE REFERENCE's DiffusionTraj.get_loss (build container only, as make_golden.py):

    python tests/golden/make_golden_loss.py

get_loss (MID/models/diffusion.py:448-476) is called in eval mode with explicit per-row timesteps `t`, the masks of the reference's own
generate_mask (MID/dataset/preprocessing.py:35-89) made from NaN-padded futures, and `torch.Tensor.cuda` patched to the identity (the
function moves its operands with .cuda(); there is no GPU in the build container).  torch.manual_seed(dseed) precedes the call, so the
e_rand it draws (`torch.randn_like(x_0)`, its only draw) is re-drawn here and stored; a spy on net.forward captures e_theta.

Per fixture: x0 [E, A, T, 2] and ctx [E, A, ctx_dim] (zeros in the padded agents' rows, as masked_fill leaves them), t [E, A], n_agents [E]
(absent for iMID), e, the reference's e_theta and loss, dims, seeds and the weight checksum: data only.  The script asserts that the masked
e_theta agrees with the UNMASKED branch on each episode compacted to A = n_agents[e] to 1e-5 and that the loss is the fp64 mean over the
compacted episodes (stored: `compact_err`, `loss_rel`).  t holds 1 and 100 and both repeated and distinct values inside one scene.
"""
import os

import numpy as np

from make_golden import build_ref_sampler, install_shims, np32  # noqa: F401  (install_shims runs on import)
from make_golden_padded import row_mask

import torch  # noqa: E402

from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims  # noqa: E402
from sicnav_diffusion.JMID.MID.dataset.preprocessing import generate_mask  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def timesteps(E, A, n_agents, rng):
    """[E, A] in 1..100: 1 and 100 present on real rows, a repeated value and distinct values inside one scene where it has the rows."""
    t = rng.integers(2, 100, size=(E, A))
    real = [(e, a) for e in range(E) for a in range(n_agents[e])]
    t[real[0]] = 100
    t[real[-1]] = 1
    big = max(range(E), key=lambda e: n_agents[e])
    if n_agents[big] >= 3:
        t[big, 1] = t[big, 2] = 37          # repeated inside one scene, next to a distinct one
    elif n_agents[big] == 2 and E >= 2:
        other = [e for e in range(E) if e != big][0]
        t[other, 0] = t[big, 0]             # (two-agent scenes: repeated across scenes, distinct inside)
    return t


def gen(tag, ctx_dim, A, T, n_agents, joint, wseed, dseed):
    weights = JMIDWeights.from_seed(NetDims(ctx_dim=ctx_dim), wseed)
    sampler = build_ref_sampler(weights, joint)
    E = len(n_agents)
    g = torch.Generator().manual_seed(dseed)
    x0 = torch.randn([E, A, T, 2], generator=g)
    ctx = torch.randn([E, A, ctx_dim], generator=g)
    real = torch.tensor([[a < n for a in range(A)] for n in n_agents])                 # [E, A]
    t = timesteps(E, A, n_agents, np.random.default_rng(dseed))
    tl = t.reshape(-1).tolist()
    seen = {}

    def spy(module, args, kwargs, out):
        seen["e_theta"] = out.detach().clone()

    hook = sampler.net.register_forward_hook(spy, with_kwargs=True)
    cuda, torch.Tensor.cuda = torch.Tensor.cuda, lambda self, *a, **k: self
    try:
        with torch.no_grad():
            if joint:
                y_nan = x0.clone()
                y_nan[~real] = float("nan")
                batch = [None, None, y_nan.reshape(E * A, T, 2)]
                attn_mask, loss_mask = generate_mask(batch, E, T)
                assert torch.equal(attn_mask, row_mask(n_agents, A, 1, T))               # the mask the padded entry points are tested with
                x0 = x0 * real[:, :, None, None]                                          # masked_fill: NaN -> 0
                ctx = ctx * real[:, :, None]
                torch.manual_seed(dseed)
                loss = sampler.get_loss(x0.reshape(E * A, T, 2), ctx.reshape(E * A, ctx_dim), batch_size=E, attn_mask=attn_mask,
                                        loss_mask=loss_mask, t=tl)
            else:
                torch.manual_seed(dseed)
                loss = sampler.get_loss(x0.reshape(E * A, T, 2), ctx.reshape(E * A, ctx_dim), t=tl)
            torch.manual_seed(dseed)
            e = torch.randn_like(x0.reshape(E * A, T, 2)).reshape(E, A, T, 2)
            e_theta = seen["e_theta"].reshape(E, A, T, 2)
            assert torch.isfinite(e_theta).all() and torch.isfinite(loss)
            # the unmasked branch on every episode compacted to its real agents, fed the x_t get_loss formed
            vs = sampler.var_sched
            tt = torch.as_tensor(t)
            ab = vs.alpha_bars[tt]
            x_t = torch.sqrt(ab)[..., None, None] * x0 + torch.sqrt(1 - ab)[..., None, None] * e
            err, sq = 0.0, []
            for ep, n in enumerate(n_agents):
                ec = sampler.net([x_t[ep, :n], ctx[ep, :n]], beta=vs.betas[tt[ep, :n]])
                err = max(err, float((ec - e_theta[ep, :n]).abs().max()))
                sq.append(((ec - e[ep, :n]) ** 2).double().reshape(-1))
            mean64 = float(torch.cat(sq).mean())
    finally:
        torch.Tensor.cuda = cuda
        hook.remove()
    loss_rel = abs(float(loss) - mean64) / mean64
    assert err <= 1e-5, err
    assert loss_rel <= 1e-5, loss_rel
    vals = t[real.numpy()]
    assert 1 in vals and 100 in vals
    name = f"loss_{tag}.npz"
    extra = dict(n_agents=np.asarray(n_agents, np.int32)) if joint else {}
    np.savez_compressed(os.path.join(HERE, name), ctx_dim=ctx_dim, A=A, T=T, joint=int(joint), wseed=wseed, dseed=dseed, wsum=weights.checksum(),
                        x0=np32(x0), ctx=np32(ctx), t=t.astype(np.int32), e=np32(e), e_theta=np32(e_theta), loss=np.float32(float(loss)),
                        compact_err=err, loss_rel=loss_rel, **extra)
    print(f"wrote {name}: {os.path.getsize(os.path.join(HERE, name)) / 1024:.1f} KB, loss {float(loss):.6f}, masked vs compact {err:.2e}, "
          f"loss vs fp64 mean {loss_rel:.2e}")


def main():
    gen("jmid_w32_e3a3t6", 32, 3, 6, [2, 3, 1], True, 71, 801)            # head_dim 16, S = 18 cut inside the first key tile, a one-agent scene
    gen("jmid_w256_e3a4t12", 256, 4, 12, [4, 1, 3], True, 72, 802)        # head_dim 128: the LDS-DMA kernel, S = 48
    gen("jmid_w256_e2a25t12", 256, 25, 12, [25, 17], True, 73, 803)       # S = 300: three 128-key tiles, a partial mask word inside a tile
    gen("jmid_w32_e2a2t4_full", 32, 2, 4, [2, 2], True, 74, 804)          # no padding, mask branch
    gen("imid_w32_e3a3t6", 32, 3, 6, [3, 3, 3], False, 75, 805)           # TransformerConcatLinear: no mask


if __name__ == "__main__":
    main()
