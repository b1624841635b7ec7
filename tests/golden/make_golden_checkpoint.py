#!/usr/bin/env python3
"""Generate tests/golden/ckpt_ref_{jmid,imid}_w32.pt.xz + ckpt_ref_{jmid,imid}_w32_eval.npz by RUNNING THE REFERENCE.

What tests/test_checkpoint_export.py reads: a checkpoint written in the reference's own pickled container format
(MID._save_model, sicnav_diffusion/JMID/MID/mid.py:1501-1509: {"encoder": registrar.model_dict - a pickled nn.ModuleDict of
the reference's classes -, "ddpm": model.state_dict()}) of the predictor make_golden.make_forecaster builds (encoder_dim 32,
seeded weights), and one net evaluation of the reference on it.  The tensors the predictor never reads (the encoder modules
other than the four live ones, the never-executed template `layer.*` copy of the net) are zeroed before the save, so that
the file compresses to a few hundred KB; the evaluation is repeated after the zeroing and must not change.

Run where the reference is importable (make_golden.py's import shims):  python tests/golden/make_golden_checkpoint.py
"""
import importlib.util
import lzma
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_golden_tools():
    path = os.path.join(HERE, "make_golden.py")
    argv = sys.argv
    sys.argv = [path]                    # make_golden reads sys.argv[1] as a fixture-name filter at import
    try:
        spec = importlib.util.spec_from_file_location("make_golden_for_checkpoint", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)     # installs the import shims and imports the reference; generates nothing
    finally:
        sys.argv = argv
    return mod


def main():
    import torch
    mg = load_golden_tools()
    from safe_interactive_crowdnav_amd.weights import EDGE_INFL, EDGE_PED, EDGE_ROBOT, NODE_HIST

    for joint in (True, False):
        tag = f"ckpt_ref_{'jmid' if joint else 'imid'}_w32"
        f, weights = mg.make_forecaster(joint, 32, N=3, K=4, k_ret=4, H=8, step=2, wseed=61)
        mid = f.mid_model
        net = mid.model.vel_predictor.net.eval()        # dropout off, as in inference
        g = torch.Generator().manual_seed(1)
        x, ctx = torch.randn([4, 8, 2], generator=g), torch.randn([4, 32], generator=g)
        beta = mid.model.vel_predictor.var_sched.betas[[100] * 4].clone()
        with torch.no_grad():
            e_ref = net([x, ctx], beta=beta)
            live = (NODE_HIST, EDGE_PED, EDGE_ROBOT, EDGE_INFL)
            for name, m in mid.registrar.model_dict.items():
                if name not in live:
                    for t in m.state_dict().values():
                        t.zero_()
            for k, t in mid.model.state_dict().items():
                kk = k[len("vel_predictor.net."):] if k.startswith("vel_predictor.net.") else k
                if kk.startswith("layer.") and kk not in weights.tensors:
                    t.zero_()
            assert torch.equal(net([x, ctx], beta=beta), e_ref)
        ckpt = {"encoder": mid.registrar.model_dict, "ddpm": mid.model.state_dict()}       # MID._save_model, mid.py:1501-1509
        pt = os.path.join(HERE, tag + ".pt.xz")
        tmp = pt[:-3] + ".tmp"
        torch.save(ckpt, tmp)
        with open(tmp, "rb") as src, lzma.open(pt, "wb", preset=9) as dst:
            dst.write(src.read())
        os.unlink(tmp)
        np.savez_compressed(os.path.join(HERE, tag + "_eval.npz"), joint=int(joint), ctx_dim=32, wseed=61, wsum=weights.checksum(),
                            x=x.numpy(), ctx=ctx.numpy(), beta=beta.numpy(), e_ref=e_ref.numpy())
        print(f"wrote {tag}.pt.xz ({os.path.getsize(pt) / 1024:.1f} KB) and {tag}_eval.npz")


if __name__ == "__main__":
    main()
