"""Another build of the production library (a checkout of the parent commit, say) and this tree's side by side in one process:

    ab_entries.py PATH/TO/OTHER/libjmid_hip.so

Every compute entry of the C ABI with fixed seeds at one cfg2 scene and at the shipped point, f32 and f16mx, host and device mode:
outputs array_equal and equal launch counts per kernel class (jmid_profile_get), else exit status 1.  Then one cfg2 scene through
jmid_predict in f16mx in alternating blocks, two handles of the other build and one of this tree's (docs/NOTEBOOK.md sections 12, 23)."""
import os, sys, time, hashlib
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from safe_interactive_crowdnav_amd.engine import JmidEngine
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims
from tests.test_scene_device_inputs import DT, random_positions
PARENT = os.path.abspath(sys.argv[1])
NEW = os.path.join(REPO, "safe-interactive-crowdnav_amd", "csrc", "libjmid_hip.so")
w = JMIDWeights.from_seed(NetDims(ctx_dim=256), 0)

def host(a):
    return None if a is None else a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
def put(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if dev else a

def run_all(eng, N, K, k, T, precision, dev):
    """every entry of the list, fixed seeds -> (dict name -> arrays, launch counts)"""
    g = torch.Generator().manual_seed(7)
    E, A = 1, N
    x_st = torch.randn([E * A, 6, 6], generator=g).numpy(); nbr = torch.randn([E * A, 2, 6, 6], generator=g).numpy()
    em = torch.rand([E * A, 2], generator=g).numpy(); x_T = torch.randn([E, K * A, T, 2], generator=g).numpy()
    p0 = torch.randn([E, A, 2], generator=g).numpy(); gt = torch.randn([E, A, T, 2], generator=g).numpy()
    fut = (torch.rand([E, A, T], generator=g) < 0.2).numpy()
    out = {}
    eng.profile_reset(); eng.profile_enable()
    ctx = eng.encode(put(x_st, dev), put(nbr, dev), put(em, dev))
    out["encode"] = [ctx]
    vel, pos = eng.denoise(put(x_T, dev), put(host(ctx).reshape(E, A, -1), dev), put(p0, dev), dt=0.25, precision=precision)
    out["denoise"] = [vel, pos]
    out["stats_null"] = [*eng.eval_statistics(None, put(gt, dev), dims=(E, A, K, T)), *eng.collision_statistics(None, dims=(E, A, K, T), pairs=True)]
    if k < K:
        out["topk_null"] = list(eng.topk(None, k, dims=(E, A, K, T)))
        out["topk"] = list(eng.topk(pos, k))
    out["stats"] = list(eng.eval_statistics(pos, put(gt, dev)))
    out["masked"] = list(eng.eval_statistics_masked(pos, put(gt, dev), put(fut, dev), cutoffs=(2, 5)))
    out["collision"] = list(eng.collision_statistics(pos, pairs=True))
    if not dev:
        out["predict"] = list(eng.predict(x_st, nbr, em, x_T, p0, k, dt=0.25, precision=precision))
        hum, rob = random_positions(1, N, 5, half_width=2.0)
        b = eng.build_scene(hum, rob, DT, horizon=T, force_all_in_cluster=True)
        out["scene"] = [b["in_cluster"], b["cv"], *eng.scene_arrays().values()]
        out["forecast"] = list(eng.forecast_scene(x_T, k, dt=0.25, precision=precision))
    prof = {c: n for c, (n, ms) in eng.profile_get().items()}
    eng.profile_disable()
    return out, prof

bad = 0
for tag, (N, K, k, T, step) in {"cfg2": (5, 20, 20, 12, 50), "shipped": (3, 100, 15, 8, 2)}.items():
    engs = {name: JmidEngine(w, joint=True, step=step, lib_path=path) for name, path in (("parent", PARENT), ("new", NEW))}
    for precision in ("f32", "f16mx"):
        for dev in (False, True):
            res = {name: run_all(e, N, K, k, T, precision, dev) for name, e in engs.items()}
            (po, pp), (no, np_) = res["parent"], res["new"]
            diffs = [key for key in po for a, b in zip(po[key], no[key])
                     if not (a is None and b is None) and not np.array_equal(host(a), host(b), equal_nan=True)]
            h = hashlib.sha256(b"".join(np.ascontiguousarray(host(a)).tobytes() for key in sorted(no) for a in no[key] if a is not None)).hexdigest()[:16]
            print(f"AB {tag} {precision} {'device' if dev else 'host'}: {sum(len(v) for v in po.values())} arrays in {len(po)} entries, "
                  f"differing: {diffs or 0}; launches parent {sum(pp.values())} new {sum(np_.values())} per class equal: {pp == np_}; sha {h}", flush=True)
            bad += bool(diffs) + (pp != np_)
    for e in engs.values():
        assert e.erange_count() == 0 and e.timeout_count() == 0
        e.close()
print("AB differences:", bad, flush=True)
if bad:
    raise SystemExit(1)

# ---- speed: one cfg2 scene through jmid_predict, f16mx, alternating blocks
A, K, T = 5, 20, 12
g = torch.Generator().manual_seed(1)
hx = torch.randn([A, 6, 6], generator=g).numpy(); hn = torch.randn([A, 2, 6, 6], generator=g).numpy(); he = torch.rand([A, 2], generator=g).numpy()
hxT = torch.randn([1, K * A, T, 2], generator=g).numpy(); hp0 = torch.randn([1, A, 2], generator=g).numpy()
engs = [("parentA", JmidEngine(w, joint=True, step=50, lib_path=PARENT)), ("new", JmidEngine(w, joint=True, step=50, lib_path=NEW)),
        ("parentB", JmidEngine(w, joint=True, step=50, lib_path=PARENT))]
for _, e in engs:
    for _ in range(10): e.predict(hx, hn, he, hxT, hp0, K, dt=0.25, precision="f16mx")
blocks = {n: [] for n, _ in engs}
for b in range(8):
    for n, e in engs:
        ts = []
        for _ in range(30):
            t = time.perf_counter(); e.predict(hx, hn, he, hxT, hp0, K, dt=0.25, precision="f16mx"); ts.append(time.perf_counter() - t)
        blocks[n].append(1e3 * float(np.median(ts)))
for n, v in blocks.items():
    print(f"PREDICT cfg2 f16mx {n}: median of 8 block medians {np.median(v):.4f} ms, block medians {min(v):.4f} .. {max(v):.4f}", flush=True)
for _, e in engs:
    e.close()
