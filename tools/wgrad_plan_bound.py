"""The element-wise difference, relative to the tensor's maximum, between two range plans of ONE build (DPN_LIB: a -DDPN_EXPERIMENT_SPLITS library) at n = 5197:
what a change of the summation order alone does to the gradients.  usage: DPN_LIB=<-DDPN_EXPERIMENT_SPLITS build> python tools/wgrad_plan_bound.py 0,13,14,15 0,15,13,14"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location('wgrad_digest', os.path.join(ROOT, 'tools', 'wgrad_digest.py'))
D = importlib.util.module_from_spec(spec)
spec.loader.exec_module(D)

for prec in D.PRECS:
    runs = []
    for plan in sys.argv[1:3]:
        os.environ['DPN_WGRAD_PLAN'] = plan
        runs.append({k: v.clone() for k, v in D.run_case('raw', 5197, prec).items()})
    worst = (0.0, None)
    same = 0
    for k in runs[0]:
        if k == 'operands':
            continue
        a, b = runs[0][k].double(), runs[1][k].double()
        mx = float(a.abs().max())
        rel = float((a - b).abs().max()) / mx if mx > 0 else 0.0
        same += int(rel == 0.0)
        worst = max(worst, (rel, k))
    a, b = runs[0]['g_heads'].double(), runs[1]['g_heads'].double()
    s = slice(None, None, D.STRIDE)
    print('%s plans %s vs %s: worst tensor %s rel-to-max %.3e; g_heads %.3e, its strided sample %.3e; %d of %d tensors identical' % (
        prec, sys.argv[1], sys.argv[2], worst[1], worst[0], float((a - b).abs().max() / a.abs().max()),
        float((a.reshape(-1)[s] - b.reshape(-1)[s]).abs().max() / a.abs().max()), same, len(runs[0]) - 1), flush=True)
