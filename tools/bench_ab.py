"""Alternated plain bench.py runs of several library builds on one box (the boxes of a pool differ by more than most changes are worth).

    python tools/bench_ab.py ROUNDS OUT.jsonl SPEC [SPEC ...] [-- bench.py arguments]
    SPEC = name[:ENV=VALUE ...]:path of a library relative to the repository | name:product

Every run is its own process under its own time limit, in the order round 0 of every SPEC, round 1 of every SPEC, ...; the first failure ends the
job.  Prints ms_per_step per run and min / max per SPEC; OUT.jsonl gets every run's whole result line."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rounds, out_path = int(sys.argv[1]), sys.argv[2]
rest = sys.argv[3:]
bench_args = []
if '--' in rest:
    k = rest.index('--')
    bench_args, rest = rest[k + 1:], rest[:k]
specs = rest
res = {}
with open(out_path, 'a') as log:
    for r in range(rounds):
        for spec in specs:
            parts = spec.split(':')
            name, lib, envs = parts[0], parts[-1], parts[1:-1]
            env = dict(os.environ)
            for kv in envs:
                k_, v_ = kv.split('=', 1)
                env[k_] = v_
            if lib != 'product':
                env['DPN_LIB'] = os.path.join(ROOT, lib)
            else:
                env.pop('DPN_LIB', None)
            p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + bench_args, env=env, capture_output=True, text=True, timeout=170, cwd=ROOT)
            if p.returncode != 0:
                print('FAILED', spec, p.returncode, p.stdout[-2000:], p.stderr[-3000:])
                sys.exit(p.returncode if p.returncode > 0 else 1)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1]
            d = json.loads(line)
            res.setdefault(name, []).append(d['ms_per_step'])
            log.write(json.dumps({'name': name, 'round': r, 'args': bench_args, 'result': d}) + '\n')
            log.flush()
            print('round %d %-12s %.4f ms  %s' % (r, name, d['ms_per_step'], {k: d[k] for k in ('blocks_finite',) if k in d}), flush=True)
for name, v in res.items():
    print('%-12s min %.4f max %.4f  all %s' % (name, min(v), max(v), ' '.join('%.4f' % x for x in v)))
