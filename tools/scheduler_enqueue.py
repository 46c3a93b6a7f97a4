"""Host enqueue time of one forward: the wall clock around ``model(x)``, which returns without a synchronise (the synchronise
runs outside the timed span).  One fresh process per run; an A/B build of the library through tools/with_lib.py:

    python tools/scheduler_enqueue.py --tag new >> runs.jsonl
    python tools/with_lib.py <libempanada_hip_parent.so> tools/scheduler_enqueue.py --tag parent >> runs.jsonl
    python tools/scheduler_enqueue.py --merge runs.jsonl --out profiles/scheduler_enqueue.json

--merge: per configuration the medians of every process and the margin -- every "new" median at most the slowest "parent"
median plus the parent's own spread (max - min over its processes)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, network, precision, batch, size): three sizes a user runs
CONFIGS = (('fp16-pdl-b1-1024', 'pdl', 'fp16', 1, 1024),
           ('default-pdl-b1-1024', 'pdl', 'fp16x3', 1, 1024),
           ('default-mini-b1-512', 'mini', 'fp16x3', 1, 512))


def measure(tag, iters, warmup):
    import torch
    import __graft_entry__ as graft
    graft.load_package()
    from empanada_napari_amd import synth, weights
    from empanada_napari_amd.engines import HipPanopticDeepLab
    from empanada_napari_amd.preprocess import normalize
    for name, net, precision, batch, size in CONFIGS:
        cfg = dict(weights.MITONET_PDL_CFG if net == 'pdl' else weights.MITONET_MINI_CFG)
        P = weights.fold_state_dict(weights.seeded_state_dict(cfg, seed=0 if net == 'pdl' else 3), cfg)
        model = HipPanopticDeepLab(P, cfg, folded=True, precision=precision)
        x = torch.from_numpy(normalize(synth.em_tiles(batch, size, seed=5), 0.57571, 0.12765))[:, None].cuda()
        out = tuple(model(x, 2, False).values())      # the heads' buffers, reused: no allocation inside the timed span
        ms = []
        for i in range(warmup + iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model(x, 2, False, out=out)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if i >= warmup:
                ms.append((t1 - t0) * 1e3)
        ms.sort()
        print(json.dumps({'tag': tag, 'config': name, 'iters': iters, 'median_ms': round(statistics.median(ms), 4),
                          'p10_ms': round(ms[len(ms) // 10], 4), 'p90_ms': round(ms[len(ms) * 9 // 10], 4)}), flush=True)
        del model


def merge(path, out):
    runs = [json.loads(line) for line in open(path) if line.startswith('{')]
    doc = {'what': 'host enqueue time of one forward (ms): median over the iterations of each fresh process',
           'iters': runs[0]['iters'], 'configs': {}}
    ok = True
    for name, *_ in CONFIGS:
        med = {tag: [r['median_ms'] for r in runs if r['config'] == name and r['tag'] == tag] for tag in ('parent', 'new')}
        limit = max(med['parent']) + (max(med['parent']) - min(med['parent']))
        within = max(med['new']) <= limit
        ok = ok and within
        doc['configs'][name] = {'parent_medians_ms': med['parent'], 'new_medians_ms': med['new'], 'limit_ms': round(limit, 4),
                                'within_margin': within}
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps(doc['configs'], indent=1))
    return 0 if ok else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--tag', default='new')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--merge')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scheduler_enqueue.json'))
    a = ap.parse_args()
    sys.exit(merge(a.merge, a.out) if a.merge else measure(a.tag, a.iters, a.warmup))
