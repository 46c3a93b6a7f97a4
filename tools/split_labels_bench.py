"""Time Split Labels on the device (csrc/split.hip through labels.split_labels) against its numpy / scipy statement
(tests/split_case.py: scipy's distance transform and maximum filter, the greedy spacing and a heap flood in Python) on the same
machine, and write one JSON object.  One 2-D and one 3-D case of touching blobs (tests/split_case.py ``blobs``), every label picked,
distance mode.  Per case:
  call_ms      host clock around ``split_labels`` on a device tensor, in place, ending in a device synchronise: the label table,
               the launches, the candidates' trip to the host, spacing, marker ids and bookkeeping there, the flood's change flags
               every 8 sweeps -- median, min and max of --reps calls after a warm-up call, each on a fresh copy of the input
  stages_ms    HIP events around each entry of the library in the last call: edt, peaks, flood (its host waits included), write
  turns, boxes, entries (voxels of the boxes), candidates, markers, sweeps
  statement_s  the statement's loop, timed once; equal_to_statement: the two results compared on every voxel
There is no threshold: this file is where the first measurement lives.
Usage: python tools/split_labels_bench.py [--reps 5] [--quick] [--out profiles/split_labels_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import __graft_entry__ as ge  # noqa: E402

ge.load_package()
import split_case as SC  # noqa: E402
from empanada_napari_amd import labels as L  # noqa: E402
from empanada_napari_amd._labelstream import ebytes  # noqa: E402


def device_case(arr, ids, d, reps):
    t0 = torch.from_numpy(arr).cuda()
    eb = ebytes(t0.dtype)
    call, stages, stats, res = [], {}, None, None
    for i in range(reps + 1):      # the first call is the warm-up
        t = t0.clone()
        stages = {}
        torch.cuda.synchronize()
        c0 = time.perf_counter()
        _, stats = L._split_device(t, eb, tuple(arr.shape), points=None, ids=ids, min_distance=d, points_as_markers=False, start_label=None,
                                    device=t.device, stages=stages)
        torch.cuda.synchronize()
        c1 = time.perf_counter()
        if i > 0:
            call.append((c1 - c0) * 1e3)
        res = t
    spread = {'median': round(float(np.median(call)), 3), 'min': round(min(call), 3), 'max': round(max(call), 3)}
    return {'call_ms': spread, 'stages_ms': {k: round(v, 3) for k, v in stages.items()}, **stats}, res.cpu().numpy()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--quick', action='store_true', help='small cases (a rehearsal of the tool, not a measurement)')
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'split_labels_bench needs the MI355X'
    q = args.quick
    cases = {
        'image_768^2_12_blobs_d8': ((128, 128) if q else (768, 768), 4 if q else 12, 3 if q else 8),
        'volume_96x128x128_5_blobs_d5': ((24, 40, 40) if q else (96, 128, 128), 2 if q else 5, 3 if q else 5),
    }
    out = {'reps': args.reps, 'quick': bool(q), 'cases': {}}
    for seed, (name, (shape, n, d)) in enumerate(cases.items()):
        arr = SC.blobs(shape, n, 100 + seed)
        ids = np.unique(arr)[1:]
        rec = {'shape': list(shape), 'labels': int(len(ids)), 'min_distance': d, 'label_voxels': int((arr != 0).sum())}
        dev, got = device_case(arr, ids, d, args.reps)
        t0 = time.perf_counter()
        want, report = SC.split(arr, ids=ids, min_distance=d)
        dev['statement_s'] = round(time.perf_counter() - t0, 4)
        dev['equal_to_statement'] = bool(np.array_equal(got, want))
        dev['labels_split'] = int(sum(not isinstance(r, str) for _, r in report))
        dev['statement_over_call'] = round(dev['statement_s'] * 1e3 / max(dev['call_ms']['median'], 1e-6), 1)
        rec.update(dev)
        out['cases'][name] = rec
    line = json.dumps(out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)
