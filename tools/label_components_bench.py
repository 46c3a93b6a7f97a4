"""Time labels.label_components against sparse.ccl26 on one 256 x 512 x 512 blob-label volume (one ball per 64^3 cell, int32):
ccl26 on the whole device volume is the existing code and the yardstick; against it the streamed components with slabs of 32 and
64 slices, from the device tensor and from the same volume as a numpy array (staged through pinned memory and downloaded again).
HIP events around one call each, after one call on a small volume that loads the kernels; the host rows include the host's share
(the copies into the staging buffers and out of the download buffer), which the events span.  The results are compared with
ccl26's, so a row is only written for an identical result.
Usage: python tools/label_components_bench.py [--out profiles/label_components_bench.json]   -> one JSON line"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.load_package()
from empanada_napari_amd import labels as L, sparse  # noqa: E402
from overlap_bench import blob_labels  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = fn()
    e1.record()
    torch.cuda.synchronize()
    return res, e0.elapsed_time(e1)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    args = ap.parse_args()
    small = blob_labels((8, 64, 64), 16, 1)
    sparse.ccl26(small)
    L.label_components(small, slab=4)
    L.label_components(small.cpu().numpy(), slab=4)
    vol = blob_labels((256, 512, 512), 64, 0)
    host = vol.cpu().numpy()
    want, ms_ccl = timed(lambda: sparse.ccl26(vol))
    out = {'volume': '256x512x512 int32, one ball per 64^3 cell', 'components': int(want.max().item()),
           'ccl26_whole_volume_ms': round(ms_ccl, 3), 'label_components': {}}
    for name, src in (('device', vol), ('numpy', host)):
        for slab in (32, 64):
            stats = {}
            (got, count), ms = timed(lambda: L.label_components(src, slab=slab, _stats=stats))
            same = torch.equal(got, want) if name == 'device' else bool(np.array_equal(got, want.cpu().numpy()))
            if not same or count != out['components']:
                raise SystemExit(f'label_components({name}, slab={slab}) differs from ccl26')
            out['label_components'][f'{name}_slab{slab}'] = {'ms': round(ms, 3), 'over_ccl26': round(ms / ms_ccl, 2), 'slabs': stats['slabs'],
                                                             'ccl_runs': stats['ccl_runs'], 'provisional_ids': stats['provisional']}
            del got
    line = json.dumps(out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(line)
