"""Time the Measure Labels kernel (csrc/measure.hip) by HIP events against the label table kernel (csrc/labels.hip) on the same
device arrays, and against the host statement of the same table on the same arrays: median of --reps calls after two warm-up
calls.  The timed interval of a device call is one accumulate: the kernel plus the 8-byte flag read-back and its stream
synchronisation.  Cases: a 256 x 512 x 512 blob-label volume (one ball per 64^3 cell) and a 64 x 512 x 512 salt-and-pepper one
(every voxel another label: every run has length 1 and every face is exposed), each as uint8, uint32 and int64.  To tell which
part of the kernel the time goes to, the uint32 blob shape is also timed all background (the loads and the face compares and
nothing else: label 0 is never entered), filled with one label (one run head per wave on top of that) and per slice (no read of
the slice below).  The host statement is numpy: np.bincount for the count and for the nine coordinate sums, and per axis one
shifted compare with two np.bincount of the differing pairs; it is timed once.
Usage: python tools/measure_labels_bench.py [--reps 10] [--quick] [--out profiles/measure_labels_bench.json]   -> one JSON line"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.load_package()
from empanada_napari_amd import _abi  # noqa: E402
from empanada_napari_amd._labelstream import GrowableTable  # noqa: E402
from overlap_bench import COPY_TBS, blob_labels  # noqa: E402

FAMILIES = {'measure': ('emp_label_measure', lambda D: (D, None, 0, 1)), 'measure_per_slice': ('emp_label_measure', lambda D: (D, None, 1, 1)),
            'table': ('emp_label_table', None)}


def timed(a, eb, family, reps, capacity):
    """one accumulate of the whole array, table reset before every call"""
    D, H, W = a.shape
    prefix, tail = FAMILIES[family]
    t = GrowableTable(prefix, family, capacity, a.device)
    args = (a.data_ptr(), eb, 0, D, H, W) + (tail(D) if tail else (0,))
    ms = []
    for i in range(reps + 2):
        t._call('reset', _abi.ptr(t.buf), t.capacity, _abi.stream_ptr(a.device))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t.add(*args)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    nbytes = a.numel() * a.element_size()
    return {'ms_median': round(med, 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4), 'TB_per_s': round(nbytes / med / 1e9, 3),
            'fraction_of_copy_rate': round(nbytes / med / 1e9 / COPY_TBS, 3), 'doublings': t.doublings}


def host_statement(ah):
    """the same table on the host, timed once -> seconds"""
    t0 = time.perf_counter()
    flat = ah.reshape(-1).astype(np.int64)
    k = int(flat.max()) + 1
    np.bincount(flat, minlength=k)
    coords = [np.broadcast_to(np.arange(s, dtype=np.float64).reshape([-1 if i == a else 1 for i in range(3)]), ah.shape).reshape(-1)
              for a, s in enumerate(ah.shape)]
    for a in range(3):
        np.bincount(flat, weights=coords[a], minlength=k)
    for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)):
        np.bincount(flat, weights=coords[a] * coords[b], minlength=k)
    for a in range(3):
        lo = ah[tuple(slice(0, -1) if i == a else slice(None) for i in range(3))]
        hi = ah[tuple(slice(1, None) if i == a else slice(None) for i in range(3))]
        d = lo != hi
        np.bincount(lo[d].astype(np.int64), minlength=k)
        np.bincount(hi[d].astype(np.int64), minlength=k)
    return time.perf_counter() - t0


def case(a, eb, reps, capacity, host):
    out = {'measure': timed(a, eb, 'measure', reps, capacity), 'table': timed(a, eb, 'table', reps, capacity)}
    out['measure_ms_over_table_ms'] = round(out['measure']['ms_median'] / out['table']['ms_median'], 2)
    if host:
        s = host_statement(a.cpu().numpy())
        out['host_statement_s'] = round(s, 2)
        out['host_s_over_measure_s'] = round(s / (out['measure']['ms_median'] / 1e3), 1)
    return out


def as_dtypes(a32):
    """an int32 label tensor as the three element types: uint8 (labels folded into 1..251), uint32 (the same bytes, read
    unsigned) and int64"""
    a8 = torch.where(a32 > 0, a32 % 251 + 1, a32).to(torch.uint8)
    return (('u8', a8, 1), ('u32', a32, 4), ('i64', a32.to(torch.int64), -8))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--quick', action='store_true', help='device cases only (no host statement)')
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    args = ap.parse_args()
    out = {'blobs_256x512x512': {}, 'salt_and_pepper_64x512x512': {}}
    blobs = blob_labels((256, 512, 512), 64, 0)
    for name, a, eb in as_dtypes(blobs):
        out['blobs_256x512x512'][name] = case(a, eb, args.reps, 1 << 16, not args.quick)
        del a
    parts = {'all_background': timed(torch.zeros_like(blobs), 4, 'measure', args.reps, 1 << 16),
             'one_label': timed(torch.full_like(blobs, 5), 4, 'measure', args.reps, 1 << 16),
             'blobs': out['blobs_256x512x512']['u32']['measure'],
             'blobs_per_slice': timed(blobs, 4, 'measure_per_slice', args.reps, 1 << 20)}
    out['parts_256x512x512_u32'] = parts
    del blobs
    g = torch.Generator(device='cuda').manual_seed(2)
    salt = torch.randint(1, 1 << 20, (64, 512, 512), device='cuda', generator=g, dtype=torch.int32)
    for name, a, eb in as_dtypes(salt):
        out['salt_and_pepper_64x512x512'][name] = case(a, eb, args.reps, 1 << 22, not args.quick)
        del a
    line = json.dumps(out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(line)
