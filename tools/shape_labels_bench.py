"""Time the Shape Labels kernel (csrc/shape.hip) by HIP events against the Measure Labels kernel (csrc/measure.hip) on the same
device arrays, and against the host statement of the same table: median of --reps calls after two warm-up calls.  The timed
interval of a device call is one accumulate: the kernel plus the 8-byte flag read-back and its stream synchronisation.  Cases: the
volumes of tools/measure_labels_bench.py -- a 256 x 512 x 512 blob-label volume (one ball per 64^3 cell) and a 64 x 512 x 512
salt-and-pepper one (every voxel another label: every pair differs and every vertex has eight labels), each as uint8, uint32 and
int64.  To tell which part of the kernel the time goes to, the uint32 blob shape is also timed all background (the five window
loads and the compares and nothing else: a lane whose windows are all background does nothing), filled with one label (on top of that one run
head per wave, and the lanes at the row ends, which lie on a face of the array and walk their voxels) and per slice (two windows instead of
five, four directions, 2 x 2 vertices).  The kernel reads 13 neighbours where measure reads 3, so it is expected behind measure;
nothing gates on these numbers.  The host statement is numpy -- per direction one shifted compare with two np.bincount of the
differing pairs, per kind of cell the sorted stack of the voxels that touch it -- timed once on a 32 x 256 x 256 crop of each
volume (the stacks of the whole volume do not fit a workstation's memory) and compared per voxel.
Usage: python tools/shape_labels_bench.py [--reps 10] [--quick] [--out profiles/shape_labels_bench.json]   -> one JSON line"""
import argparse
import itertools
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
from empanada_napari_amd._labelplan import shape_directions  # noqa: E402
from empanada_napari_amd._labelstream import GrowableTable  # noqa: E402
from overlap_bench import COPY_TBS, blob_labels  # noqa: E402

FAMILIES = {'shape': ('emp_label_shape', 0), 'shape_per_slice': ('emp_label_shape', 1), 'measure': ('emp_label_measure', 0)}
CROP = (32, 256, 256)


def timed(a, eb, family, reps, capacity):
    """one accumulate of the whole array, table reset before every call"""
    D, H, W = a.shape
    prefix, per_slice = FAMILIES[family]
    t = GrowableTable(prefix, family, capacity, a.device)
    args = (a.data_ptr(), eb, 0, D, H, W, D, None, per_slice, 1)
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
    labels, idx = np.unique(ah, return_inverse=True)
    idx = idx.reshape(ah.shape).astype(np.int64) + (labels[0] != 0)      # 0: the background
    k = len(labels) + 1
    np.bincount(idx.reshape(-1), minlength=k)
    padded = np.pad(idx, 1, constant_values=-1)
    for d in shape_directions(3):
        lo = tuple(slice(1, -1) if v == 0 else (slice(0, -1) if v > 0 else slice(1, None)) for v in d)
        hi = tuple(slice(1, -1) if v == 0 else (slice(1, None) if v > 0 else slice(0, -1)) for v in d)
        p, q = padded[lo], padded[hi]
        differ = p != q
        for side in (p, q):
            np.bincount(side[differ & (side >= 0)], minlength=k)
    m = np.pad(idx, 1)
    for j in range(4):
        for axes in itertools.combinations(range(3), j):
            stack = [m]
            for a in axes:
                stack = stack + [np.roll(s, 1, axis=a) for s in stack]
            s = np.sort(np.stack(stack).reshape(len(stack), -1), axis=0)
            new = np.concatenate([s[:1] != 0, (s[1:] != s[:-1]) & (s[1:] != 0)])
            np.bincount(s[new], minlength=k)
            np.bincount(s[0][(s[0] == s[-1]) & (s[0] != 0)], minlength=k)
    return time.perf_counter() - t0


def case(a, eb, reps, capacity, host):
    out = {'shape': timed(a, eb, 'shape', reps, capacity), 'measure': timed(a, eb, 'measure', reps, capacity)}
    out['shape_ms_over_measure_ms'] = round(out['shape']['ms_median'] / out['measure']['ms_median'], 2)
    if host:
        crop = a[:CROP[0], :CROP[1], :CROP[2]].contiguous()
        s = host_statement(crop.cpu().numpy())
        out['host_statement_s_on_crop'] = round(s, 2)
        per_voxel_device = out['shape']['ms_median'] / 1e3 / a.numel()
        out['host_s_per_voxel_over_shape_s_per_voxel'] = round(s / crop.numel() / per_voxel_device, 1)
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
    out = {'what': 'one accumulate (kernel + flag read-back), HIP events, median of %d after 2 warm-up calls; host statement once on a '
                   '%d x %d x %d crop' % ((args.reps,) + CROP),
           'blobs_256x512x512': {}, 'salt_and_pepper_64x512x512': {}}
    blobs = blob_labels((256, 512, 512), 64, 0)
    for name, a, eb in as_dtypes(blobs):
        out['blobs_256x512x512'][name] = case(a, eb, args.reps, 1 << 16, not args.quick)
        del a
    parts = {'all_background': timed(torch.zeros_like(blobs), 4, 'shape', args.reps, 1 << 16),
             'one_label': timed(torch.full_like(blobs, 5), 4, 'shape', args.reps, 1 << 16),
             'blobs': out['blobs_256x512x512']['u32']['shape'],
             'blobs_per_slice': timed(blobs, 4, 'shape_per_slice', args.reps, 1 << 20)}
    parts['where_the_time_goes'] = ('all_background: loads and compares; one_label - all_background: one run head per wave and the lanes at the row '
                                    'ends (on a face of the array: they walk their voxels); blobs - one_label: the voxels on object surfaces; '
                                    'salt and pepper: LDS and global atomics of every voxel')
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
