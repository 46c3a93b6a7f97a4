"""Time the label table kernel and the edit kernel (csrc/labels.hip) by HIP events: median of --reps calls after warm-up, bytes
moved over time against the 6.3 TB/s of a float4 copy (the table reads the array once; the edit reads and writes it).  Cases, as
tools/overlap_bench.py: a 512^3 uint32 blob-label volume, one 16 x 4096^2 slab, and the salt-and-pepper worst case (every run of
length 1).  In the same process and on the same tensors it times label_overlap(x, x) -- the contingency kernel of
csrc/overlap.hip, which reads two arrays where the table reads one -- as the comparator.  The timed interval of a table call is
one accumulate: the kernel plus the 8-byte flag read-back and its stream synchronisation (the kernel alone: rocprofv3
--kernel-trace --stats).  The edit is timed as the small-label filter's map (the smaller half of the labels -> 0) out of place.
Without --quick the 512^3 case is also done once on the host the way the reference does it: np.unique + scipy.ndimage.find_objects +
one `labels == l` pass per removed label (at most --host-labels of them are timed, the rest extrapolated).
Usage: python tools/label_table_bench.py [--reps 10] [--quick] [--out profiles/labels_bench.json]   -> one JSON line"""
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
from empanada_napari_amd import _abi, labels as L, metrics  # noqa: E402
from empanada_napari_amd._labelstream import GrowableTable  # noqa: E402
from overlap_bench import COPY_TBS, blob_labels, timed as overlap_timed  # noqa: E402


def _rate(nbytes, ms):
    med = float(np.median(ms))
    return {'ms_median': round(med, 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4), 'TB_per_s': round(nbytes / med / 1e9, 3),
            'fraction_of_copy_rate': round(nbytes / med / 1e9 / COPY_TBS, 3)}


def table_timed(a, reps, per_slice=False, capacity=None):
    D, H, W = a.shape
    t = GrowableTable('emp_label_table', 'label_table', capacity or metrics.initial_capacity(a.numel()), a.device)
    ms = []
    for i in range(reps + 2):
        _abi.check(t.lib.emp_label_table_reset(_abi.ptr(t.buf), t.capacity, _abi.stream_ptr(a.device)), 'reset')
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t.add(a.data_ptr(), a.element_size(), 0, D, H, W, int(per_slice))
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    keys, cnt, _ = (x.cpu().numpy() for x in t.finalize(extra=[(6, torch.int32)]))
    out = _rate(a.numel() * a.element_size(), ms)
    out.update({'distinct_keys': int(len(keys)), 'doublings': t.doublings})
    return out, keys, cnt


def edit_timed(a, keys, cnt, reps):
    """the map of the small-label filter at the median area (background excluded), out of place"""
    D, H, W = a.shape
    fg = keys != 0
    ids = keys[fg][cnt[fg] <= np.median(cnt[fg])] if fg.any() else keys[:0]
    m = L._Map(ids.astype(np.uint64), np.zeros(len(ids), np.uint64), a.device)
    out = torch.empty_like(a)
    ms = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.apply(a.data_ptr(), a.element_size(), a.data_ptr(), a.element_size(), out.data_ptr(), 0, D, H, W, False, a.device)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    res = _rate(2 * a.numel() * a.element_size(), ms)
    res['map_entries'] = int(len(ids))
    return res, ids


def case(a, reps, capacity=None, overlap_capacity=None):
    tab, keys, cnt = table_timed(a, reps, capacity=capacity)
    edit, ids = edit_timed(a, keys, cnt, reps)
    ov = overlap_timed(a, a, reps, capacity=overlap_capacity)
    return {'table': tab, 'table_per_slice': table_timed(a, reps, per_slice=True, capacity=capacity)[0], 'edit': edit,
            'label_overlap_x_x': ov, 'table_bytes_per_s_over_overlap': round(tab['TB_per_s'] / ov['TB_per_s'], 3)}, ids


def host_reference(ah, ids, max_labels):
    """the reference's route on the host, timed once: np.unique, find_objects, and `labels == l` passes"""
    from scipy import ndimage
    out = {}
    t0 = time.perf_counter()
    np.unique(ah, return_counts=True)
    out['np_unique_s'] = round(time.perf_counter() - t0, 2)
    t0 = time.perf_counter()
    ndimage.find_objects(ah.astype(np.int32))
    out['find_objects_s'] = round(time.perf_counter() - t0, 2)
    work = ah.copy()
    k = min(max_labels, len(ids))
    t0 = time.perf_counter()
    for l in ids[:k]:
        work[work == l] = 0
    dt = time.perf_counter() - t0
    out.update({'removed_labels': int(len(ids)), 'passes_timed': int(k), 'label_passes_s': round(dt, 2),
                'label_passes_extrapolated_s': round(dt / max(k, 1) * len(ids), 1)})
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--quick', action='store_true', help='device cases only (no host reference)')
    ap.add_argument('--host-labels', type=int, default=8)
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    args = ap.parse_args()
    out = {}
    a = blob_labels((512, 512, 512), 64, 0)
    out['blobs_512^3_u32'], ids = case(a, args.reps)
    if not args.quick:
        out['host_reference_512^3'] = host_reference(a.cpu().numpy().view(np.uint32), ids, args.host_labels)
    del a
    a = blob_labels((16, 4096, 4096), 128, 1)
    out['slab_16x4096^2_u32'], _ = case(a, args.reps)
    del a
    g = torch.Generator(device='cuda').manual_seed(2)
    a = torch.randint(1, 1 << 20, (64, 512, 512), device='cuda', generator=g, dtype=torch.int32)
    out['salt_and_pepper_2^24_u32'], _ = case(a, args.reps, capacity=1 << 22, overlap_capacity=1 << 22)
    del a
    line = json.dumps(out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(line)
