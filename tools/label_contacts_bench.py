"""Time the Contact Labels kernel (csrc/contacts.hip) by HIP events against the Shape Labels kernel (csrc/shape.hip) on the same
device arrays, and against the host statement of the same table: median of --reps calls after two warm-up calls.  The timed interval
of a device call is one accumulate: the kernel plus the 8-byte flag read-back and its stream synchronisation.  Cases: the
256 x 512 x 512 blob-label volume of tools/shape_labels_bench.py (one ball per 64^3 cell) as uint8, uint32 and int64; the same shape
all background (the five window loads and the compares and nothing else) and filled with one label (the same: a lane whose windows
are one value does nothing, whatever the value); and a 64 x 512 x 512 salt-and-pepper volume with labels 1 .. 250 (the same array in
all three types; nearly every pair differs, about 13 credits per voxel to some 31 000 keys, far more than a workgroup's 256 LDS slots
hold).  Contacts are timed without and with the pairs of the background.  Nothing gates on these numbers.  The host statement is
numpy -- per direction one shifted compare, the keys of the differing pairs, np.unique and np.add.at -- timed once on a
32 x 256 x 256 crop of each volume and compared per voxel.
Usage: python tools/label_contacts_bench.py [--reps 10] [--quick] [--out profiles/label_contacts_bench.json]   -> one JSON line"""
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
from empanada_napari_amd._labelplan import shape_directions  # noqa: E402
from empanada_napari_amd._labelstream import GrowableTable  # noqa: E402
from overlap_bench import COPY_TBS, blob_labels  # noqa: E402

# family -> (prefix, what follows (.., total_depth, d_halo) in its accumulate)
FAMILIES = {'contacts': ('emp_label_contacts', (0,)), 'contacts_with_background': ('emp_label_contacts', (1,)),
            'shape': ('emp_label_shape', (0, 1)), 'shape_no_border_faces': ('emp_label_shape', (0, 0))}
CROP = (32, 256, 256)


def timed(a, eb, family, reps, capacity):
    """one accumulate of the whole array, table reset before every call"""
    D, H, W = a.shape
    prefix, tail = FAMILIES[family]
    t = GrowableTable(prefix, family, capacity, a.device)
    args = (a.data_ptr(), eb, 0, D, H, W, D, None) + tail
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


def host_statement(ah, background):
    """the same table on the host, timed once -> (seconds, rows)"""
    t0 = time.perf_counter()
    u = ah.astype(np.uint64)
    keys, cols = [], []
    for k, d in enumerate(shape_directions(3)):
        lo = tuple(slice(max(0, -v), u.shape[a] - max(0, v)) for a, v in enumerate(d))
        hi = tuple(slice(max(0, v), u.shape[a] - max(0, -v)) for a, v in enumerate(d))
        p, q = u[lo], u[hi]
        m = p != q
        if not background:
            m &= (p != 0) & (q != 0)
        p, q = p[m], q[m]
        keys.append((np.minimum(p, q) << np.uint64(32)) | np.maximum(p, q))
        cols.append(np.full(len(p), k, np.int64))
    uniq, inv = np.unique(np.concatenate(keys), return_inverse=True)
    pairs = np.zeros((len(uniq), 13), np.int64)
    np.add.at(pairs, (inv.reshape(-1), np.concatenate(cols)), 1)
    return time.perf_counter() - t0, len(uniq)


def case(a, eb, reps, capacity, host):
    out = {f: timed(a, eb, f, reps, capacity) for f in ('contacts', 'contacts_with_background', 'shape')}
    out['contacts_ms_over_shape_ms'] = round(out['contacts']['ms_median'] / out['shape']['ms_median'], 2)
    if host:
        crop = a[:CROP[0], :CROP[1], :CROP[2]].contiguous()
        s, rows = host_statement(crop.cpu().numpy(), True)
        out['host_statement_s_on_crop'] = round(s, 2)
        out['host_statement_rows_on_crop'] = rows
        per_voxel_device = out['contacts_with_background']['ms_median'] / 1e3 / a.numel()
        out['host_s_per_voxel_over_contacts_s_per_voxel'] = round(s / crop.numel() / per_voxel_device, 1)
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
           'device': torch.cuda.get_device_name(0), 'blobs_256x512x512': {}, 'salt_and_pepper_64x512x512': {}}
    blobs = blob_labels((256, 512, 512), 64, 0)
    for name, a, eb in as_dtypes(blobs):
        out['blobs_256x512x512'][name] = case(a, eb, args.reps, 1 << 16, not args.quick)
        del a
    out['parts_256x512x512_u32'] = {
        'all_background': timed(torch.zeros_like(blobs), 4, 'contacts_with_background', args.reps, 1 << 16),
        'one_label': timed(torch.full_like(blobs, 5), 4, 'contacts_with_background', args.reps, 1 << 16),
        'blobs': out['blobs_256x512x512']['u32']['contacts_with_background'],
        'where_the_time_goes': 'all_background and one_label: loads and compares, no lane has anything to add; blobs - all_background: the voxels '
                               'on object surfaces; salt and pepper: LDS and global atomics of every voxel'}
    del blobs
    g = torch.Generator(device='cuda').manual_seed(2)
    salt = torch.randint(1, 251, (64, 512, 512), device='cuda', generator=g, dtype=torch.int32)
    for name, a, eb in (('u8', salt.to(torch.uint8), 1), ('u32', salt, 4), ('i64', salt.to(torch.int64), -8)):
        out['salt_and_pepper_64x512x512'][name] = case(a, eb, args.reps, 1 << 17, not args.quick)
        del a
    line = json.dumps(out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    print(line)
