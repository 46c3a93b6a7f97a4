"""Time the label contingency kernel (csrc/overlap.hip) by HIP events: median of --reps calls after warm-up, bytes read over
time against the 6.3 TB/s of a float4 copy.  Cases: a 512^3 uint32 blob-label pair (prediction = ground truth rolled by two
voxels), one 16 x 4096^2 slab pair, and the salt-and-pepper worst case (every run of length 1).
--stack3d adds the pair the issue of this kernel names: bench.py's 512^3 stack3d volume through Engine3d x 3 axes + consensus in
precision fp32 against the default precision, uint32 consensus volumes.  The timed interval is one accumulate call: the count
kernel plus the 8-byte flag read-back and its stream synchronisation (the kernel alone: rocprofv3 --kernel-trace --stats).
Diagnostic builds of the library: python tools/with_lib.py <lib.so> tools/overlap_bench.py --quick
Usage: python tools/overlap_bench.py [--reps 10] [--quick] [--stack3d]   -> one JSON line"""
import argparse
import ctypes as C
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
from empanada_napari_amd import _abi, metrics  # noqa: E402
from empanada_napari_amd._labelstream import GrowableTable  # noqa: E402

COPY_TBS = 6.3


def blob_labels(shape, cell, seed):
    """device uint32 labels: one ball per grid cell of ``cell`` voxels, id = cell index + 1"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    idx = [torch.arange(s, device='cuda') for s in shape]
    cid = [(i // cell) for i in idx]
    off = [((i % cell) - cell // 2) for i in idx]
    ncell = [(-(-s // cell)) for s in shape]
    rad = torch.randint(cell // 5, cell // 2, (ncell[0] * ncell[1] * ncell[2],), device='cuda', generator=g)
    c = (cid[0][:, None, None] * ncell[1] + cid[1][None, :, None]) * ncell[2] + cid[2][None, None, :]
    d2 = off[0][:, None, None] ** 2 + off[1][None, :, None] ** 2 + off[2][None, None, :] ** 2
    return torch.where(d2 < rad[c] ** 2, c + 1, torch.zeros_like(c)).to(torch.int32)


def timed(a, b, reps, capacity=None):
    t = GrowableTable('emp_label_overlap', 'label_overlap', capacity or metrics.initial_capacity(a.numel()), a.device)
    n, eb = a.numel(), a.element_size()
    ms = []
    for i in range(reps + 2):
        _abi.check(t.lib.emp_label_overlap_reset(_abi.ptr(t.buf), t.capacity, _abi.stream_ptr(a.device)), 'reset')
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t.add(a.data_ptr(), eb, b.data_ptr(), eb, n)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    keys, _ = t.finalize()
    med = float(np.median(ms))
    return {'ms_median': round(med, 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4), 'distinct_pairs': int(keys.numel()),
            'doublings': t.doublings, 'TB_per_s': round(2 * n * eb / med / 1e9, 3), 'fraction_of_copy_rate': round(2 * n * eb / med / 1e9 / COPY_TBS, 3)}


def stack3d_pair():
    """consensus label volumes (uint32, host) of bench.py's stack3d job in precision fp32 and in the default precision"""
    from empanada_napari_amd import synth, weights
    from empanada_napari_amd.engines import HipPanopticDeepLab
    from empanada_napari_amd.inference import Engine3d, tracker_consensus
    vol = synth.blob_volume(512, 512, 512, seed=0, n_blobs=256, fast=True)
    cfg = dict(weights.MITONET_PDL_CFG)
    P = weights.fold_state_dict(weights.seeded_state_dict(cfg, seed=0), cfg)
    out = []
    for prec in ('fp32', 'fp16x3'):
        model = HipPanopticDeepLab(P, cfg, folded=True, precision=prec)
        mc = {'model': model, 'thing_list': [1], 'labels': [1], 'class_names': {1: 'mito'}, 'padding_factor': 16,
              'norms': {'mean': 0.57571, 'std': 0.12765}}
        e3 = Engine3d(mc, label_divisor=10000, median_kernel_size=3, nms_kernel=3, nms_threshold=0.1, confidence_thr=0.5, min_size=500,
                      min_extent=5)
        trs = {name: e3.infer_on_axis(vol, name)[1] for name in ('xy', 'xz', 'yz')}
        cvol = list(tracker_consensus(trs, None, mc, label_divisor=10000, pixel_vote_thr=2, cluster_iou_thr=0.75, allow_one_view=False,
                                      min_size=500, min_extent=5, dtype=np.uint32, chunk_size=(256, 256, 256)))[0][0]
        out.append(np.ascontiguousarray(np.asarray(cvol), dtype=np.uint32))
        del e3, model
        torch.cuda.empty_cache()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--quick', action='store_true', help='device cases only (no host np.unique)')
    ap.add_argument('--stack3d', action='store_true')
    args = ap.parse_args()
    out = {}
    a = blob_labels((512, 512, 512), 64, 0)
    b = torch.roll(a, 2, 2)
    out['blobs_512^3_u32'] = timed(a, b, args.reps)
    if not args.quick:
        ah, bh = a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)
        t0 = time.perf_counter()
        np.unique(ah.astype(np.uint64) * np.uint64(1 << 32) | bh.astype(np.uint64), return_counts=True)
        out['host_np_unique_512^3_s'] = round(time.perf_counter() - t0, 2)
    del a, b
    a = blob_labels((16, 4096, 4096), 128, 1)
    b = torch.roll(a, 3, 1)
    out['slab_16x4096^2_u32'] = timed(a, b, args.reps)
    del a, b
    g = torch.Generator(device='cuda').manual_seed(2)
    a = torch.randint(0, 1024, (1 << 24,), device='cuda', generator=g, dtype=torch.int32)
    b = torch.randint(0, 1024, (1 << 24,), device='cuda', generator=g, dtype=torch.int32)
    out['salt_and_pepper_2^24_u32'] = timed(a, b, args.reps, capacity=1 << 22)
    del a, b
    if args.stack3d:
        ah, bh = stack3d_pair()
        a, b = torch.from_numpy(ah.view(np.int32)).cuda(), torch.from_numpy(bh.view(np.int32)).cuda()
        out['stack3d_consensus_fp32_vs_default_512^3_u32'] = timed(a, b, args.reps)
        t0 = time.perf_counter()
        keys, cnt = np.unique((ah.astype(np.uint64) * np.uint64(1 << 32) | bh.astype(np.uint64))[(ah > 0) & (bh > 0)], return_counts=True)
        out['stack3d_host_np_unique_foreground_s'] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        np.unique(ah.astype(np.uint64) * np.uint64(1 << 32) | bh.astype(np.uint64), return_counts=True)
        out['stack3d_host_np_unique_all_voxels_s'] = round(time.perf_counter() - t0, 3)
        ev = metrics.evaluate(a.view(torch.uint32), b.view(torch.uint32))
        out['stack3d_objects'] = {'fp32': int(len(ev['gt_matched']) + len(ev['gt_unmatched'])),
                                  'default': int(len(ev['pred_matched']) + len(ev['pred_unmatched'])), 'matched_iou50': int(len(ev['gt_matched'])),
                                  'semantic_iou': float(ev['iou']), 'min_matched_iou': float(ev['matched_ious'].min()) if len(ev['matched_ious']) else None}
    print(json.dumps(out))
