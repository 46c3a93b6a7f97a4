"""Score two label volumes on the device and print one JSON object: the model-performance tool's pixel and instance metrics
and the evaluator's quantities, from one pass over the volumes.
Usage: python tools/score_volumes.py GT PRED [--divisor N --class-id C] [--iou-threshold T]   (--divisor and --class-id go together)
GT / PRED: .npy files (memory-mapped and streamed in slabs) or zarr array directories."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.load_package()
from empanada_napari_amd import metrics, zstore  # noqa: E402


def _open(path):
    return np.load(path, mmap_mode='r') if path.endswith('.npy') else zstore.DirArray(path)


def _plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (np.floating, float)):
        return None if np.isnan(v) else float(v)
    return int(v) if isinstance(v, np.integer) else v


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('gt')
    ap.add_argument('pred')
    ap.add_argument('--divisor', type=int, default=None)
    ap.add_argument('--class-id', type=int, default=None)
    ap.add_argument('--iou-threshold', type=float, default=0.5)
    args = ap.parse_args()
    if (args.divisor is None) != (args.class_id is None):
        ap.error('--divisor and --class-id go together')
    ov = metrics.label_overlap(_open(args.gt), _open(args.pred))
    overall, per_label, miou, mdice = metrics.compute_pixel_metrics(ov)
    kw = dict(class_id=args.class_id, label_divisor=args.divisor) if args.divisor else {}
    out = {'shape': list(ov.shape), 'distinct_pairs': len(ov.counts),
           'pixel': {'overall_accuracy': overall, 'per_label_accuracy': per_label, 'mean_iou': miou, 'mean_dice': mdice},
           'instance': metrics.compute_instance_metrics(ov, iou_threshold=args.iou_threshold),
           'evaluation': metrics.evaluate(ov, **kw)}
    print(json.dumps(_plain(out)))
