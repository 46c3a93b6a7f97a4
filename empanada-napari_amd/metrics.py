"""Scoring of label volumes on the device.

``label_overlap`` counts, in one pass over two label arrays, how many voxels carry each pair of labels that occurs (the
sparse contingency table; csrc/overlap.hip).  Everything the reference's two scoring paths report follows from that
table on the host:

* the plugin's *model performance* tool (empanada_napari/_accuracy_metrics.py:10-177): ``compute_pixel_metrics`` and
  ``compute_instance_metrics``, same signatures, same return structures, same edge cases;
* the offline evaluator (empanada/evaluation/evaluator.py:23-122 with instance_metrics.py, panoptic_metrics.py,
  semantic_metrics.py): ``evaluate``.

The reference builds ``np.histogram2d`` over ``(gt.max() + 2) x (pred.max() + 2)`` bins, a dense matrix over label VALUES;
here no matrix over label values exists at any point.  There is no numpy fallback: without the HIP library or a device
``label_overlap`` raises like every other entry of the package.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _abi
from ._labelstream import GrowableTable, hp, initial_capacity, need_device, pick_device, source, stream_slabs

__all__ = ['LabelOverlap', 'label_overlap', 'overlap_from_cells', 'compute_pixel_metrics', 'compute_instance_metrics', 'evaluate',
           'initial_capacity']


@dataclass
class LabelOverlap:
    """The contingency table of two label arrays ``a`` and ``b`` of one shape.

    ``a_labels`` / ``b_labels``: the distinct values of each side, ascending, background 0 included where it occurs
    (``np.unique``), with their voxel counts ``a_areas`` / ``b_areas``.  ``pairs`` (k, 2): the pairs (a, b) that occur,
    sorted by (a, b); ``counts`` (k,): their voxel counts.  ``shape``: the arrays' shape; ``doublings``: how often the
    device table had to grow while counting.  By convention ``a`` is the ground truth and ``b`` the prediction."""
    a_labels: np.ndarray
    a_areas: np.ndarray
    b_labels: np.ndarray
    b_areas: np.ndarray
    pairs: np.ndarray
    counts: np.ndarray
    shape: tuple = ()
    doublings: int = 0


def overlap_from_cells(a, b, counts, shape=(), doublings=0):
    """LabelOverlap from cells (a[i], b[i]) -> counts[i] sorted by (a, b), each pair once."""
    a = np.ascontiguousarray(a, dtype=np.int64)
    b = np.ascontiguousarray(b, dtype=np.int64)
    counts = np.ascontiguousarray(counts, dtype=np.int64)

    def side(v):
        labels, inv = np.unique(v, return_inverse=True)
        areas = np.zeros(len(labels), dtype=np.int64)
        np.add.at(areas, inv.reshape(-1), counts)
        return labels.astype(np.int64), areas
    al, aa = side(a)
    bl, ba = side(b)
    return LabelOverlap(al, aa, bl, ba, np.stack([a, b], axis=1), counts, tuple(shape), doublings)


@torch.no_grad()
def label_overlap(a, b, device=None, slab=None, capacity=None):
    """The contingency table of two label arrays of one shape (2-D or 3-D; any integer dtype of 1, 2, 4 or 8 bytes, values in
    [0, 2^32)): see ``LabelOverlap``.

    ``a``, ``b``: torch tensors on the device (read in place: no copy, no host round trip), numpy arrays, or chunked stores
    (``zstore.DirArray``, zarr arrays), in any combination.  Host data is streamed in slabs of ``slab`` leading-axis slices
    (default: about 64 MiB of the wider side) through pinned staging buffers.  What overlaps: the host-to-device copy of slab
    k + 1 runs on a copy stream under the count of slab k.  What does not: reading slab k + 1 from the store and copying it into
    the pinned buffer happens on the host before the count of slab k is launched, and every count ends in a stream
    synchronisation (it reads the table's overflow / range flags), so a slab costs one host round trip -- for a store whose
    decoding dominates, the decode is the wall time.  The counts are integers: the result does not depend on ``slab`` and is bit-reproducible.  ``capacity``: first size of
    the device table in slots (default ``initial_capacity(n)``); the table doubles when it is too small.  A value outside
    [0, 2^32) raises ``EmpError``."""
    need_device()
    device = pick_device(device, a, b)
    with torch.cuda.device(device):
        sa, sb = source(a, device), source(b, device)
        if sa.shape != sb.shape:
            raise ValueError('The shape of the prediction and ground truth images must match.')
        table = GrowableTable('emp_label_overlap', 'label_overlap', capacity or initial_capacity(sa.rows * sa.row_elems), device)
        for _, z0, z1, (pa, pb) in stream_slabs((sa, sb), slab, device):
            # n voxels at device addresses pa / pb (element sizes negative = signed)
            table.add(pa, sa.ebytes, pb, sb.ebytes, (z1 - z0) * sa.row_elems)
        keys, cnt = table.finalize()      # sorted by key = a << 32 | b
        keys = keys.cpu().numpy().view(np.uint64)
        cnt = cnt.cpu().numpy()
    av = (keys >> np.uint64(32)).astype(np.int64)
    bv = (keys & np.uint64(0xffffffff)).astype(np.int64)
    return overlap_from_cells(av, bv, cnt, sa.shape, table.doublings)


# ----------------------------------------------------------------------------
# host: matching and the scores
# ----------------------------------------------------------------------------
def _match(ov, index_space):
    """emp_overlap_match on the table: non-zero labels and areas of both sides, and the assigned pairs with an overlap
    (rows ascending) as (row index, column index, IoU, intersection)"""
    lib = _abi.load()
    k = len(ov.counts)
    a = np.ascontiguousarray(ov.pairs[:, 0], dtype=np.int64)
    b = np.ascontiguousarray(ov.pairs[:, 1], dtype=np.int64)
    c = np.ascontiguousarray(ov.counts, dtype=np.int64)
    m = max(k, 1)
    al, aa, bl, ba = (np.zeros(m, np.int64) for _ in range(4))
    rows, cols, inter = (np.zeros(m, np.int64) for _ in range(3))
    iou = np.zeros(m, np.float64)
    na, nb, nm = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _abi.check(lib.emp_overlap_match(k, hp(a), hp(b), hp(c), int(index_space), hp(al), hp(aa), C.byref(na), hp(bl), hp(ba),
                                     C.byref(nb), hp(rows), hp(cols), hp(iou), hp(inter), C.byref(nm)), 'emp_overlap_match')
    na, nb, nm = na.value, nb.value, nm.value
    return al[:na], aa[:na], bl[:nb], ba[:nb], rows[:nm], cols[:nm], iou[:nm], inter[:nm]


def _as_overlap(gt, pred, what):
    if isinstance(gt, LabelOverlap):
        if pred is not None:
            raise TypeError(f'{what}: pass either one LabelOverlap or two label arrays')
        return gt
    if gt is None or pred is None:
        raise TypeError(f'{what}: two label arrays (or one LabelOverlap) are needed')
    return label_overlap(gt, pred)


def compute_pixel_metrics(pred, gt=None):
    """_accuracy_metrics.py:10-59: (overall accuracy, {0: acc, 1: acc}, mean IoU, mean Dice) of the binarised volumes.
    ``pred`` may be a ``LabelOverlap`` of (gt, pred) instead (then ``gt`` is omitted)."""
    ov = _as_overlap(pred, None, 'compute_pixel_metrics') if isinstance(pred, LabelOverlap) and gt is None else \
        _as_overlap(gt, pred, 'compute_pixel_metrics')
    g, p, c = ov.pairs[:, 0] > 0, ov.pairs[:, 1] > 0, ov.counts
    # cell[gt binarised][pred binarised]
    cell = [[np.int64(c[~g & ~p].sum()), np.int64(c[~g & p].sum())], [np.int64(c[g & ~p].sum()), np.int64(c[g & p].sum())]]
    n = cell[0][0] + cell[0][1] + cell[1][0] + cell[1][1]
    with np.errstate(invalid='ignore', divide='ignore'):
        overall = np.float64(cell[0][0] + cell[1][1]) / np.float64(n)
    ious, dices, acc = [], [], {}
    for lab in (0, 1):
        inter = cell[lab][lab]
        gt_total = cell[lab][0] + cell[lab][1]
        pred_total = cell[0][lab] + cell[1][lab]
        union = gt_total + pred_total - inter
        ious.append(inter / union if union != 0 else np.nan)
        denom = pred_total + gt_total
        dices.append((2 * inter) / denom if denom != 0 else np.nan)
        acc[lab] = inter / gt_total if gt_total else np.nan
    return overall, acc, np.nanmean(ious), np.nanmean(dices)


def compute_instance_metrics(gt, pred=None, iou_threshold=0.5):
    """_accuracy_metrics.py:74-177: one-to-one matching of the instances by IoU (linear_sum_assignment on -IoU), matches
    below ``iou_threshold`` dropped; TP / FP / FN, precision, recall, F1, mean IoU and mean Dice of the kept matches, with the
    reference's NaN / 0.0 pattern for empty sides.  ``gt`` may be a ``LabelOverlap`` of (gt, pred) instead.

    The assignment runs in the tool's index space (a row / column per integer up to the largest label, as its histogram's
    bins make it) while the labels stay below 2^24, and in the space of the labels that occur beyond: the two can differ only
    in which of several equally good assignments is returned.  ``iou_threshold`` must be positive: a pair without overlap is
    never a match here."""
    if not iou_threshold > 0:
        raise ValueError('compute_instance_metrics: iou_threshold must be > 0')
    ov = _as_overlap(gt, pred, 'compute_instance_metrics')
    ng = int((ov.a_labels != 0).sum())
    npred = int((ov.b_labels != 0).sum())
    nan = np.nan
    if ng == 0 and npred == 0:
        return {'TP': 0, 'FP': 0, 'FN': 0, 'precision': nan, 'recall': nan, 'f1': nan, 'mean_instance_iou': nan, 'mean_instance_dice': nan}
    if ng == 0:
        return {'TP': 0, 'FP': npred, 'FN': 0, 'precision': 0.0, 'recall': nan, 'f1': nan, 'mean_instance_iou': nan, 'mean_instance_dice': nan}
    if npred == 0:
        return {'TP': 0, 'FP': 0, 'FN': ng, 'precision': nan, 'recall': 0.0, 'f1': nan, 'mean_instance_iou': nan, 'mean_instance_dice': nan}
    per_value = max(int(ov.a_labels[-1]), int(ov.b_labels[-1])) < (1 << 24)
    al, aa, bl, ba, rows, cols, iou, inter = _match(ov, 1 if per_value else 0)
    keep = iou >= iou_threshold
    final_iou = iou[keep]
    final_dice = (2.0 * inter[keep].astype(np.float64)) / (aa[rows[keep]] + ba[cols[keep]]).astype(np.float64)
    tp = int(keep.sum())
    fn, fp = ng - tp, npred - tp
    precision = tp / (tp + fp) if (tp + fp) > 0 else nan
    recall = tp / (tp + fn) if (tp + fn) > 0 else nan
    f1 = (2 * precision * recall) / (precision + recall) if (precision + recall) > 0 else nan
    return {'TP': tp, 'FP': fp, 'FN': fn, 'precision': precision, 'recall': recall, 'f1': f1,
            'mean_instance_iou': np.mean(final_iou) if tp > 0 else nan, 'mean_instance_dice': np.mean(final_dice) if tp > 0 else nan}


def _restrict(ov, lo, hi):
    """the table of the two volumes with every label outside [lo, hi) set to background"""
    a = np.where((ov.pairs[:, 0] >= lo) & (ov.pairs[:, 0] < hi), ov.pairs[:, 0], 0)
    b = np.where((ov.pairs[:, 1] >= lo) & (ov.pairs[:, 1] < hi), ov.pairs[:, 1], 0)
    key = (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)
    uk, inv = np.unique(key, return_inverse=True)
    cnt = np.zeros(len(uk), dtype=np.int64)
    np.add.at(cnt, inv.reshape(-1), ov.counts)
    return overlap_from_cells((uk >> np.uint64(32)).astype(np.int64), (uk & np.uint64(0xffffffff)).astype(np.int64), cnt, ov.shape, ov.doublings)


def _detection_scores(n_tp, n_failed, n_gt_un, n_pred_un):
    """(f1, ap, precision, recall) at one threshold from the counts instance_metrics.py:3-206 derives them from; 1 by
    convention where nothing is there to detect"""
    fn, fp = n_gt_un + n_failed, n_pred_un + n_failed
    f1 = 1 if n_tp + fp + fn == 0 else n_tp / (n_tp + 0.5 * fp + 0.5 * fn)
    ap = 1 if n_tp + fp + fn == 0 else n_tp / (n_tp + fp + fn)
    precision = 1 if n_tp + fp == 0 else n_tp / (n_tp + fp)
    recall = 1 if n_tp + fn == 0 else n_tp / (n_tp + fn)
    return f1, ap, precision, recall


def evaluate(gt, pred=None, iou_thr=0.5, class_id=None, label_divisor=None):
    """The quantities of the reference's Evaluator (evaluation/evaluator.py:59-122) for one class: semantic ``iou``
    (semantic_metrics.py: 1 if both sides are empty, 0 if one is), ``f1_50, f1_75, precision_50, precision_75, recall_50,
    recall_75, ap_50, ap_75`` (instance_metrics.py), ``pq`` (panoptic_metrics.py), and ``gt_matched, pred_matched, gt_unmatched,
    pred_unmatched, matched_ious`` as ``return_instances=True`` gives them.  Instances are matched one to one on the IoU matrix of
    the labels that occur (matcher.py:194-224), matches below ``iou_thr`` dropped.  ``class_id`` with ``label_divisor``
    restricts both volumes to the labels of [class_id * divisor, (class_id + 1) * divisor), as the reference scores one class
    file at a time.  ``gt`` may be a ``LabelOverlap`` of (gt, pred) instead."""
    ov = _as_overlap(gt, pred, 'evaluate')
    if (class_id is None) != (label_divisor is None):
        raise ValueError('evaluate: class_id and label_divisor go together')
    if class_id is not None:
        ov = _restrict(ov, int(class_id) * int(label_divisor), (int(class_id) + 1) * int(label_divisor))
    g, p = ov.pairs[:, 0] > 0, ov.pairs[:, 1] > 0
    n_g, n_p, n_gp = int(ov.counts[g].sum()), int(ov.counts[p].sum()), int(ov.counts[g & p].sum())
    if n_g == 0 and n_p == 0:
        sem = 1
    elif n_g == 0 or n_p == 0:
        sem = 0
    else:
        sem = n_gp / (n_g + n_p - n_gp)
    al, aa, bl, ba, rows, cols, iou, inter = _match(ov, 0)
    keep = iou >= iou_thr if iou_thr is not None else np.ones(len(iou), bool)
    gt_matched, pred_matched, matched_ious = al[rows[keep]], bl[cols[keep]], iou[keep]
    gt_unmatched, pred_unmatched = np.setdiff1d(al, gt_matched), np.setdiff1d(bl, pred_matched)
    out = {'iou': sem}
    for name, thr in (('50', 0.5), ('75', 0.75)):
        tp = int(np.count_nonzero(matched_ious >= thr))
        failed = int(np.count_nonzero(matched_ious < thr))
        f1, ap, precision, recall = _detection_scores(tp, failed, len(gt_unmatched), len(pred_unmatched))
        out.update({f'f1_{name}': f1, f'ap_{name}': ap, f'precision_{name}': precision, f'recall_{name}': recall})
    tp_ious = matched_ious[matched_ious >= 0.5]
    tp, failed = len(tp_ious), int(np.count_nonzero(matched_ious < 0.5))
    fn, fp = len(gt_unmatched) + failed, len(pred_unmatched) + failed
    out['pq'] = 1 if tp + fp + fn == 0 else (tp_ious.sum() / (tp + 1e-5)) * (tp / (tp + 0.5 * fp + 0.5 * fn))
    out.update({'gt_matched': gt_matched, 'pred_matched': pred_matched, 'gt_unmatched': gt_unmatched, 'pred_unmatched': pred_unmatched,
                'matched_ious': matched_ious})
    return out
