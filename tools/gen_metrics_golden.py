"""Record the reference's scores on small label pairs: tests/golden/metrics.npz (tests/test_metrics_host.py,
tests/test_gpu_metrics.py).

    python tools/gen_metrics_golden.py /path/to/empanada-napari [out.npz]      # CPU only, a minute or two

The reference checkout (the directory that holds ``empanada/`` and ``empanada_napari/``) is imported, not copied: its
``compute_pixel_metrics`` / ``compute_instance_metrics`` (empanada_napari/_accuracy_metrics.py, loaded by file so that the
plugin's package import stays out of the way; thresholds 0.1 / 0.5 / 0.9) and ``Evaluator.__call__(..., return_instances=True)``
(empanada/evaluation) on JSON run-length files that this script writes from the same volumes with the reference's own
``rle_encode`` / ``rle_to_string``.  cv2, magicgui, napari, numba and skimage are replaced by empty shims (the numba-decorated
functions then run as plain Python).  The file is written with fixed zip timestamps: the same reference gives the same bytes.

Where the reference's evaluator cannot score a side it records that instead of a number:
  * an empty ground truth makes its semantic branch raise (np.concatenate of an empty list, evaluator.py:80): ``sem_raises`` = 1,
    ``iou`` = NaN, the instance / panoptic part is taken from an Evaluator without semantic metrics;
  * fewer than two predicted instances make it score a placeholder run [-1, -1] instead of the prediction (evaluator.py:10-21):
    ``sem_placeholder`` = 1, ``iou`` = whatever it returns.
"""
import functools
import importlib.util
import io
import json
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (0.1, 0.5, 0.9)
INSTANCE_KEYS = ('TP', 'FP', 'FN', 'precision', 'recall', 'f1', 'mean_instance_iou', 'mean_instance_dice')
EVAL_KEYS = ('iou', 'f1_50', 'f1_75', 'precision_50', 'precision_75', 'recall_50', 'recall_75', 'ap_50', 'ap_75', 'pq')
INSTANCE_LISTS = ('gt_matched', 'pred_matched', 'gt_unmatched', 'pred_unmatched', 'matched_ious')


def _shims():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules.setdefault(name, m)
        return sys.modules[name]
    nb = module('numba', jit=lambda *a, **k: (lambda f: f), int64=int)
    nb.types = module('numba.types')
    nb.typed = module('numba.typed', List=list)
    sk = module('skimage')
    sk.measure = module('skimage.measure')
    module('cv2')
    module('magicgui', magicgui=lambda *a, **k: (lambda f: f))
    nap = module('napari')
    nap.layers = module('napari.layers', Image=object, Labels=object)


def _blobs(shape, n, seed, first=1):
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, np.uint16)
    grid = np.indices(shape)
    for i in range(n):
        c = [rng.uniform(0.1, 0.9) * s for s in shape]
        r = [rng.uniform(0.06, 0.14) * s + 1 for s in shape]
        v[sum(((g - ci) / ri) ** 2 for g, ci, ri in zip(grid, c, r)) < 1] = first + i
    return v


def cases():
    """name -> (gt, pred, class_id or None); uint16, labels below 3 000, at most 64 x 128 x 128"""
    gt = _blobs((32, 64, 64), 40, 1, first=1001)
    out = {'identical': (gt, gt.copy(), None), 'shifted': (gt, np.roll(gt, 2, axis=2), None)}
    p = gt.copy()
    ids = np.unique(p[p > 0])
    p[p == ids[0]] = 0                                             # one object deleted
    m = p == ids[1]
    p[m & (np.indices(p.shape)[2] > np.nonzero(m)[2].mean())] = 1900      # one split into two ids
    p[p == ids[3]] = ids[2]                                        # two merged into one
    out['edited'] = (gt, p, None)
    z = np.zeros_like(gt)
    out['both_empty'], out['gt_empty'], out['pred_empty'] = (z, z.copy(), None), (z, gt, None), (gt, z, None)
    two = gt.copy()
    other = _blobs(gt.shape, 12, 5, first=2001)
    two[other > 0] = other[other > 0]
    out['two_classes'] = (two, np.roll(two, 1, axis=1), 1)         # label_divisor 1000: class 1 = 1001.., class 2 = 2001..
    flat = _blobs((128, 128), 14, 7)
    out['flat'] = (flat, np.roll(flat, 3, axis=0), None)
    # equal blocks, the prediction shifted by half a block: every IoU is exactly 1/3, and descending prediction ids
    a = np.zeros((8, 64, 64), np.uint16)
    b = np.zeros_like(a)
    k = 1
    for y in range(0, 64, 16):
        for x in range(0, 64, 8):
            a[:, y:y + 8, x:x + 8] = k
            b[:, y:y + 8, (x + 4) % 64:(x + 4) % 64 + 4] = 100 - k
            b[:, y:y + 8, (x + 8) % 64:(x + 8) % 64 + 4] = 100 - k
            k += 1
    out['ties'] = (a, b, None)
    return out


def _rle_json(vol, class_id, au):
    """the reference's instance file for one class: labels ascending, box with exclusive upper ends, rle of the raveled indices"""
    inst = {}
    flat = vol.ravel()
    for lab in np.unique(flat[flat > 0]):
        idx = np.flatnonzero(flat == lab)
        starts, runs = au.rle_encode(idx)
        coords = np.unravel_index(idx, vol.shape)
        box = [int(c.min()) for c in coords] + [int(c.max()) + 1 for c in coords]
        inst[str(int(lab))] = {'box': box, 'rle': au.rle_to_string(starts, runs)}
    return {'class_id': int(class_id), 'shape': list(vol.shape), 'instances': inst}


def main(ref_root, out_path):
    _shims()
    sys.path.insert(0, ref_root)
    spec = importlib.util.spec_from_file_location('_ref_accuracy_metrics', os.path.join(ref_root, 'empanada_napari', '_accuracy_metrics.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    import empanada.array_utils as au
    from empanada.evaluation import Evaluator, f1_50, f1_75, iou, panoptic_quality, precision_50, precision_75, recall_50, recall_75
    from empanada.evaluation.instance_metrics import ap
    inst_metrics = {'f1_50': f1_50, 'f1_75': f1_75, 'precision_50': precision_50, 'precision_75': precision_75, 'recall_50': recall_50,
                    'recall_75': recall_75, 'ap_50': functools.partial(ap, iou_thr=0.5), 'ap_75': functools.partial(ap, iou_thr=0.75)}
    pan_metrics = {'pq': panoptic_quality}
    arrays = {}
    names = []
    for name, (gt, pred, class_id) in cases().items():
        names.append(name)
        arrays[f'{name}/gt'], arrays[f'{name}/pred'] = gt, pred
        arrays[f'{name}/class_id'] = np.int64(-1 if class_id is None else class_id)
        g64, p64 = gt.astype(np.int64), pred.astype(np.int64)
        with np.errstate(all='ignore'):
            overall, acc, miou, mdice = tool.compute_pixel_metrics(p64, g64)
            arrays[f'{name}/pixel'] = np.array([overall, acc[0], acc[1], miou, mdice], dtype=np.float64)
            for thr in THRESHOLDS:
                m = tool.compute_instance_metrics(g64, p64, iou_threshold=thr)
                arrays[f'{name}/instance_{thr}'] = np.array([m[k] for k in INSTANCE_KEYS], dtype=np.float64)
        # the evaluator scores one class file at a time
        ge, pe = g64, p64
        if class_id is not None:
            lo, hi = class_id * 1000, (class_id + 1) * 1000
            ge, pe = np.where((g64 >= lo) & (g64 < hi), g64, 0), np.where((p64 >= lo) & (p64 < hi), p64, 0)
        with tempfile.TemporaryDirectory() as tmp:
            gp, pp = os.path.join(tmp, 'gt.json'), os.path.join(tmp, 'pred.json')
            json.dump(_rle_json(ge, class_id or 0, au), open(gp, 'w'))
            json.dump(_rle_json(pe, class_id or 0, au), open(pp, 'w'))
            raises = 0
            try:
                res, inst = Evaluator({'iou': iou}, inst_metrics, pan_metrics)(gp, pp, return_instances=True)
            except ValueError:
                raises = 1
                res, inst = Evaluator(None, inst_metrics, pan_metrics)(gp, pp, return_instances=True)
                res['iou'] = np.nan
        arrays[f'{name}/eval'] = np.array([res[k] for k in EVAL_KEYS], dtype=np.float64)
        arrays[f'{name}/sem_raises'] = np.int64(raises)
        arrays[f'{name}/sem_placeholder'] = np.int64(len(np.unique(pe[pe > 0])) < 2)
        for k in INSTANCE_LISTS:
            arrays[f'{name}/{k}'] = np.asarray(inst[k], dtype=np.float64 if k == 'matched_ious' else np.int64)
        print(name, {k: float(res[k]) for k in ('iou', 'f1_50', 'pq')}, 'sem_raises' if raises else '', flush=True)
    arrays['names'] = np.array(names)
    with zipfile.ZipFile(out_path, 'w', zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(out_path, os.path.getsize(out_path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]), sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden', 'metrics.npz'))
