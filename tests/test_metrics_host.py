"""Host side of the scoring module (empanada_napari_amd/metrics.py, emp_overlap_match in csrc/overlap.hip), no GPU needed: the
cells are computed here with np.unique, as the device kernel's contract states them.

* the score functions reproduce the outputs RECORDED FROM THE IMPORTED REFERENCE (tools/gen_metrics_golden.py ->
  tests/golden/metrics.npz: compute_pixel_metrics, compute_instance_metrics at 0.1 / 0.5 / 0.9 and
  Evaluator.__call__(..., return_instances=True) on run-length JSON files) on the golden inputs: identical volumes, a prediction
  shifted by two voxels, one object deleted / one split / two merged, both sides empty, either side empty, two classes with
  label_divisor 1000, a 2-D pair, and equal blocks with exactly tied IoUs.  Integers and label arrays exactly; IoU, dice,
  precision, recall, F1, AP, PQ, accuracies bit for bit (the same float64 operations); the two np.mean results of
  compute_instance_metrics within 4 ulp, because the order of summation may differ;
* the semantic IoU of the evaluator is compared bit for bit wherever the reference's evaluator scores the prediction.  It
  cannot in two situations, which the golden file flags: an empty ground truth makes it raise (np.concatenate of an empty
  list, evaluator.py:80; sem_raises), and fewer than two predicted instances make it score a placeholder run [-1, -1]
  instead of the prediction (evaluator.py:10-21; sem_placeholder).  There evaluate() follows the conventions of
  semantic_metrics.py:21-24 (1 if both sides are empty, 0 if one is), asserted as such;
* property test: the matching equals scipy.optimize.linear_sum_assignment on the dense IoU matrix, in both index spaces (the
  labels that occur: the evaluator's matrix; every integer up to the largest label: the performance tool's), on 200 seeded
  random sparse tables per space, tie-heavy ones included."""
import os

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from empanada_napari_amd import metrics


def _cells(a, b):
    key = (a.astype(np.uint64).ravel() << np.uint64(32)) | b.astype(np.uint64).ravel()
    uk, cnt = np.unique(key, return_counts=True)
    return metrics.overlap_from_cells((uk >> np.uint64(32)).astype(np.int64), (uk & np.uint64(0xffffffff)).astype(np.int64), cnt, a.shape)


def _dense_iou(ov, per_value):
    """dense IoU (and intersection) matrix of the non-zero labels; per_value: a row / column per integer 1..max"""
    al, bl = ov.a_labels[ov.a_labels > 0], ov.b_labels[ov.b_labels > 0]
    aa, ba = ov.a_areas[ov.a_labels > 0], ov.b_areas[ov.b_labels > 0]
    if per_value:
        nr, nc = int(al[-1]), int(bl[-1])
        ri, ci = {int(v): int(v) - 1 for v in al}, {int(v): int(v) - 1 for v in bl}
        ga, pa = np.zeros(nr, np.int64), np.zeros(nc, np.int64)
        ga[al - 1], pa[bl - 1] = aa, ba
    else:
        nr, nc = len(al), len(bl)
        ri, ci = {int(v): i for i, v in enumerate(al)}, {int(v): i for i, v in enumerate(bl)}
        ga, pa = aa, ba
    inter = np.zeros((nr, nc))
    for (x, y), c in zip(ov.pairs, ov.counts):
        if x > 0 and y > 0:
            inter[ri[int(x)], ci[int(y)]] = c
    union = ga[:, None] + pa[None, :] - inter
    with np.errstate(invalid='ignore', divide='ignore'):
        iou = np.where(union > 0, inter / union, 0)
    return iou, inter, ga, pa


def _random_table(rng, ties):
    G, P = int(rng.integers(1, 25)), int(rng.integers(1, 25))
    gl = np.sort(rng.choice(np.arange(1, 60), G, replace=False))
    pl = np.sort(rng.choice(np.arange(1, 60), P, replace=False))
    cells = {}
    for g in gl:
        for p in pl:
            if rng.random() < 0.15:
                cells[(int(g), int(p))] = int(rng.choice([4, 8, 8, 16])) if ties else int(rng.integers(1, 400))
    for g in gl:
        cells[(int(g), 0)] = int(rng.choice([0, 8, 16])) if ties else int(rng.integers(0, 300))
    for p in pl:
        cells[(0, int(p))] = int(rng.choice([0, 8, 16])) if ties else int(rng.integers(0, 300))
    # every label must occur
    for g in gl:
        if not any(k[0] == g and v > 0 for k, v in cells.items()):
            cells[(int(g), 0)] = 8
    for p in pl:
        if not any(k[1] == p and v > 0 for k, v in cells.items()):
            cells[(0, int(p))] = 8
    cells[(0, 0)] = 1000
    keys = sorted(k for k, v in cells.items() if v > 0)
    return metrics.overlap_from_cells([k[0] for k in keys], [k[1] for k in keys], [cells[k] for k in keys])


@pytest.mark.parametrize('per_value', [0, 1])
def test_match_equals_scipy_on_the_dense_matrix(per_value):
    rng = np.random.default_rng(11 + per_value)
    nonempty = 0
    for it in range(200):
        ov = _random_table(rng, ties=it % 2 == 0)
        al, aa, bl, ba, rows, cols, iou, inter = metrics._match(ov, per_value)
        dense, dinter, _, _ = _dense_iou(ov, per_value)
        r, c = linear_sum_assignment(dense, maximize=True)
        keep = dense[r, c] > 0
        if per_value:
            want = [(int(x) + 1, int(y) + 1) for x, y in zip(r[keep], c[keep])]
        else:
            want = [(int(al[x]), int(bl[y])) for x, y in zip(r[keep], c[keep])]
        got = [(int(al[x]), int(bl[y])) for x, y in zip(rows, cols)]
        assert got == want, (it, got, want)
        assert np.array_equal(iou, dense[r, c][keep])          # bit for bit: the same float64 operations
        assert np.array_equal(inter, dinter[r, c][keep].astype(np.int64))
        assert np.array_equal(al, ov.a_labels[ov.a_labels > 0]) and np.array_equal(aa, ov.a_areas[ov.a_labels > 0])
        assert np.array_equal(bl, ov.b_labels[ov.b_labels > 0]) and np.array_equal(ba, ov.b_areas[ov.b_labels > 0])
        nonempty += len(got) > 0
    assert nonempty > 150


# ---- the reference's recorded outputs ------------------------------------------------------------------------------------
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'metrics.npz'))
NAMES = [str(n) for n in GOLD['names']]
THRESHOLDS = (0.1, 0.5, 0.9)
INSTANCE_KEYS = ('TP', 'FP', 'FN', 'precision', 'recall', 'f1', 'mean_instance_iou', 'mean_instance_dice')
EVAL_KEYS = ('iou', 'f1_50', 'f1_75', 'precision_50', 'precision_75', 'recall_50', 'recall_75', 'ap_50', 'ap_75', 'pq')
INSTANCE_LISTS = ('gt_matched', 'pred_matched', 'gt_unmatched', 'pred_unmatched', 'matched_ious')


def same_bits(got, want):
    """equal as float64 bit patterns (NaN equals NaN)"""
    return np.array_equal(np.asarray(got, np.float64).view(np.uint64), np.asarray(want, np.float64).view(np.uint64)) or \
        (np.isnan(got) and np.isnan(want))


def ulps(a, b):
    return abs(float(a) - float(b)) / np.spacing(abs(float(b)))


def check_pixel(name, got):
    overall, acc, miou, mdice = got
    want = GOLD[f'{name}/pixel']
    for g, w, what in zip((overall, acc[0], acc[1], miou, mdice), want, ('overall', 'acc0', 'acc1', 'mean_iou', 'mean_dice')):
        assert same_bits(g, w), (name, what, g, w)
    assert list(acc) == [0, 1]


def check_instance(name, thr, got):
    want = dict(zip(INSTANCE_KEYS, GOLD[f'{name}/instance_{thr}']))
    assert list(got) == list(INSTANCE_KEYS)
    for k in ('TP', 'FP', 'FN'):
        assert got[k] == int(want[k]), (name, thr, k, got[k], want[k])
    for k in ('precision', 'recall', 'f1'):
        assert same_bits(got[k], want[k]), (name, thr, k, got[k], want[k])
    for k in ('mean_instance_iou', 'mean_instance_dice'):      # np.mean: the order of summation may differ
        assert (np.isnan(got[k]) and np.isnan(want[k])) or ulps(got[k], want[k]) <= 4, (name, thr, k, got[k], want[k])


def check_evaluate(name, got):
    want = dict(zip(EVAL_KEYS, GOLD[f'{name}/eval']))
    for k in EVAL_KEYS[1:]:
        assert same_bits(got[k], want[k]), (name, k, got[k], want[k])
    for k in INSTANCE_LISTS:
        w = GOLD[f'{name}/{k}']
        assert len(got[k]) == len(w) and (same_bits(got[k], w) if k == 'matched_ious' else np.array_equal(got[k], w)), (name, k)
    gt, pred = GOLD[f'{name}/gt'], GOLD[f'{name}/pred']
    cid = int(GOLD[f'{name}/class_id'])
    if cid >= 0:
        gt, pred = np.where(gt // 1000 == cid, gt, 0), np.where(pred // 1000 == cid, pred, 0)
    if int(GOLD[f'{name}/sem_raises']) or int(GOLD[f'{name}/sem_placeholder']):
        # the reference's evaluator does not score this prediction (module docstring): semantic_metrics.py:21-24's conventions
        empty_g, empty_p = not (gt > 0).any(), not (pred > 0).any()
        assert empty_g or empty_p, name      # none of the golden cases has exactly one predicted instance
        assert got['iou'] == (1 if empty_g and empty_p else 0), (name, got['iou'], want['iou'])
    else:
        assert same_bits(got['iou'], want['iou']), (name, got['iou'], want['iou'])


def eval_kwargs(name):
    cid = int(GOLD[f'{name}/class_id'])
    return dict(class_id=cid, label_divisor=1000) if cid >= 0 else {}


def test_golden_cases_are_the_ones_the_scores_are_pinned_on():
    assert NAMES == ['identical', 'shifted', 'edited', 'both_empty', 'gt_empty', 'pred_empty', 'two_classes', 'flat', 'ties']
    assert GOLD['flat/gt'].ndim == 2 and GOLD['two_classes/gt'].max() > 2000 and int(GOLD['two_classes/class_id']) == 1
    assert all(GOLD[f'{n}/gt'].dtype == np.uint16 and GOLD[f'{n}/gt'].max() < 3000 for n in NAMES)
    assert np.all(GOLD['ties/matched_ious'] < 0.5) and len(GOLD['ties/gt_unmatched']) == 32      # every IoU is 1/3


@pytest.mark.parametrize('name', NAMES)
def test_pixel_metrics_reproduce_the_reference(name):
    check_pixel(name, metrics.compute_pixel_metrics(_cells(GOLD[f'{name}/gt'], GOLD[f'{name}/pred'])))


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('thr', THRESHOLDS)
def test_instance_metrics_reproduce_the_reference(name, thr):
    check_instance(name, thr, metrics.compute_instance_metrics(_cells(GOLD[f'{name}/gt'], GOLD[f'{name}/pred']), iou_threshold=thr))


@pytest.mark.parametrize('name', NAMES)
def test_evaluate_reproduces_the_reference(name):
    check_evaluate(name, metrics.evaluate(_cells(GOLD[f'{name}/gt'], GOLD[f'{name}/pred']), **eval_kwargs(name)))


def test_tie_case_in_both_index_spaces():
    """the tool's matrix has empty rows / columns for absent label values, the evaluator's has none.  On the tie golden (every
    IoU exactly 1/3, two candidates per object) the reference's tool output at 0.1 is reproduced by the per-value space
    (test above); here: which matches each space keeps, compared"""
    ov = _cells(GOLD['ties/gt'], GOLD['ties/pred'])
    m0, m1 = metrics._match(ov, 0), metrics._match(ov, 1)
    assert np.all(m0[6] == 256 / 768) and np.all(m1[6] == 256 / 768)
    assert len(m0[4]) == len(m1[4]) == int(GOLD['ties/instance_0.1'][0])
    same = np.array_equal(m0[4], m1[4]) and np.array_equal(m0[5], m1[5])
    print('tie golden: compact and per-value index spaces keep', 'the same' if same else 'different', 'matches')


def test_argument_errors():
    ov = _cells(GOLD['identical/gt'], GOLD['identical/pred'])
    with pytest.raises(ValueError):
        metrics.compute_instance_metrics(ov, iou_threshold=0.0)
    with pytest.raises(TypeError):
        metrics.evaluate(ov, GOLD['identical/pred'])


def test_score_volumes_tool_helpers(tmp_path):
    """tools/score_volumes.py without a device: argument rule, the .npy / store openers, and the JSON form of a result with NaNs"""
    import importlib.util
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, 'tools', 'score_volumes.py')
    spec = importlib.util.spec_from_file_location('_score_volumes', tool)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ov = _cells(GOLD['gt_empty/gt'], GOLD['gt_empty/pred'])
    out = mod._plain({'instance': metrics.compute_instance_metrics(ov), 'pixel': metrics.compute_pixel_metrics(ov)[1],
                      'evaluation': metrics.evaluate(ov)})
    back = json.loads(json.dumps(out))
    assert back['instance']['recall'] is None and back['instance']['precision'] == 0.0 and back['pixel'] == {'0': out['pixel']['0'], '1': None}
    assert back['evaluation']['gt_matched'] == [] and len(back['evaluation']['pred_unmatched']) == back['instance']['FP']
    np.save(tmp_path / 'a.npy', GOLD['flat/gt'])
    assert np.array_equal(mod._open(str(tmp_path / 'a.npy')), GOLD['flat/gt'])
    r = subprocess.run([sys.executable, tool, 'a.npy', 'b.npy', '--divisor', '1000'], capture_output=True, text=True)
    assert r.returncode == 2 and 'go together' in r.stderr
