"""Device side of the scoring module: the sparse label contingency kernel (csrc/overlap.hip) through
empanada_napari_amd.metrics.label_overlap.  The statement of the table is numpy's:
np.unique(a.astype(u64) << 32 | b, return_counts=True); counts are integers, so every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _want(a, b):
    key = (a.astype(np.int64).astype(np.uint64).ravel() << np.uint64(32)) | b.astype(np.int64).astype(np.uint64).ravel()
    uk, cnt = np.unique(key, return_counts=True)
    return np.stack([(uk >> np.uint64(32)).astype(np.int64), (uk & np.uint64(0xffffffff)).astype(np.int64)], 1), cnt.astype(np.int64)


def _check(ov, a, b):
    pairs, cnt = _want(a, b)
    assert np.array_equal(ov.pairs, pairs) and np.array_equal(ov.counts, cnt)
    for labels, areas, v in ((ov.a_labels, ov.a_areas, a), (ov.b_labels, ov.b_areas, b)):
        ul, uc = np.unique(v, return_counts=True)
        assert np.array_equal(labels, ul.astype(np.int64)) and np.array_equal(areas, uc)


def _labels(n, seed, dtype, run=37, top=200):
    """runs of equal labels (mean length ``run``), values below ``top``"""
    rng = np.random.default_rng(seed)
    starts = rng.random(n) < 1.0 / run
    vals = rng.integers(0, top, n) * (rng.random(n) < 0.6)
    idx = np.maximum.accumulate(np.where(starts, np.arange(n), 0))
    return vals[idx].astype(dtype)


def _dev(x):
    import torch
    if x.dtype in (np.uint16, np.uint32):      # no arithmetic is needed on the tensor: reinterpret the bytes
        return torch.from_numpy(x.view({2: np.int16, 4: np.int32}[x.itemsize])).cuda().view({2: torch.uint16, 4: torch.uint32}[x.itemsize])
    return torch.from_numpy(x).cuda()


DTYPES = [np.uint8, np.uint16, np.int32, np.uint32, np.int64]


@pytest.mark.parametrize('da', DTYPES)
@pytest.mark.parametrize('db', DTYPES)
def test_every_dtype_pair(da, db):
    from empanada_napari_amd import metrics
    n = 300_001
    a, b = _labels(n, 1, da), _labels(n, 2, db, run=23)
    if da in (np.uint32, np.int64):
        a[a == 7] = np.iinfo(np.uint32).max       # the largest legal label, on both sides: the table's empty-slot marker as a pair
    if db in (np.uint32, np.int64):
        b[a == np.iinfo(np.uint32).max] = np.iinfo(np.uint32).max
    _check(metrics.label_overlap(_dev(a), _dev(b)), a, b)
    _check(metrics.label_overlap(a, b), a, b)       # host arrays through the staging buffers


@pytest.mark.parametrize('n', [1, 63, 64, 65, 4097, 1_000_003])
def test_sizes_off_the_vector_width_and_the_tile(n):
    from empanada_napari_amd import metrics
    a, b = _labels(n, n, np.uint32), _labels(n, n + 1, np.int32)
    _check(metrics.label_overlap(_dev(a), _dev(b)), a, b)


def test_misaligned_base_and_single_pair():
    from empanada_napari_amd import metrics
    a, b = _labels(70_001, 3, np.uint8), _labels(70_001, 4, np.int64)
    _check(metrics.label_overlap(_dev(a)[1:], _dev(b)[1:]), a[1:], b[1:])
    one = np.full((16, 64, 64), 5, np.uint32)
    ov = metrics.label_overlap(_dev(one), _dev(one))
    assert ov.pairs.tolist() == [[5, 5]] and ov.counts.tolist() == [one.size]


def test_salt_and_pepper_forces_the_table_to_double():
    from empanada_napari_amd import metrics
    rng = np.random.default_rng(9)
    n = 1 << 21
    a, b = rng.integers(0, 1024, n).astype(np.uint32), rng.integers(0, 1024, n).astype(np.uint32)      # ~9e5 distinct pairs
    ov = metrics.label_overlap(_dev(a), _dev(b), capacity=1 << 16)
    assert ov.doublings >= 4          # 2^16 slots cannot hold them: the overflow path ran, the result is exact all the same
    _check(ov, a, b)
    assert len(ov.counts) > 800_000


def test_table_doubles_while_a_host_stream_is_in_flight():
    """the arrays of the test above as host arrays in three slabs of (3, 3, 2) slices: both staging slots are used again, the
    last slab is partial, and the table overflows and grows in the middle of the stream; exact all the same, and byte for byte
    what device tensors give in one slab"""
    from empanada_napari_amd import metrics
    rng = np.random.default_rng(9)
    n = 1 << 21
    a, b = rng.integers(0, 1024, n).astype(np.uint32), rng.integers(0, 1024, n).astype(np.uint32)
    a, b = a.reshape(8, 512, 512), b.reshape(8, 512, 512)
    ov = metrics.label_overlap(a, b, capacity=1 << 16, slab=3)
    assert ov.doublings >= 1
    _check(ov, a, b)
    whole = metrics.label_overlap(_dev(a), _dev(b))
    for f in ('a_labels', 'a_areas', 'b_labels', 'b_areas', 'pairs', 'counts'):
        assert getattr(ov, f).tobytes() == getattr(whole, f).tobytes() and getattr(ov, f).dtype == getattr(whole, f).dtype, f
    assert ov.shape == whole.shape == (8, 512, 512)


def test_slabs_and_directory_store(tmp_path):
    from empanada_napari_amd import metrics, zstore
    shape = (128, 256, 256)
    a = _labels(int(np.prod(shape)), 5, np.uint32, run=90, top=3000).reshape(shape)
    b = np.roll(a, 2, axis=2)
    b[b == 17] = 0
    whole = metrics.label_overlap(_dev(a), _dev(b))
    _check(whole, a, b)
    for slab in (1, 7, 64):
        for src in ((a, b), (_dev(a), _dev(b)), (a, _dev(b))):
            ov = metrics.label_overlap(*src, slab=slab)
            assert np.array_equal(ov.pairs, whole.pairs) and np.array_equal(ov.counts, whole.counts), slab
    za = zstore.DirArray.create(str(tmp_path / 'a'), shape, np.uint32, (32, 128, 128))
    zb = zstore.DirArray.create(str(tmp_path / 'b'), shape, np.uint32, (32, 128, 128))
    za[...], zb[...] = a, b
    ov = metrics.label_overlap(zstore.DirArray(str(tmp_path / 'a')), zstore.DirArray(str(tmp_path / 'b')), slab=48)
    assert np.array_equal(ov.pairs, whole.pairs) and np.array_equal(ov.counts, whole.counts)
    again = metrics.label_overlap(_dev(a), _dev(b))      # two runs: byte-identical
    assert again.pairs.tobytes() == whole.pairs.tobytes() and again.counts.tobytes() == whole.counts.tobytes()


@pytest.mark.parametrize('bad', [-1, 1 << 32])
def test_out_of_range_values_are_an_error(bad):
    from empanada_napari_amd import _abi, metrics
    a = _labels(5000, 6, np.int64)
    b = a.copy()
    b[4321] = bad
    with pytest.raises(_abi.EmpError, match='outside'):
        metrics.label_overlap(_dev(a), _dev(b))
    c = _labels(5000, 6, np.int32)
    c[77] = -1
    with pytest.raises(_abi.EmpError, match='outside'):
        metrics.label_overlap(_dev(c), _dev(a))


def test_public_functions_reproduce_the_reference_through_the_device_path():
    """the golden inputs (tests/golden/metrics.npz, recorded from the imported reference by tools/gen_metrics_golden.py) as device
    tensors, as host arrays and as one LabelOverlap shared by all three functions: the reference's outputs, under the
    comparisons of tests/test_metrics_host.py (integers exact, floats bit for bit, the two means within 4 ulp)"""
    import test_metrics_host as H
    from empanada_napari_amd import metrics
    for name in H.NAMES:
        gt, pred = H.GOLD[f'{name}/gt'], H.GOLD[f'{name}/pred']
        dg, dp = _dev(gt), _dev(pred)
        ov = metrics.label_overlap(dg, dp)
        _check(ov, gt, pred)
        H.check_pixel(name, metrics.compute_pixel_metrics(dp, dg))
        H.check_pixel(name, metrics.compute_pixel_metrics(ov))
        for thr in H.THRESHOLDS:
            H.check_instance(name, thr, metrics.compute_instance_metrics(dg, dp, iou_threshold=thr))
            H.check_instance(name, thr, metrics.compute_instance_metrics(ov, iou_threshold=thr))
        H.check_evaluate(name, metrics.evaluate(dg, dp, **H.eval_kwargs(name)))
        H.check_evaluate(name, metrics.evaluate(gt, pred, **H.eval_kwargs(name)))
        H.check_evaluate(name, metrics.evaluate(ov, **H.eval_kwargs(name)))
    with pytest.raises(ValueError):
        metrics.compute_pixel_metrics(np.zeros((4, 4), np.uint8), np.zeros((4, 5), np.uint8))


def test_engine3d_volumes_scored_on_the_device():
    """Engine3d on a 64-slice blob stack in two precisions; the per-slice panoptic maps stay where the engine leaves them (int64
    device tensors), are stacked there and scored by evaluate without a host copy of either volume.  Consistency only (no
    quality threshold)."""
    import torch
    from empanada_napari_amd import metrics, synth, weights
    from empanada_napari_amd.engines import HipPanopticDeepLab
    from empanada_napari_amd.inference import Engine3d
    vol = synth.blob_volume(64, 256, 256, seed=0, n_blobs=24, fast=True)
    cfg = dict(weights.MITONET_PDL_CFG)
    P = weights.fold_state_dict(weights.seeded_state_dict(cfg, seed=0), cfg)
    out = {}
    for prec in ('fp32', 'fp16x3'):
        model = HipPanopticDeepLab(P, cfg, folded=True, precision=prec)
        mc = {'model': model, 'thing_list': [1], 'labels': [1], 'class_names': {1: 'mito'}, 'padding_factor': 16,
              'norms': {'mean': 0.57571, 'std': 0.12765}}
        e3 = Engine3d(mc, label_divisor=10000, median_kernel_size=3, nms_kernel=3, nms_threshold=0.1, confidence_thr=0.5, min_size=50,
                      min_extent=2)
        out[prec] = torch.stack([p for pans in e3.iter_slice_chunks(vol, 0) for p in pans])
        e3.engine.reset()
        assert out[prec].is_cuda and out[prec].dtype == torch.int64 and tuple(out[prec].shape) == vol.shape
        del e3, model
    a, b = out['fp32'], out['fp16x3']
    ev = metrics.evaluate(a, b)
    n_gt, n_pred = int(torch.unique(a[a > 0]).numel()), int(torch.unique(b[b > 0]).numel())
    tp = len(ev['matched_ious'])
    assert tp + len(ev['gt_unmatched']) == n_gt and tp + len(ev['pred_unmatched']) == n_pred
    inter, union = int(((a > 0) & (b > 0)).sum()), int(((a > 0) | (b > 0)).sum())
    want = 1 if n_gt == 0 and n_pred == 0 else (0 if n_gt == 0 or n_pred == 0 else inter / union)
    assert ev['iou'] == want
    print('engine3d fp32 vs fp16x3:', n_gt, 'and', n_pred, 'slice objects,', tp, 'matched at IoU 0.5, semantic IoU', ev['iou'])
