"""The statements the label clean-up tests compare against, in numpy / scipy (tests/test_labels_host.py, tests/test_gpu_labels.py).
Everything is integer: every comparison is exact.

* table:            np.unique(return_counts=True), boxes from np.nonzero per label (upper ends exclusive, as regionprops.bbox)
* small filter:     np.where(np.isin(img, ids with area <= minimum), 0, img)
* boundary labels:  per distinct value scipy.ndimage.label(img == v, structure=np.ones((3,) * ndim)); the components that touch a
                    face are cleared (skimage.segmentation.clear_border's documented behaviour, restated: skimage itself is not
                    available here)"""
import numpy as np
from scipy import ndimage


def want_table(arr):
    """(labels, areas, boxes) of one array, labels ascending, background included"""
    arr = np.asarray(arr)
    labels, areas = np.unique(arr, return_counts=True)
    boxes = []
    for v in labels:
        nz = np.nonzero(arr == v)
        boxes.append([int(c.min()) for c in nz] + [int(c.max()) + 1 for c in nz])
    return labels.astype(np.int64), areas.astype(np.int64), np.asarray(boxes, dtype=np.int64).reshape(len(labels), 2 * arr.ndim)


def want_table_fast(arr):
    """the same table without the pass per label (for arrays with very many labels): np.minimum.at / np.maximum.at of the
    coordinates over np.unique's inverse"""
    arr = np.asarray(arr)
    labels, inv, areas = np.unique(arr, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    boxes = np.empty((len(labels), 2 * arr.ndim), np.int64)
    for ax, c in enumerate(np.unravel_index(np.arange(arr.size), arr.shape)):
        lo = np.full(len(labels), arr.shape[ax], np.int64)
        hi = np.full(len(labels), -1, np.int64)
        np.minimum.at(lo, inv, c)
        np.maximum.at(hi, inv, c)
        boxes[:, ax], boxes[:, arr.ndim + ax] = lo, hi + 1
    return labels.astype(np.int64), areas.astype(np.int64), boxes


def want_table_per_slice(vol):
    """(slices, labels, areas, boxes (k, 4)): a Python loop of per-image tables"""
    s, l, a, b = [], [], [], []
    for z in range(vol.shape[0]):
        labels, areas, boxes = want_table(vol[z])
        s.append(np.full(len(labels), z, np.int64))
        l.append(labels)
        a.append(areas)
        b.append(boxes)
    return np.concatenate(s), np.concatenate(l), np.concatenate(a), np.concatenate(b)


def check_table(t, arr):
    labels, areas, boxes = want_table(arr)
    assert t.slices is None and t.shape == tuple(arr.shape)
    assert np.array_equal(t.labels, labels), (t.labels, labels)
    assert np.array_equal(t.areas, areas)
    assert np.array_equal(t.boxes, boxes), (t.boxes[t.boxes != boxes], boxes[t.boxes != boxes])


def check_table_per_slice(t, vol):
    s, l, a, b = want_table_per_slice(vol)
    assert np.array_equal(t.slices, s) and np.array_equal(t.labels, l) and np.array_equal(t.areas, a) and np.array_equal(t.boxes, b)


def want_small_filter(img, minimum):
    labels, areas = np.unique(img, return_counts=True)
    ids = labels[(areas <= minimum) & (labels != 0)]
    return np.where(np.isin(img, ids), 0, img).astype(img.dtype), len(ids)


def want_clear_border(img):
    """clear_border restated -> (image, number of labels that vanish entirely)"""
    out = img.copy()
    structure = np.ones((3,) * img.ndim)
    border = np.zeros(img.shape, bool)
    for ax in range(img.ndim):
        idx = [slice(None)] * img.ndim
        for end in (0, -1):
            idx[ax] = end
            border[tuple(idx)] = True
    for v in np.unique(img):
        if v == 0:
            continue
        comp, n = ndimage.label(img == v, structure=structure)
        touching = np.unique(comp[border & (comp > 0)])
        out[np.isin(comp, touching) & (comp > 0)] = 0
    removed = len(np.setdiff1d(np.unique(img), np.unique(out)))
    return out, removed


def want_whole_label_border(img):
    """every voxel of a label whose box touches a face goes -> (image, number of labels removed)"""
    labels, _, boxes = want_table(img)
    nd = img.ndim
    touch = ((boxes[:, :nd] == 0) | (boxes[:, nd:] == np.asarray(img.shape))).any(axis=1) & (labels != 0)
    return np.where(np.isin(img, labels[touch]), 0, img).astype(img.dtype), int(touch.sum())


def per_slice(fn, vol, *args):
    """fn on every image of a stack -> (stack, total count)"""
    out, total = np.empty_like(vol), 0
    for z in range(vol.shape[0]):
        out[z], n = fn(vol[z], *args)
        total += n
    return out, total


def blobs(shape, n, seed, dtype=np.uint32, first=1):
    """n ellipsoids with labels first, first + 1, ... (later ones overwrite earlier ones: some labels end up in several pieces)"""
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, dtype)
    grid = np.indices(shape)
    for i in range(n):
        c = [rng.uniform(0.0, 1.0) * s for s in shape]
        r = [rng.uniform(0.05, 0.16) * s + 1 for s in shape]
        v[sum(((g - ci) / ri) ** 2 for g, ci, ri in zip(grid, c, r)) < 1] = first + i
    return v


def runs(n, seed, dtype, run=37, top=200):
    """a raveled array of runs of equal labels (mean length ``run``), values below ``top``, about 40 % background"""
    rng = np.random.default_rng(seed)
    starts = rng.random(n) < 1.0 / run
    vals = rng.integers(0, top, n) * (rng.random(n) < 0.6)
    idx = np.maximum.accumulate(np.where(starts, np.arange(n), 0))
    return vals[idx].astype(dtype)
