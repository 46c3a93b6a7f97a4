"""The statements the Measure Labels tests compare against, in numpy (tests/test_measure_case_host.py, tests/test_gpu_measure.py).
Everything raw is an integer: every comparison is exact.

* want_measures:    per label != 0 the voxel count, the box, np.add.at of the coordinates and of their products, and the exposed
                    faces by shifted compares per axis on the array padded by one (the pad is `outside`)
* model_measures:   the same table the way the kernel forms it -- runs cut at row ends with closed-form sums, faces against the
                    -z / -y / -x neighbour with both sides credited, slabs with a halo slice -- with one rule at a time broken
                    on request, to show that the cases of the device test notice each of them
* the case generators of the device test"""
import numpy as np

import labels_case as LC

PAIRS = {3: [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)], 2: [(0, 0), (1, 1), (0, 1)]}      # the columns of sum2


def want_measures(vol, border_faces=True):
    """dict(labels, areas, boxes, sum1, sum2, faces) of one array, labels ascending, background 0 left out"""
    vol = np.asarray(vol)
    nd = vol.ndim
    labels, inv = np.unique(vol, return_inverse=True)
    inv = inv.reshape(vol.shape)
    k, flat = len(labels), inv.reshape(-1)
    coords = [c.reshape(-1).astype(np.int64) for c in np.indices(vol.shape)]
    areas = np.bincount(flat, minlength=k).astype(np.int64)
    sum1 = np.zeros((k, nd), np.int64)
    sum2 = np.zeros((k, len(PAIRS[nd])), np.int64)
    boxes = np.zeros((k, 2 * nd), np.int64)
    for a in range(nd):
        np.add.at(sum1[:, a], flat, coords[a])
        lo, hi = np.full(k, vol.shape[a], np.int64), np.full(k, -1, np.int64)
        np.minimum.at(lo, flat, coords[a])
        np.maximum.at(hi, flat, coords[a])
        boxes[:, a], boxes[:, nd + a] = lo, hi + 1
    for j, (a, b) in enumerate(PAIRS[nd]):
        np.add.at(sum2[:, j], flat, coords[a] * coords[b])
    faces = np.zeros((k, nd), np.int64)
    padded = np.pad(inv, 1, constant_values=-1)      # -1: outside the array
    inner = tuple(slice(1, -1) for _ in range(nd))
    for a in range(nd):
        lo = tuple(slice(0, -1) if i == a else inner[i] for i in range(nd))
        hi = tuple(slice(1, None) if i == a else inner[i] for i in range(nd))
        p, q = padded[lo], padded[hi]      # every pair of neighbours along the axis, the two pairs with the outside included
        differ = p != q
        if not border_faces:
            differ &= (p >= 0) & (q >= 0)
        for side in (p, q):
            np.add.at(faces[:, a], side[differ & (side >= 0)], 1)
    keep = labels != 0
    return {'labels': labels[keep].astype(np.int64), 'areas': areas[keep], 'boxes': boxes[keep], 'sum1': sum1[keep], 'sum2': sum2[keep],
            'faces': faces[keep]}


def want_measures_per_slice(vol, border_faces=True):
    """the same per image of a stack, with a leading `slices` column: a Python loop of want_measures"""
    parts = [want_measures(vol[z], border_faces) for z in range(vol.shape[0])]
    out = {f: np.concatenate([p[f] for p in parts]) for f in parts[0]}
    out['slices'] = np.concatenate([np.full(len(p['labels']), z, np.int64) for z, p in enumerate(parts)])
    return out


def scaled(want, factors):
    """want_measures of np.repeat(vol, f_a, axis=a) for every axis from want_measures(vol), in Python integers: a voxel at i becomes
    the block [f i, f i + f), whose coordinate sum is f^2 i + f (f - 1) / 2 and whose sum of squares is f^3 i^2 + f^2 (f - 1) i +
    (f - 1) f (2 f - 1) / 6; a face becomes the product of the other axes' factors"""
    f = [int(v) for v in factors]
    nd = len(f)
    n = want['areas'].astype(object)
    s1 = want['sum1'].astype(object)
    vol = int(np.prod(f))
    sum1 = np.stack([vol // f[a] * (f[a] ** 2 * s1[:, a] + f[a] * (f[a] - 1) // 2 * n) for a in range(nd)], axis=1)
    cols = []
    for j, (a, b) in enumerate(PAIRS[nd]):
        s2 = want['sum2'][:, j].astype(object)
        if a == b:
            others = vol // f[a]
            cols.append(others * (f[a] ** 3 * s2 + f[a] ** 2 * (f[a] - 1) * s1[:, a] + (f[a] - 1) * f[a] * (2 * f[a] - 1) // 6 * n))
        else:      # (f_a i + u)(f_b j + v) summed over u, v and the third axis
            others = vol // (f[a] * f[b])
            ua, ub = f[a] * (f[a] - 1) // 2, f[b] * (f[b] - 1) // 2
            cols.append(others * (f[a] ** 2 * f[b] ** 2 * s2 + f[a] ** 2 * ub * s1[:, a] + f[b] ** 2 * ua * s1[:, b] + ua * ub * n))
    out = dict(want)
    out['areas'] = (n * vol).astype(np.int64)
    out['boxes'] = want['boxes'] * np.array(f + f)
    out['sum1'] = sum1.astype(np.int64)
    out['sum2'] = np.stack(cols, axis=1).astype(np.int64)
    out['faces'] = want['faces'] * np.array([vol // f[a] for a in range(nd)])
    return out


# ----------------------------------------------------------------------------
# the kernel's rules, one at a time breakable
# ----------------------------------------------------------------------------
DEFECTS = ('run_not_cut_at_row_end', 'z_face_dropped_at_slab_border', 'border_face_dropped_at_last_index', 'one_side_credited',
           'label_0_entered')


def _sum1(a, b):
    return (a + b) * (b - a + 1) // 2


def _sum2(a, b):
    p = lambda n: n * (n + 1) * (2 * n + 1) // 6
    return p(b) - (p(a - 1) if a else 0)


def model_measures(vol, border_faces=True, slab=None, defect=None):
    """want_measures of a 3-D array by the kernel's rules; ``defect``: one of DEFECTS, or None"""
    vol = np.asarray(vol)
    D, H, W = vol.shape
    assert defect is None or defect in DEFECTS
    rows = {}

    def row(l):
        return rows.setdefault(int(l), {'n': 0, 'lo': [D, H, W], 'hi': [-1, -1, -1], 's1': [0, 0, 0], 's2': [0] * 6, 'f': [0, 0, 0]})

    flat = vol.reshape(-1)
    cut = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    if defect != 'run_not_cut_at_row_end':
        cut = np.union1d(cut, np.arange(W, flat.size, W))
    for i0, i1 in zip(np.concatenate([[0], cut]), np.concatenate([cut, [flat.size]])):
        l = int(flat[i0])
        if l == 0 and defect != 'label_0_entered':
            continue
        z, y, x0 = int(i0) // (H * W), int(i0) // W % H, int(i0) % W
        x1, n = x0 + int(i1 - i0) - 1, int(i1 - i0)      # a run that was not cut runs on beyond the row's end
        r = row(l)
        sx = _sum1(x0, x1)
        r['n'] += n
        for a, (c0, c1) in enumerate(((z, z), (y, y), (x0, x1))):
            r['lo'][a], r['hi'][a] = min(r['lo'][a], c0), max(r['hi'][a], c1)
        for a, v in enumerate((z * n, y * n, sx)):
            r['s1'][a] += v
        for j, v in enumerate((z * z * n, y * y * n, _sum2(x0, x1), z * y * n, z * sx, y * sx)):
            r['s2'][j] += v

    def credit(values, axis):
        for l, c in zip(*np.unique(values, return_counts=True)):
            if l != 0 or defect == 'label_0_entered':
                row(l)['f'][axis] += int(c)

    def pairs(cur, nb, axis):      # nb: the -axis neighbours of cur
        d = cur != nb
        credit(cur[d], axis)
        if defect != 'one_side_credited':
            credit(nb[d], axis)

    slab = D if slab is None else slab
    for z0 in range(0, D, slab):
        for z in range(z0, min(D, z0 + slab)):
            s = vol[z]
            if z > z0 or (z0 > 0 and defect != 'z_face_dropped_at_slab_border'):      # z0 > 0: the halo slice
                pairs(s, vol[z - 1], 0)
            pairs(s[1:], s[:-1], 1)
            pairs(s[:, 1:], s[:, :-1], 2)
            if border_faces:
                last = defect != 'border_face_dropped_at_last_index'
                if z == 0:
                    credit(s, 0)
                if z == D - 1 and last:
                    credit(s, 0)
                credit(s[0], 1)
                credit(s[:, 0], 2)
                if last:
                    credit(s[-1], 1)
                    credit(s[:, -1], 2)
    keys = sorted(k for k, r in rows.items() if r['n'])
    get = lambda f: np.array([rows[k][f] for k in keys], dtype=np.int64).reshape(len(keys), -1)
    return {'labels': np.array(keys, np.int64), 'areas': get('n')[:, 0], 'boxes': np.concatenate([get('lo'), get('hi') + 1], axis=1),
            'sum1': get('s1'), 'sum2': get('s2'), 'faces': get('f')}


def same(got, want):
    return all(got[f].shape == want[f].shape and np.array_equal(got[f], want[f]) for f in want)


# ----------------------------------------------------------------------------
# the cases of the device test
# ----------------------------------------------------------------------------
DTYPES = [np.uint8, np.uint16, np.int32, np.uint32, np.int64]


def volume(dtype, shape=(5, 37, 61), seed=1):
    """runs of mean length 29 that cross row and slice ends, about 40 % background"""
    return LC.runs(int(np.prod(shape)), seed, dtype, run=29, top=120 if np.dtype(dtype).itemsize == 1 else 200).reshape(shape)


def slab_volume():
    """depth 11 (no multiple of 2 or 3): blobs, plus boxes that start and end exactly at the borders of slabs of 2 and of 3
    slices, one that spans all of them and one of a single slice"""
    vol = LC.blobs((11, 40, 48), 30, 5, np.uint32, first=1000)
    vol[3:6, 2:9, 3:12] = 7        # slab 3: starts at a border, ends at the next
    vol[2:6, 20:30, 30:41] = 8     # slab 2: the same
    vol[1:11, 12:18, 20:26] = 9    # spans every border
    vol[6:7, 30:38, 2:10] = 10     # one slice, the first of a slab of 2 and of 3
    vol[0:2, 0:4, 40:48] = 11      # touches three faces of the array
    return vol


def checkerboard(shape=(6, 10, 14)):
    """labels 1 and 2 alternating in every direction: every voxel is a run head and every face is exposed"""
    z, y, x = np.indices(shape)
    return (1 + (z + y + x) % 2).astype(np.uint16)


def check(m, want, shape):
    """a LabelMeasures against want_measures' dict"""
    assert m.shape == tuple(shape)
    for f in ('slices',) if 'slices' in want else ():
        assert np.array_equal(m.slices, want['slices'])
    for f in ('labels', 'areas', 'boxes', 'sum1', 'sum2', 'faces'):
        got = getattr(m, f)
        assert got.shape == want[f].shape and np.array_equal(got, want[f]), (f, got[got != want[f]][:8], want[f][got != want[f]][:8])
