"""Split Labels (empanada_napari/_merge_split_widget.py:422-634) stated with numpy / scipy: what empanada_napari_amd.labels.
split_labels and the emp_split_* kernels must compute.  Integers throughout, so every comparison with it is exact.

PINNED here against scipy: the distance transform (``edt2``) and the maximum filter inside ``candidates``.
RESTATED FROM MEMORY of skimage's source, which is not available here and so cannot be pinned: ``peak_local_max``'s defaults
(``candidates``), ``ensure_spacing`` (``spaced``: greedy by value, a kept peak rejects those at Euclidean distance < d, strictly;
the strictness and the norm are named parameters because they are the part of the recollection most likely to be off --
``peak_local_max`` has a ``p_norm`` argument whose default may be the maximum norm in recent versions) and the order of
``watershed``'s queue (``flood_sequential``).

The flood that is built is ``flood_levels``, the level-synchronous form of the watershed; ``flood_sequential`` is the heap
restatement of skimage's, and tests/test_split_case_host.py says how far the two are apart: nowhere on one plateau (points mode),
a few per cent of a label's voxels next to the border between two regions in distance mode."""
import heapq
import itertools

import numpy as np
from scipy import ndimage as ndi


# ----------------------------------------------------------------------------
# the statements
# ----------------------------------------------------------------------------
def tight_box(img, label, pad=0):
    """the slices of regionprops' bbox of ``label`` (:519); ``pad`` > 0 is a wrong variant"""
    where = np.nonzero(img == label)
    return tuple(slice(max(int(w.min()) - pad, 0), min(int(w.max()) + 1 + pad, n)) for w, n in zip(where, img.shape))


def edt2(binary, outside_background=False):
    """``np.rint(ndi.distance_transform_edt(binary) ** 2)`` as int32: the exact squared distance to the nearest voxel of the crop
    that is not the label.  ``outside_background`` (wrong): what lies outside the crop counts as background"""
    binary = np.asarray(binary, bool)
    if outside_background:
        inner = tuple(slice(1, -1) for _ in binary.shape)
        return edt2(np.pad(binary, 1))[inner]
    return np.rint(ndi.distance_transform_edt(binary) ** 2).astype(np.int32)


def candidates(d2, d, exclude_border=True, squeeze=True):
    """skimage's ``peak_local_max(image, min_distance=d)`` before its spacing rule -> (coords (n, ndim) in raster order, values).
    threshold = image.min(); footprint = the full (2d + 1)^n window, ``mode='nearest'``; a candidate has image == max and
    image > threshold; if image == max at every voxel there is none; the d outermost voxels of every axis are cleared
    (``exclude_border=True``); size-1 axes are squeezed before all of this (:434-440).  The two flags are wrong variants."""
    d2 = np.asarray(d2)
    img = np.squeeze(d2) if squeeze else d2
    if img.ndim == 0:
        return np.zeros((0, d2.ndim), np.int64), np.zeros(0, d2.dtype)
    mask = img == ndi.maximum_filter(img, size=2 * d + 1, mode='nearest')
    if mask.all():
        mask[...] = False
    mask &= img > img.min()
    if exclude_border:
        for a in range(img.ndim):
            edge = [slice(None)] * img.ndim
            edge[a] = slice(0, d)
            mask[tuple(edge)] = False
            edge[a] = slice(max(img.shape[a] - d, 0), None)
            mask[tuple(edge)] = False
    coords = np.argwhere(mask.reshape(d2.shape))
    return coords, d2[tuple(coords.T)]


def spaced(coords, values, d, strict=True, chebyshev=False):
    """``ensure_spacing`` restated: the candidates by value descending, stable over raster order; one is kept unless a kept one lies
    at distance < d (``strict``; ``<=`` is a wrong variant) -> the kept coordinates in the order they were kept"""
    order = np.argsort(-np.asarray(values, np.int64), kind='stable')
    kept = []
    for c in np.asarray(coords, np.int64)[order]:
        if kept:
            diff = np.abs(np.asarray(kept) - c)
            dist2 = (diff.max(axis=1) ** 2) if chebyshev else (diff ** 2).sum(axis=1)
            if ((dist2 < d * d) if strict else (dist2 <= d * d)).any():
                continue
        kept.append(c)
    return np.asarray(kept, np.int64).reshape(-1, np.asarray(coords).shape[1])


def marker_image(shape, coords):
    """``ndi.label`` (connectivity 1) of the marker mask (:446, :454) -> (markers int32, their number)"""
    mask = np.zeros(shape, bool)
    if len(coords):
        mask[tuple(np.asarray(coords).T)] = True
    lab, n = ndi.label(mask)
    return lab.astype(np.int32), int(n)


def _padded(energy, markers, mask, connectivity):
    """flat views of the arrays padded by one voxel of non-mask, and the flat neighbour offsets in raster order"""
    mask = np.pad(np.asarray(mask, bool), 1)
    shape = mask.shape
    strides = [int(np.prod(shape[a + 1:])) for a in range(len(shape))]
    offs = []
    for o in itertools.product((-1, 0, 1), repeat=len(shape)):
        n = sum(abs(v) for v in o)
        if n and n <= connectivity:
            offs.append(sum(v * s for v, s in zip(o, strides)))
    e = np.pad(np.asarray(energy, np.int64), 1).reshape(-1)
    m = np.pad(np.asarray(markers, np.int64), 1).reshape(-1)
    m = np.where(mask.reshape(-1), m, 0)
    return e.tolist(), m.tolist(), mask.reshape(-1).tolist(), sorted(offs), shape


def flood_levels(energy, markers, mask, tie_max=False, connectivity=1, return_times=False):
    """THE RULE THAT IS BUILT.  Every mask voxel gets a time (L, g) and a label.  A marker voxel has time (e, 0) and its marker's id.
    Any other voxel q takes the label of the face neighbour p in the mask with the lexicographically smallest (L_p, g_p, label_p),
    and the time (L_p, g_p + 1) if e(q) <= L_p, else (e(q), 0).  Times strictly increase along a claim chain, so the solution is
    unique; this is a Dijkstra over the times: when a voxel is popped every neighbour with a smaller time is final, and the smallest
    of them claims it.  A part of the mask that no marker reaches stays 0.  ``tie_max`` (the larger label wins a tie) and
    ``connectivity=2`` are wrong variants."""
    e, m, inmask, offs, shape = _padded(energy, markers, mask, connectivity)
    n = len(e)
    done = [False] * n
    TL, TG, lab = [0] * n, [0] * n, [0] * n
    heap = [(e[i], 0, i) for i in range(n) if m[i] > 0]
    for _, _, i in heap:
        lab[i] = m[i]
    heapq.heapify(heap)
    while heap:
        L, g, i = heapq.heappop(heap)
        if done[i] or (m[i] > 0 and (L, g) != (e[i], 0)):
            continue
        if m[i] == 0:
            best = None
            for o in offs:
                p = i + o
                if done[p]:
                    key = (TL[p], TG[p], -lab[p] if tie_max else lab[p])
                    if best is None or key < best:
                        best = key
            lab[i] = -best[2] if tie_max else best[2]
        done[i], TL[i], TG[i] = True, L, g
        for o in offs:
            q = i + o
            if inmask[q] and not done[q] and m[q] == 0:
                heapq.heappush(heap, (L, g + 1, q) if e[q] <= L else (e[q], 0, q))
    inner = tuple(slice(1, -1) for _ in shape)
    out = np.asarray(lab, np.int32).reshape(shape)[inner]
    if return_times:
        return out, np.asarray(TL, np.int64).reshape(shape)[inner], np.asarray(TG, np.int64).reshape(shape)[inner]
    return out


def flood_sequential(energy, markers, mask, connectivity=1):
    """skimage's ``watershed(energy, markers, mask=mask)`` restated from memory: one priority queue over (value, age); the marker
    voxels enter in raster order; a popped voxel labels each still unlabelled mask neighbour (offsets in raster order) at once and
    pushes it with its own value and the next age."""
    e, m, inmask, offs, shape = _padded(energy, markers, mask, connectivity)
    lab = list(m)
    age = 0
    heap = []
    for i in range(len(e)):
        if m[i] > 0:
            heap.append((e[i], age, i))
            age += 1
    heapq.heapify(heap)
    while heap:
        _, _, i = heapq.heappop(heap)
        for o in offs:
            q = i + o
            if inmask[q] and lab[q] == 0:
                lab[q] = lab[i]
                age += 1
                heapq.heappush(heap, (e[q], age, q))
    return np.asarray(lab, np.int32).reshape(shape)[tuple(slice(1, -1) for _ in shape)]


def distance_markers(binary, d, **v):
    """``_distance_markers`` (:428-447) -> (d2, markers, their number); the energy is -d2, which orders like -sqrt(d2)"""
    d2 = edt2(binary, outside_background=v.get('outside_background', False))
    coords, values = candidates(d2, d, exclude_border=v.get('exclude_border', True), squeeze=v.get('squeeze', True))
    kept = spaced(coords, values, d, strict=v.get('strict', True))
    markers, n = marker_image(d2.shape, kept)
    return d2, markers, n


# ----------------------------------------------------------------------------
# the loop
# ----------------------------------------------------------------------------
def _split_image(img, points, ids, d, points_as_markers, start_label, v):
    """the loop of :517-547 on the writable array ``img`` (an image, or a volume with apply3d) -> the report"""
    if points is not None:
        points = np.asarray(points, np.int64).reshape(-1, img.ndim)
        under = img[tuple(points.T)].astype(np.int64)
        points, under = points[under != 0], under[under != 0]
        turns = np.unique(under)
    else:
        turns = np.unique(np.asarray(ids, np.int64).reshape(-1))
        turns = turns[turns > 0]
    top = int(np.iinfo(img.dtype).max)
    first_max = int(img.max())
    report = []
    for label in turns.tolist():
        if not (img == label).any():
            report.append((label, 'label absent'))
            continue
        box = tight_box(img, label, pad=v.get('pad', 0))
        crop = img[box]
        binary = crop == label
        if points_as_markers:
            local = points[under == label] - np.asarray([s.start for s in box])
            markers, n = marker_image(binary.shape, local)
            energy = np.zeros(binary.shape, np.int64)
        elif binary.all():
            report.append((label, 'nothing to split'))
            continue
        else:
            d2, markers, n = distance_markers(binary, d, **v)
            energy = -d2.astype(np.int64)
        if n < 2:
            report.append((label, 'nothing to split'))
            continue
        new = flood_levels(energy, markers, binary, tie_max=v.get('tie_max', False), connectivity=v.get('connectivity', 1))
        now = int(img.max()) if v.get('update_max', True) else first_max
        max_label = int(start_label) - 1 if start_label is not None else now
        if now >= 1 + max_label:
            report.append((label, 'ids in use'))
            continue
        if max_label + n > top:
            raise ValueError(f'split: the new ids up to {max_label + n} do not fit {img.dtype}')
        crop[binary] = (new[binary].astype(np.int64) + max_label).astype(img.dtype)
        report.append((label, max_label + np.arange(1, n + 1, dtype=np.int64)))
    return report


def split(arr, points=None, ids=None, min_distance=10, points_as_markers=False, start_label=None, plane=None, axis=0, **variant):
    """Split Labels on a copy of ``arr`` -> (the array, the report: per turn (label, new ids | 'nothing to split' | 'ids in use' |
    'label absent')).  An image, a volume (the widget's apply3d), or with ``plane`` the image ``take(arr, plane, axis)`` of a
    volume (:549-588), whose ``max_label`` is the image's.  Turns run in ``np.unique`` order of the ids under the points (zeros
    dropped, :501-515) or of ``ids``.  ``max_label`` is the array's maximum as it is when the turn comes, or ``start_label - 1``;
    the write is refused when the maximum is >= the smallest new id (:540).  ``variant``: the wrong variants below."""
    out = np.array(arr)
    if arr.ndim == 3 and plane is not None:
        img = np.ascontiguousarray(np.take(out, plane, axis))
        if points is not None:
            points = np.asarray(points, np.int64).reshape(-1, 3)
            assert (points[:, axis] == plane).all()
            points = np.delete(points, axis, axis=1)
        report = _split_image(img, points, ids, min_distance, points_as_markers, start_label, variant)
        index = [slice(None)] * 3
        index[axis] = plane
        out[tuple(index)] = img
        return out, report
    return out, _split_image(out, points, ids, min_distance, points_as_markers, start_label, variant)


# wrong variants: each must change the result of at least one case (tests/test_split_case_host.py)
WRONG = {
    'connectivity 2': dict(connectivity=2),
    'padded box': dict(pad=1),
    'outside the crop is background': dict(outside_background=True),
    'tie by the larger label': dict(tie_max=True),
    'spacing not strict': dict(strict=False),
    'no border exclusion': dict(exclude_border=False),
    'no squeeze': dict(squeeze=False),
    'max_label not updated between turns': dict(update_max=False),
}


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
def blobs(shape, n_labels, seed, dtype=np.int32, first=1):
    """``n_labels`` labels, each a union of two to four overlapping discs / balls: organelles that touch and want splitting"""
    rng = np.random.default_rng(seed)
    arr = np.zeros(shape, dtype)
    grid = np.indices(shape)
    for k in range(n_labels):
        centre = np.asarray([rng.integers(s // 6, s - s // 6) for s in shape], float)
        for _ in range(int(rng.integers(2, 5))):
            r = float(rng.uniform(0.08, 0.2)) * min(s for s in shape if s > 1)
            r = max(r, 2.0)
            ball = sum((g - c) ** 2 for g, c in zip(grid, centre)) <= r * r
            arr[ball] = first + k
            step = rng.normal(size=len(shape))
            centre = centre + step / np.linalg.norm(step) * r * float(rng.uniform(1.0, 1.6))
            centre = np.clip(centre, 0, np.asarray(shape) - 1)
    return arr


# the fixed cases of tests/test_split_case_host.py and tests/test_gpu_split_labels.py: name -> (shape, labels, seed, min_distance)
CASES = {
    'image_d3': ((72, 90), 4, 3, 3),
    'image_d1': ((60, 67), 3, 5, 1),
    'image_d6': ((96, 130), 3, 7, 6),
    'image_d10': ((150, 140), 2, 11, 10),
    'volume_d2': ((20, 33, 47), 3, 13, 2),
    'volume_d3': ((24, 40, 40), 2, 17, 3),
    'row_d4': ((5, 25), 1, None, 4),
}


def case(name):
    """-> (the array, min_distance).  'row_d4' is made by hand: a label of one row (its crop is squeezed) whose two highest peaks
    are exactly min_distance apart (the spacing rule is strict: both stay) and whose other pieces no marker reaches"""
    shape, n, seed, d = CASES[name]
    if seed is None:
        arr = np.zeros(shape, np.int32)
        arr[2, 3:22] = np.asarray([1, 0, 1, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 0, 1, 0, 1]) * 7
        return arr, d
    return blobs(shape, n, seed), d


def case_points(arr, per_label, seed):
    """``per_label`` random voxels of every label, as the widget's points layer would hold them (and one on the background)"""
    rng = np.random.default_rng(seed)
    pts = []
    for label in np.unique(arr)[1:]:
        where = np.argwhere(arr == label)
        pts.extend(where[rng.choice(len(where), size=min(per_label, len(where)), replace=False)])
    pts.append(np.argwhere(arr == 0)[0])
    return np.asarray(pts, np.int64)


def regions_ok(new, markers, mask):
    """every region of a flood is connected (connectivity 1) and holds its marker"""
    for k in range(1, int(markers.max()) + 1):
        region = (new == k) & mask
        if not region[markers == k].all() or ndi.label(region)[1] != 1:
            return False
    return True
