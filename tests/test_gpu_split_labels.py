"""Device side of Split Labels (csrc/split.hip): the four emp_split_* entries through the ABI and
empanada_napari_amd.labels.split_labels, against the numpy / scipy statements of tests/split_case.py.  Everything is integer, so
every comparison is exact.  The distance transform and the maximum filter are pinned against scipy; the peak predicate and the
flood are the statements restated there (tests/test_split_case_host.py says how far the flood lies from skimage's)."""
import ctypes as C
import functools

import numpy as np
import pytest

import split_case as SC

pytestmark = pytest.mark.gpu

INF = 1 << 30


def _lib():
    from empanada_napari_amd import _abi
    return _abi, _abi.load()


def _boxes(shapes3, starts=None, labels=None):
    """(n, 8) int64 {z0, y0, x0, nz, ny, nx, offset, label}"""
    b = np.zeros((len(shapes3), 8), np.int64)
    b[:, 3:6] = shapes3
    if starts is not None:
        b[:, :3] = starts
    vox = b[:, 3:6].prod(axis=1)
    b[:, 6] = np.cumsum(vox) - vox
    b[:, 7] = 1 if labels is None else labels
    return b


def _as3(a):
    return a.reshape((1,) * (3 - a.ndim) + a.shape)


def _edt(vol, boxes):
    """emp_split_edt on an int32 array -> the flat d2 of the boxes"""
    import torch
    abi, lib = _lib()
    vol3 = _as3(np.ascontiguousarray(vol, dtype=np.int32))
    t = torch.from_numpy(vol3).cuda()
    N = int(boxes[:, 3:6].prod(axis=1).sum())
    d_boxes = torch.empty(boxes.size, dtype=torch.int64, device='cuda')
    d2 = torch.full((N,), -7, dtype=torch.int32, device='cuda')
    work = torch.empty(int(lib.emp_split_edt_work_bytes(N)), dtype=torch.uint8, device='cuda')
    abi.check(lib.emp_split_edt(abi.ptr(t), -4, *vol3.shape, boxes.ctypes.data, len(boxes), abi.ptr(d_boxes), abi.ptr(d2), N, abi.ptr(work),
                                abi.stream_ptr()), 'emp_split_edt')
    assert np.array_equal(t.cpu().numpy(), vol3)      # only read
    return d2.cpu().numpy()


def _peaks(images, d, capacity=None):
    """emp_split_peaks on a list of int32 images, one box each -> per image the (coords, values) of its candidates"""
    import torch
    abi, lib = _lib()
    boxes = _boxes([_as3(i).shape for i in images])
    flat = np.concatenate([np.asarray(i, np.int32).reshape(-1) for i in images])
    N = len(flat)
    dims = _as3(images[0]).shape if len(images) == 1 else (max(b[3] for b in boxes), max(b[4] for b in boxes), max(b[5] for b in boxes))
    d_boxes = torch.empty(boxes.size, dtype=torch.int64, device='cuda')
    d2 = torch.from_numpy(flat).cuda()
    cap = capacity or N
    cand = torch.full((3 * cap,), -1, dtype=torch.int32, device='cuda')
    counts = torch.full((len(images),), -1, dtype=torch.int32, device='cuda')
    work = torch.empty(int(lib.emp_split_peaks_work_bytes(N, len(images))), dtype=torch.uint8, device='cuda')
    abi.check(lib.emp_split_peaks(boxes.ctypes.data, len(images), abi.ptr(d_boxes), *[int(v) for v in dims], abi.ptr(d2), N, d, abi.ptr(cand), cap,
                                  abi.ptr(counts), abi.ptr(work), abi.stream_ptr()), 'emp_split_peaks')
    counts = counts.cpu().numpy()
    cand = cand.cpu().numpy().reshape(-1, 3)
    if capacity is not None:
        return counts, cand
    out, at = [], 0
    for k, img in enumerate(images):
        mine = cand[at:at + counts[k]]
        at += counts[k]
        assert (mine[:, 0] == k).all()
        out.append((np.stack(np.unravel_index(mine[:, 1], img.shape), axis=1).reshape(-1, img.ndim), mine[:, 2]))
    assert (cand[at:] == -1).all()
    return out


def _check_peaks(images, d):
    for (coords, values), img in zip(_peaks(images, d), images):
        wc, wv = SC.candidates(img, d)
        assert np.array_equal(coords, wc) and np.array_equal(values, wv), (img.shape, d, len(coords), len(wc))


def _flood(items, plateau):
    """emp_split_flood on a list of (d2, markers) images, one box each -> (per image the labels, the sweeps)"""
    import torch
    abi, lib = _lib()
    boxes = _boxes([_as3(d2).shape for d2, _ in items])
    flat = np.concatenate([np.asarray(d2, np.int32).reshape(-1) for d2, _ in items])
    N = len(flat)
    marks = []
    for k, (_, m) in enumerate(items):
        lin = np.flatnonzero(m.reshape(-1))
        marks.append(np.stack([np.full(len(lin), k), lin, m.reshape(-1)[lin]], axis=1))
    marks = np.ascontiguousarray(np.concatenate(marks).astype(np.int32))
    dims = [int(boxes[:, 3 + a].max()) for a in range(3)]
    d_boxes = torch.empty(boxes.size, dtype=torch.int64, device='cuda')
    d2 = torch.from_numpy(flat).cuda()
    out = torch.full((N,), -1, dtype=torch.int32, device='cuda')
    work = torch.empty(int(lib.emp_split_flood_work_bytes(N, len(marks))), dtype=torch.uint8, device='cuda')
    sweeps = C.c_int64(0)
    abi.check(lib.emp_split_flood(boxes.ctypes.data, len(items), abi.ptr(d_boxes), *dims, abi.ptr(d2), N, int(plateau), marks.ctypes.data, len(marks),
                                  abi.ptr(out), abi.ptr(work), abi.stream_ptr(), C.byref(sweeps)), 'emp_split_flood')
    out = out.cpu().numpy()
    return [out[b[6]:b[6] + b[3] * b[4] * b[5]].reshape(d2.shape) for b, (d2, _) in zip(boxes, items)], int(sweeps.value)


def _check_flood(items, plateau):
    got, sweeps = _flood(items, plateau)
    for g, (d2, m) in zip(got, items):
        energy = np.zeros(d2.shape, np.int64) if plateau else -d2.astype(np.int64)
        want = SC.flood_levels(energy, m, d2 > 0)
        assert np.array_equal(g, want), int((g != want).sum())
    return got, sweeps


def _random_mask(shape, seed, p=0.8):
    return np.random.default_rng(seed).random(shape) < p


# ----------------------------------------------------------------------------
# the distance transform and the candidates, through the ABI
# ----------------------------------------------------------------------------
WIDTHS = (1, 2, 63, 64, 65, 130)


@pytest.mark.parametrize('shape', [(9, w) for w in WIDTHS] + [(w, 9) for w in WIDTHS] + [(1, 200), (200, 1), (20, 33, 47)], ids=str)
def test_edt_and_peaks_at_word_and_tile_tails(shape):
    """rows of one word less one, one word, one word and one, three words; a row and a column as the whole crop; a volume"""
    for seed, p in ((1, 0.8), (2, 0.97)):
        mask = _random_mask(shape, seed, p)
        if mask.all():
            mask.reshape(-1)[0] = False
        boxes = _boxes([_as3(mask).shape])
        d2 = _edt(mask.astype(np.int32), boxes).reshape(shape)
        assert np.array_equal(d2, SC.edt2(mask))
        _check_peaks([d2], 1)
        _check_peaks([d2], 2)


def test_edt_rows_and_planes_without_background_and_a_full_box():
    img = np.ones((40, 70), np.int32)
    img[3, 5] = 0      # every other row has no background: the sentinel must survive the pass along y
    assert np.array_equal(_edt(img, _boxes([(1, 40, 70)])).reshape(img.shape), SC.edt2(img == 1))
    vol = np.ones((9, 12, 70), np.int32)
    vol[7, 2, 66] = 0      # every other plane has none
    assert np.array_equal(_edt(vol, _boxes([vol.shape])).reshape(vol.shape), SC.edt2(vol == 1))
    for full in (np.ones((40, 70), np.int32), np.ones((5, 6, 70), np.int32)):
        assert (_edt(full, _boxes([_as3(full).shape])) == INF).all()      # no background at all: "nothing to split" for the caller


def test_edt_of_a_box_inside_a_larger_array_sees_the_crop_only():
    """other labels and the background around the box are not background of the crop; a label value that is not 1"""
    arr = np.zeros((50, 90), np.int32)
    arr[10:30, 20:85] = 5
    arr[15:20, 30:40] = 0
    arr[22:25, 60:70] = 9
    boxes = _boxes([(1, 20, 65)], starts=[(0, 10, 20)], labels=[5])
    crop = arr[10:30, 20:85] == 5
    got = _edt(arr, boxes).reshape(crop.shape)
    assert np.array_equal(got, SC.edt2(crop)) and not np.array_equal(got, SC.edt2(crop, outside_background=True))


def test_two_boxes_in_one_launch():
    arr, _ = SC.case('volume_d2')
    ids = np.unique(arr)[1:3]
    sl = [SC.tight_box(arr, l) for l in ids]
    boxes = _boxes([[s.stop - s.start for s in b] for b in sl], starts=[[s.start for s in b] for b in sl], labels=ids)
    d2 = _edt(arr, boxes)
    parts = []
    for b, s, l in zip(boxes, sl, ids):
        part = d2[b[6]:b[6] + b[3] * b[4] * b[5]].reshape(tuple(b[3:6]))
        assert np.array_equal(part, SC.edt2(arr[s] == l))
        parts.append(part)
    _check_peaks(parts, 2)
    img = [SC.edt2(_random_mask((30, 41), 3, 0.9)), SC.edt2(_random_mask((7, 150), 4, 0.9))]
    _check_peaks(img, 1)
    _check_peaks(img, 3)


def test_edt_and_peaks_over_many_blocks():
    """600 x 600: 352 chunks of 1024 voxels, so the one-block scan of the chunk counts carries over its 256-wide step, and every
    kernel's grid has hundreds of blocks"""
    mask = _random_mask((600, 600), 6, 0.98)
    d2 = _edt(mask.astype(np.int32), _boxes([(1, 600, 600)])).reshape(mask.shape)
    assert np.array_equal(d2, SC.edt2(mask))
    _check_peaks([d2], 2)
    assert len(SC.candidates(d2, 2)[0]) > 2000
    big = np.full((9, 70), 0x7f7f7f80, np.int32)      # any int32 image: values above 0x7f7f7f7f
    big[4, 30] += 5
    _check_peaks([big], 1)


@pytest.mark.parametrize('d', [1, 2, 10, 100])
def test_peaks_by_min_distance(d):
    """window 2d + 1 against scipy's maximum filter, the border of d voxels; d = 100 is larger than the crops: no candidate"""
    arr, _ = SC.case('image_d10')
    d2 = SC.edt2(arr[SC.tight_box(arr, 2)] == 2)
    vol = SC.edt2(SC.case('volume_d3')[0] == 1)
    got = _peaks([d2, vol], d)
    _check_peaks([d2, vol], d)
    assert (len(got[0][0]) == 0) == (d == 100) and (d < 10 or len(got[1][0]) == 0)


def test_peaks_plateau_threshold_and_capacity():
    flat = np.full((20, 70), 5, np.int32)      # every voxel is a maximum: no candidate
    assert len(_peaks([flat], 1)[0][0]) == 0
    ridge = np.zeros((9, 300), np.int32)
    ridge[4] = 3      # a ridge of equal values: every voxel of it is a candidate, more than the capacity given
    _check_peaks([ridge], 2)
    counts, cand = _peaks([ridge], 2, capacity=10)
    assert counts[0] == 296 and np.array_equal(cand[:, 1], 4 * 300 + 2 + np.arange(10))
    shifted = np.full((12, 12), 4, np.int32)      # the threshold is the image's minimum, not 0
    shifted[6, 6] = 9
    shifted[3, 3] = 4
    _check_peaks([shifted], 1)
    assert len(_peaks([shifted], 1)[0][0]) == 1


# ----------------------------------------------------------------------------
# the flood, through the ABI
# ----------------------------------------------------------------------------
def _dumbbell():
    yy, xx = np.mgrid[:41, :100]
    mask = ((yy - 20) ** 2 + (xx - 22) ** 2 <= 18 ** 2) | ((yy - 20) ** 2 + (xx - 76) ** 2 <= 15 ** 2) | ((abs(yy - 20) <= 2) & (xx > 22) & (xx < 76))
    return mask


def test_flood_dumbbell_both_modes():
    mask = _dumbbell()
    d2 = SC.edt2(mask)
    markers = np.zeros(mask.shape, np.int32)
    markers[20, 22], markers[20, 76] = 1, 2
    got, _ = _check_flood([(d2, markers)], plateau=False)
    assert SC.regions_ok(got[0], markers, mask)
    _check_flood([(d2, markers)], plateau=True)


def test_flood_spiral_has_a_long_claim_chain():
    """a corridor of one voxel wound up: the claim chain is as long as the corridor, one sweep per step"""
    n = 41
    mask = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    length = 0
    seen = set()
    for _ in range(n * n):
        mask[y, x] = True
        seen.add((y, x))
        length += 1
        ny, nx = y + dy, x + dx
        ahead = (ny + dy, nx + dx)
        if not (0 <= ny < n and 0 <= nx < n) or (ny, nx) in seen or ahead in seen:
            dy, dx = dx, -dy
            ny, nx = y + dy, x + dx
            if not (0 <= ny < n and 0 <= nx < n) or (ny, nx) in seen or (ny + dy, nx + dx) in seen:
                break
        y, x = ny, nx
    markers = np.zeros(mask.shape, np.int32)
    markers[0, 0], markers[y, x] = 1, 2
    d2 = SC.edt2(mask)
    got, sweeps = _check_flood([(d2, markers)], plateau=True)
    assert length > 400 and length // 2 <= sweeps <= length + 2
    assert set(np.unique(got[0])) == {0, 1, 2}


def test_flood_side_basin_without_a_marker():
    """three discs in a row, markers in the two outer ones: the middle basin is entered over a saddle, so its voxels have
    e(q) < L and are claimed at the saddle's level, step by step"""
    yy, xx = np.mgrid[:31, :96]
    mask = np.zeros((31, 96), bool)
    for cx, r in ((14, 12), (46, 14), (80, 11)):
        mask |= (yy - 15) ** 2 + (xx - cx) ** 2 <= r * r
    mask |= (abs(yy - 15) <= 1) & (xx > 14) & (xx < 80)
    d2 = SC.edt2(mask)
    markers = np.zeros(mask.shape, np.int32)
    markers[15, 14], markers[15, 80] = 1, 2
    got, _ = _check_flood([(d2, markers)], plateau=False)
    _, TL, _ = SC.flood_levels(-d2.astype(np.int64), markers, mask, return_times=True)
    assert ((-d2.astype(np.int64) < TL) & mask).sum() > 100      # the case has what it is for
    vol = np.zeros((3,) + mask.shape, bool)
    vol[1] = mask
    vol[0, 10:20, 40:52] = vol[2, 12:18, 10:18] = True
    m3 = np.zeros(vol.shape, np.int32)
    m3[1] = markers
    _check_flood([(SC.edt2(vol), m3)], plateau=False)


def test_flood_marker_components_and_a_single_marker():
    """adjacent point markers are one marker (ndi.label): both voxels start with the same id; one marker floods everything"""
    mask = _dumbbell()
    d2 = SC.edt2(mask)
    m, n = SC.marker_image(mask.shape, [(20, 22), (20, 23), (20, 76)])
    assert n == 2
    _check_flood([(d2, m)], plateau=True)
    one = np.zeros(mask.shape, np.int32)
    one[20, 22] = 1
    got, _ = _check_flood([(d2, one)], plateau=True)
    assert np.array_equal(got[0] == 1, mask)
    # two boxes at once, one of them without any marker: it stays 0
    got, _ = _check_flood([(d2, m), (SC.edt2(_random_mask((13, 70), 5)), np.zeros((13, 70), np.int32))], plateau=False)
    assert not got[1].any()


# ----------------------------------------------------------------------------
# the public function
# ----------------------------------------------------------------------------
def _dev(x):
    import torch
    return torch.from_numpy(x).cuda()


@functools.lru_cache(maxsize=None)
def _case(name):
    arr, d = SC.case(name)
    arr.setflags(write=False)
    return arr, d


@functools.lru_cache(maxsize=None)
def _want_distance(name):
    arr, d = _case(name)
    out, report = SC.split(arr, ids=np.unique(arr)[1:], min_distance=d)
    out.setflags(write=False)
    return out, report


def _same_report(got, want):
    assert len(got) == len(want)
    for (gl, g), (wl, w) in zip(got, want):
        assert gl == wl and (g == w if isinstance(w, str) else np.array_equal(g, w)), (gl, g, w)


@pytest.mark.parametrize('name', list(SC.CASES))
def test_distance_mode_several_labels_in_one_call(name):
    from empanada_napari_amd import labels as L
    arr, d = _case(name)
    want, wrep = _want_distance(name)
    got, rep = L.split_labels(_dev(np.array(arr)), ids=np.unique(arr)[1:], min_distance=d, apply3d=arr.ndim == 3, report=True)
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
    _same_report(rep, wrep)
    assert not np.array_equal(want, arr)


@pytest.mark.parametrize('name', ['image_d3', 'image_d1', 'volume_d2', 'row_d4'])
def test_points_choose_the_labels_and_can_be_the_markers(name):
    from empanada_napari_amd import labels as L
    arr, d = _case(name)
    pts = SC.case_points(arr, 3, 1)      # the last one lies on the background
    assert arr[tuple(pts[-1])] == 0
    split_any = False
    for as_markers in (False, True):
        want, wrep = SC.split(arr, points=pts, min_distance=d, points_as_markers=as_markers)
        split_any = split_any or any(not isinstance(r, str) for _, r in wrep)
        got, rep = L.split_labels(_dev(np.array(arr)), points=pts, min_distance=d, points_as_markers=as_markers, apply3d=arr.ndim == 3, report=True)
        assert np.array_equal(got.cpu().numpy(), want)
        _same_report(rep, wrep)
    assert split_any
    only_background = L.split_labels(_dev(np.array(arr)), points=pts[-1:], apply3d=arr.ndim == 3, report=True)
    assert np.array_equal(only_background[0].cpu().numpy(), arr) and only_background[1] == []


def test_the_wrong_variants_differ_on_the_device_result():
    from empanada_napari_amd import labels as L
    for variant, kw in SC.WRONG.items():
        differs = False
        for name in SC.CASES:
            arr, d = _case(name)
            ids = np.unique(arr)[1:]
            got = L.split_labels(np.array(arr), ids=ids, min_distance=d, apply3d=arr.ndim == 3)
            assert np.array_equal(got, _want_distance(name)[0])
            differs = differs or not np.array_equal(got, SC.split(arr, ids=ids, min_distance=d, **kw)[0])
            if differs:
                break
        assert differs, variant


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_plane_of_a_volume(axis):
    from empanada_napari_amd import labels as L
    img, d = _case('image_d3')
    vol = np.zeros((5,) + img.shape, np.int32)
    vol[:] = 200      # the volume's maximum is not the plane's: max_label is the image's (:577)
    vol[2] = img
    vol = np.ascontiguousarray(np.moveaxis(vol, 0, axis))
    ids = np.unique(img)[1:]
    want, wrep = SC.split(vol, ids=ids, min_distance=d, plane=2, axis=axis)
    got, rep = L.split_labels(_dev(vol.copy()), ids=ids, min_distance=d, plane=2, axis=axis, report=True)
    assert np.array_equal(got.cpu().numpy(), want) and not np.array_equal(want, vol)
    _same_report(rep, wrep)
    assert wrep[0][1][0] == int(img.max()) + 1
    pts = np.insert(SC.case_points(img, 2, 3), axis, 2, axis=1)
    want, wrep = SC.split(vol, points=pts, points_as_markers=True, plane=2, axis=axis)
    got, rep = L.split_labels(vol.copy(), points=pts, points_as_markers=True, plane=2, axis=axis, report=True)
    assert np.array_equal(got, want)
    _same_report(rep, wrep)
    with pytest.raises(ValueError, match='plane'):
        L.split_labels(vol.copy(), points=pts + np.eye(3, dtype=np.int64)[axis], plane=2, axis=axis)
    with pytest.raises(ValueError, match='apply3d'):
        L.split_labels(vol.copy(), ids=ids)


@pytest.mark.parametrize('dtype', [np.uint8, np.int32, np.int64])
def test_dtypes_with_ids_near_the_top(dtype):
    from empanada_napari_amd import labels as L
    arr, d = _case('image_d3')      # four labels, 2 + 6 + 2 + 2 pieces
    top = int(np.iinfo(dtype).max)
    high = np.where(arr > 0, arr.astype(np.int64) + (top - 16), 0).astype(dtype)      # the labels end 12 below the top: all fit
    ids = np.unique(high)[1:]
    want, wrep = SC.split(high, ids=ids, min_distance=d)
    got, rep = L.split_labels(high.copy(), ids=ids, min_distance=d, report=True)
    assert got.dtype == dtype and np.array_equal(got, want) and int(want.max()) == top
    _same_report(rep, wrep)
    assert np.array_equal(L.split_labels(_dev(high.copy()), ids=ids, min_distance=d).cpu().numpy(), want)
    higher = np.where(arr > 0, arr.astype(np.int64) + (top - 15), 0).astype(dtype)      # one id too many
    with pytest.raises(ValueError):
        SC.split(higher, ids=np.unique(higher)[1:], min_distance=d)
    mine = higher.copy()
    with pytest.raises(ValueError, match='do not fit'):
        L.split_labels(mine, ids=np.unique(higher)[1:], min_distance=d, inplace=True)
    assert np.array_equal(mine, higher)      # nothing was written


def test_start_label_accepted_refused_and_refused_on_the_second_turn():
    from empanada_napari_amd import labels as L
    arr, d = _case('image_d3')
    ids = np.unique(arr)[1:]
    for start in (100, int(arr.max()) + 1, int(arr.max()), 1):
        want, wrep = SC.split(arr, ids=ids, min_distance=d, start_label=start)
        got, rep = L.split_labels(np.array(arr), ids=ids, min_distance=d, start_label=start, report=True)
        assert np.array_equal(got, want)
        _same_report(rep, wrep)
        if start > arr.max():      # the first turn takes the ids, every later one finds them in use
            assert rep[0][1][0] == start and all(r == 'ids in use' for _, r in rep[1:])
        else:
            assert all(r == 'ids in use' for _, r in rep) and np.array_equal(got, arr)
    got, rep = L.split_labels(np.array(arr), ids=[2, 77, 0], min_distance=d, report=True)
    _same_report(rep, SC.split(arr, ids=[2, 77, 0], min_distance=d)[1])
    assert rep[1] == (77, 'label absent')
    block = np.zeros((20, 30), np.int32)
    block[4:15, 3:25] = 3      # a label that fills its box: no background, nothing to split, nothing launched
    got, rep = L.split_labels(block, ids=[3], min_distance=2, report=True)
    assert rep == [(3, 'nothing to split')] and np.array_equal(got, block)
    pts = np.asarray([(6, 5), (12, 20)])      # ... but its points split it
    got, rep = L.split_labels(block, points=pts, points_as_markers=True, report=True)
    want, wrep = SC.split(block, points=pts, points_as_markers=True)
    assert np.array_equal(got, want) and np.array_equal(rep[0][1], [4, 5])


def test_an_unreached_part_becomes_the_largest_label_which_then_has_its_turn():
    """label 1's corner voxel is joined to it by a corner only: no marker reaches it and it becomes max_label = 2 (:544), which
    is a label with a later turn, inside its box and face-joined to it: the loop lets that turn flood it"""
    from empanada_napari_amd import labels as L
    img = np.zeros((16, 30), np.int32)
    img[2:8, 2:12] = 1
    img[8, 12] = 1      # the corner voxel
    img[9:15, 10:28] = 2
    img[8, 13:20] = 2
    pts = np.asarray([(4, 3), (4, 10), (12, 11), (12, 26)])
    want, wrep = SC.split(img, points=pts, points_as_markers=True)
    assert want[8, 12] > 2 and np.array_equal(wrep[0][1], [3, 4])
    for _ in range(2):
        got, rep = L.split_labels(img.copy(), points=pts, points_as_markers=True, report=True)
        assert np.array_equal(got, want)
        _same_report(rep, wrep)
    t = _dev(np.where(img > 0, img + 250, 0).astype(np.uint8))      # 251, 252 -> 253, 254 fit; the second pass (255, 256) overflows, the first is undone
    keep = t.clone()
    with pytest.raises(ValueError, match='do not fit'):
        L.split_labels(t, points=pts, points_as_markers=True, inplace=True)
    assert bool((t == keep).all())


def test_return_kinds_arguments_and_reproducibility():
    import torch
    from empanada_napari_amd import labels as L
    arr, d = _case('image_d3')
    arr = np.array(arr)
    ids = np.unique(arr)[1:]
    want = _want_distance('image_d3')[0]
    t = _dev(arr.copy())
    res = L.split_labels(t, ids=ids, min_distance=d)
    assert isinstance(res, torch.Tensor) and res.data_ptr() != t.data_ptr() and np.array_equal(t.cpu().numpy(), arr)
    assert L.split_labels(t, ids=ids, min_distance=d, inplace=True) is t and np.array_equal(t.cpu().numpy(), want)
    new = L.split_labels(arr, ids=ids, min_distance=d)
    assert isinstance(new, np.ndarray) and new is not arr and np.array_equal(new, want) and np.array_equal(arr, _case('image_d3')[0])
    mine = arr.copy()
    assert L.split_labels(mine, ids=ids, min_distance=d, inplace=True) is mine and np.array_equal(mine, want)
    for name in ('image_d6', 'volume_d3'):
        a, dd = _case(name)
        runs = [L.split_labels(np.array(a), ids=np.unique(a)[1:], min_distance=dd, apply3d=a.ndim == 3).tobytes() for _ in range(2)]
        assert runs[0] == runs[1]
    for bad in (dict(ids=ids, points=np.zeros((1, 2), int)), dict(), dict(ids=ids, points_as_markers=True), dict(ids=ids, min_distance=0),
                dict(ids=ids, min_distance=101), dict(points=np.asarray([[0, 500]])), dict(points=np.asarray([[0.5, 1.0]])),
                dict(ids=ids, start_label=0)):
        with pytest.raises(ValueError):
            L.split_labels(arr, **bad)
    with pytest.raises(ValueError, match='2-D or 3-D'):
        L.split_labels(np.zeros((2, 2, 8, 8), np.int32), ids=[1])

    class Store:
        shape, dtype = arr.shape, arr.dtype

        def __getitem__(self, k):
            return arr[k]
    with pytest.raises(ValueError, match='chunked store'):
        L.split_labels(Store(), ids=ids)


def test_the_statistics_of_the_device_loops():
    """What only the callers of ``_split_device``, ``_morph_device`` and ``_fill_device`` see, the statistics, on shapes of a few
    thousand voxels: the values are those recorded before the planning moved to _labelplan.py (the flood's sweeps are
    reproducible: every sweep reads one buffer and writes the other)."""
    import torch
    import fill_holes_case as FC
    import morph_case as MC
    from empanada_napari_amd import labels as L
    dev = torch.device('cuda', 0)
    for name, want in (('image_d3', {'turns': 4, 'boxes': 4, 'entries': 4357, 'candidates': 22, 'markers': 12, 'sweeps': 39}),
                       ('volume_d2', {'turns': 3, 'boxes': 3, 'entries': 2265, 'candidates': 6, 'markers': 5, 'sweeps': 9})):
        arr, d = _case(name)
        t = _dev(np.array(arr))
        report, stats = L._split_device(t, -4, arr.shape, None, np.unique(arr)[1:], d, False, None, dev)
        assert stats == want
        _same_report(report, _want_distance(name)[1])
        assert np.array_equal(t.cpu().numpy(), _want_distance(name)[0])
    arr, d = _case('image_d3')
    stats = L._split_device(_dev(np.array(arr)), -4, arr.shape, SC.case_points(arr, 3, 1), None, d, True, None, dev)[1]
    assert stats == {'turns': 4, 'boxes': 4, 'entries': 4357, 'candidates': 0, 'markers': 12, 'sweeps': 53}
    for shape, close, erode, fill in (((40, 50), (5, 12, 14), (1, 12, 2), {'turns': 15, 'levels': 6, 'tiles': 15, 'launches': 29, 'scratch_entries': 701}),
                                      ((12, 30, 34), (9, 21, 26), (1, 21, 2), {'turns': 16, 'levels': 11, 'tiles': 25, 'launches': 54, 'scratch_entries': 3240})):
        blobs = MC.blobs(shape, 12, 3)
        for op, (levels, tiles, launches) in (('Close', close), ('Erode', erode)):
            stats = L._morph_device(_dev(blobs.copy()), -4, shape, op, 2, len(shape) == 3, None, dev)
            assert stats == {'turns': 12, 'turns_scheduled': 12, 'levels': levels, 'tiles': tiles, 'launches': launches}
        stats = L._fill_device(_dev(FC.holes(shape, 12, 3)), -4, shape, 2, 64, len(shape) == 3, None, dev)
        assert stats == {**fill, 'turns_scheduled': fill['turns']}


def test_clean_labels_tool_split_mode(tmp_path, capsys):
    import importlib.util
    import json
    import os
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'clean_labels.py')
    spec = importlib.util.spec_from_file_location('_clean_labels_split', tool)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    arr, d = _case('image_d3')
    src, dst = tmp_path / 'in.npy', tmp_path / 'out.npy'
    np.save(src, arr)
    capsys.readouterr()
    res = mod.main([str(src), str(dst), '--split', '1,2,3,4', '--min-distance', str(d)])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    assert res['labels_affected'] == 4 and np.array_equal(np.load(dst), _want_distance('image_d3')[0])
    vol, d = _case('volume_d2')
    np.save(src, vol)
    res = mod.main([str(src), str(dst), '--split', '1,2,3', '--min-distance', str(d), '--3d'])
    assert res['labels_affected'] == 2 and np.array_equal(np.load(dst), _want_distance('volume_d2')[0])
