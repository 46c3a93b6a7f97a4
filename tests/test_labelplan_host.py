"""The host planning of Morph Labels, Fill holes and Split Labels (empanada_napari_amd/_labelplan.py) on its own: no device is
needed.  The Split bookkeeping is held against the statement of the loop (tests/split_case.py), the size limits against
hand-written tables, so that no array of such a size is allocated."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import split_case as SC
from empanada_napari_amd import _labelplan as P
from empanada_napari_amd import labels as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEVERAL = [name for name, (_, n, _, _) in SC.CASES.items() if n > 1]


def test_the_module_imports_numpy_only():
    """In a fresh interpreter, after the import, torch is not loaded and neither is the rest of the package.  numpy loads ctypes
    for itself, so ``'ctypes' not in sys.modules`` cannot be asked after it; instead ctypes and torch are barred once numpy is in
    (a None entry makes every later import of them fail), which asks more: no module on the way may even try."""
    code = ('import sys, numpy\n'
            'sys.modules["torch"] = sys.modules["ctypes"] = None\n'
            f'sys.path.insert(0, {ROOT!r})\n'
            'import __graft_entry__ as g\n'
            'g.load_package()\n'
            'import empanada_napari_amd._labelplan as P\n'
            'assert sys.modules["torch"] is None and sys.modules["ctypes"] is None\n'
            'mine = sorted(m for m in sys.modules if m.startswith("empanada_napari_amd"))\n'
            'assert mine == ["empanada_napari_amd", "empanada_napari_amd._labelplan"], mine\n'
            'print(len(P.morph_footprint_rows(2, True)))\n')
    res = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert res.stdout.split() == ['13']


def _table(arr):
    """the LabelTable of a host array, as the device gives it: every value that occurs, the background included"""
    ids = np.unique(arr)
    boxes = [[s.start for s in SC.tight_box(arr, l)] + [s.stop for s in SC.tight_box(arr, l)] for l in ids]
    return L.table_from_arrays(ids, [int((arr == l).sum()) for l in ids], boxes, arr.shape)


def _planned(arr, ids, d, start_label=None):
    """The report of a distance-mode call as the planners put it together -- passes, screening, the id loop -- with the marker
    counts of the statement (``tight_box``, ``distance_markers``) in place of the device stages; after a pass the array is the
    statement's.  Also checks the bases of every launch against the report."""
    eb = arr.itemsize * (-1 if arr.dtype.kind == 'i' else 1)
    turns, _, _ = P.split_turns(None, None, ids)
    report = []
    for mine in P.split_passes(_table(arr), turns, start_label):
        table = _table(arr)
        rep, todo = P.split_screen(table, mine, False)
        counts = np.asarray([SC.distance_markers(arr[SC.tight_box(arr, l)] == l, d)[2] for l in mine[todo[:, 0]]], np.int64)
        rep, (bases,) = P.split_ids(mine, rep, [(todo[:, 0], counts)], int(table.labels.max()), start_label, eb)
        for i, base in zip(todo[:, 0], bases):
            assert (base == -1) if isinstance(rep[i], str) else (base == rep[i][0] - 1 and len(rep[i]) >= 2)
        assert all(r is not None for r in rep)
        report += list(zip(mine.tolist(), rep))
        arr = SC.split(arr, ids=mine, min_distance=d, start_label=start_label)[0]
    return report


def _same_report(got, want):
    assert len(got) == len(want)
    for (gl, g), (wl, w) in zip(got, want):
        assert gl == wl and (g == w if isinstance(w, str) else np.array_equal(g, w)), (gl, g, w)


@functools.lru_cache(maxsize=None)
def _case(name):
    arr, d = SC.case(name)
    arr.setflags(write=False)
    return arr, d


@pytest.mark.parametrize('name', SEVERAL)
def test_the_id_loop_is_the_statements(name):
    arr, d = _case(name)
    ids = np.unique(arr)[1:]
    split_any = False
    for start in (None, 100, int(arr.max())):      # max_label moves with every split; accepted once; in use
        want = SC.split(arr, ids=ids, min_distance=d, start_label=start)[1]
        _same_report(_planned(arr, ids, d, start), want)
        split_any = split_any or any(not isinstance(r, str) for _, r in want)
        if start == int(arr.max()):
            assert all(r in ('ids in use', 'nothing to split') for _, r in want)
    assert split_any
    absent = int(arr.max()) + 1000      # beyond every id the splits hand out
    want = SC.split(arr, ids=[absent, *ids, 0], min_distance=d)[1]
    _same_report(_planned(arr, [absent, *ids, 0], d), want)
    assert want[-1] == (absent, 'label absent')
    # a uint8 array whose new ids pass 255: raised by the id loop itself, so before any base is handed out and anything is written
    high = np.where(arr > 0, arr + (255 - int(arr.max())), 0).astype(np.uint8)
    with pytest.raises(ValueError, match='do not fit the array\'s 1-byte unsigned type; nothing was written'):
        _planned(high, np.unique(high)[1:], d)
    with pytest.raises(ValueError):
        SC.split(high, ids=np.unique(high)[1:], min_distance=d)


def _corner_case():
    """the array of test_gpu_split_labels.py::test_an_unreached_part_becomes_the_largest_label_which_then_has_its_turn"""
    img = np.zeros((16, 30), np.int32)
    img[2:8, 2:12] = 1
    img[8, 12] = 1      # the corner voxel
    img[9:15, 10:28] = 2
    img[8, 13:20] = 2
    return img, np.asarray([(4, 3), (4, 10), (12, 11), (12, 26), (0, 0)])      # the last point lies on the background


def test_the_largest_label_runs_after_the_others():
    img, pts = _corner_case()
    turns, kept, under = P.split_turns(pts, img[tuple(pts.T)].astype(np.int64), None)
    assert turns.tolist() == [1, 2] and np.array_equal(kept, pts[:4]) and under.tolist() == [1, 1, 2, 2]
    table = _table(img)
    for start in (None, 3):      # max_label is 2, the largest label, which has the last turn
        passes = P.split_passes(table, turns, start)
        assert [p.tolist() for p in passes] == [[1], [2]]
    assert [p.tolist() for p in P.split_passes(table, turns, 100)] == [[1, 2]]      # start_label points elsewhere
    assert [p.tolist() for p in P.split_passes(table, turns[1:], None)] == [[2]]      # a single turn
    assert [p.tolist() for p in P.split_passes(table, turns[:1], None)] == [[1]]
    assert [p.tolist() for p in P.split_passes(table, np.asarray([1, 5]), None)] == [[1, 5]]      # the last turn is not the largest label
    assert [p.tolist() for p in P.split_passes(L.table_from_arrays([], [], [], img.shape), turns, None)] == [[1, 2]]
    assert P.split_turns(None, None, [[2, 0], [7, 2]])[0].tolist() == [2, 7] and len(P.split_turns(None, None, [])[0]) == 0


def test_screening_outcomes_and_size_limits():
    block = np.zeros((20, 30), np.int32)
    block[4:15, 3:25] = 3      # a label that fills its box
    turns = np.asarray([3, 8])
    report, todo = P.split_screen(_table(block), turns, False)
    assert report == ['nothing to split', 'label absent'] and todo.shape == (0, 7)
    report, todo = P.split_screen(_table(block), turns, True)      # ... is kept for its points
    assert report == [None, 'label absent'] and todo.tolist() == [[0, 0, 4, 3, 1, 11, 22]]
    vol = np.zeros((6, 7, 8), np.int32)
    vol[1:4, 2:6, 3:8] = 5
    vol[2, 3, 4] = 0
    report, todo = P.split_screen(_table(vol), np.asarray([5]), False)
    assert report == [None] and todo.tolist() == [[0, 1, 2, 3, 3, 4, 5]]
    assert P.split_boxes(np.asarray([4, 5]), np.asarray([[1, 0, 2, 3, 1, 4, 5], [0, 1, 2, 3, 3, 4, 5]])).tolist() == \
        [[0, 2, 3, 1, 4, 5, 0, 5], [1, 2, 3, 3, 4, 5, 20, 4]]
    # the squares of the sides: 1 + 1 + 32767^2 < 2^30 <= 32768^2
    ok = L.table_from_arrays([1], [9], [[0, 0, 1, 32767]], (1, 40000))
    assert P.split_screen(ok, np.asarray([1]), False)[1].tolist() == [[0, 0, 0, 0, 1, 1, 32767]]
    for points_mode in (False, True):
        with pytest.raises(ValueError, match='the box of label 1, .1, 32768., is too large'):
            P.split_screen(L.table_from_arrays([1], [9], [[0, 0, 1, 32768]], (1, 40000)), np.asarray([1]), points_mode)
    # the voxels: 1290^3 < SPLIT_MAX_ENTRIES < 1290^2 * 1291, both far below the diagonal's limit
    assert 1290 ** 3 <= P.SPLIT_MAX_ENTRIES < 1290 * 1290 * 1291 and 3 * 1291 ** 2 < P.SPLIT_MAX_DIAGONAL2
    ok = L.table_from_arrays([4], [9], [[5, 5, 5, 1295, 1295, 1295]], (2000, 2000, 2000))
    assert P.split_screen(ok, np.asarray([4]), False)[1].tolist() == [[0, 5, 5, 5, 1290, 1290, 1290]]
    with pytest.raises(ValueError, match='the box of label 4, .1290, 1290, 1291., is too large'):
        P.split_screen(L.table_from_arrays([4], [9], [[5, 5, 5, 1295, 1295, 1296]], (2000, 2000, 2000)), np.asarray([4]), False)


@pytest.mark.parametrize('name', ['image_d3', 'volume_d2', 'row_d4'])
def test_the_markers_of_a_launch_are_the_statements(name):
    """the boxes of all labels as one launch; the candidates of the statement stand in for emp_split_peaks"""
    arr, d = _case(name)
    turns = np.unique(arr)[1:].astype(np.int64)
    _, todo = P.split_screen(_table(arr), turns, False)
    boxes = P.split_boxes(turns, todo)
    crops = [arr[SC.tight_box(arr, l)] == l for l in turns[todo[:, 0]]]
    assert np.array_equal(boxes[:, 3:6].prod(axis=1), [c.size for c in crops]) and boxes[0, 6] == 0
    assert np.array_equal(boxes[1:, 6], np.cumsum([c.size for c in crops])[:-1]) and np.array_equal(boxes[:, 7], turns[todo[:, 0]])
    cand = []
    for k, crop in enumerate(crops):
        d2 = SC.edt2(crop)
        coords, values = SC.candidates(d2, d)
        cand.append(np.stack([np.full(len(coords), k), np.ravel_multi_index(tuple(coords.T), crop.shape), values], axis=1).reshape(-1, 3))
    counts = np.asarray([len(c) for c in cand], np.int64)
    per_box = P.split_peak_markers(np.concatenate(cand).astype(np.int64), counts, boxes, d)
    markers, n_markers = P.split_marker_array(per_box, boxes)
    assert markers.dtype == np.int32 and markers.flags.c_contiguous
    for k, crop in enumerate(crops):
        _, want, n = SC.distance_markers(crop, d)
        assert n_markers[k] == n
        mine = markers[markers[:, 0] == k]
        assert len(mine) == (int((want > 0).sum()) if n >= 2 else 0)      # fewer than two markers: nothing to flood
        assert np.array_equal(want.reshape(-1)[mine[:, 1]], mine[:, 2])
    # points mode: the points of a label, in its box, each once; neighbours are one marker
    pts = SC.case_points(arr, 3, 1)
    pts = np.concatenate([pts, pts[:2]])
    under = arr[tuple(pts.T)].astype(np.int64)
    _, kept, under = P.split_turns(pts, under, None)
    for k, coords in enumerate(P.split_point_markers(kept, under, boxes)):
        want = np.unique(kept[under == boxes[k, 7]], axis=0) - boxes[k, 3 - arr.ndim:3]
        assert np.array_equal(coords[:, 3 - arr.ndim:], want) and not coords[:, :3 - arr.ndim].any()


def test_fill_placement_within_levels():
    frames = np.asarray([[0, 0, 0, 1, 4, 5], [0, 2, 2, 1, 6, 7], [0, 9, 9, 1, 3, 3], [1, 1, 1, 2, 2, 2]], np.int64)
    placed, entries = P.fill_placement(frames, [[0, 2, 3], [1]])
    assert np.array_equal(placed[:, :6], frames)
    assert placed[:, 6].tolist() == [0, 0, 20, 29] and entries == 42      # running sums within a level; the largest level
    placed, entries = P.fill_placement(frames, [[0], [1, 2], [3]])
    assert placed[:, 6].tolist() == [0, 0, 42, 0] and entries == 51
    assert P.fill_placement(frames[:0], [])[1] == 0
    big = np.asarray([[0, 0, 0, 1024, 1024, 1024], [0, 0, 0, 1024, 1024, 1024]], np.int64)      # 2^30 voxels each
    with pytest.raises(ValueError, match='fill_label_holes: the padded boxes of the turns of level 1 hold 2147483648 voxels'):
        P.fill_placement(np.concatenate([frames, big]), [[0, 1], [4, 5]])
    placed, entries = P.fill_placement(big, [[0], [1]])      # the same frames in two levels
    assert placed[:, 6].tolist() == [0, 0] and entries == 1 << 30
    just = np.asarray([[0, 0, 0, 1, 1, (1 << 31) - 2]], np.int64)      # 2^31 - 2 entries are the most
    assert P.fill_placement(just, [[0]])[1] == (1 << 31) - 2
    with pytest.raises(ValueError, match='level 0'):
        P.fill_placement(just + [0, 0, 0, 0, 0, 1], [[0]])


def test_row_lookup():
    table = L.table_from_arrays([9, 0, 5, 2], [1, 50, 3, 4], np.zeros((4, 4)), (10, 10))      # sorted: 0, 2, 5, 9
    ids = [0, 1, 2, 5, 9, 10, 1 << 40, -3, 5]
    assert P.table_rows(table, ids).tolist() == [-1, -1, 1, 2, 3, -1, -1, -1, 2]
    assert P.table_rows(table, []).shape == (0,)
    empty = L.table_from_arrays([], [], [], (10, 10))
    assert P.table_rows(empty, ids).tolist() == [-1] * len(ids) and P.table_rows(empty, []).shape == (0,)
    assert P.box3(np.asarray([4, 5]), np.asarray([6, 9]))[0].tolist() == [0, 4, 5] and P.box3(np.asarray([4, 5]), np.asarray([6, 9]))[1].tolist() == [1, 6, 9]
    assert P.box3(np.asarray([1, 4, 5]), np.asarray([2, 6, 9]))[1].tolist() == [2, 6, 9]
    assert P.dims3((7, 8)) == (1, 7, 8) and P.dims3((6, 7, 8)) == (6, 7, 8)


def test_labels_still_exposes_what_moved():
    for name in ('morph_footprint_rows', 'morph_footprint_offsets', 'morph_schedule', 'split_spacing', 'split_marker_ids', '_morph_args',
                 '_morph_turns', '_morph_tiles', '_split_batches', 'MORPH_OPS', 'MORPH_MAX_RADIUS', 'FILL_MAX_HOLE_SIZE', 'FILL_MAX_LEVEL_VOXELS',
                 'SPLIT_MAX_DISTANCE', 'SPLIT_MAX_BOXES', 'SPLIT_MAX_ENTRIES', 'SPLIT_MAX_DIAGONAL2'):
        assert getattr(L, name) is getattr(P, name), name
    assert set(L.__all__) <= set(dir(L))
