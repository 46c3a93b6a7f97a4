"""Host side of the label clean-up module (empanada_napari_amd/labels.py), no GPU needed: the policy functions are pure numpy on a
LabelTable, built here with table_from_arrays from the numpy statement of the table (tests/labels_case.py), as the device kernel's
contract states it.

* count_labels reproduces the outputs RECORDED FROM THE IMPORTED REFERENCE (tools/gen_labels_golden.py -> tests/golden/labels.npz:
  _label_counter_widget.py:105-118, divisors 0 / 1000 / 10000, empty inputs);
* small_labels: the reference's `<=` (_filter_small_labels.py:23), background never;
* boundary_labels: four edges of an image, six faces of a volume, four edges per image in per-slice mode;
* next_available_labels / next_available_label: the widget's queue (_merge_split_widget.py:730-759), a class that does not occur
  included;
* label_bbox raises on an absent id as the widget does (:658-659);
* slab_plan (empanada_napari_amd/_labelstream.py): the slab every streamed tool cuts its input into."""
import os

import numpy as np
import pytest

import labels_case as LC
from empanada_napari_amd import _labelstream as S, labels as L

GOLD = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'labels.npz')))


def _table(arr):
    return L.table_from_arrays(*LC.want_table(arr), arr.shape)


def _table_per_slice(vol):
    s, l, a, b = LC.want_table_per_slice(vol)
    return L.table_from_arrays(l, a, b, vol.shape, slices=s)


def _image():
    """10 x 12: label 1 (area 4) in the corner, 2 (area 6) interior, 3 (area 1) interior, 4 on the right edge, 7 on the bottom edge"""
    img = np.zeros((10, 12), np.int32)
    img[0:2, 0:2] = 1
    img[3:5, 3:6] = 2
    img[6, 6] = 3
    img[4:6, 11] = 4
    img[9, 2:5] = 7
    return img


@pytest.mark.parametrize('name', [str(n) for n in GOLD['names']])
def test_count_labels_reproduces_the_reference(name):
    queue, class_ids = L.count_labels(GOLD[f'{name}/values'], int(GOLD[f'{name}/divisor']))
    assert class_ids == GOLD[f'{name}/class_ids'].tolist()
    assert list(queue) == GOLD[f'{name}/keys'].tolist()
    off, lists = GOLD[f'{name}/offsets'], GOLD[f'{name}/lists']
    for i, k in enumerate(queue):
        assert queue[k] == lists[off[i]:off[i + 1]].tolist()


def test_count_labels_groups_by_class_in_the_order_given():
    """the grouping against its plain statement, on values that are neither sorted nor distinct (the golden's inputs come from
    np.unique): per class ascending, the values with value // divisor == class, in the order they were given"""
    rng = np.random.default_rng(5)
    for divisor in (1, 7, 1000):
        values = rng.integers(1, 5 * divisor + 3, 200)
        queue, class_ids = L.count_labels(values, divisor)
        assert class_ids == sorted(set((values // divisor).tolist())) == list(queue)
        for c in class_ids:
            assert queue[c] == [v for v in values.tolist() if v // divisor == c]
    assert L.count_labels(np.array([], np.int64), 1000) == ({}, [])
    assert L.count_labels([2000, 1999], 1000) == ({1: [1999], 2: [2000]}, [1, 2])


def test_golden_covers_the_divisors():
    assert {int(GOLD[f'{n}/divisor']) for n in GOLD['names']} >= {0, 1000, 10000}
    q, c = L.count_labels(np.array([5, 6]), 0)
    assert (q, c) == ({1: [5, 6]}, [1])


def test_table_from_arrays_sorts_and_checks():
    t = L.table_from_arrays([5, 2, 0], [1, 2, 3], [[0, 0, 1, 1], [1, 1, 2, 3], [0, 0, 4, 4]], (4, 4))
    assert t.labels.tolist() == [0, 2, 5] and t.areas.tolist() == [3, 2, 1] and t.boxes[1].tolist() == [1, 1, 2, 3]
    assert t.slices is None and not t.per_slice and t.shape == (4, 4) and t.doublings == 0
    with pytest.raises(ValueError):
        L.table_from_arrays([1, 2], [1], [[0, 0, 1, 1]], (4, 4))
    with pytest.raises(ValueError):
        L.table_from_arrays([1], [1], [[0, 0, 1, 1]], (4, 4), slices=[0])
    fast = LC.want_table_fast(_image())
    for a, b in zip(fast, LC.want_table(_image())):
        assert np.array_equal(a, b)


def test_small_labels_uses_less_or_equal():
    t = _table(_image())
    assert L.small_labels(t, 0).tolist() == []
    assert L.small_labels(t, 1).tolist() == [3]
    assert L.small_labels(t, 3).tolist() == [3, 4, 7]      # 4 has area 2, 7 area 3
    assert L.small_labels(t, 4).tolist() == [1, 3, 4, 7]      # area == minimum goes: `<=`
    assert L.small_labels(t, 5).tolist() == [1, 3, 4, 7]
    assert L.small_labels(t, 6).tolist() == [1, 2, 3, 4, 7]
    assert L.small_labels(t, 10 ** 9).tolist() == [1, 2, 3, 4, 7]      # never the background
    img = _image()
    for m in (0, 1, 4, 6):
        ids = L.small_labels(t, m)
        want, n = LC.want_small_filter(img, m)
        assert np.array_equal(np.where(np.isin(img, ids), 0, img), want) and n == len(ids)


def test_boundary_labels_of_an_image_and_of_a_volume():
    img = _image()
    assert L.boundary_labels(_table(img)).tolist() == [1, 4, 7]
    # the same image as the middle slice of a volume: only what touches a face of the VOLUME
    vol = np.zeros((3,) + img.shape, np.int32)
    vol[1] = img
    assert L.boundary_labels(_table(vol)).tolist() == [1, 4, 7]
    vol[0, 3, 3] = 2      # label 2 reaches the first slice: a face of the volume
    assert L.boundary_labels(_table(vol)).tolist() == [1, 2, 4, 7]
    # as a stack of images every slice has its own four edges, and the first / last slice is no face
    ids = L.boundary_labels(_table_per_slice(vol))
    assert ids.tolist() == [[1, 1], [1, 4], [1, 7]]
    one = np.zeros((5, 5), np.uint8)
    one[2, 2] = 9
    assert L.boundary_labels(_table(one)).tolist() == []
    thin = np.ones((1, 5, 5), np.uint8)      # one slice: every label touches the z faces
    assert L.boundary_labels(_table(thin)).tolist() == [1]


def test_per_slice_keys_and_tables():
    vol = np.zeros((3, 6, 6), np.uint16)
    vol[0, 1:3, 1:3] = 5
    vol[2, 1:3, 1:3] = 5
    vol[2, 4:6, 0:1] = 8
    t = _table_per_slice(vol)
    assert t.per_slice and t.slices.tolist() == [0, 0, 1, 2, 2, 2] and t.labels.tolist() == [0, 5, 0, 0, 5, 8]
    assert t.boxes.shape == (6, 4) and t.boxes[1].tolist() == [1, 1, 3, 3] and t.boxes[5].tolist() == [4, 0, 6, 1]
    assert L.small_labels(t, 2).tolist() == [[2, 8]]
    assert L.small_labels(t, 4).tolist() == [[0, 5], [2, 5], [2, 8]]
    assert L.boundary_labels(t).tolist() == [[2, 8]]
    assert L.label_bbox(t, 5, slice_index=2) == (1, 1, 3, 3)
    with pytest.raises(Exception, match='No label'):
        L.label_bbox(t, 5, slice_index=1)
    assert L.class_label_lists(t, 0) == {0: {1: [5]}, 1: {1: []}, 2: {1: [5, 8]}}
    assert L.next_available_labels(t, 10)[2] == {0: [1, 2, 3, 4, 6, 7, 9]}


def test_class_lists_and_next_available_labels():
    img = np.zeros((8, 8), np.int64)
    img[0, 0:4] = [1001, 1002, 1004, 3001]
    img[1, 0:2] = [1999, 2000]
    t = _table(img)
    assert L.class_label_lists(t, 1000) == {1: [1001, 1002, 1004, 1999], 2: [2000], 3: [3001]}
    assert L.class_label_lists(t, 0) == {1: [1001, 1002, 1004, 1999, 2000, 3001]}
    queue = L.next_available_labels(t, 1000)
    assert sorted(queue) == [1, 2, 3]
    for ci in queue:      # the widget's statement (_merge_split_widget.py:738-744)
        used = t.labels[1:]
        want = np.setdiff1d(np.arange(ci * 1000 + 1, (ci + 1) * 1000), used[(used >= ci * 1000 + 1) & (used < (ci + 1) * 1000)])
        assert queue[ci] == want.tolist()
    assert queue[1][:3] == [1003, 1005, 1006] and queue[2][0] == 2001 and 2000 not in queue[2]
    assert L.next_available_label(queue, 1, 1000) == 1003
    assert L.next_available_label(queue, 1, 1000) == 1005      # popped
    # a class that does not occur: its whole register, the first id handed out (:754-759)
    assert 7 not in queue
    assert L.next_available_label(queue, 7, 1000) == 7001
    assert queue[7][0] == 7002 and queue[7][-1] == 7999 and len(queue[7]) == 998
    assert L.next_available_label(queue, 7, 1000) == 7002
    with pytest.raises(ValueError):
        L.next_available_labels(t, 0)


def test_label_bbox():
    vol = np.zeros((4, 10, 12), np.int32)
    vol[1:3, 2:5, 7:9] = 42
    t = _table(vol)
    assert L.label_bbox(t, 42) == (1, 2, 7, 3, 5, 9)
    for absent in (41, 0):
        with pytest.raises(Exception, match='No label'):
            L.label_bbox(t, absent)


def test_statements_of_the_boundary_modes_differ_where_they_should():
    """a label with one border component and one interior component: clear_border keeps the interior one (the label does not
    count as removed), the whole-label mode removes it"""
    img = np.zeros((12, 12), np.int32)
    img[0:2, 0:2] = 5
    img[5:7, 5:7] = 5
    img[8:10, 2:4] = 6
    ref, n_ref = LC.want_clear_border(img)
    assert n_ref == 0 and ref[5, 5] == 5 and ref[0, 0] == 0 and ref[8, 2] == 6
    whole, n_whole = LC.want_whole_label_border(img)
    assert n_whole == 1 and not (whole == 5).any() and whole[8, 2] == 6
    assert L.boundary_labels(_table(img)).tolist() == [5]


@pytest.mark.parametrize('host_row_bytes, default', [(None, None), (1, S.SLAB_BYTES), (1 << 20, 64), (S.SLAB_BYTES + 1, 1)])
def test_slab_plan(host_row_bytes, default):
    """slab=None: everything at once without a host source (default None here), else SLAB_BYTES // row bytes, at least 1; the
    slab is clamped to [1, max(rows, 1)]; the bounds tile [0, rows) in steps of the slab, none for rows == 0"""
    assert S.SLAB_BYTES == 64 << 20
    for rows in (0, 1, 5, 128):
        for slab in (None, 1, 3, 128, 1000):
            asked = slab if slab is not None else (rows if default is None else default)
            want = max(1, min(asked, max(rows, 1)))
            got, bounds = S.slab_plan(rows, host_row_bytes, slab)
            assert got == want and type(got) is int, (rows, slab)
            if rows == 0:
                assert bounds == []
                continue
            assert bounds[0][0] == 0 and bounds[-1][1] == rows
            assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))      # no gap, no overlap
            assert all(z1 - z0 == want for z0, z1 in bounds[:-1]) and 0 < bounds[-1][1] - bounds[-1][0] <= want
            assert S.slab_plan(rows, host_row_bytes, got) == (got, bounds)      # a plan made from its own slab is the same plan


def test_no_cpu_fallback(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # the refusal comes first, with or without a device
    for call in (lambda: L.label_table(_image()), lambda: L.delete_labels(_image(), [1]), lambda: L.merge_labels(_image(), [1, 2]),
                 lambda: L.filter_out_small_label_areas(_image(), 3), lambda: L.remove_boundary_labels(_image())):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
