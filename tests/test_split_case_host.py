"""The statements of Split Labels (tests/split_case.py) against each other, on the fixed cases that tests/test_gpu_split_labels.py
runs on the device: how far the level-synchronous flood that is built lies from the sequential one of skimage (restated), and that
every wrong variant of the loop changes a result.  No device is needed."""
import functools

import numpy as np
import pytest
from scipy import ndimage as ndi

import split_case as SC

NAMES = list(SC.CASES)


@functools.lru_cache(maxsize=None)
def _turns(name):
    """per label of the case that has at least two markers in distance mode: (binary, d2, markers)"""
    arr, d = SC.case(name)
    out = []
    for label in np.unique(arr)[1:]:
        binary = arr[SC.tight_box(arr, label)] == label
        if binary.all():
            continue
        d2, markers, n = SC.distance_markers(binary, d)
        if n >= 2:
            out.append((binary, d2, markers))
    return out


def test_the_distance_transform_is_exact_in_integers():
    """rint(edt^2) is the squared distance itself: against the brute-force minimum over the background"""
    arr, _ = SC.case('image_d3')
    binary = arr[SC.tight_box(arr, 1)] == 1
    bg = np.argwhere(~binary)
    want = np.zeros(binary.shape, np.int32)
    for p in np.argwhere(binary):
        want[tuple(p)] = ((bg - p) ** 2).sum(axis=1).min()
    assert np.array_equal(SC.edt2(binary), want)
    assert not np.array_equal(SC.edt2(binary, outside_background=True), want)


@pytest.mark.parametrize('name', NAMES)
def test_points_mode_equals_the_sequential_flood(name):
    """one plateau: the smallest label wins a tie, which is what a first-in-first-out queue does"""
    arr, _ = SC.case(name)
    for seed in (1, 2):
        pts = SC.case_points(arr, 3, seed)
        under = arr[tuple(pts.T)]
        for label in np.unique(arr)[1:]:
            box = SC.tight_box(arr, label)
            binary = arr[box] == label
            markers, n = SC.marker_image(binary.shape, pts[under == label] - np.asarray([s.start for s in box]))
            energy = np.zeros(binary.shape, np.int64)
            assert np.array_equal(SC.flood_levels(energy, markers, binary), SC.flood_sequential(energy, markers, binary)), (name, label)


@pytest.mark.parametrize('name', NAMES)
def test_distance_mode_stays_near_the_sequential_flood(name):
    """at most 5 % of a label's voxels differ, and every region is connected and holds its marker"""
    turns = _turns(name)
    assert turns
    for binary, d2, markers in turns:
        energy = -d2.astype(np.int64)
        ours, theirs = SC.flood_levels(energy, markers, binary), SC.flood_sequential(energy, markers, binary)
        share = float((ours != theirs)[binary].mean())
        print(name, int(binary.sum()), share)
        assert share <= 0.05, (name, share)
        assert SC.regions_ok(ours, markers, binary)
        assert not ours[~binary].any()


def test_the_time_rule_holds_at_every_voxel():
    """flood_levels is the fixed point of the rule it states: recomputed from its own times, nothing changes"""
    binary, d2, markers = _turns('image_d3')[0]
    energy = -d2.astype(np.int64)
    lab, TL, TG = SC.flood_levels(energy, markers, binary, return_times=True)
    for q in np.argwhere(binary & (markers == 0)):
        best = None
        for a in range(binary.ndim):
            for s in (-1, 1):
                p = q.copy()
                p[a] += s
                if 0 <= p[a] < binary.shape[a] and binary[tuple(p)]:
                    key = (TL[tuple(p)], TG[tuple(p)], lab[tuple(p)])
                    best = key if best is None or key < best else best
        want = (best[0], best[1] + 1) if energy[tuple(q)] <= best[0] else (energy[tuple(q)], 0)
        assert (TL[tuple(q)], TG[tuple(q)], lab[tuple(q)]) == (*want, best[2])


@pytest.mark.parametrize('variant', list(SC.WRONG))
def test_every_wrong_variant_changes_a_result(variant):
    changed = []
    for name in NAMES:
        arr, d = SC.case(name)
        ids = np.unique(arr)[1:]
        want, _ = SC.split(arr, ids=ids, min_distance=d)
        if not np.array_equal(want, SC.split(arr, ids=ids, min_distance=d, **SC.WRONG[variant])[0]):
            changed.append(name)
    assert changed, variant


def test_the_loop_bookkeeping():
    arr, d = SC.case('image_d3')
    ids = np.unique(arr)[1:]
    out, report = SC.split(arr, ids=ids, min_distance=d)
    top = int(arr.max())
    for label, new in report:      # every label of this case splits; the maximum moves after each
        assert new[0] == top + 1 and not (out == label).any()
        top = int(new[-1])
    assert out.max() == top and np.array_equal(out == 0, arr == 0)
    # start_label: accepted once, the second turn is refused; in use: every turn is refused
    out, report = SC.split(arr, ids=ids, min_distance=d, start_label=100)
    assert report[0][1][0] == 100 and all(r == 'ids in use' for _, r in report[1:])
    out, report = SC.split(arr, ids=ids, min_distance=d, start_label=int(arr.max()))
    assert all(r == 'ids in use' for _, r in report) and np.array_equal(out, arr)
    assert SC.split(arr, ids=[99], min_distance=d)[1] == [(99, 'label absent')]
    with pytest.raises(ValueError):
        SC.split(np.where(arr > 0, arr + 250, 0).astype(np.uint8), ids=[251], min_distance=d)


def test_the_sparse_helpers_of_the_package_are_the_statements():
    """labels.split_spacing and labels.split_marker_ids run on the host in the product: against ensure_spacing restated and ndi.label"""
    from empanada_napari_amd import labels as L
    rng = np.random.default_rng(0)
    for nd in (2, 3):
        for _ in range(10):
            mask = rng.random((7,) * nd) < 0.4
            coords = rng.permutation(np.argwhere(mask))
            ids, n = L.split_marker_ids(coords)
            lab, k = ndi.label(mask)
            assert n == k and np.array_equal(lab[tuple(coords.T)], ids)
            values = rng.integers(1, 4, len(coords))
            for d in (1, 2, 3):
                assert np.array_equal(coords[L.split_spacing(coords, values, d)], SC.spaced(coords, values, d))
    assert len(L.split_spacing(np.zeros((0, 3), np.int64), np.zeros(0, np.int64), 3)) == 0      # a label without any candidate
    assert L.split_marker_ids(np.zeros((0, 3), np.int64))[1] == 0
