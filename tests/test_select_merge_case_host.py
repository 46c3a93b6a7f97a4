"""tests/select_merge_case.py checked on the CPU alone: its two constants are the ones of csrc/pointrend.hip, the inputs of the
GPU A/B test (tests/test_gpu_select_merge_ab.py) reach the fast path, the overflow path and both sides of the candidate
buffer's capacity, and the numpy model of the two-read select returns the array the contract asks for."""
import os
import re

import numpy as np
import pytest

import pointrend_case as PC
import select_merge_case as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'empanada-napari_amd', 'csrc', 'pointrend.hip')


def _constant(name):
    with open(SOURCE) as f:
        m = re.findall(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, f.read())
    assert len(m) == 1, f'{name}: {len(m)} definitions in pointrend.hip'
    return int(m[0])


def test_constants_mirror_the_source():
    assert SM.SEL_BITS == _constant('SEL_BITS')
    assert SM.SEL_CAP == _constant('SEL_CAP')
    assert PC.CHUNK == _constant('CHUNK')
    assert SM.SEL_SHIFT + SM.SEL_BITS == 31 and sum(b for _, b in SM.LEVELS) == 31      # bit 31 of a key is never set
    assert SM.SEL_CAP % 256 == 0      # sel_resolve_kernel holds SEL_CAP / 256 candidates per thread


def test_inputs_reach_both_paths():
    plane = 530437
    pops = {d: SM.threshold_bin(PC.topk_keys(d, plane), 8192)[2] for d in PC.topk_dists(plane)}
    for d in ('random', 'straddle', 'with_inf', 'byte3'):
        assert 1 <= pops[d] <= SM.SEL_CAP, (d, pops[d])
    for d in ('byte2', 'all_equal', 'all_zero', 'byte0', 'byte1', 'two_valued'):
        assert pops[d] > SM.SEL_CAP, (d, pops[d])
    for d in ('all_equal', 'all_zero', 'byte0', 'byte1'):
        assert pops[d] == plane                                                          # the whole plane in one bin
    keys = PC.topk_keys('with_inf', plane)
    assert SM.path_of(keys, plane - 1) == 'overflow'                                     # the bin of +inf
    # below SEL_CAP + 1 keys nothing can overflow; the smallest plane that does
    assert all(SM.path_of(PC.topk_keys(d, p), k) != 'overflow'
               for p in PC.TOPK_PLANES if p <= SM.SEL_CAP for d in PC.topk_dists(p) for k in SM.select_ks(d, PC.topk_keys(d, p)))
    assert SM.path_of(PC.topk_keys('all_equal', 16384), 1) == 'overflow'


def test_boundary_inputs_sit_on_the_capacity():
    for n_cand, path in ((SM.SEL_CAP, 'fast'), (SM.SEL_CAP + 1, 'overflow')):
        keys, k = SM.boundary_keys(n_cand)
        b, krem, pop = SM.threshold_bin(keys, k)
        assert pop == n_cand and 1 <= krem <= pop and SM.path_of(keys, k) == path
        assert len(keys) % 4 != 0
        t = np.sort(keys)[k - 1]
        assert (keys == t).sum() > k - (keys < t).sum() >= 1, 'k must cut a tied group'


def test_mixed_batch_overflows_in_the_middle_only():
    for plane in SM.MIXED_PLANES:
        keys = SM.mixed_batch(plane)
        for k in (1, min(8192, plane), plane - 1):
            paths = [SM.path_of(row, k) for row in keys]
            assert paths[1] == 'overflow', (plane, k, paths)
        assert [SM.path_of(row, min(8192, plane)) for row in keys] == ['fast', 'overflow', 'fast']


@pytest.mark.parametrize('dist,plane', PC.topk_cases(), ids=lambda v: str(v))
def test_model_equals_the_reference(dist, plane):
    keys = PC.topk_keys(dist, plane)
    for k in SM.select_ks(dist, keys):
        got, _ = SM.select2_model(keys, k)
        np.testing.assert_array_equal(got, SM.ordered_ref(keys, k))
        np.testing.assert_array_equal(np.sort(got), PC.topk_ref(keys, k)[0])


def test_model_equals_the_reference_on_the_boundary():
    for n_cand in (SM.SEL_CAP, SM.SEL_CAP + 1):
        keys, k = SM.boundary_keys(n_cand)
        got, path = SM.select2_model(keys, k)
        assert path == ('fast' if n_cand == SM.SEL_CAP else 'overflow')
        np.testing.assert_array_equal(got, SM.ordered_ref(keys, k))
        np.testing.assert_array_equal(np.sort(got), PC.topk_ref(keys, k)[0])


def test_merge_inputs_cover_their_cases():
    for H, W in SM.MERGE_SHAPES:
        for C in SM.MERGE_CLASSES:
            for max_ids in SM.MERGE_MAX_IDS:
                sem, cells = SM.merge_input(H, W, C, max_ids)
                assert sem.shape == (SM.MERGE_N + 1, C, H, W) and cells.shape == (SM.MERGE_N + 1, H, W)
                assert (cells == 0).any() and (cells > max_ids).any() and cells.min() >= 0
                if max_ids:
                    assert ((cells > 0) & (cells <= max_ids)).any()
    assert [h * w % 4 for h, w in SM.MERGE_SHAPES] == [3, 3, 0]      # two planes off the vector path, one on it
    sem, _ = SM.merge_input(64, 64, 3, 300)
    cls = sem.argmax(1)
    n1, n2 = int((cls[2] == 2).sum()), int((cls[3] == 2).sum())
    assert n1 < 64 < n2, (n1, n2)      # stuff_area = 64 falls between the two images' counts of class 2
