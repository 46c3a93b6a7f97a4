"""csrc/sparse.hip against numpy / scipy at the sizes where its branches are reached: chunk scans that take a second and a third
pass, capped grids that take a second step, every 8-neighbourhood, degenerate geometries, one component across many workgroups,
a run buffer that regrows, the plain run fill (no Python caller) and the cross morphology called directly.  Inputs and references
are tests/stitch_case.py; that each input reaches its branch is asserted on the CPU in tests/test_stitch_case_host.py.
All integer: every comparison is exact.  Label values stay below 2^31 in the morphology tests (what the reference does above
that is not established here)."""
import numpy as np
import pytest
import torch

import stitch_case as SC

pytestmark = pytest.mark.gpu

LO, HI = SC.DIV, 2 * SC.DIV


def _ps():
    from empanada_napari_amd import sparse
    return sparse


def _osp():
    from oracle import sparse as osp
    return osp


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _ccl8(imgs):
    out, num = _ps().ccl8(_dev(imgs, torch.int32))
    return out.cpu().numpy(), num.cpu().numpy()


def _check_ccl8_all_ways(imgs, want, counts, junk_seed=0, lo=LO, hi=HI):
    """ccl8 on the int32 map (labels and counts) and ccl8_range on an int64 map whose background holds junk outside [lo, hi)"""
    got, num = _ccl8(imgs)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(num, counts)
    junk = SC.with_junk(imgs, lo, hi, junk_seed)
    np.testing.assert_array_equal(_ps().ccl8_range(_dev(junk, torch.int64), lo, hi).cpu().numpy(), want)


def _check_runs(got, imgs):
    assert len(got) == len(imgs)
    for g, img in zip(got, imgs):
        assert g.dtype == np.int64 and g.shape[1:] == (3,)
        np.testing.assert_array_equal(g, SC.runs_ref(img))


# ----------------------------------------------------------------------------
# A. every neighbourhood
# ----------------------------------------------------------------------------
@pytest.fixture(scope='module', params=['all_3x3', 'all_binary_3x5'])
def exhaustive(request):
    imgs = getattr(SC, request.param)()
    want, counts = SC.components_batch(imgs)
    return imgs, want, counts


def test_ccl8_every_neighbourhood(exhaustive):
    imgs, want, counts = exhaustive
    got, num = _ccl8(imgs)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(num, counts)


def test_ccl8_range_every_neighbourhood(exhaustive):
    imgs, want, _ = exhaustive
    shifted = np.where(imgs != 0, LO + imgs, 0)
    np.testing.assert_array_equal(_ps().ccl8_range(_dev(shifted, torch.int64), LO, HI).cpu().numpy(), want)
    # one of the two labels alone: the other reads as background
    only1, _ = SC.components_batch(np.where(imgs == 1, 1, 0))
    np.testing.assert_array_equal(_ps().ccl8_range(_dev(shifted, torch.int64), LO + 1, LO + 2).cpu().numpy(), only1)


# ----------------------------------------------------------------------------
# B. geometry sweep
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SC.SWEEP_2D, ids=lambda s: 'x'.join(map(str, s)))
def test_geometry_sweep_2d(shape):
    imgs = SC.sweep_images(shape)
    want = np.stack([_osp().label_nd(m) for m in imgs])
    _check_ccl8_all_ways(imgs, want, want.reshape(len(imgs), -1).max(axis=1), junk_seed=shape[1])
    _check_runs(_ps().extract_runs(_dev(imgs, torch.int32)), imgs)
    junk = SC.with_junk(imgs, LO, HI, shape[0])
    _check_runs(_ps().extract_runs(_dev(junk, torch.int64), lo=LO, hi=HI), imgs)


# ----------------------------------------------------------------------------
# C. multi-pass scans and strided loops
# ----------------------------------------------------------------------------
@pytest.fixture(scope='module', params=['multipass_513', 'multipass_1025'])
def multipass(request):
    imgs = getattr(SC, request.param)()
    want = np.stack([_osp().label_nd(m) for m in imgs])
    return request.param, imgs, want


def test_multipass_ccl8(multipass):
    _, imgs, want = multipass
    _check_ccl8_all_ways(imgs, want, want.reshape(len(imgs), -1).max(axis=1), lo=LO, hi=3 * SC.DIV)      # both classes
    want1 = np.stack([_osp().label_nd(SC.in_range(m, LO, HI)) for m in imgs])         # class 1 of the two-class map
    np.testing.assert_array_equal(_ps().ccl8_range(_dev(imgs, torch.int64), LO, HI).cpu().numpy(), want1)


def test_multipass_extract_runs_regrows(multipass):
    _, imgs, want = multipass
    _check_runs(_ps().extract_runs(_dev(imgs, torch.int32)), imgs)                      # default max_runs: 65 536
    _check_runs(_ps().extract_runs(_dev(want, torch.int32)), want)                      # runs of the components
    _check_runs(_ps().extract_runs(_dev(imgs, torch.int64), lo=LO, hi=HI), [SC.in_range(m, LO, HI) for m in imgs])


def test_multipass_force_connected(multipass):
    _, imgs, _ = multipass
    got = _ps().force_connected(_dev(imgs, torch.int64), [1, 2], SC.DIV).cpu().numpy()
    for n in range(len(imgs)):
        np.testing.assert_array_equal(got[n], SC.force_connected_ref(imgs[n], [1, 2], SC.DIV))


def test_multipass_pan_seg_to_rle_seg():
    pan = SC.multipass_513()[0]
    got = _ps().pan_seg_to_rle_seg(pan, [1, 2], SC.DIV, [1])
    want = SC.rle_seg_ref(pan, [1, 2], SC.DIV, [1])
    assert list(got) == list(want)
    for c in want:
        assert list(got[c]) == list(want[c])
        assert [tuple(a['box']) for a in got[c].values()] == [tuple(a['box']) for a in want[c].values()]
        for k in ('starts', 'runs'):
            np.testing.assert_array_equal(np.concatenate([a[k] for a in got[c].values()]),
                                          np.concatenate([a[k] for a in want[c].values()]))
            assert [len(a[k]) for a in got[c].values()] == [len(a[k]) for a in want[c].values()]


# ----------------------------------------------------------------------------
# D. one component across many workgroups
# ----------------------------------------------------------------------------
def _timed_ccl8(name, img, count):
    """correctness only; the device time of a second call is printed for FINDINGS.md (no assertion on it)"""
    want = _osp().label_nd(img)
    assert int(want.max()) == count
    d = _dev(img[None], torch.int32)
    out, num = _ps().ccl8(d)
    np.testing.assert_array_equal(out[0].cpu().numpy(), want)
    assert int(num[0]) == count
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    _ps().ccl8(d)
    t1.record()
    t1.synchronize()
    print(f'\nccl8 {name} {img.shape[0]}x{img.shape[1]}: {t0.elapsed_time(t1):.3f} ms on the device')


@pytest.mark.parametrize('name,gen,count', SC.ADVERSARIAL, ids=[a[0] for a in SC.ADVERSARIAL])
def test_one_component_across_workgroups(name, gen, count):
    _timed_ccl8(name, gen(257, 259), count)


@pytest.mark.parametrize('shape', [(4099, 1), (4099, 3)], ids=['4099x1', '4099x3'])
def test_vertical_line(shape):
    _timed_ccl8('vertical line', SC.vertical_line(*shape), 1)


# ----------------------------------------------------------------------------
# E. ccl26
# ----------------------------------------------------------------------------
def _ccl26(vol, dtype=torch.int32, lo=None, hi=None):
    return _ps().ccl26(_dev(vol, dtype), lo, hi).cpu().numpy()


def test_ccl26_every_2x2x2_neighbourhood():
    vol = SC.mosaic_2x2x2()
    np.testing.assert_array_equal(_ccl26(vol), _osp().label_nd(vol))


@pytest.mark.parametrize('shape', SC.SWEEP_3D, ids=lambda s: 'x'.join(map(str, s)))
def test_geometry_sweep_3d(shape):
    for k, vol in enumerate(SC.sweep_volumes(shape)):
        want = _osp().label_nd(vol)
        np.testing.assert_array_equal(_ccl26(vol), want)
        np.testing.assert_array_equal(_ccl26(SC.with_junk(vol, LO, HI, k), torch.int64, LO, HI), want)


@pytest.fixture(scope='module')
def strided():
    vol = SC.strided_volume()
    return vol, _osp().label_nd(vol), _osp().label_nd(SC.in_range(vol, 3, 4))


def test_ccl26_strided_volume(strided):
    vol, want, _ = strided
    np.testing.assert_array_equal(_ccl26(vol), want)


@pytest.mark.parametrize('dtype', [torch.int64, torch.int32], ids=['int64', 'int32'])
def test_ccl26_range_strided_volume(strided, dtype):
    vol, want, want3 = strided
    np.testing.assert_array_equal(_ccl26(vol, dtype, 3, 5), want)
    np.testing.assert_array_equal(_ccl26(vol, dtype, 3, 4), want3)


def test_volume_to_instances_runs_cross_rows_and_planes():
    vol = SC.blobs((2, 3, 2049), 14, 0.2, 41)
    vol[:, :, :3] = vol[:, :, -3:] = vol[0, 0, :] = 1002      # one component whose runs go over every row end and the plane end
    got = _ps().volume_to_instances(vol, [1, 2], SC.DIV, [1])
    want = _osp().filters_pan_seg_to_rle_seg(vol, [1, 2], SC.DIV, [1])
    assert list(got) == list(want) and len(want) > 10
    crossing = np.zeros(2, int)
    for k in want:
        assert tuple(got[k]['box']) == tuple(want[k]['box']), k
        np.testing.assert_array_equal(got[k]['starts'], want[k]['starts'])
        np.testing.assert_array_equal(got[k]['runs'], want[k]['runs'])
        s, e = want[k]['starts'], want[k]['starts'] + want[k]['runs'] - 1
        crossing += np.array([int((s // 2049 != e // 2049).sum()), int((s // (3 * 2049) != e // (3 * 2049)).sum())])
    assert crossing[0] >= 5 and crossing[1] >= 1               # rows, planes


# ----------------------------------------------------------------------------
# F. run extraction edges
# ----------------------------------------------------------------------------
def test_every_pixel_a_run_and_one_run_for_all():
    y, x = np.indices((70, 67))
    img = 1 + (y * 67 + x) % 2
    runs = _ps().extract_runs(_dev(img[None], torch.int32))[0]
    assert len(runs) == 70 * 67
    np.testing.assert_array_equal(runs, SC.runs_ref(img))
    one = SC.full((1, 1025, 1031), 7)
    assert _ps().extract_runs(_dev(one, torch.int32))[0].tolist() == [[0, 1025 * 1031, 7]]


def test_runs_at_thread_chunk_and_image_boundaries():
    imgs = SC.boundary_runs()
    _check_runs(_ps().extract_runs(_dev(imgs, torch.int32)), imgs)


@pytest.mark.parametrize('max_runs', [1, 4, 1000])
def test_max_runs_does_not_change_the_result(max_runs):
    imgs = SC.max_runs_batch()
    d = _dev(imgs, torch.int32)
    want = _ps().extract_runs(d, max_runs=1 << 20)
    _check_runs(want, imgs)
    got = _ps().extract_runs(d, max_runs=max_runs)
    assert len(got) == 3
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_range_reads_negative_and_wide_values_as_background():
    imgs = SC.sweep_images((70, 67))
    junk = SC.with_junk(imgs, LO, HI, 1)
    _check_runs(_ps().extract_runs(_dev(junk, torch.int64), lo=LO, hi=HI), imgs)
    _check_runs(_ps().extract_runs(_dev(junk, torch.int64), lo=LO + 1, hi=LO + 2), np.where(imgs == LO + 1, imgs, 0))


# ----------------------------------------------------------------------------
# G. run fills
# ----------------------------------------------------------------------------
_TORCH = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _rle_fill(starts, lens, vals, dvol, size):
    from empanada_napari_amd import _abi
    ds, dl, dv = (_dev(a, torch.int64) for a in (starts, lens, vals))
    _abi.check(_abi.load().emp_rle_fill(_abi.ptr(ds), _abi.ptr(dl), _abi.ptr(dv), len(starts), _abi.ptr(dvol), size,
                                        dvol.element_size(), _abi.stream_ptr(dvol.device)), 'emp_rle_fill')
    torch.cuda.synchronize()


@pytest.fixture(scope='module')
def fill_case():
    starts, lens, vals, size = SC.fill_runs()
    want = np.full(size, 77, np.int64)                              # what the runs do not cover keeps its content
    want[SC.run_indices(starts, lens)] = np.repeat(vals, lens)
    return starts, lens, vals, size, want


@pytest.mark.parametrize('elem_bytes', [1, 2, 4, 8])
def test_rle_fill_direct(fill_case, elem_bytes):
    starts, lens, vals, size, want = fill_case
    dvol = torch.full((size,), 77, dtype=_TORCH[elem_bytes], device='cuda')
    _rle_fill(starts, lens, vals, dvol, size)
    np.testing.assert_array_equal(dvol.cpu().numpy().astype(np.int64), want)


@pytest.mark.parametrize('elem_bytes', [1, 2, 4, 8])
def test_rle_fill_stops_at_size(elem_bytes):
    """a run whose end exceeds ``size`` is cut there (min(size, start + length)): the allocation is 64 elements longer"""
    size = 5000
    starts, lens, vals = np.array([10, size - 130, size - 10], np.int64), np.array([70, 65, 50], np.int64), np.array([3, 4, 5], np.int64)
    dvol = torch.full((size + 64,), 77, dtype=_TORCH[elem_bytes], device='cuda')
    _rle_fill(starts, lens, vals, dvol, size)
    want = np.full(size + 64, 77, np.int64)
    want[10:80], want[size - 130:size - 65], want[size - 10:size] = 3, 4, 5
    np.testing.assert_array_equal(dvol.cpu().numpy().astype(np.int64), want)


@pytest.mark.parametrize('dtype', [np.uint8, np.int32, np.int64])
def test_fill_volume_overlapping_instances(dtype):
    shape = (16, 256, 256)
    inst = SC.overlapping_instances(shape)
    want = SC.fill_ref(np.zeros(shape, dtype), inst)
    for _ in range(3):                                              # deterministic, not a lucky race
        np.testing.assert_array_equal(_ps().fill_volume(np.zeros(shape, dtype), inst), want)


# ----------------------------------------------------------------------------
# H. the cross morphology, directly
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 5, 7), (3, 1, 9), (4, 6, 1), SC.VOLUME_SHAPE], ids=lambda s: 'x'.join(map(str, s)))
def test_morph_cross3d_direct(shape):
    from empanada_napari_amd import _abi
    vol = SC.noise(shape, (0, 5, 9, 1000003, (1 << 31) - 1), seed=shape[1])
    a = _dev(vol, torch.int32)
    D, H, W = shape
    for op in (0, 1):
        b = torch.full_like(a, -1)
        _abi.check(_abi.load().emp_morph_cross3d(_abi.ptr(a), _abi.ptr(b), D, H, W, op, _abi.stream_ptr(a.device)),
                   'emp_morph_cross3d')
        np.testing.assert_array_equal(b.cpu().numpy().astype(np.int64), SC.cross_morph_ref(vol, op))
