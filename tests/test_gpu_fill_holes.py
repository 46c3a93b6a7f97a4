"""Device side of Fill holes (csrc/morph.hip, emp_fill_holes_labels) through empanada_napari_amd.labels.fill_label_holes.  The
expected values are the scipy statement of the reference's loop (tests/fill_holes_case.py), computed once per case and shared.
Everything is integer, so every comparison is exact."""
import functools
import itertools

import numpy as np
import pytest

import fill_holes_case as FC

pytestmark = pytest.mark.gpu

RADII = (1, 3, 7)
HOLE_SIZES = (1, 8, 64, 10 ** 6)


def _dev(x):
    import torch
    if x.dtype in (np.uint16, np.uint32):      # no arithmetic is needed on the tensor: reinterpret the bytes
        return torch.from_numpy(x.view({2: np.int16, 4: np.int32}[x.itemsize])).cuda().view({2: torch.uint16, 4: torch.uint32}[x.itemsize])
    return torch.from_numpy(x).cuda()


def _host(t):
    import torch
    if t.dtype in (torch.uint16, torch.uint32):
        return t.view({torch.uint16: torch.int16, torch.uint32: torch.int32}[t.dtype]).cpu().numpy().view(
            {torch.uint16: np.uint16, torch.uint32: np.uint32}[t.dtype])
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(name):
    arr = {'image': lambda: FC.holes((96, 96), 40, 11),
           'volume': lambda: FC.holes((24, 40, 40), 30, 13),
           'w67': lambda: FC.holes((45, 67), 14, 13),
           'flat': lambda: FC.holes((5, 9, 130), 12, 14)}[name]()
    arr.setflags(write=False)
    return arr


@functools.lru_cache(maxsize=None)
def _want(name, radius, hole_size):
    out, skipped = FC.fill(_case(name), radius, hole_size)
    out.setflags(write=False)
    return out, skipped


def _run(arr, radius, hole_size, **kw):
    from empanada_napari_amd import labels as L
    return _host(L.fill_label_holes(_dev(np.array(arr)), hole_size=hole_size, radius=radius, apply3d=arr.ndim == 3, **kw))


def _check(arr, radius, hole_size, **kw):
    want, _ = FC.fill(arr, radius, hole_size, **kw)
    got = _run(arr, radius, hole_size, **kw)
    assert np.array_equal(got, want), (radius, hole_size, int((got != want).sum()))
    return got


@pytest.mark.parametrize('name,radius,hole_size', itertools.product(('image', 'volume'), RADII, HOLE_SIZES))
def test_main_shapes(name, radius, hole_size):
    """other labels inside small components are overwritten, labels disappear and their turns are skipped, whole crops fill
    (tests/test_fill_holes_host.py says that these inputs have all of that)"""
    want, _ = _want(name, radius, hole_size)
    got = _run(_case(name), radius, hole_size)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got, _case(name)) == (hole_size == 1)


@pytest.mark.parametrize('name,radius,hole_size', itertools.product(('w67', 'flat'), RADII, HOLE_SIZES))
def test_word_and_tile_tails(name, radius, hole_size):
    """W = 67: a row of tiles ends three voxels into its second tile; (5, 9, 130): a row over three tiles, a frame shorter than a
    tile along z and y, and from radius 3 on a pad that is taller than the array"""
    want, _ = _want(name, radius, hole_size)
    got = _run(_case(name), radius, hole_size)
    assert np.array_equal(got, want), int((got != want).sum())


def test_the_wrong_variants_differ():
    """connectivity 2, `<=`, the whole array instead of the crop, crops from the original boxes: none of them can pass"""
    arr = _case('image')
    got = _run(arr, 1, 64)
    assert np.array_equal(got, _want('image', 1, 64)[0])
    for wrong in (FC.fill_connectivity2, FC.fill_le, FC.fill_whole_array, FC.fill_original_boxes):
        assert not np.array_equal(got, wrong(arr, 1, 64)), wrong.__name__
    vol = _case('volume')
    assert not np.array_equal(_run(vol, 1, 64), FC.fill_connectivity2(vol, 1, 64))
    assert not np.array_equal(_run(vol, 1, 8), FC.fill_le(vol, 1, 8))
    assert not np.array_equal(_run(vol, 3, 10 ** 6), FC.fill_original_boxes(vol, 3, 10 ** 6))


def test_the_threshold_across_tiles():
    """one hole over many tiles: its size is the sum over all of them, and the comparison is strict"""
    img = np.zeros((150, 200), np.int32)
    img[5:145, 5:195] = 5
    img[8:142, 8:192] = 0
    assert (img[8:142, 8:192] == 0).sum() == 24656
    assert (_check(img, 1, 24656)[8:142, 8:192] == 0).all()
    assert (_check(img, 1, 24657)[8:142, 8:192] == 5).all()
    vol = np.zeros((10, 24, 150), np.int32)
    vol[1:9, 2:22, 3:147] = 7
    vol[2:8, 3:21, 4:146] = 0
    assert (vol[2:8, 3:21, 4:146] == 0).sum() == 15336
    assert (_check(vol, 1, 15336)[2:8, 3:21, 4:146] == 0).all()
    assert (_check(vol, 1, 15337)[2:8, 3:21, 4:146] == 7).all()


def test_a_long_thin_component():
    """a serpentine of 2 127 voxels through three tiles per row: one component, a deep union-find tree"""
    img = np.zeros((40, 140), np.int32)
    img[2:38, 2:138] = 9
    rows = list(range(4, 35, 2))
    for k, y in enumerate(rows):
        img[y, 4:136] = 0
        if k + 1 < len(rows):
            img[y + 1, 135 if k % 2 == 0 else 4] = 0
    snake = (img == 0) & (np.pad(np.ones((36, 136), bool), 2))
    assert snake.sum() == 2127
    assert (_check(img, 2, 2127)[snake] == 0).all()
    assert (_check(img, 2, 2128)[snake] == 9).all()


def test_no_diagonals():
    img = np.zeros((12, 12), np.int32)
    img[2:9, 2:9] = 3
    img[3:8, 3:8] = 0
    img[2, 2] = 0      # the hole's corner voxel (3, 3) touches the outside diagonally only
    got = _check(img, 1, 30)
    assert (got[3:8, 3:8] == 3).all() and got[2, 2] == 0
    assert not np.array_equal(got, FC.fill_connectivity2(img, 1, 30))


def test_degenerate_arrays():
    for shape in ((23, 70), (6, 11, 70)):
        full = np.full(shape, 7, np.int32)      # one label filling the array: no background at all
        empty = np.zeros(shape, np.int32)       # no label at all
        corner = np.zeros(shape, np.int32)
        corner[(0,) * len(shape)] = 5           # a single voxel in the first corner
        far = np.zeros(shape, np.int32)
        far[tuple(s - 1 for s in shape)] = 9    # ... and in the last one
        for arr, radius in itertools.product((full, empty, corner, far), (1, 4)):
            got = _check(arr, radius, 64)
            if arr is full or arr is empty:
                assert np.array_equal(got, arr)
    img = np.zeros((23, 70), np.int32)
    img[0, 0] = 5
    assert (_run(img, 4, 64)[:5, :5] == 5).all()      # the whole crop fills: 24 voxels of background


def test_ids_in_any_order_with_repeats_zeros_and_absent_ids():
    for name in ('image', 'volume'):
        arr = _case(name)
        present = np.unique(arr)[1:]
        ids = list(present[::-1][:12]) + [0, int(present.max()) + 9, int(present[-2]), int(present[-2]), 0, int(present[3])]
        for radius, hole_size in ((2, 64), (3, 10 ** 6)):
            _check(arr, radius, hole_size, ids=ids)
    assert np.array_equal(_run(_case('image'), 2, 64, ids=[0, 10 ** 6]), _case('image'))      # nothing to do


@pytest.mark.parametrize('axis', [0, 2])
def test_plane_of_a_volume(axis):
    from empanada_napari_amd import labels as L
    vol = _case('volume')
    plane = vol.shape[axis] // 2
    want = FC.fill_plane(vol, 2, 64, plane, axis)
    got = _host(L.fill_label_holes(_dev(np.array(vol)), hole_size=64, radius=2, plane=plane, axis=axis))
    assert np.array_equal(got, want)
    other = [k for k in range(vol.shape[axis]) if k != plane]
    assert np.array_equal(np.take(got, other, axis), np.take(vol, other, axis))
    assert not np.array_equal(np.take(got, plane, axis), np.take(vol, plane, axis))
    ids = np.unique(np.take(vol, plane, axis))[1:][::-1][:5]
    want = FC.fill_plane(vol, 3, 10 ** 6, plane, axis, ids=ids)
    assert np.array_equal(L.fill_label_holes(np.array(vol), hole_size=10 ** 6, radius=3, plane=plane, axis=axis, ids=ids), want)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.int32, np.int64])
def test_dtypes(dtype):
    from empanada_napari_amd import labels as L
    for name in ('w67', 'flat'):
        arr = _case(name)
        if dtype == np.uint8:      # the fresh ids from 1000 on as ids that fit
            arr = np.where(arr >= 1000, arr - 1000 + 200, arr)
        arr = arr.astype(dtype)
        if dtype == np.int64:
            arr = np.where(arr > 0, arr + (1 << 40), 0)      # labels above 2^32
        for radius, hole_size in ((1, 64), (2, 10 ** 6)):
            want, _ = FC.fill(arr, radius, hole_size)
            got = L.fill_label_holes(arr, hole_size=hole_size, radius=radius, apply3d=arr.ndim == 3)
            assert got.dtype == dtype and np.array_equal(got, want) and not np.array_equal(got, arr)
            assert np.array_equal(_run(arr, radius, hole_size), want)
    if dtype == np.int64:
        assert arr.max() > 1 << 32


def test_return_kinds():
    import torch
    from empanada_napari_amd import labels as L
    arr = np.array(_case('image'))
    want, _ = _want('image', 3, 64)
    t = _dev(arr)
    res = L.fill_label_holes(t, hole_size=64, radius=3)
    assert isinstance(res, torch.Tensor) and res.is_cuda and res.data_ptr() != t.data_ptr()
    assert np.array_equal(_host(res), want) and np.array_equal(_host(t), arr)      # the caller's tensor is not written
    same = L.fill_label_holes(t, hole_size=64, radius=3, inplace=True)
    assert same is t and np.array_equal(_host(t), want)
    new = L.fill_label_holes(arr, hole_size=64, radius=3)
    assert isinstance(new, np.ndarray) and new is not arr and np.array_equal(new, want) and np.array_equal(arr, _case('image'))
    mine = arr.copy()
    assert L.fill_label_holes(mine, hole_size=64, radius=3, inplace=True) is mine and np.array_equal(mine, want)
    view = np.zeros((96, 200), arr.dtype)[:, 3:99]      # a view that is not contiguous, edited in place
    view[...] = arr
    assert L.fill_label_holes(view, hole_size=64, radius=3, inplace=True) is view and np.array_equal(view, want)
    # hole_size 0 and 1 change nothing and come back as the same kinds
    for hole_size in (0, 1):
        unchanged = L.fill_label_holes(arr, hole_size=hole_size)
        assert unchanged is not arr and np.array_equal(unchanged, arr)
    # out= is for chunked stores, as in morph_labels: arrays and tensors come back as what they are
    for x in (arr, t):
        with pytest.raises(TypeError, match='out='):
            L.fill_label_holes(x, hole_size=64, radius=3, out=np.empty_like(arr))


def test_statistics_and_scratch_follow_the_boxes_not_the_array():
    """one small label picked in a large image: the work arrays hold its padded box"""
    import torch
    from empanada_napari_amd import labels as L
    img = np.zeros((1500, 1500), np.int32)
    img[700:720, 900:930] = 4
    img[705:710, 905:910] = 0
    img[10:400, 10:400] = 8
    t = torch.from_numpy(img).cuda()
    stats = L._fill_device(t, -4, img.shape, 2, 64, False, [4], t.device)
    assert stats['scratch_entries'] == 24 * 34 and stats['levels'] == 1 and stats['launches'] == 4 and stats['tiles'] == 1
    assert np.array_equal(t.cpu().numpy(), FC.fill(img, 2, 64, ids=[4])[0])
    assert L._fill_device(t, -4, img.shape, 2, 64, False, [5], t.device)['launches'] == 0      # an absent id: nothing to launch


def test_two_runs_are_bit_identical():
    for name, radius, hole_size in (('image', 3, 64), ('volume', 1, 10 ** 6)):
        a = _run(_case(name), radius, hole_size)
        b = _run(_case(name), radius, hole_size)
        assert a.tobytes() == b.tobytes()


def test_clean_labels_tool_fill_holes_mode(tmp_path, capsys):
    """tools/clean_labels.py --fill-holes on a small .npy: the JSON line and the file written"""
    import importlib.util
    import json
    import os
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'clean_labels.py')
    spec = importlib.util.spec_from_file_location('_clean_labels_fill', tool)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def run(*argv):
        capsys.readouterr()
        res = mod.main([str(a) for a in argv])
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
        return res

    img, vol = _case('w67'), _case('flat')
    src, dst = tmp_path / 'in.npy', tmp_path / 'out.npy'
    np.save(src, img)
    n = len(np.unique(img)) - 1
    assert run(src, dst, '--fill-holes', 10 ** 6, '--radius', 3) == {'shape': list(img.shape), 'labels_affected': n, 'out': str(dst)}
    assert np.array_equal(np.load(dst), _want('w67', 3, 10 ** 6)[0]) and np.array_equal(np.load(src), img)
    np.save(src, vol)
    assert run(src, dst, '--fill-holes', '--3d')['labels_affected'] == len(np.unique(vol)) - 1      # defaults: 64 voxels, radius 1
    assert np.array_equal(np.load(dst), _want('flat', 1, 64)[0])
