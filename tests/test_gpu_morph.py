"""Device side of Morph Labels (csrc/morph.hip) through empanada_napari_amd.labels.morph_labels.  The expected values are the
scipy statement of the reference's loop (tests/morph_case.py), computed once per case and shared.  Everything is integer, so
every comparison is exact."""
import functools
import itertools

import numpy as np
import pytest

import morph_case as MC

pytestmark = pytest.mark.gpu

RADII = (1, 3, 7)


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
    arr = {'image': lambda: MC.blobs((96, 96), 40, 11),
           'volume': lambda: MC.blobs((24, 40, 40), 30, 13),
           'w67': lambda: MC.blobs((45, 67), 14, 13),
           'flat': lambda: MC.blobs((5, 9, 130), 12, 14)}[name]()
    arr.setflags(write=False)
    return arr


@functools.lru_cache(maxsize=None)
def _want(name, operation, radius):
    out, skipped = MC.morph(_case(name), operation, radius)
    out.setflags(write=False)
    return out, skipped


def _run(arr, operation, radius, **kw):
    from empanada_napari_amd import labels as L
    return _host(L.morph_labels(_dev(np.array(arr)), operation, radius=radius, apply3d=arr.ndim == 3, **kw))


@pytest.mark.parametrize('name,operation,radius', itertools.product(('image', 'volume'), MC.OPS, RADII))
def test_main_shapes(name, operation, radius):
    want, _ = _want(name, operation, radius)
    got = _run(_case(name), operation, radius)
    assert np.array_equal(got, want), int((got != want).sum())


def test_main_shapes_have_what_they_are_for():
    """deep schedules and, at radius 3, a label that is eaten before its turn under Dilate (skipped, not an error)"""
    from empanada_napari_amd import labels as L
    import labels_case as LC
    for name in ('image', 'volume'):
        arr = _case(name)
        assert _want(name, 'Dilate', 3)[1] >= 1
        labels, areas, boxes = LC.want_table(arr)
        t = L.table_from_arrays(labels, areas, boxes, arr.shape)
        assert len(L.morph_schedule(t, labels[labels != 0], 3, 'Dilate')) >= 5
        # a label that touches the border, for the erosion's border rule
        nd = arr.ndim
        assert (((boxes[:, :nd] == 0) | (boxes[:, nd:] == np.asarray(arr.shape))).any(axis=1) & (labels != 0)).any()


@pytest.mark.parametrize('name,operation,radius', itertools.product(('w67', 'flat'), MC.OPS, RADII))
def test_word_tails_and_a_ball_taller_than_the_array(name, operation, radius):
    """W = 67: a row of tiles ends three voxels into its last word; (5, 9, 130): a mask row over three words, and from radius
    3 on a ball that is taller than the array"""
    want, _ = _want(name, operation, radius)
    got = _run(_case(name), operation, radius)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize('operation', MC.OPS)
def test_border_rules(operation):
    for shape in ((23, 70), (6, 11, 70)):
        full = np.full(shape, 7, np.int32)      # one label filling the array: erosion sees true beyond every face
        corner = np.zeros(shape, np.int32)
        corner[(0,) * len(shape)] = 5           # a single voxel in a corner
        far = np.zeros(shape, np.int32)
        far[tuple(s - 1 for s in shape)] = 9
        for arr, radius in itertools.product((full, corner, far), (1, 4)):
            want, _ = MC.morph(arr, operation, radius)
            assert np.array_equal(_run(arr, operation, radius), want), (shape, radius)
    assert np.array_equal(MC.morph(np.full((9, 9), 7, np.int32), 'Erode', 2)[0], np.full((9, 9), 7))      # not eroded from outside


def test_close_inside_the_crop_is_not_whole_image_closing():
    arr = _case('image')
    want, _ = _want('image', 'Close', 3)
    whole = MC.morph_whole_image(arr, 'Close', 3)
    assert (want != whole).sum() > 0      # the statement itself depends on the crop: ignoring the rule cannot pass
    got = _run(arr, 'Close', 3)
    assert np.array_equal(got, want) and not np.array_equal(got, whole)


@pytest.mark.parametrize('operation', MC.OPS)
def test_ids_in_any_order_with_repeats_zeros_and_absent_ids(operation):
    for name in ('image', 'volume'):
        arr = _case(name)
        present = np.unique(arr)[1:]
        ids = list(present[::-1][:12]) + [0, int(present.max()) + 9, int(present[-2]), int(present[-2]), 0, int(present[3])]
        want, _ = MC.morph(arr, operation, 2, ids=ids)
        assert np.array_equal(_run(arr, operation, 2, ids=ids), want)
    assert np.array_equal(_run(_case('image'), operation, 2, ids=[0, 10 ** 6]), _case('image'))      # nothing to do


@pytest.mark.parametrize('axis', [0, 2])
def test_plane_of_a_volume(axis):
    from empanada_napari_amd import labels as L
    vol = _case('volume')
    plane = vol.shape[axis] // 2
    for operation in ('Dilate', 'Open'):
        want = MC.morph_plane(vol, operation, 2, plane, axis)
        got = _host(L.morph_labels(_dev(np.array(vol)), operation, radius=2, plane=plane, axis=axis))
        assert np.array_equal(got, want)
        other = [k for k in range(vol.shape[axis]) if k != plane]
        assert np.array_equal(np.take(got, other, axis), np.take(vol, other, axis))
        assert not np.array_equal(np.take(got, plane, axis), np.take(vol, plane, axis))
    ids = np.unique(np.take(vol, plane, axis))[1:][::-1][:5]
    want = MC.morph_plane(vol, 'Close', 3, plane, axis, ids=ids)
    assert np.array_equal(L.morph_labels(np.array(vol), 'Close', radius=3, plane=plane, axis=axis, ids=ids), want)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.int32, np.int64])
def test_dtypes(dtype):
    from empanada_napari_amd import labels as L
    for name in ('w67', 'flat'):
        arr = _case(name).astype(dtype)
        if dtype == np.int64:
            arr = np.where(arr > 0, arr + (1 << 40), 0)      # labels above 2^32
        for operation in ('Dilate', 'Open'):
            want, _ = MC.morph(arr, operation, 2)
            got = L.morph_labels(arr, operation, radius=2, apply3d=arr.ndim == 3)
            assert got.dtype == dtype and np.array_equal(got, want)
            assert np.array_equal(_run(arr, operation, 2), want)
    if dtype == np.int64:
        assert arr.max() > 1 << 32


def test_return_kinds():
    import torch
    from empanada_napari_amd import labels as L
    arr = np.array(_case('image'))
    want, _ = _want('image', 'Dilate', 3)
    t = _dev(arr)
    res = L.morph_labels(t, 'Dilate', radius=3)
    assert isinstance(res, torch.Tensor) and res.is_cuda and res.data_ptr() != t.data_ptr()
    assert np.array_equal(_host(res), want) and np.array_equal(_host(t), arr)      # the caller's tensor is not written
    same = L.morph_labels(t, 'Dilate', radius=3, inplace=True)
    assert same is t and np.array_equal(_host(t), want)
    new = L.morph_labels(arr, 'Dilate', radius=3)
    assert isinstance(new, np.ndarray) and new is not arr and np.array_equal(new, want) and np.array_equal(arr, _case('image'))
    mine = arr.copy()
    assert L.morph_labels(mine, 'Dilate', radius=3, inplace=True) is mine and np.array_equal(mine, want)
    view = np.zeros((96, 200), arr.dtype)[:, 3:99]      # a view that is not contiguous, edited in place
    view[...] = arr
    assert L.morph_labels(view, 'Dilate', radius=3, inplace=True) is view and np.array_equal(view, want)
    # out= is for chunked stores, as in delete_labels: arrays and tensors come back as what they are
    for x in (arr, t):
        with pytest.raises(TypeError, match='out='):
            L.morph_labels(x, 'Dilate', radius=3, out=np.empty_like(arr))


def test_two_runs_are_bit_identical():
    for name, operation in (('image', 'Close'), ('volume', 'Dilate')):
        a = _run(_case(name), operation, 3)
        b = _run(_case(name), operation, 3)
        assert a.tobytes() == b.tobytes()


def test_clean_labels_tool_morph_mode(tmp_path, capsys):
    """tools/clean_labels.py --morph on a small .npy: the JSON line and the file written"""
    import importlib.util
    import json
    import os
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'clean_labels.py')
    spec = importlib.util.spec_from_file_location('_clean_labels_morph', tool)
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
    assert run(src, dst, '--morph', 'Close', '--radius', 3) == {'shape': list(img.shape), 'labels_affected': n, 'out': str(dst)}
    assert np.array_equal(np.load(dst), _want('w67', 'Close', 3)[0]) and np.array_equal(np.load(src), img)
    np.save(src, vol)
    assert run(src, dst, '--morph', 'Erode', '--3d')['labels_affected'] == len(np.unique(vol)) - 1      # the default radius is 1
    assert np.array_equal(np.load(dst), _want('flat', 'Erode', 1)[0])
