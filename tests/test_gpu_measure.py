"""Device side of Measure Labels: the kernel of csrc/measure.hip through empanada_napari_amd.labels.measure_labels.  The expected
values are the numpy statements of tests/measure_case.py (np.add.at of coordinate products, shifted compares on the padded
array).  Everything raw is an integer, so every comparison is exact."""
import numpy as np
import pytest

import measure_case as MC

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch
    if x.dtype in (np.uint16, np.uint32):      # no arithmetic is needed on the tensor: reinterpret the bytes
        return torch.from_numpy(x.view({2: np.int16, 4: np.int32}[x.itemsize])).cuda().view({2: torch.uint16, 4: torch.uint32}[x.itemsize])
    return torch.from_numpy(x).cuda()


def _check_all_modes(vol, sources=('device',)):
    from empanada_napari_amd import labels as L
    for src in sources:
        x = _dev(vol) if src == 'device' else vol
        for bf in (True, False):
            MC.check(L.measure_labels(x, border_faces=bf), MC.want_measures(vol, bf), vol.shape)
            MC.check(L.measure_labels(x, per_slice=True, border_faces=bf), MC.want_measures_per_slice(vol, bf), vol.shape)


@pytest.mark.parametrize('dtype', MC.DTYPES)
def test_measures_every_dtype_device_and_host(dtype):
    from empanada_napari_amd import labels as L
    vol = MC.volume(dtype)
    if dtype in (np.uint32, np.int64):
        vol[vol == 7] = np.iinfo(np.uint32).max
    if dtype == np.int64:
        big = vol.copy()
        big[1, 3:5, 7:20] = (1 << 32) + 5      # beyond 2^32: legal for the whole volume
        big[4, 30, 60] = (1 << 62) + 1
        m = L.measure_labels(_dev(big))
        MC.check(m, MC.want_measures(big), big.shape)
        assert (1 << 32) + 5 in m.labels and (1 << 62) + 1 in m.labels
    _check_all_modes(vol, ('device', 'host'))
    img = np.ascontiguousarray(vol[2])      # a 2-D image: (y, x) columns
    for bf in (True, False):
        m = L.measure_labels(_dev(img), border_faces=bf)
        assert m.ndim == 2 and m.sum2.shape[1] == 3
        MC.check(m, MC.want_measures(img, bf), img.shape)


@pytest.mark.parametrize('W', [1, 3, 61, 64, 65])
def test_measures_widths_off_the_vector_width(W):
    """D = 1: 16-byte loads straddle the row ends when W is no multiple of the vector width, the read of the row above is
    unaligned, and a uniform run covers many whole rows when W is small"""
    H = 4099 if W <= 3 else 67      # more than one tile also for the narrow ones
    for dtype, seed in ((np.uint32, W), (np.uint8, W + 100)):
        _check_all_modes(MC.LC.runs(H * W, seed, dtype, run=11 if W > 3 else 700, top=90).reshape(1, H, W))
    _check_all_modes(MC.LC.runs(3 * 5 * W, W + 7, np.uint16, run=9, top=50).reshape(3 * 5, 1, W))      # H = 1: runs cross slices


def test_measures_stretches_of_several_tiles():
    """The size rule: label_measure_kernel's grid is at most MZ_MAX_GRID = 2048 workgroups and a tile is 256 lanes x 16 bytes, so
    beyond 2048 * 1024 uint32 voxels a workgroup walks several tiles and carries its tile's coordinates from one to the next.  The
    volume is a small one blown up by whole factors (2.3 M voxels, a width that is no multiple of 4); its table follows from
    the small one's (measure_case.scaled)."""
    from empanada_napari_amd import labels as L
    small = MC.LC.runs(4 * 33 * 17, 2, np.uint32, run=5, top=300).reshape(4, 33, 17)
    f = (6, 8, 21)
    vol = np.repeat(np.repeat(np.repeat(small, f[0], 0), f[1], 1), f[2], 2)
    assert vol.size > 2048 * 1024 and vol.shape[2] % 4
    for bf in (True, False):
        MC.check(L.measure_labels(_dev(vol), border_faces=bf), MC.scaled(MC.want_measures(small, bf), f), vol.shape)
    want = MC.want_measures_per_slice(small)
    m = L.measure_labels(_dev(vol), per_slice=True)
    per = [MC.scaled({k: v[want['slices'] == z // f[0]] for k, v in want.items() if k != 'slices'}, f[1:]) for z in range(vol.shape[0])]
    for k in ('labels', 'areas', 'boxes', 'sum1', 'sum2', 'faces'):
        if k == 'labels':
            assert np.array_equal(m.labels, np.concatenate([p[k] for p in per]))
        else:
            assert np.array_equal(getattr(m, k), np.concatenate([p[k] for p in per])), k
    assert np.array_equal(m.slices, np.concatenate([np.full(len(p['labels']), z) for z, p in enumerate(per)]))


def test_measures_misaligned_base_one_label_and_checkerboard():
    from empanada_napari_amd import labels as L
    flat = MC.LC.runs(1 + 6 * 50 * 70, 3, np.uint8, run=31, top=100)
    vol = flat[1:].reshape(6, 50, 70)
    MC.check(L.measure_labels(_dev(flat)[1:].view(6, 50, 70)), MC.want_measures(vol), vol.shape)      # 1 byte off the vector alignment
    flat32 = MC.LC.runs(1 + 6 * 50 * 70, 4, np.int32, run=31)
    vol = flat32[1:].reshape(6, 50, 70)
    MC.check(L.measure_labels(_dev(flat32)[1:].view(6, 50, 70)), MC.want_measures(vol), vol.shape)
    one = np.full((16, 64, 64), 5, np.uint32)      # one label filling the volume: every face is a border face
    m = L.measure_labels(_dev(one))
    assert m.labels.tolist() == [5] and m.areas.tolist() == [one.size] and m.boxes.tolist() == [[0, 0, 0, 16, 64, 64]]
    assert m.faces.tolist() == [[2 * 64 * 64, 2 * 16 * 64, 2 * 16 * 64]]
    MC.check(m, MC.want_measures(one), one.shape)
    m = L.measure_labels(_dev(one), border_faces=False)
    assert m.faces.tolist() == [[0, 0, 0]] and np.array_equal(m.sum2, MC.want_measures(one)['sum2'])
    m = L.measure_labels(_dev(one), per_slice=True)
    assert m.labels.tolist() == [5] * 16 and m.faces.tolist() == [[2 * 64, 2 * 64]] * 16
    board = MC.checkerboard()      # every voxel a run head, every face exposed
    m = L.measure_labels(_dev(board))
    MC.check(m, MC.want_measures(board), board.shape)
    assert np.array_equal(m.faces, np.repeat(2 * m.areas[:, None], 3, axis=1))
    _check_all_modes(board, ('device', 'host'))


def test_measures_label_domain_and_moment_guard():
    import ctypes as C
    import torch
    from empanada_napari_amd import _abi, labels as L
    vol = MC.volume(np.int64, seed=6)
    vol[1, 3:5, 7:20] = (1 << 32) + 5
    with pytest.raises(_abi.EmpError, match='outside'):      # per slice the slice takes the upper half of the key
        L.measure_labels(_dev(vol), per_slice=True)
    neg = MC.volume(np.int64, seed=6)
    neg[2, 5, 5] = -1
    for per_slice in (False, True):
        with pytest.raises(_abi.EmpError, match='outside'):
            L.measure_labels(_dev(neg), per_slice=per_slice)
    neg32 = MC.volume(np.int32, seed=6)
    neg32[0, 0, 0] = -7
    with pytest.raises(_abi.EmpError, match='outside'):
        L.measure_labels(neg32)
    # max(D, H, W)^2 * D * H * W >= 2^63: refused from the shape alone (a broadcast view: nothing that size exists)
    huge = np.broadcast_to(np.zeros(1, np.uint8), (4096, 1 << 20, 1 << 20))
    with pytest.raises(ValueError, match='second moment could wrap'):
        L.measure_labels(huge)
    # the entry itself, on an empty slab of a volume of that shape
    lib = _abi.load()
    cap = 64
    buf = torch.empty(lib.emp_label_measure_work_bytes(cap), dtype=torch.uint8, device='cuda')
    _abi.check(lib.emp_label_measure_reset(_abi.ptr(buf), cap, _abi.stream_ptr()), 'reset')
    ov = C.c_int(0)
    for shape, fits in (((1 << 14, 1 << 14, 1 << 6), True), ((1 << 14, 1 << 14, 1 << 7), False), ((4096, 1 << 20, 1 << 20), False)):
        D, H, W = shape
        assert (max(shape) ** 2 * D * H * W < 1 << 63) == fits
        rc = lib.emp_label_measure_accumulate(None, 1, 0, 0, H, W, D, None, 0, 1, _abi.ptr(buf), cap, _abi.stream_ptr(), C.byref(ov))
        assert (rc == 0) == fits
        if not fits:
            assert b'second moment could wrap' in lib.emp_last_error()


def test_measures_salt_and_pepper_forces_the_table_to_double():
    from empanada_napari_amd import labels as L
    rng = np.random.default_rng(9)
    vol = rng.integers(0, 300_000, (8, 256, 256)).astype(np.uint32)      # ~250 000 distinct labels in 2^19 voxels
    want = MC.want_measures(vol)
    assert len(want['labels']) > 200_000
    m = L.measure_labels(_dev(vol), capacity=1 << 16)
    assert m.doublings >= 1          # 2^16 slots cannot hold them: the overflow path ran, the result is exact all the same
    MC.check(m, want, vol.shape)
    # slab by slab the overflow and its undo come in the middle of the stream
    m = L.measure_labels(vol, capacity=1 << 16, slab=3)
    assert m.doublings >= 1
    MC.check(m, want, vol.shape)


def test_measures_slabs_and_directory_store(tmp_path):
    from empanada_napari_amd import labels as L, zstore
    vol = MC.slab_volume()
    whole = L.measure_labels(_dev(vol))
    MC.check(whole, MC.want_measures(vol), vol.shape)
    whole_ps = L.measure_labels(_dev(vol), per_slice=True)
    MC.check(whole_ps, MC.want_measures_per_slice(vol), vol.shape)
    za = zstore.DirArray.create(str(tmp_path / 'a'), vol.shape, np.uint32, (4, 32, 32))
    za[...] = vol
    store = zstore.DirArray(str(tmp_path / 'a'))
    fields = ('labels', 'areas', 'boxes', 'sum1', 'sum2', 'faces')
    for slab in (1, 2, 3):
        for src in (vol, store, _dev(vol)):
            for bf in (True, False):
                m = L.measure_labels(src, slab=slab, border_faces=bf)
                ref = whole if bf else L.measure_labels(_dev(vol), border_faces=False)
                for f in fields:
                    assert np.array_equal(getattr(m, f), getattr(ref, f)), (slab, f)
        m = L.measure_labels(store, slab=slab, per_slice=True)
        for f in fields + ('slices',):
            assert np.array_equal(getattr(m, f), getattr(whole_ps, f)), (slab, f)
    img = vol[5]
    for slab in (1, 5, 40):      # an image is streamed by rows: the halo is a row
        MC.check(L.measure_labels(img, slab=slab), MC.want_measures(img), img.shape)
    again = L.measure_labels(_dev(vol))      # two runs: byte-identical
    assert all(getattr(again, f).tobytes() == getattr(whole, f).tobytes() for f in fields)


def test_measure_labels_tool(tmp_path, capsys):
    """tools/measure_labels.py end to end on a small .npy: argument parsing, the opener, the summary line and the CSV"""
    import csv
    import importlib.util
    import json
    import os
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'measure_labels.py')
    spec = importlib.util.spec_from_file_location('_measure_labels', tool)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    vol = np.zeros((9, 11, 13), np.uint16)
    vol[2:5, 3:8, 4:11] = 3      # the 3 x 5 x 7 box
    vol[6:8, 1:3, 1:3] = 9
    np.save(tmp_path / 'v.npy', vol)
    out = mod.main([str(tmp_path / 'v.npy'), '--spacing', '2', '1', '0.5', '--csv', str(tmp_path / 'v.csv')])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == out and line['labels'] == 2 and line['shape'] == [9, 11, 13] and line['voxels_labelled'] == 105 + 8
    rows = list(csv.DictReader(open(tmp_path / 'v.csv')))
    assert [int(r['label']) for r in rows] == [3, 9] and [int(r['area']) for r in rows] == [105, 8]
    box = rows[0]
    assert [int(box[f'bbox-{i}']) for i in range(6)] == [2, 3, 4, 5, 8, 11]
    assert [float(box[f'centroid-{i}']) for i in range(3)] == [3 * 2.0, 5 * 1.0, 7 * 0.5]
    assert float(box['volume']) == 105.0 and float(box['surface_area']) == 70 * 0.5 + 42 * 1.0 + 30 * 2.0
    want_var = sorted([(k * k - 1) / 12 * s * s for k, s in ((3, 2.0), (5, 1.0), (7, 0.5))], reverse=True)
    assert np.allclose([float(box[f'principal_variance-{i}']) for i in range(3)], want_var, rtol=1e-12, atol=0)
    out = mod.main([str(tmp_path / 'v.npy'), '--per-slice'])
    assert out['labels'] == 3 + 2 and out['per_slice'] is True
