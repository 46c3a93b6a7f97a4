"""Device side of Shape Labels: the kernel of csrc/shape.hip through empanada_napari_amd.labels.shape_labels.  The expected values
are the numpy statements of tests/shape_case.py (shifted compares with np.bincount; the cells of the cubical complex), which
tests/test_shape_case_host.py checks against the per-mask definitions.  Everything raw is an integer, so every comparison is exact."""
import numpy as np
import pytest

import shape_case as SC

pytestmark = pytest.mark.gpu

FIELDS = ('labels', 'areas', 'intercepts', 'euler')


def _dev(x):
    import torch
    if x.dtype in (np.uint16, np.uint32):      # no arithmetic is needed on the tensor: reinterpret the bytes
        return torch.from_numpy(x.view({2: np.int16, 4: np.int32}[x.itemsize])).cuda().view({2: torch.uint16, 4: torch.uint32}[x.itemsize])
    return torch.from_numpy(x).cuda()


def _check_all_modes(vol, sources=('device',)):
    from empanada_napari_amd import labels as L
    for bf in (True, False):
        want, want_ps = SC.want_shapes(vol, bf), SC.want_shapes_per_slice(vol, bf)
        for src in sources:
            x = _dev(vol) if src == 'device' else vol
            SC.check(L.shape_labels(x, border_faces=bf), want, vol.shape)
            SC.check(L.shape_labels(x, per_slice=True, border_faces=bf), want_ps, vol.shape)


@pytest.mark.parametrize('dtype', SC.DTYPES)
def test_shapes_every_dtype_device_and_host(dtype):
    from empanada_napari_amd import labels as L
    vol = SC.volume(dtype)
    if dtype in (np.uint32, np.int64):
        vol[vol == 7] = np.iinfo(np.uint32).max
    if dtype == np.int64:
        big = vol.copy()
        big[1, 3:5, 7:20] = (1 << 32) + 5      # beyond 2^32: legal for the whole volume
        big[4, 30, 60] = (1 << 62) + 1
        m = L.shape_labels(_dev(big))
        SC.check(m, SC.want_shapes(big), big.shape)
        assert (1 << 32) + 5 in m.labels and (1 << 62) + 1 in m.labels
    _check_all_modes(vol, ('device', 'host'))
    img = np.ascontiguousarray(vol[2])      # a 2-D image: four directions
    for bf in (True, False):
        for x in (_dev(img), img):
            m = L.shape_labels(x, border_faces=bf)
            assert m.ndim == 2 and m.intercepts.shape[1] == 4
            SC.check(m, SC.want_shapes(img, bf), img.shape)


@pytest.mark.parametrize('W', [1, 2, 3, 61, 64, 65])
def test_shapes_widths_off_the_vector_width(W):
    """D = 1: 16-byte loads straddle the row ends when W is no multiple of the vector width, x - 1 at x = 0 and x + 1 at x = W - 1
    are the neighbouring rows' ends in the raveled slab (for W = 1 and 2 every voxel), and the reads of the rows around are
    unaligned; H = 1: the same across slices"""
    H = 4099 if W <= 3 else 67      # more than one tile also for the narrow ones
    for dtype, seed in ((np.uint32, W), (np.uint8, W + 100)):
        _check_all_modes(SC.LC.runs(H * W, seed, dtype, run=11 if W > 3 else 5, top=90).reshape(1, H, W))
        _check_all_modes(SC.LC.runs(15 * W, seed + 7, dtype, run=4, top=50).reshape(15, 1, W))


def test_shapes_slabs_device_host_and_directory_store(tmp_path):
    """objects that cross every seam diagonally; the tables of every source and slab are identical"""
    from empanada_napari_amd import labels as L, zstore
    vol = SC.seam_volume()
    whole = {bf: L.shape_labels(_dev(vol), border_faces=bf) for bf in (True, False)}
    for bf in (True, False):
        SC.check(whole[bf], SC.want_shapes(vol, bf), vol.shape)
    whole_ps = L.shape_labels(_dev(vol), per_slice=True)
    SC.check(whole_ps, SC.want_shapes_per_slice(vol), vol.shape)
    za = zstore.DirArray.create(str(tmp_path / 'a'), vol.shape, np.uint32, (4, 16, 16))
    za[...] = vol
    store = zstore.DirArray(str(tmp_path / 'a'))
    for slab in (1, 2, 3, 5, vol.shape[0]):
        for src in (vol, store, _dev(vol)):
            for bf in (True, False):
                m = L.shape_labels(src, slab=slab, border_faces=bf)
                for f in FIELDS:
                    assert np.array_equal(getattr(m, f), getattr(whole[bf], f)), (slab, f)
            m = L.shape_labels(src, slab=slab, per_slice=True)
            for f in FIELDS + ('slices',):
                assert np.array_equal(getattr(m, f), getattr(whole_ps, f)), (slab, f)
    img = vol[5]
    for slab in (1, 5, 24):      # an image is streamed by rows: the halo is a row
        SC.check(L.shape_labels(img, slab=slab), SC.want_shapes(img), img.shape)
    again = L.shape_labels(_dev(vol))      # two runs: byte-identical
    assert all(getattr(again, f).tobytes() == getattr(whole[True], f).tobytes() for f in FIELDS)


def test_shapes_stretches_of_several_tiles():
    """The size rule: label_shape_kernel's grid is at most SH_MAX_GRID = 2048 workgroups and a tile is 256 lanes x 16 bytes, so
    beyond 2048 * 1024 uint32 voxels a workgroup walks several tiles and carries its tile's coordinates from one to the next.
    2.3 M voxels, a width that is no multiple of 4, against the vectorised reference."""
    from empanada_napari_amd import labels as L
    shape = (24, 264, 357)
    vol = SC.LC.blobs(shape, 40, 2, np.uint32, first=3)
    vol[:, ::37, :] = 0
    vol[5:19, 100:140, 300:357] = SC.LC.runs(14 * 40 * 57, 4, np.uint32, run=3, top=60).reshape(14, 40, 57)      # a busy corner
    assert vol.size > 2048 * 1024 and vol.shape[2] % 4
    SC.check(L.shape_labels(_dev(vol)), SC.want_shapes(vol), vol.shape)
    m = L.shape_labels(_dev(vol), per_slice=True, border_faces=False)
    want = SC.want_shapes_per_slice(vol, False)
    SC.check(m, want, vol.shape)


def test_shapes_closed_forms_and_misaligned_base():
    from empanada_napari_amd import labels as L
    shape = (16, 64, 64)
    one = np.full(shape, 5, np.uint32)      # one label filling the volume: every intercept is a border intercept
    m = L.shape_labels(_dev(one))
    assert m.labels.tolist() == [5] and m.areas.tolist() == [one.size]
    assert m.intercepts.tolist() == [SC.full_intercepts(shape)] and m.euler.tolist() == [[1, 1]]
    m = L.shape_labels(_dev(one), border_faces=False)
    assert not m.intercepts.any() and m.euler.tolist() == [[1, 1]] and m.areas.tolist() == [one.size]
    m = L.shape_labels(_dev(one), per_slice=True)
    assert m.labels.tolist() == [5] * 16 and m.intercepts.tolist() == [SC.full_intercepts(shape[1:])] * 16 and m.euler.tolist() == [[1, 1]] * 16
    board = SC.checkerboard()      # every axis and body-diagonal neighbour differs, every face-diagonal one is the same label
    m = L.shape_labels(_dev(board), border_faces=False)
    SC.check(m, SC.want_shapes(board, False), board.shape)
    odd = np.abs(np.array(SC.half_dirs(3))).sum(axis=1) % 2 == 1
    assert not m.intercepts[:, ~odd].any() and m.intercepts[:, odd].all()
    _check_all_modes(board, ('device', 'host'))
    blocks = SC.distinct_blocks()      # eight labels around every vertex
    _check_all_modes(blocks, ('device', 'host'))
    _check_all_modes(blocks.astype(np.int64))
    flat = SC.LC.runs(1 + 6 * 50 * 70, 3, np.uint8, run=31, top=100)      # 1 byte off the vector alignment
    vol = flat[1:].reshape(6, 50, 70)
    SC.check(L.shape_labels(_dev(flat)[1:].view(6, 50, 70)), SC.want_shapes(vol), vol.shape)
    SC.check(L.shape_labels(_dev(flat)[1:].view(6, 50, 70), slab=4), SC.want_shapes(vol), vol.shape)
    flat16 = SC.LC.runs(1 + 6 * 50 * 70, 4, np.uint16, run=31)
    vol = flat16[1:].reshape(6, 50, 70)
    SC.check(L.shape_labels(_dev(flat16)[1:].view(6, 50, 70), per_slice=True), SC.want_shapes_per_slice(vol), vol.shape)


def test_shapes_salt_and_pepper_forces_the_table_to_double():
    """2^18 labels of two voxels each, (z, 2a, x) and (z, 2a + 1, x + 1): no run is longer than one voxel.  A table of 64 slots
    doubles several times, each time after the slab has been undone.  The vertex between the two voxels of a label adds -1 to
    its closed Euler sum (the pair is one object under full connectivity and two under face connectivity), so the undo adds and
    removes negative values: they survive because the sums wrap"""
    from empanada_napari_amd import labels as L
    D, H, W = 8, 256, 256
    z, y, x = np.indices((D, H, W))
    ids = 1 + np.random.default_rng(9).permutation(D * (H // 2) * W)
    vol = ids[(z * (H // 2) + y // 2) * W + (x - y % 2) % W].astype(np.uint32)
    want = SC.want_shapes(vol)
    assert len(want['labels']) == 1 << 18 and (want['areas'] == 2).all()
    inner = vol[0, 0, :W - 1]      # pairs that do not wrap around the row end
    assert (want['euler'][inner - 1] == [1, 2]).all()
    m = L.shape_labels(_dev(vol), capacity=64)
    assert m.doublings >= 3
    SC.check(m, want, vol.shape)
    m = L.shape_labels(vol, capacity=64, slab=3)      # slab by slab the overflow and its undo come in the middle of the stream
    assert m.doublings >= 3
    SC.check(m, want, vol.shape)


def test_shapes_cross_checks_with_measure_and_table():
    from empanada_napari_amd import labels as L
    vol = SC.volume(np.uint16, seed=11)
    cols = list(SC.AXIS_COLUMNS[3])
    for bf in (True, False):
        s, m = L.shape_labels(_dev(vol), border_faces=bf), L.measure_labels(_dev(vol), border_faces=bf)
        assert np.array_equal(s.labels, m.labels) and np.array_equal(s.areas, m.areas) and np.array_equal(s.intercepts[:, cols], m.faces)
        s, m = L.shape_labels(_dev(vol), per_slice=True, border_faces=bf), L.measure_labels(_dev(vol), per_slice=True, border_faces=bf)
        assert np.array_equal(s.slices, m.slices) and np.array_equal(s.intercepts[:, list(SC.AXIS_COLUMNS[2])], m.faces)
        img = np.ascontiguousarray(vol[3])
        assert np.array_equal(L.shape_labels(_dev(img), border_faces=bf).intercepts[:, list(SC.AXIS_COLUMNS[2])],
                              L.measure_labels(_dev(img), border_faces=bf).faces)
    t = L.label_table(_dev(vol))
    s = L.shape_labels(_dev(vol))
    assert np.array_equal(s.labels, t.labels[t.labels != 0]) and np.array_equal(s.areas, t.areas[t.labels != 0])
    # the derived columns against the case module's formulas: a 13-term float64 sum
    for sp in ((1.0, 1.0, 1.0), (2.0, 1.0, 0.5)):
        s = L.shape_labels(_dev(vol), spacing=sp)
        surf = SC.crofton(s.intercepts, sp)
        assert np.allclose(s.surface_area, surf, rtol=1e-12, atol=0) and np.allclose(s.sphericity, SC.sphericity(s.areas, surf, sp), rtol=1e-12, atol=0)
        s = L.shape_labels(_dev(vol), spacing=sp, per_slice=True)
        per = SC.crofton(s.intercepts, sp[1:])
        assert np.allclose(s.perimeter, per, rtol=1e-12, atol=0) and np.allclose(s.circularity, SC.circularity(s.areas, per, sp[1:]), rtol=1e-12, atol=0)


def test_shapes_known_objects():
    from empanada_napari_amd import labels as L
    for name, obj in SC.known_objects().items():
        s = L.shape_labels(_dev(obj))
        assert s.euler.tolist() == [list(SC.KNOWN_EULER[name])], name
        assert s.euler_number().tolist() == [SC.KNOWN_EULER[name][0]] and s.euler_number(1).tolist() == [SC.KNOWN_EULER[name][1]]
    ball = SC.ball(16)
    s, m = L.shape_labels(_dev(ball)), L.measure_labels(_dev(ball))
    SC.check(s, SC.want_shapes(ball), ball.shape)
    assert s.sphericity[0] > 0.95 and m.sphericity[0] < 0.7
    assert abs(s.surface_area[0] / (4 * np.pi * 16 * 16) - 1) < 0.05


def test_shapes_refusals():
    import torch
    from empanada_napari_amd import _abi, labels as L
    vol = SC.volume(np.int64, seed=6)
    neg = vol.copy()
    neg[2, 5, 5] = -1
    for per_slice in (False, True):
        with pytest.raises(_abi.EmpError, match='outside'):
            L.shape_labels(_dev(neg), per_slice=per_slice)
    neg32 = SC.volume(np.int32, seed=6)
    neg32[0, 0, 0] = -7
    with pytest.raises(_abi.EmpError, match='outside'):
        L.shape_labels(neg32)
    big = vol.copy()
    big[1, 3:5, 7:20] = (1 << 32) + 5
    with pytest.raises(_abi.EmpError, match='outside'):      # per slice the slice takes the upper half of the key
        L.shape_labels(_dev(big), per_slice=True)
    with pytest.raises(ValueError, match='2-D or 3-D'):
        L.shape_labels(torch.zeros((2, 3, 4, 5), dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError, match='per_slice needs a 3-D'):
        L.shape_labels(_dev(vol[0]), per_slice=True)
    for sp in ((1, 1), (1, 0, 1), (1, -2, 1), (1, 1, float('nan'))):
        with pytest.raises(ValueError, match='spacing'):
            L.shape_labels(_dev(vol), spacing=sp)
    SC.check(L.shape_labels(_dev(vol)), SC.want_shapes(vol), vol.shape)      # the device is fine afterwards


def test_shape_labels_tool(tmp_path, capsys):
    """tools/shape_labels.py end to end on a small .npy: argument parsing, the opener, the summary line and the CSV"""
    import csv
    import importlib.util
    import json
    import os
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'shape_labels.py')
    spec = importlib.util.spec_from_file_location('_shape_labels', tool)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    vol = np.zeros((20, 21, 22), np.uint16)
    vol[1:18, 1:18, 1:18][SC.hollow_ball() > 0] = 3      # a ball with a cavity
    vol[18:20, 1:3, 1:3] = 9
    np.save(tmp_path / 'v.npy', vol)
    out = mod.main([str(tmp_path / 'v.npy'), '--spacing', '2', '1', '0.5', '--csv', str(tmp_path / 'v.csv')])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = SC.want_shapes(vol)
    assert line == out and line['labels'] == 2 and line['shape'] == [20, 21, 22] and line['voxels_labelled'] == int(want['areas'].sum())
    assert line['labels_with_euler_number_not_1'] == 1
    rows = list(csv.DictReader(open(tmp_path / 'v.csv')))
    assert [int(r['label']) for r in rows] == [3, 9] and [int(r['euler_number']) for r in rows] == [2, 1]
    assert np.allclose([float(r['surface_area']) for r in rows], SC.crofton(want['intercepts'], (2, 1, 0.5)), rtol=1e-12, atol=0)
    out = mod.main([str(tmp_path / 'v.npy'), '--per-slice'])
    assert out['labels'] == len(SC.want_shapes_per_slice(vol)['labels']) and out['per_slice'] is True
