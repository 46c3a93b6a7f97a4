"""Device side of Contact Labels: the kernel of csrc/contacts.hip through empanada_napari_amd.labels.label_contacts.  The expected
values are the numpy statement of tests/contacts_case.py (per half-direction one shifted compare, keys min << 32 | max), which
tests/test_contacts_case_host.py checks against the pair-by-pair definition and against Shape Labels' intercepts.  Everything raw is
an integer, so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import contacts_case as CC
import shape_case as SC

pytestmark = pytest.mark.gpu

FIELDS = ('a', 'b', 'pairs')
TOP = int(np.iinfo(np.uint32).max)      # the top of the key's domain


def _dev(x):
    import torch
    if x.dtype in (np.uint16, np.uint32):      # no arithmetic is needed on the tensor: reinterpret the bytes
        return torch.from_numpy(x.view({2: np.int16, 4: np.int32}[x.itemsize])).cuda().view({2: torch.uint16, 4: torch.uint32}[x.itemsize])
    return torch.from_numpy(x).cuda()


def _check_both(vol, sources=('device',), **kw):
    from empanada_napari_amd import labels as L
    for bg in (False, True):
        want = CC.want_contacts(vol, bg)
        for src in sources:
            m = L.label_contacts(_dev(vol) if src == 'device' else vol, background=bg, **kw)
            CC.check(m, want, vol.shape)
            assert m.background == bg


@pytest.mark.parametrize('dtype', SC.DTYPES)
def test_contacts_every_dtype_device_and_host(dtype):
    from empanada_napari_amd import labels as L
    vol = SC.volume(dtype)
    if dtype in (np.uint32, np.int64):
        vol[vol == 7] = TOP      # as a partner: the low half of its keys is all ones
        assert TOP in CC.want_contacts(vol)['b']
    _check_both(vol, ('device', 'host'))
    img = np.ascontiguousarray(vol[2])      # a 2-D image: four directions
    for bg in (False, True):
        for x in (_dev(img), img):
            m = L.label_contacts(x, background=bg)
            assert m.ndim == 2 and m.pairs.shape[1] == 4
            CC.check(m, CC.want_contacts(img, bg), img.shape)


@pytest.mark.parametrize('W', [1, 2, 3, 61, 64, 65])
def test_contacts_widths_off_the_vector_width(W):
    """D = 1: 16-byte loads straddle the row ends when W is no multiple of the vector width, x - 1 at x = 0 and x + 1 at x = W - 1
    are the neighbouring rows' ends in the raveled slab (for W = 1 and 2 every voxel); H = 1: the same across slices"""
    H = 4099 if W <= 3 else 67      # more than one tile also for the narrow ones
    for dtype, seed in ((np.uint32, W), (np.uint8, W + 100)):
        _check_both(SC.LC.runs(H * W, seed, dtype, run=11 if W > 3 else 5, top=90).reshape(1, H, W))
        _check_both(SC.LC.runs(15 * W, seed + 7, dtype, run=4, top=50).reshape(15, 1, W))


def test_contacts_slabs_device_host_and_directory_store(tmp_path):
    """objects that cross every seam diagonally; the tables of every source and slab are identical"""
    from empanada_napari_amd import labels as L, zstore
    vol = SC.seam_volume()
    whole = {bg: L.label_contacts(_dev(vol), background=bg) for bg in (False, True)}
    for bg in (False, True):
        CC.check(whole[bg], CC.want_contacts(vol, bg), vol.shape)
    za = zstore.DirArray.create(str(tmp_path / 'a'), vol.shape, np.uint32, (4, 16, 16))
    za[...] = vol
    store = zstore.DirArray(str(tmp_path / 'a'))
    for slab in (1, 2, 3, 5, vol.shape[0]):
        for src in (vol, store, _dev(vol)):
            for bg in (False, True):
                m = L.label_contacts(src, slab=slab, background=bg)
                for f in FIELDS:
                    assert np.array_equal(getattr(m, f), getattr(whole[bg], f)), (slab, bg, f)
    img = vol[5]
    for slab in (1, 5, 24):      # an image is streamed by rows: the halo is a row
        CC.check(L.label_contacts(img, slab=slab, background=True), CC.want_contacts(img, True), img.shape)
    again = L.label_contacts(_dev(vol), background=True)      # two runs: byte-identical
    assert all(getattr(again, f).tobytes() == getattr(whole[True], f).tobytes() for f in FIELDS)


def test_contacts_stretches_of_several_tiles():
    """label_contacts_kernel's grid is at most CT_MAX_GRID = 2048 workgroups and a tile is 256 lanes x 16 bytes, so beyond
    2048 * 1024 uint32 voxels a workgroup walks several tiles and carries its tile's coordinates from one to the next"""
    shape = (24, 264, 357)
    vol = SC.LC.blobs(shape, 40, 2, np.uint32, first=3)
    vol[:, ::37, :] = 0
    vol[5:19, 100:140, 300:357] = SC.LC.runs(14 * 40 * 57, 4, np.uint32, run=3, top=60).reshape(14, 40, 57)      # a busy corner
    assert vol.size > 2048 * 1024 and vol.shape[2] % 4
    _check_both(vol)


def test_contacts_closed_forms_and_misaligned_base():
    from empanada_napari_amd import labels as L
    one = np.full((16, 64, 64), 5, np.uint32)      # one label filling the volume: no pair, with or without the background
    for bg in (False, True):
        m = L.label_contacts(_dev(one), background=bg)
        assert len(m.a) == 0 and m.pairs.shape == (0, 13) and len(m.labels) == 0
    board = SC.checkerboard()
    m = L.label_contacts(_dev(board))
    CC.check(m, CC.want_contacts(board), board.shape)
    odd = np.abs(np.array(SC.half_dirs(3))).sum(axis=1) % 2 == 1
    assert m.a.tolist() == [1] and m.b.tolist() == [2] and not m.pairs[0, ~odd].any() and m.pairs[0, odd].all()
    D, H, W, c = 6, 5, 7, 3
    m = L.label_contacts(_dev(CC.half_spaces((D, H, W), c)))
    assert m.pairs.tolist() == [[(H - abs(dy)) * (W - abs(dx)) if dz else 0 for dz, dy, dx in SC.half_dirs(3)]] and m.faces.tolist() == [[H * W, 0, 0]]
    _check_both(SC.distinct_blocks(), ('device', 'host'))      # eight labels in every neighbourhood
    _check_both(SC.distinct_blocks().astype(np.int64))
    flat = SC.LC.runs(1 + 6 * 50 * 70, 3, np.uint8, run=31, top=100)      # 1 byte off the vector alignment
    vol = flat[1:].reshape(6, 50, 70)
    flat16 = SC.LC.runs(1 + 6 * 50 * 70, 4, np.uint16, run=31)
    vol16 = flat16[1:].reshape(6, 50, 70)
    for f, v in ((flat, vol), (flat16, vol16)):
        want = CC.want_contacts(v, True)
        CC.check(L.label_contacts(_dev(f)[1:].view(6, 50, 70), background=True), want, v.shape)
        CC.check(L.label_contacts(_dev(f)[1:].view(6, 50, 70), background=True, slab=4), want, v.shape)


def test_contacts_all_distinct_forces_the_table_to_double():
    """every voxel another label: every pair of the array is a row.  A table of 64 slots doubles many times, each time after the
    slab has been undone; slab by slab the overflow and its undo come in the middle of the stream"""
    from empanada_napari_amd import labels as L
    shape = (4, 64, 64)
    vol = CC.all_distinct(shape)
    want = CC.want_contacts(vol)
    assert len(want['a']) == CC.distinct_rows(shape)
    m = L.label_contacts(_dev(vol), capacity=64)
    assert m.doublings >= 3 and len(m.a) == CC.distinct_rows(shape) and (m.counts == 1).all()
    CC.check(m, want, shape)
    m = L.label_contacts(vol, capacity=64, slab=3)
    assert m.doublings >= 3
    CC.check(m, want, shape)


def _raw_rows(lib, buf, capacity):
    """{key: (count, 13 pairs)} through the raw finalize"""
    import torch
    from empanada_napari_amd import _abi
    num = C.c_int64(-1)
    _abi.check(lib.emp_label_contacts_finalize(_abi.ptr(buf), capacity, None, None, None, 0, C.byref(num), _abi.stream_ptr()), 'finalize')
    k = num.value
    keys, cnt = (torch.zeros(max(k, 1), dtype=torch.int64, device='cuda') for _ in range(2))
    pairs = torch.zeros((max(k, 1), 13), dtype=torch.int64, device='cuda')
    _abi.check(lib.emp_label_contacts_finalize(_abi.ptr(buf), capacity, _abi.ptr(keys), _abi.ptr(cnt), _abi.ptr(pairs), k, C.byref(num),
                                               _abi.stream_ptr()), 'finalize')
    assert num.value == k
    out = {int(key): (int(c),) + tuple(map(int, row)) for key, c, row in zip(keys[:k].cpu().numpy().view(np.uint64), cnt[:k].cpu().numpy(),
                                                                             pairs[:k].cpu().numpy())}
    assert len(out) == k
    return out


def test_contacts_overflow_contract_through_the_raw_entries():
    """a 64-slot table that holds a few pairs is fed a slab with more pairs than it has slots: *h_overflow = 1, and it finalizes to
    exactly what it held before; grown, it takes the slab"""
    import torch
    from empanada_napari_amd import _abi
    lib = _abi.load()
    D, H, W = 2, 16, 16
    A = SC.LC.runs(D * H * W, 21, np.uint32, run=40, top=9).reshape(D, H, W)
    B = (1000 + np.arange(D * H * W, dtype=np.uint32)).reshape(D, H, W)
    want_a, want_ab = CC.want_contacts(A, True), CC.want_contacts(np.concatenate([A, B]), True)
    assert 3 <= len(want_a['a']) <= 40 and len(want_ab['a']) - len(want_a['a']) > 64

    def as_rows(w):
        return {(int(a) << 32) | int(b): (int(p.sum()),) + tuple(map(int, p)) for a, b, p in zip(w['a'], w['b'], w['pairs'])}

    def table(capacity):
        buf = torch.empty(lib.emp_label_contacts_work_bytes(capacity), dtype=torch.uint8, device='cuda')
        _abi.check(lib.emp_label_contacts_reset(_abi.ptr(buf), capacity, _abi.stream_ptr()), 'reset')
        return buf

    def add(buf, capacity, d_slab, z0, below):
        ov = C.c_int(-1)
        _abi.check(lib.emp_label_contacts_accumulate(_abi.ptr(d_slab), 4, z0, D, H, W, 2 * D, below, 1, _abi.ptr(buf), capacity, _abi.stream_ptr(),
                                                     C.byref(ov)), 'accumulate')
        return ov.value

    assert lib.emp_label_contacts_work_bytes(64) == 64 + 64 * 120 and lib.emp_label_contacts_work_bytes(100) == 0
    dA, dB = _dev(A), _dev(B)
    small = table(64)
    assert add(small, 64, dA, 0, None) == 0
    assert _raw_rows(lib, small, 64) == as_rows(want_a)
    below = dA.data_ptr() + (D - 1) * H * W * 4      # A's last slice
    assert add(small, 64, dB, D, below) == 1      # by pigeonhole
    assert _raw_rows(lib, small, 64) == as_rows(want_a)      # every column of every row as before the call
    big = table(16384)
    ov = C.c_int(-1)
    _abi.check(lib.emp_label_contacts_grow(_abi.ptr(small), 64, _abi.ptr(big), 16384, _abi.stream_ptr(), C.byref(ov)), 'grow')
    assert ov.value == 0 and _raw_rows(lib, big, 16384) == as_rows(want_a)
    assert add(big, 16384, dB, D, below) == 0
    assert _raw_rows(lib, big, 16384) == as_rows(want_ab)
    ov = C.c_int(-1)      # a slab above slice 0 needs the slice below it
    assert lib.emp_label_contacts_accumulate(_abi.ptr(dB), 4, D, D, H, W, 2 * D, None, 1, _abi.ptr(big), 16384, _abi.stream_ptr(), C.byref(ov)) != 0


def test_contacts_row_sums_are_the_merged_kernels_columns():
    """per label and direction, summed over its partners with the background among them: shape_labels' intercepts without border
    faces; the axis columns: measure_labels' faces"""
    from empanada_napari_amd import labels as L
    vol = SC.volume(np.uint16, seed=11)
    c = L.label_contacts(_dev(vol), background=True)
    s, m = L.shape_labels(_dev(vol), border_faces=False), L.measure_labels(_dev(vol), border_faces=False)
    sums = np.zeros_like(s.intercepts)
    for side in (c.a, c.b):
        keep = side != 0
        np.add.at(sums, np.searchsorted(s.labels, side[keep]), c.pairs[keep])
    assert np.array_equal(sums, s.intercepts)
    assert np.array_equal(m.labels, s.labels) and np.array_equal(sums[:, list(SC.AXIS_COLUMNS[3])], m.faces)
    faces = np.zeros_like(m.faces)
    for side in (c.a, c.b):
        keep = side != 0
        np.add.at(faces, np.searchsorted(m.labels, side[keep]), c.faces[keep])
    assert np.array_equal(faces, m.faces)
    for sp in ((1.0, 1.0, 1.0), (2.0, 1.0, 0.5)):
        c = L.label_contacts(_dev(vol), spacing=sp)
        assert np.allclose(c.contact_area, CC.crofton(c.pairs, sp), rtol=1e-12, atol=0) and np.allclose(c.face_area, CC.face_size(c.pairs, sp), rtol=1e-12, atol=0)


def test_contacts_merge_groups_feed_merge_labels():
    """a ball that a plane cut into two ids, and one apart from it: the contact table finds the cut, merge_labels closes it"""
    from empanada_napari_amd import labels as L
    vol = np.zeros((40, 44, 90), np.uint32)
    ball = SC.ball(16) > 0
    n = ball.shape[0]
    vol[2:2 + n, 3:3 + n, 4:4 + n][ball] = 5
    vol[2:2 + n, 3:3 + n, 4:4 + n][ball & (np.indices(ball.shape).sum(axis=0) > 3 * (n // 2))] = 6      # cut by a plane with normal (1, 1, 1)
    vol[2:2 + n, 3:3 + n, 50:50 + n][ball] = 9
    vol[20, 20, 86] = 12      # 12 touches 9 by one voxel face only
    vol[20, 20, 50 + n - 1] = 9
    vol[20, 20, 50 + n:86] = 9
    before = L.label_table(_dev(vol))
    c = L.label_contacts(_dev(vol), background=True)
    CC.check(c, CC.want_contacts(vol, True), vol.shape)
    assert [g.tolist() for g in c.merge_groups()] == [[5, 6], [9, 12]]
    groups = c.merge_groups(min_fraction=0.2)      # the cut is about a third of either half's surface; one face of 26 neighbours is not
    assert [g.tolist() for g in groups] == [[5, 6]]
    merged = L.merge_labels(_dev(vol), ids=groups[0])
    after = L.label_contacts(merged, background=True)
    assert not ((after.a == 5) & (after.b == 6)).any() and 6 not in after.labels and 5 in after.labels
    t = L.label_table(merged)
    area = dict(zip(before.labels.tolist(), before.areas.tolist()))
    assert t.labels.tolist() == [0, 5, 9, 12] and t.areas[1] == area[5] + area[6]
    want = vol.copy()
    want[want == 6] = 5
    CC.check(after, CC.want_contacts(want, True), vol.shape)


def test_contacts_refusals():
    import torch
    from empanada_napari_amd import _abi, labels as L
    vol = SC.volume(np.int64, seed=6)
    neg = vol.copy()
    neg[2, 5, 5] = -1
    with pytest.raises(_abi.EmpError, match='outside'):
        L.label_contacts(_dev(neg))
    neg32 = SC.volume(np.int32, seed=6)
    neg32[0, 0, 0] = -7
    with pytest.raises(_abi.EmpError, match='outside'):
        L.label_contacts(neg32, background=True)
    big = vol.copy()
    big[1, 3:5, 7:20] = 1 << 32      # one past the top of the domain
    with pytest.raises(_abi.EmpError, match='outside'):
        L.label_contacts(_dev(big))
    with pytest.raises(ValueError, match='2-D or 3-D'):
        L.label_contacts(torch.zeros((2, 3, 4, 5), dtype=torch.uint8, device='cuda'))
    for sp in ((1, 1), (1, 0, 1), (1, -2, 1), (1, 1, float('nan'))):
        with pytest.raises(ValueError, match='spacing'):
            L.label_contacts(_dev(vol), spacing=sp)
    with pytest.raises(ValueError, match='capacity'):
        L.label_contacts(_dev(vol), capacity=100)
    CC.check(L.label_contacts(_dev(vol)), CC.want_contacts(vol), vol.shape)      # the device is fine afterwards


def test_label_contacts_tool(tmp_path, capsys):
    """tools/label_contacts.py end to end on a small .npy: argument parsing, the opener, the summary line, the CSV and the classes"""
    import csv
    import importlib.util
    import json
    import os
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'label_contacts.py')
    spec = importlib.util.spec_from_file_location('_label_contacts', tool)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    vol = np.zeros((12, 20, 22), np.uint16)
    vol[1:11, 1:10, 1:10] = 1001      # two instances of class 1 side by side, one of class 2 on top of both
    vol[1:11, 1:10, 10:20] = 1002
    vol[1:11, 10:18, 1:20] = 2001
    np.save(tmp_path / 'v.npy', vol)
    sp = (2.0, 1.0, 0.5)
    out = mod.main([str(tmp_path / 'v.npy'), '--spacing', '2', '1', '0.5', '--csv', str(tmp_path / 'v.csv')])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = CC.want_contacts(vol)
    area = CC.crofton(want['pairs'], sp)
    assert line == out and line['shape'] == [12, 20, 22] and line['labels'] == 3 and line['pairs'] == 3 and line['background'] is False
    big = int(np.argmax(area))
    assert line['largest']['a'] == int(want['a'][big]) and line['largest']['b'] == int(want['b'][big])
    assert np.isclose(line['largest']['contact_area'], area[big], rtol=1e-12) and 'classes' not in line
    rows = list(csv.DictReader(open(tmp_path / 'v.csv')))
    assert [(int(r['a']), int(r['b'])) for r in rows] == [(1001, 1002), (1001, 2001), (1002, 2001)]
    assert np.allclose([float(r['contact_area']) for r in rows], area, rtol=1e-12, atol=0)
    assert [int(r['count']) for r in rows] == want['pairs'].sum(axis=1).tolist()
    out = mod.main([str(tmp_path / 'v.npy'), '--background', '--label-divisor', '1000'])
    wb = CC.want_contacts(vol, True)
    assert out['background'] is True and out['pairs'] == len(wb['a']) and out['labels'] == 4
    ab = CC.crofton(wb['pairs'], (1, 1, 1))
    classes = {(c['a'], c['b']): c['contact_area'] for c in out['classes']}
    assert sorted(classes) == [(0, 1), (0, 2), (1, 1), (1, 2)]
    assert np.isclose(classes[(1, 1)], ab[(wb['a'] == 1001) & (wb['b'] == 1002)].sum(), rtol=1e-12)
    assert np.isclose(classes[(1, 2)], ab[(wb['a'] > 1000) & (wb['b'] == 2001)].sum(), rtol=1e-12)
