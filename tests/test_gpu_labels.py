"""Device side of the label clean-up module: the table kernel and the edit kernel (csrc/labels.hip) through
empanada_napari_amd.labels.  The expected values are numpy / scipy statements (tests/labels_case.py): np.unique with boxes from
np.nonzero per label, np.where(np.isin(...)) for the edits, scipy.ndimage.label per value for clear_border.  Everything is
integer, so every comparison is exact."""
import numpy as np
import pytest

import labels_case as LC

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint16, np.int32, np.uint32, np.int64]


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


def _volume(dtype, shape=(5, 37, 61), seed=1):
    return LC.runs(int(np.prod(shape)), seed, dtype, run=29, top=120 if np.dtype(dtype).itemsize == 1 else 200).reshape(shape)


# ----------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_table_every_dtype_device_and_host(dtype):
    from empanada_napari_amd import labels as L
    vol = _volume(dtype)
    if dtype in (np.uint32, np.int64):
        vol[vol == 7] = np.iinfo(np.uint32).max
    LC.check_table(L.label_table(_dev(vol)), vol)
    LC.check_table(L.label_table(vol), vol)       # host array through the staging buffers
    LC.check_table_per_slice(L.label_table(_dev(vol), per_slice=True), vol)
    img = vol[2]
    LC.check_table(L.label_table(_dev(np.ascontiguousarray(img))), img)      # a 2-D image: (y0, x0, y1, x1) boxes


@pytest.mark.parametrize('W', [1, 3, 61, 64, 65])
def test_table_widths_off_the_vector_width(W):
    """D = 1: 16-byte loads straddle the row ends when W is no multiple of the vector width, and a uniform run covers many
    whole rows when W is small"""
    from empanada_napari_amd import labels as L
    H = 4099 if W <= 3 else 67      # more than one tile also for the narrow ones
    for dtype, seed in ((np.uint32, W), (np.uint8, W + 100)):
        vol = LC.runs(H * W, seed, dtype, run=11 if W > 3 else 700, top=90).reshape(1, H, W)
        LC.check_table(L.label_table(_dev(vol)), vol)
        LC.check_table_per_slice(L.label_table(_dev(vol), per_slice=True), vol)
    thin = LC.runs(3 * 5 * W, W + 7, np.uint16, run=9, top=50).reshape(3 * 5, 1, W)      # H = 1: runs cross slices
    LC.check_table(L.label_table(_dev(thin)), thin)
    LC.check_table_per_slice(L.label_table(_dev(thin), per_slice=True), thin)


def test_table_stretches_of_several_tiles():
    """beyond 8 192 tiles a workgroup walks several tiles and carries the coordinates of its tile from one to the next: the
    smallest uint32 volume that gets there (8.5 M voxels), a small one blown up by whole factors, whose table follows from the
    small one's"""
    from empanada_napari_amd import labels as L
    small = LC.runs(4 * 67 * 33, 2, np.uint32, run=5, top=400).reshape(4, 67, 33)
    f = (8, 8, 15)
    vol = np.repeat(np.repeat(np.repeat(small, f[0], 0), f[1], 1), f[2], 2)
    assert vol.size > 8192 * 1024 and vol.shape[2] % 4
    labels, areas, boxes = LC.want_table(small)
    scale = np.array(f + f)
    for per_slice in (False, True):
        t = L.label_table(_dev(vol), per_slice=per_slice)
        if not per_slice:
            assert np.array_equal(t.labels, labels) and np.array_equal(t.areas, areas * np.prod(f)) and np.array_equal(t.boxes, boxes * scale)
        else:
            s, l, a, b = LC.want_table_per_slice(small)
            rep = lambda x: np.concatenate([x[s == z // f[0]] for z in range(vol.shape[0])])
            assert np.array_equal(t.labels, rep(l)) and np.array_equal(t.areas, rep(a) * f[1] * f[2])
            assert np.array_equal(t.boxes, rep(b) * np.array([f[1], f[2]] * 2))
            assert np.array_equal(t.slices, np.concatenate([np.full((s == z // f[0]).sum(), z) for z in range(vol.shape[0])]))


def test_table_misaligned_base_and_one_label_filling_the_volume():
    from empanada_napari_amd import labels as L
    flat = LC.runs(1 + 6 * 50 * 70, 3, np.uint8, run=31, top=100)
    vol = flat[1:].reshape(6, 50, 70)
    LC.check_table(L.label_table(_dev(flat)[1:].view(6, 50, 70)), vol)      # base pointer 1 byte off the vector alignment
    flat32 = LC.runs(1 + 6 * 50 * 70, 4, np.int32, run=31)
    LC.check_table(L.label_table(_dev(flat32)[1:].view(6, 50, 70)), flat32[1:].reshape(6, 50, 70))
    one = np.full((16, 64, 64), 5, np.uint32)
    t = L.label_table(_dev(one))
    assert t.labels.tolist() == [5] and t.areas.tolist() == [one.size] and t.boxes.tolist() == [[0, 0, 0, 16, 64, 64]]
    t = L.label_table(_dev(one), per_slice=True)
    assert t.labels.tolist() == [5] * 16 and t.areas.tolist() == [64 * 64] * 16 and t.slices.tolist() == list(range(16))
    assert (t.boxes == np.array([0, 0, 64, 64])).all()


def test_table_label_domain():
    from empanada_napari_amd import _abi, labels as L
    vol = _volume(np.int64, seed=6)
    big = (1 << 32) + 5
    vol[1, 3:5, 7:20] = big      # beyond 2^32: legal for the whole volume
    vol[4, 30, 60] = (1 << 62) + 1
    t = L.label_table(_dev(vol))
    LC.check_table(t, vol)
    assert big in t.labels and (1 << 62) + 1 in t.labels
    with pytest.raises(_abi.EmpError, match='outside'):      # ... but not per slice, where the slice takes the upper half of the key
        L.label_table(_dev(vol), per_slice=True)
    neg = _volume(np.int64, seed=6)
    neg[2, 5, 5] = -1
    for per_slice in (False, True):
        with pytest.raises(_abi.EmpError, match='outside'):
            L.label_table(_dev(neg), per_slice=per_slice)
    neg32 = _volume(np.int32, seed=6)
    neg32[0, 0, 0] = -7
    with pytest.raises(_abi.EmpError, match='outside'):
        L.label_table(neg32)


def test_table_salt_and_pepper_forces_the_table_to_double():
    from empanada_napari_amd import labels as L
    rng = np.random.default_rng(9)
    vol = rng.integers(0, 300_000, (8, 256, 256)).astype(np.uint32)      # ~250 000 distinct labels in 2^19 voxels
    t = L.label_table(_dev(vol), capacity=1 << 16)
    assert t.doublings >= 1          # 2^16 slots cannot hold them: the overflow path ran, the result is exact all the same
    labels, areas, boxes = LC.want_table_fast(vol)
    assert len(labels) > 200_000
    assert np.array_equal(t.labels, labels) and np.array_equal(t.areas, areas) and np.array_equal(t.boxes, boxes)
    # slab by slab the overflow comes in the middle of the stream: counts restored, boxes still right
    t = L.label_table(vol, capacity=1 << 16, slab=3)
    assert t.doublings >= 1
    assert np.array_equal(t.labels, labels) and np.array_equal(t.areas, areas) and np.array_equal(t.boxes, boxes)


def test_table_slabs_and_directory_store(tmp_path):
    from empanada_napari_amd import labels as L, zstore
    shape = (40, 96, 80)
    vol = LC.blobs(shape, 60, 5, np.uint32, first=1000)
    whole = L.label_table(_dev(vol))
    LC.check_table(whole, vol)
    whole_ps = L.label_table(_dev(vol), per_slice=True)
    LC.check_table_per_slice(whole_ps, vol)
    za = zstore.DirArray.create(str(tmp_path / 'a'), shape, np.uint32, (16, 64, 64))
    za[...] = vol
    store = zstore.DirArray(str(tmp_path / 'a'))
    for slab in (1, 7, 16, 40):
        for src in (vol, store, _dev(vol)):
            t = L.label_table(src, slab=slab)
            for f in ('labels', 'areas', 'boxes'):      # global z in the boxes, whatever the slab
                assert np.array_equal(getattr(t, f), getattr(whole, f)), (slab, f)
        t = L.label_table(store, slab=slab, per_slice=True)
        for f in ('slices', 'labels', 'areas', 'boxes'):
            assert np.array_equal(getattr(t, f), getattr(whole_ps, f)), (slab, f)
    img = vol[20]
    for slab in (1, 5, 96):      # an image is streamed by rows
        LC.check_table(L.label_table(img, slab=slab), img)
    again = L.label_table(_dev(vol))      # two runs: byte-identical
    assert again.boxes.tobytes() == whole.boxes.tobytes() and again.areas.tobytes() == whole.areas.tobytes()


# ----------------------------------------------------------------------------
# the edits
# ----------------------------------------------------------------------------
def _edit_cases(vol):
    from empanada_napari_amd import labels as L
    ids = np.unique(vol)
    ids = ids[ids > 0]
    dele, merge = ids[::3], ids[1::4]
    cut = int(np.median(np.unique(vol, return_counts=True)[1]))
    return [
        (lambda x, **k: L.delete_labels(x, np.concatenate([dele, [0]]), **k), np.where(np.isin(vol, dele), 0, vol)),
        (lambda x, **k: L.merge_labels(x, np.concatenate([[0], merge[::-1]]), **k), np.where(np.isin(vol, merge), merge.min(), vol)),
        (lambda x, **k: L.merge_labels(x, merge, new_label_id=int(merge[2]), **k), np.where(np.isin(vol, merge), merge[2], vol)),
        (lambda x, **k: L.filter_out_small_label_areas(x, cut, **k)[0], LC.want_small_filter(vol, cut)[0]),
        (lambda x, **k: L.filter_out_small_label_areas(x, cut, per_slice=True, **k)[0], LC.per_slice(LC.want_small_filter, vol, cut)[0]),
    ]


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.int32, np.uint32, np.int64])
def test_edits_device_in_place_and_out_of_place(dtype):
    vol = _volume(dtype, shape=(6, 45, 67), seed=11)
    for fn, want in _edit_cases(vol):
        d = _dev(vol)
        out = fn(d)
        assert out is not d and out.dtype == d.dtype and np.array_equal(_host(out), want)
        assert np.array_equal(_host(d), vol)      # the input is untouched
        same = fn(d, inplace=True)
        assert same is d and np.array_equal(_host(d), want)


def test_edits_numpy_and_store_routes(tmp_path):
    from empanada_napari_amd import labels as L, zstore
    shape = (20, 48, 56)
    vol = LC.blobs(shape, 50, 8, np.uint16, first=100)
    za = zstore.DirArray.create(str(tmp_path / 'in'), shape, np.uint16, (8, 32, 32))
    za[...] = vol
    for i, (fn, want) in enumerate(_edit_cases(vol)):
        for slab in (None, 3):
            keep = vol.copy()
            out = fn(keep, slab=slab)
            assert isinstance(out, np.ndarray) and out is not keep and out.dtype == vol.dtype
            assert np.array_equal(out, want) and np.array_equal(keep, vol)      # never in place on the caller's array ...
            assert fn(keep, slab=slab, inplace=True) is keep and np.array_equal(keep, want)      # ... unless asked
            zo = zstore.DirArray.create(str(tmp_path / f'out{i}_{slab}'), shape, np.uint16, (8, 32, 32))
            res = fn(zstore.DirArray(str(tmp_path / 'in')), out=zo, slab=slab)
            assert res is zo and np.array_equal(np.asarray(zstore.DirArray(str(tmp_path / f'out{i}_{slab}'))[...]), want)
    with pytest.raises(TypeError, match='out='):
        L.delete_labels(zstore.DirArray(str(tmp_path / 'in')), [100])
    n = L.filter_out_small_label_areas(vol, 10 ** 9)[1]
    assert n == len(np.unique(vol)) - 1
    empty = np.zeros((4, 8, 8), np.uint16)      # the one deliberate difference: no labels -> unchanged, 0 (the reference raises)
    out, n = L.filter_out_small_label_areas(empty, 100)
    assert n == 0 and np.array_equal(out, empty)
    with pytest.raises(ValueError, match='dtype'):
        L.merge_labels(np.ones((4, 4), np.uint8), [1, 2], new_label_id=300)


def test_map_of_a_million_entries():
    """salt and pepper: every second label of 2^21 distinct ones deleted, the others merged pairwise"""
    from empanada_napari_amd import labels as L
    rng = np.random.default_rng(3)
    vol = rng.permutation(1 << 21).astype(np.int64).reshape(8, 512, 512) + 1
    ids = np.arange(1, (1 << 21) + 1, 2)
    assert len(ids) >= 10 ** 6
    d = _dev(vol)
    out = L.delete_labels(d, ids)
    assert np.array_equal(_host(out), np.where(vol % 2 == 1, 0, vol))
    t = L.label_table(out)
    assert len(t.labels) == (1 << 20) + 1 and t.areas[0] == 1 << 20 and (t.areas[1:] == 1).all()
    out, n = L.filter_out_small_label_areas(d, 1)      # every label has one voxel: the map holds 2^21 entries
    assert n == 1 << 21 and not bool(out.any())


@pytest.mark.parametrize('entries', [1, 512, 513, 1500])
def test_map_sizes_around_the_lds_threshold(entries):
    """maps of up to 512 entries are looked up in LDS, larger ones in global memory"""
    from empanada_napari_amd import labels as L
    vol = LC.runs(7 * 90 * 101, 13, np.int32, run=3, top=2000).reshape(7, 90, 101)
    ids = np.unique(vol)
    ids = ids[ids > 0]
    assert len(ids) > 1500
    pick = ids[np.random.default_rng(entries).permutation(len(ids))[:entries]]
    assert np.array_equal(_host(L.delete_labels(_dev(vol), pick)), np.where(np.isin(vol, pick), 0, vol))
    assert np.array_equal(_host(L.merge_labels(_dev(vol), pick, new_label_id=5000)), np.where(np.isin(vol, pick), 5000, vol))
    pairs = np.stack([np.arange(entries) % 7, pick], axis=1)      # per-slice keys straight through the map
    import torch
    with torch.cuda.device(0):
        out = L._apply(_dev(vol), L._map_keys(pairs, True), np.zeros(entries, np.int64), True, torch.device('cuda', 0), None, False, None, 'test')
    want = vol.copy()
    for z, l in pairs:
        want[z][want[z] == l] = 0
    assert np.array_equal(_host(out), want)


def test_merge_labels_default_target_and_dropped_zeros():
    from empanada_napari_amd import labels as L
    img = np.zeros((9, 13), np.int32)
    img[1, 1:4] = 30
    img[3, 2:9] = 12
    img[5, 5] = 44
    img[7, 0:13] = 9
    out = _host(L.merge_labels(_dev(img), [44, 0, 30, 12, 0]))
    assert np.array_equal(out, np.where(np.isin(img, [44, 30, 12]), 12, img))      # min(ids), :378-381; zeros dropped
    out = _host(L.merge_labels(_dev(img), [44, 30], new_label_id=9))
    assert np.array_equal(out, np.where(np.isin(img, [44, 30]), 9, img))
    out = _host(L.delete_labels(_dev(img), [0, 9, 0]))
    assert np.array_equal(out, np.where(img == 9, 0, img)) and (out == 0).sum() == (img == 0).sum() + 13
    with pytest.raises(ValueError):
        L.merge_labels(_dev(img), [0, 0])


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.int64])
def test_edit_destinations_with_an_uneven_last_slab(dtype, tmp_path):
    """every destination of an edit -- a new and the caller's own device tensor, a new and the caller's own numpy array, a store
    as out= and a store edited in place -- with slabs of 3 rows: 7 rows end in a slab of one, 6 rows in a whole one"""
    from empanada_napari_amd import labels as L, zstore
    for rows in (7, 6):
        vol = LC.runs(rows * 5 * 6, 17 + rows, dtype, run=4, top=40).reshape(rows, 5, 6)
        ids = np.unique(vol)[1::2]
        want = np.where(np.isin(vol, ids), 0, vol)
        d = _dev(vol)
        out = L.delete_labels(d, ids, slab=3)
        assert out is not d and out.dtype == d.dtype and np.array_equal(_host(out), want) and np.array_equal(_host(d), vol)
        assert L.delete_labels(d, ids, slab=3, inplace=True) is d and np.array_equal(_host(d), want)
        own = vol.copy()
        out = L.delete_labels(own, ids, slab=3)
        assert out is not own and out.dtype == vol.dtype and np.array_equal(out, want) and np.array_equal(own, vol)
        assert L.delete_labels(own, ids, slab=3, inplace=True) is own and np.array_equal(own, want)
        za = zstore.DirArray.create(str(tmp_path / f'in{rows}'), vol.shape, dtype, (2, 5, 6))
        za[...] = vol
        zo = zstore.DirArray.create(str(tmp_path / f'out{rows}'), vol.shape, dtype, (4, 5, 6))
        assert L.delete_labels(za, ids, slab=3, out=zo) is zo and np.array_equal(np.asarray(zo[...]), want)
        assert np.array_equal(np.asarray(za[...]), vol)
        assert L.delete_labels(za, ids, slab=3, inplace=True) is za
        assert np.array_equal(np.asarray(zstore.DirArray(str(tmp_path / f'in{rows}'))[...]), want)


@pytest.mark.parametrize('keys_on, data_on', [('device', 'device'), ('device', 'host'), ('host', 'device'), ('host', 'host')])
def test_apply_with_a_key_source(keys_on, data_on, tmp_path):
    """the edit keyed by a second array, as the streamed clear-border runs it: int32 keys, uint8 data, each on the device or on the
    host, slabs of 4 of 6 rows, into every destination the data's kind has"""
    import torch
    from empanada_napari_amd import labels as L, zstore
    shape = (6, 5, 7)
    keys = LC.runs(6 * 5 * 7, 5, np.int32, run=3, top=60).reshape(shape)
    data = LC.runs(6 * 5 * 7, 6, np.uint8, run=5, top=200).reshape(shape)
    ids = np.unique(keys)[1::3]
    want = np.where(np.isin(keys, ids), 0, data)
    assert 0 < (want != data).sum() < data.size
    device = torch.device('cuda', 0)

    def store(name, arr):
        za = zstore.DirArray.create(str(tmp_path / name), shape, arr.dtype, (4, 5, 7))
        za[...] = arr
        return za

    def run(k, d, out, inplace):
        with torch.cuda.device(0):
            return L._apply(d, L._map_keys(ids, False), np.zeros(len(ids), np.int64), False, device, out, inplace, 4, 'test', key_labels=k)
    for i, k in enumerate([_dev(keys)] if keys_on == 'device' else [keys, store('keys', keys)]):
        if data_on == 'device':
            d = _dev(data)
            out = run(k, d, None, False)
            assert out is not d and out.dtype == torch.uint8 and np.array_equal(_host(out), want) and np.array_equal(_host(d), data)
            assert run(k, d, None, True) is d and np.array_equal(_host(d), want)
        else:
            own = data.copy()
            out = run(k, own, None, False)
            assert isinstance(out, np.ndarray) and out is not own and np.array_equal(out, want) and np.array_equal(own, data)
            assert run(k, own, None, True) is own and np.array_equal(own, want)
            zo = zstore.DirArray.create(str(tmp_path / f'out{i}'), shape, np.uint8, (2, 5, 7))
            assert run(k, store(f'data{i}', data), zo, False) is zo and np.array_equal(np.asarray(zo[...]), want)
        if keys_on == 'host':
            assert np.array_equal(np.asarray(k[...]), keys)      # the keys are only read


# ----------------------------------------------------------------------------
# the slab stream
# ----------------------------------------------------------------------------
_SPIN = {}


def _delay(ms=3.0):
    """a few milliseconds of work on the current stream: torch's spin kernel, its cycles per millisecond measured once; without
    it large elementwise passes over a scratch tensor"""
    import torch
    if not hasattr(torch.cuda, '_sleep'):
        scratch = _SPIN.setdefault('scratch', torch.zeros(1 << 26, device='cuda'))
        for _ in range(8):
            scratch.add_(1.0)
        return
    if 'cycles_per_ms' not in _SPIN:
        torch.cuda._sleep(1000)      # loads the kernel
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(1_000_000)
        e1.record()
        e1.synchronize()
        _SPIN['cycles_per_ms'] = 1_000_000 / max(e0.elapsed_time(e1), 1e-3)
    torch.cuda._sleep(int(ms * _SPIN['cycles_per_ms']))


@pytest.mark.parametrize('dtypes', [(np.uint16,), (np.uint16, np.int32)])
def test_stream_keeps_a_slab_until_the_consumer_is_done(dtypes):
    """A consumer that never synchronises the host: per one-row slab it queues a delay and then a device copy of the slab into its
    place in a result.  The stream refills a staging slot two slabs later: were that not ordered behind the consumer's queue, the
    copy would read a later slab's rows (inside the same buffers: wrong data, never a fault).  One host source, and two of
    different row sizes, as label_overlap and the streamed clear-border have them"""
    import torch
    from empanada_napari_amd import _abi, _labelstream as S
    shape = (12, 4, 8)
    device = torch.device('cuda', 0)
    arrays = [(np.arange(12 * 4 * 8) * (3 + i) + 1 + i).astype(dt).reshape(shape) for i, dt in enumerate(dtypes)]
    lib = _abi.load()
    with torch.cuda.device(0):
        sources = [S.HostSource(a, device) for a in arrays]
        results = [torch.zeros(a.nbytes, dtype=torch.uint8, device=device) for a in arrays]
        for _, z0, z1, addresses in S.stream_slabs(sources, 1, device):
            assert z1 == z0 + 1
            for s, res, address in zip(sources, results, addresses):
                _delay()
                _abi.check(lib.emp_copy_d2d(res.data_ptr() + z0 * s.row_bytes, address, s.row_bytes, _abi.stream_ptr(device)), 'emp_copy_d2d')
        got = [res.cpu().numpy().view(a.dtype).reshape(shape) for res, a in zip(results, arrays)]
    for g, a in zip(got, arrays):
        wrong = np.flatnonzero((g != a).any(axis=(1, 2)))
        assert np.array_equal(g, a), f'rows {wrong.tolist()} hold another slab'


# ----------------------------------------------------------------------------
# boundary labels
# ----------------------------------------------------------------------------
def _two_component_volume():
    """label 5: one component on the border, one in the interior; 6 interior; 7 border only"""
    vol = np.zeros((6, 20, 24), np.int32)
    vol[0:2, 0:3, 0:3] = 5
    vol[2:4, 8:11, 8:12] = 5
    vol[2:4, 14:17, 3:6] = 6
    vol[3:6, 17:20, 20:24] = 7
    return vol


def test_boundary_reference_mode_keeps_the_interior_component():
    from empanada_napari_amd import labels as L
    vol = _two_component_volume()
    want, n_want = LC.want_clear_border(vol)
    assert n_want == 1 and (want == 5).sum() == 2 * 3 * 4 and not (want == 7).any()      # 5 is not counted as removed
    for src in (_dev(vol), vol):
        out, n = L.remove_boundary_labels(src)
        out = _host(out) if not isinstance(out, np.ndarray) else out
        assert np.array_equal(out, want) and n == 1
    # per slice: 5's interior pieces and 6 are interior in every image; nothing touches an image edge but 5's corner and 7
    want, n_want = LC.per_slice(LC.want_clear_border, vol)
    out, n = L.remove_boundary_labels(_dev(vol), per_slice=True)
    assert np.array_equal(_host(out), want) and n == n_want
    img = np.ascontiguousarray(vol[3])
    want, n_want = LC.want_clear_border(img)
    out, n = L.remove_boundary_labels(_dev(img))
    assert np.array_equal(_host(out), want) and n == n_want == 1


def test_boundary_whole_labels_mode_removes_the_label():
    from empanada_napari_amd import labels as L
    vol = _two_component_volume()
    want, n_want = LC.want_whole_label_border(vol)
    assert n_want == 2 and not (want == 5).any() and (want == 6).sum() == 2 * 3 * 3
    for src in (_dev(vol), vol):
        out, n = L.remove_boundary_labels(src, whole_labels=True)
        out = _host(out) if not isinstance(out, np.ndarray) else out
        assert np.array_equal(out, want) and n == 2


@pytest.mark.parametrize('dtype', [np.uint16, np.int64])
def test_boundary_modes_on_a_blob_volume(dtype, tmp_path):
    from empanada_napari_amd import labels as L, zstore
    vol = LC.blobs((24, 64, 72), 70, 21, dtype, first=1)
    d = _dev(vol)
    for per_slice in (False, True):
        for whole, stmt in ((False, LC.want_clear_border), (True, LC.want_whole_label_border)):
            want, n_want = LC.per_slice(stmt, vol) if per_slice else stmt(vol)
            out, n = L.remove_boundary_labels(d, whole_labels=whole, per_slice=per_slice)
            assert out.dtype == d.dtype and np.array_equal(_host(out), want) and n == n_want, (per_slice, whole)
            assert np.array_equal(_host(d), vol)
    # a store: the whole-labels mode slab by slab, the reference mode with the array on the device
    za = zstore.DirArray.create(str(tmp_path / 'in'), vol.shape, dtype, (8, 32, 32))
    za[...] = vol
    for whole, stmt in ((False, LC.want_clear_border), (True, LC.want_whole_label_border)):
        zo = zstore.DirArray.create(str(tmp_path / f'out{whole}'), vol.shape, dtype, (8, 32, 32))
        res, n = L.remove_boundary_labels(zstore.DirArray(str(tmp_path / 'in')), whole_labels=whole, out=zo, slab=5)
        want, n_want = stmt(vol)
        assert res is zo and n == n_want and np.array_equal(np.asarray(zo[...]), want)
    same, n = L.remove_boundary_labels(d, inplace=True)
    assert same is d and np.array_equal(_host(d), LC.want_clear_border(vol)[0])


def test_boundary_reference_mode_refuses_what_the_components_cannot_take():
    """through the shape check only: nothing of that size is allocated"""
    from empanada_napari_amd import labels as L
    huge = np.broadcast_to(np.zeros((), np.int32), (1024, 1024, 1024))      # 2^30 voxels, 4 bytes of memory
    with pytest.raises(ValueError, match='whole_labels=True'):
        L.remove_boundary_labels(huge)
    with pytest.raises(ValueError, match='whole_labels=True'):
        L.remove_boundary_labels(huge, per_slice=True)
    vol = np.zeros((2, 8, 8), np.int64)
    vol[1, 3, 3] = 1 << 31      # a label the component kernel would read as background
    with pytest.raises(ValueError, match='whole_labels=True'):
        L.remove_boundary_labels(vol)
    out, n = L.remove_boundary_labels(vol, whole_labels=True)
    assert n == 1 and not out.any()


def test_boundary_reference_mode_sees_a_large_label_in_any_slice():
    """per slice the table is sorted by slice first: the label the component kernel cannot take sits in slice 0, the last slice
    holds small labels only"""
    from empanada_napari_amd import labels as L
    for dtype, big in ((np.uint32, (1 << 31) - 1), (np.int64, 3 << 30)):      # per slice the table's labels end at 2^32
        vol = np.zeros((3, 8, 8), dtype)
        vol[0, 0:2, 0:2] = big      # on the border: left in place it would be a wrong result, not only a missing error
        vol[2, 3, 3] = 7
        for src in (_dev(vol), vol):
            for per_slice in (True, False):
                with pytest.raises(ValueError, match='whole_labels=True'):
                    L.remove_boundary_labels(src, per_slice=per_slice)
        out, n = L.remove_boundary_labels(vol, whole_labels=True, per_slice=True)
        assert n == 1 and out[2, 3, 3] == 7 and not out[0].any()
    ok = np.zeros((3, 8, 8), np.uint32)
    ok[0, 0:2, 0:2] = (1 << 31) - 2      # the largest label the components take
    ok[2, 3, 3] = 7
    out, n = L.remove_boundary_labels(ok, per_slice=True)
    assert n == 1 and out[2, 3, 3] == 7 and not out[0].any()


def test_boundary_reference_mode_checks_its_arguments_before_any_work(tmp_path):
    import torch
    from empanada_napari_amd import labels as L, zstore
    vol = _two_component_volume()
    d = _dev(vol)
    with pytest.raises(TypeError, match='out='):
        L.remove_boundary_labels(d, out=d)
    with pytest.raises(TypeError, match='out='):
        L.remove_boundary_labels(vol, out=vol)
    with pytest.raises(TypeError, match='device'):
        L.remove_boundary_labels(torch.from_numpy(vol))
    strided = _dev(np.zeros((6, 20, 48), np.int32))[:, :, ::2]
    with pytest.raises(ValueError, match='contiguous'):
        L.remove_boundary_labels(strided, inplace=True)
    za = zstore.DirArray.create(str(tmp_path / 'in'), vol.shape, vol.dtype, (3, 10, 12))
    za[...] = vol
    with pytest.raises(TypeError, match='out='):
        L.remove_boundary_labels(za)
    wrong = zstore.DirArray.create(str(tmp_path / 'wrong'), vol.shape, np.int64, (3, 10, 12))
    with pytest.raises(ValueError, match='shape and dtype'):
        L.remove_boundary_labels(za, out=wrong)
    assert np.array_equal(np.asarray(za[...]), vol) and np.array_equal(_host(d), vol)
    # a refusal that needs the table comes before the edit as well: in place, nothing is written
    big = vol.astype(np.int64)
    big[2, 8, 8] = 1 << 33
    for src in (_dev(big), big.copy()):
        with pytest.raises(ValueError, match='whole_labels=True'):
            L.remove_boundary_labels(src, inplace=True)
        assert np.array_equal(src if isinstance(src, np.ndarray) else _host(src), big)
    res, n = L.remove_boundary_labels(za, inplace=True)
    assert res is za and n == 1 and np.array_equal(np.asarray(za[...]), LC.want_clear_border(vol)[0])


def test_clean_labels_tool(tmp_path, capsys):
    """tools/clean_labels.py end to end on a small .npy and on a directory store: argument parsing, the openers, the JSON line
    and the file written"""
    import importlib.util
    import json
    import os
    from empanada_napari_amd import zstore
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'clean_labels.py')
    spec = importlib.util.spec_from_file_location('_clean_labels', tool)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def run(*argv):
        capsys.readouterr()
        res = mod.main([str(a) for a in argv])
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res      # one JSON line, what main returns
        return res

    vol = _two_component_volume() + 1000 * (_two_component_volume() > 0)      # labels 1005 (18 + 24 voxels), 1006 (18), 1007 (36)
    vol[0, 10, 10] = 2003
    src, dst = tmp_path / 'in.npy', tmp_path / 'out.npy'
    np.save(src, vol)
    assert run(src, '--count', '--label-divisor', 1000) == {'shape': list(vol.shape), 'labels': {'1': 3, '2': 1}}
    assert run(src, '--count', '--per-slice')['labels']['0'] == {'1': 2}
    want, n_want = LC.want_small_filter(vol, 18)
    assert run(src, dst, '--min-area', 18) == {'shape': list(vol.shape), 'labels_affected': n_want, 'out': str(dst)} and n_want == 2
    assert np.array_equal(np.load(dst), want)
    assert np.array_equal(np.load(src), vol)
    want, n_want = LC.per_slice(LC.want_small_filter, vol, 9)
    assert run(src, dst, '--min-area', 9, '--per-slice')['labels_affected'] == n_want and np.array_equal(np.load(dst), want)
    for flags, stmt in (((), LC.want_clear_border), (('--whole-labels',), LC.want_whole_label_border)):
        want, n_want = stmt(vol)
        assert run(src, dst, '--boundary', *flags)['labels_affected'] == n_want and np.array_equal(np.load(dst), want)
    # ids that do not occur, a zero and a repeated id do not count
    assert run(src, dst, '--delete', '1006,0,4,1006,2003')['labels_affected'] == 2
    assert np.array_equal(np.load(dst), np.where(np.isin(vol, [1006, 2003]), 0, vol))
    assert run(src, dst, '--merge', '1007,1005,4000')['labels_affected'] == 2
    assert np.array_equal(np.load(dst), np.where(vol == 1007, 1005, vol))
    assert run(src, dst, '--merge', '1007,1005', '--into', 12)['labels_affected'] == 2
    assert np.array_equal(np.load(dst), np.where(np.isin(vol, [1005, 1007]), 12, vol))
    # a directory store in, a directory store out with its shape, dtype and chunks
    za = zstore.DirArray.create(str(tmp_path / 'in.zarr'), vol.shape, vol.dtype, (3, 10, 12))
    za[...] = vol
    want, n_want = LC.want_small_filter(vol, 18)
    assert run(tmp_path / 'in.zarr', tmp_path / 'out.zarr', '--min-area', 18)['labels_affected'] == n_want
    zo = zstore.DirArray(str(tmp_path / 'out.zarr'))
    assert zo.chunks == (3, 10, 12) and zo.dtype == vol.dtype and np.array_equal(np.asarray(zo[...]), want)
    assert run(tmp_path / 'in.zarr', tmp_path / 'del.zarr', '--delete', '1005,5')['labels_affected'] == 1
    assert np.array_equal(np.asarray(zstore.DirArray(str(tmp_path / 'del.zarr'))[...]), np.where(vol == 1005, 0, vol))
    for argv in ((src, '--min-area', 3), (src, dst), (src, dst, '--min-area', 3, '--count')):
        with pytest.raises(SystemExit) as e:
            mod.main([str(a) for a in argv])
        assert e.value.code == 2


def test_engine3d_result_filtered_on_the_device():
    """Engine3d on a small blob stack; the per-slice panoptic maps stay on the device (int64 tensors), are stacked there and go
    through filter_out_small_label_areas without a host copy; the result equals the numpy statement on the downloaded copy"""
    import torch
    from empanada_napari_amd import labels as L, synth, weights
    from empanada_napari_amd.engines import HipPanopticDeepLab
    from empanada_napari_amd.inference import Engine3d
    vol = synth.blob_volume(16, 256, 256, seed=0, n_blobs=24, fast=True)
    cfg = dict(weights.MITONET_PDL_CFG)
    P = weights.fold_state_dict(weights.seeded_state_dict(cfg, seed=0), cfg)
    model = HipPanopticDeepLab(P, cfg, folded=True, precision='fp16x3')
    mc = {'model': model, 'thing_list': [1], 'labels': [1], 'class_names': {1: 'mito'}, 'padding_factor': 16,
          'norms': {'mean': 0.57571, 'std': 0.12765}}
    e3 = Engine3d(mc, label_divisor=10000, median_kernel_size=3, nms_kernel=3, nms_threshold=0.1, confidence_thr=0.5, min_size=50,
                  min_extent=2)
    pan = torch.stack([p for pans in e3.iter_slice_chunks(vol, 0) for p in pans])
    e3.engine.reset()
    assert pan.is_cuda and pan.dtype == torch.int64 and tuple(pan.shape) == vol.shape
    host = pan.cpu().numpy()
    areas = np.unique(host, return_counts=True)[1]
    cut = int(np.median(areas))
    for per_slice in (False, True):
        out, n = L.filter_out_small_label_areas(pan, cut, per_slice=per_slice)
        want, n_want = LC.per_slice(LC.want_small_filter, host, cut) if per_slice else LC.want_small_filter(host, cut)
        assert out.is_cuda and out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), want) and n == n_want
    LC.check_table(L.label_table(pan), host)
    print('engine3d:', len(areas) - 1, 'labels, median area', cut)
