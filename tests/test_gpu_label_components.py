"""Device side of the slab-by-slab connected components: ``labels.label_components``, the three entries of csrc/components.hip
through ctypes, and ``labels.remove_boundary_labels(streamed=True)``.  The expected values are ``oracle.sparse.label_nd`` of the
whole array (tests/components_case.py), a numpy union-find for the entries, and ``labels_case.want_clear_border``.  Everything is
integer, so every comparison is exact."""
import numpy as np
import pytest

import components_case as CC
import labels_case as LC

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint16, np.int32, np.uint32, np.int64]
CASES = CC.cases()
GROUPS = {'random': [k for k in sorted(CASES) if k.startswith('random')],
          'pairs': [k for k in sorted(CASES) if k.startswith('pair')],
          'shapes': [k for k in sorted(CASES) if not k.startswith(('random', 'pair'))]}


def _dev(x):
    import torch
    if x.dtype in (np.uint16, np.uint32):      # no arithmetic is needed on the tensor: reinterpret the bytes
        return torch.from_numpy(x.view({2: np.int16, 4: np.int32}[x.itemsize])).cuda().view({2: torch.uint16, 4: torch.uint32}[x.itemsize])
    return torch.from_numpy(x).cuda()


def _host(t):
    import torch
    if isinstance(t, np.ndarray):
        return t
    if not isinstance(t, torch.Tensor):
        return np.asarray(t[...])
    if t.dtype in (torch.uint16, torch.uint32):
        return t.view({torch.uint16: torch.int16, torch.uint32: torch.int32}[t.dtype]).cpu().numpy().view(
            {torch.uint16: np.uint16, torch.uint32: np.uint32}[t.dtype])
    return t.cpu().numpy()


def _slabs(arr):
    D = arr.shape[0]
    return sorted({s for s in CC.SLABS if s < D} | {D}) + [None]


def _store(path, arr, chunks=None):
    from empanada_napari_amd import zstore
    za = zstore.DirArray.create(str(path), arr.shape, arr.dtype, chunks or tuple(min(s, 4) for s in arr.shape))
    za[...] = arr
    return za


# ----------------------------------------------------------------------------
# label_components
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('group', sorted(GROUPS))
def test_every_case_every_slab_equals_the_reference(group):
    """... and with it every slab gives the same, which is what sparse.ccl26 gives for the whole volume"""
    import torch
    from empanada_napari_amd import labels as L, sparse
    for name in GROUPS[group]:
        arr = CASES[name]
        want = CC.cached_reference(name, arr)
        d = _dev(arr)
        if arr.ndim == 3:
            assert np.array_equal(_host(sparse.ccl26(d)), want), name
        for slab in _slabs(arr):
            got, count = L.label_components(d, slab=slab)
            assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and tuple(got.shape) == arr.shape
            assert np.array_equal(_host(got), want), (name, slab)
            assert count == int(want.max()), (name, slab)
        got, count = L.label_components(arr, slab=1)      # the host path: staging, halo copies, download
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, want) and count == int(want.max()), name


def test_image_runs_by_rows():
    from empanada_napari_amd import labels as L
    img = CASES['image']
    want = CC.cached_reference('image', img)
    assert want.max() > 50
    for src in (_dev(img), img):
        for slab in (1, 7, 40, None):
            stats = {}
            got, count = L.label_components(src, slab=slab, _stats=stats)
            assert np.array_equal(_host(got), want) and count == int(want.max())
            if slab == 7:
                assert stats['slabs'] == 6      # rows, not the one slice an image would be as a volume
    assert L.label_components(img, return_count=False).shape == img.shape


@pytest.mark.parametrize('dtype', DTYPES)
def test_every_dtype_and_every_kind_of_source(dtype, tmp_path):
    from empanada_napari_amd import labels as L
    vol = CC.random_volume(21, (7, 6, 9)).astype(dtype)
    top = {1: 255, 2: 65535}.get(np.dtype(dtype).itemsize, (1 << 31) - 2)      # the largest label the type / the components take
    vol[vol == 2] = top
    vol[3, 2, 4] = vol[4, 3, 5] = top - 1      # two voxels of one value, corner to corner across the seam 3 | 4 of slab 4 ...
    vol[3, 2, 5] = top      # ... beside a neighbour value that differs in the low bits only
    want = CC.reference(vol.astype(np.int64))
    for kind, src in (('device', _dev(vol)), ('numpy', vol), ('store', _store(tmp_path / 'in', vol))):
        for slab in (3, 4, None):
            got, count = L.label_components(src, slab=slab)
            assert np.array_equal(_host(got), want), (kind, slab)
            assert count == int(want.max())


def test_every_kind_of_out(tmp_path):
    import torch
    from empanada_napari_amd import labels as L, zstore
    vol = CASES['random_12x16x24']
    want = CC.cached_reference('random_12x16x24', vol)
    sources = {'device': _dev(vol), 'numpy': vol, 'store': _store(tmp_path / 'in', vol, (5, 16, 24))}
    for i, (kind, src) in enumerate(sources.items()):
        for slab in (5, 12):      # two passes; one slab, whose ids are the result
            outs = {'device': torch.full(vol.shape, -7, dtype=torch.int32, device='cuda'), 'numpy': np.full(vol.shape, -7, np.int32),
                    'store': zstore.DirArray.create(str(tmp_path / f'out{i}_{slab}'), vol.shape, np.int32, (4, 16, 24))}
            for okind, out in outs.items():
                got, count = L.label_components(src, out=out, slab=slab)
                assert got is out and count == int(want.max()), (kind, okind, slab)
                assert np.array_equal(_host(out), want), (kind, okind, slab)
    assert np.array_equal(np.asarray(zstore.DirArray(str(tmp_path / 'out2_5'))[...]), want)      # a store into a store, read again


def test_parent_array_doubles_and_one_slab_runs_the_ccl_once():
    from empanada_napari_amd import labels as L
    vol = CC.capacity_volume()
    want = CC.reference(vol)
    stats = {}
    got, count = L.label_components(_dev(vol), slab=2, _capacity=4, _stats=stats)
    assert np.array_equal(_host(got), want) and count == int(want.max()) > 2048
    assert stats['doublings'] >= 9 and stats['slabs'] == 8 and stats['ccl_runs'] == 16 and stats['provisional'] >= count
    got, _ = L.label_components(vol, slab=3, _capacity=4)      # an uneven last slab, from the host
    assert np.array_equal(got, want)
    for src in (_dev(vol), vol):
        stats = {}
        got, count = L.label_components(src, _stats=stats)
        assert np.array_equal(_host(got), want) and stats == {'slabs': 1, 'ccl_runs': 1, 'doublings': 0, 'provisional': count, 'count': count}


def test_refusals_come_from_the_shape_alone_and_before_any_write():
    """nothing of these sizes is allocated: a zero broadcast to the shape"""
    import torch
    from empanada_napari_amd import labels as L
    zero = np.zeros((), np.int32)
    with pytest.raises(ValueError, match='2-D or 3-D'):
        L.label_components(np.broadcast_to(zero, (2, 3, 4, 5)))
    with pytest.raises(ValueError, match='one slice'):
        L.label_components(np.broadcast_to(zero, (2, 1 << 15, 1 << 15)))
    with pytest.raises(ValueError, match='smaller slab='):
        L.label_components(np.broadcast_to(zero, (64, 1 << 13, 1 << 13)), slab=16)
    vol = CC.random_volume(2).astype(np.int64)
    for kind, out in (('device', torch.full(vol.shape, -7, dtype=torch.int32, device='cuda')), ('numpy', np.full(vol.shape, -7, np.int32))):
        big = vol.copy()
        big[6, 5, 8] = (1 << 31) - 1      # in the last slab: found before the first one is written
        for src in (_dev(big), big):
            with pytest.raises(ValueError, match=r'labels below 2\^31 - 1'):
                L.label_components(src, out=out, slab=2)
        assert (_host(out) == -7).all(), kind
    with pytest.raises(ValueError, match='int32'):
        L.label_components(vol, out=np.zeros(vol.shape, np.int64))
    with pytest.raises(ValueError, match='shape'):
        L.label_components(_dev(vol), out=torch.zeros((7, 6, 8), dtype=torch.int32, device='cuda'))
    with pytest.raises(TypeError, match='device'):
        L.label_components(vol, out=torch.zeros(vol.shape, dtype=torch.int32))
    with pytest.raises(ValueError, match='contiguous'):
        L.label_components(vol, out=torch.zeros((7, 6, 18), dtype=torch.int32, device='cuda')[:, :, ::2])
    empty, n = L.label_components(np.zeros((0, 4, 5), np.uint8))
    assert empty.shape == (0, 4, 5) and n == 0


# ----------------------------------------------------------------------------
# the entries, through ctypes
# ----------------------------------------------------------------------------
def _rank(parent, G):
    """emp_ccl_rank_roots on a host forest -> (lut, count)"""
    import torch
    from empanada_napari_amd import _abi
    lib = _abi.load()
    d_parent = torch.from_numpy(np.asarray(parent, np.int32)).cuda()
    lut = torch.full((G + 1,), -5, dtype=torch.int32, device='cuda')
    count = torch.full((1,), -5, dtype=torch.int32, device='cuda')
    work = torch.empty(int(lib.emp_ccl_rank_roots_work_bytes(G)), dtype=torch.uint8, device='cuda')
    _abi.check(lib.emp_ccl_rank_roots(_abi.ptr(d_parent), G, _abi.ptr(lut), _abi.ptr(count), _abi.ptr(work), _abi.stream_ptr()), 'emp_ccl_rank_roots')
    return lut.cpu().numpy(), int(count.item())


@pytest.mark.parametrize('shape', [(5, 7), (1, 300), (33, 65), (300, 1)])
@pytest.mark.parametrize('dtype', [np.int32, np.int64])
def test_seam_entry_against_a_numpy_union_find(shape, dtype):
    import torch
    from empanada_napari_amd import _abi
    lib = _abi.load()
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    vol = (rng.integers(1, 4, (2,) + shape) * (rng.random((2,) + shape) < 0.55)).astype(dtype)
    if dtype == np.int64:
        vol[vol == 3] = (1 << 40) + 3      # equal in the low 32 bits to no other value; the entry compares all 64
        vol[vol == 2] = (1 << 40) + 2
    pid, cid = CC.reference(vol[:1])[0], CC.reference(vol[1:])[0]
    if dtype == np.int64:      # what the CCL's range would have read as background has no id and takes no part
        pid, cid = np.where(vol[0] == (1 << 40) + 2, 0, pid), np.where(vol[1] == (1 << 40) + 2, 0, cid)
    base_prev, base_cur = 3, 3 + int(pid.max()) + 2      # ids before, and between, that nothing touches
    G = base_cur + int(cid.max())
    forest = CC.Forest()
    forest.extend(G)
    for a, b in CC.seam_unions(vol[0], pid, vol[1], cid, base_prev, base_cur):
        forest.union(a, b)
    want_lut, want_count = forest.lut()
    parent = torch.arange(G + 1 + 5, dtype=torch.int32, device='cuda')      # longer than needed: the tail stays as it is
    args = [_dev(np.ascontiguousarray(a)) for a in (vol[0], pid.astype(np.int32), vol[1], cid.astype(np.int32))]
    _abi.check(lib.emp_ccl_seam(*(_abi.ptr(a) for a in args), vol.itemsize, shape[0], shape[1], base_prev, base_cur, _abi.ptr(parent), G + 1,
                                _abi.stream_ptr()), 'emp_ccl_seam')
    got = parent.cpu().numpy()
    assert np.array_equal(got[G + 1:], np.arange(G + 1, G + 6)) and got[0] == 0
    assert (got[1:G + 1] <= np.arange(1, G + 1)).all()      # a parent is never a larger id
    lut, count = _rank(got[:G + 1], G)
    assert np.array_equal(lut, want_lut) and count == want_count
    assert want_count < G      # something was united


def test_seam_entry_refuses_bad_arguments():
    import torch
    from empanada_napari_amd import _abi
    lib = _abi.load()
    t = torch.zeros(16, dtype=torch.int32, device='cuda')
    p = _abi.ptr(t)
    for args in ((p, p, p, p, 2, 4, 4, 0, 0, p, 16), (p, p, p, p, 4, 4, 4, 5, 3, p, 16), (p, p, p, p, 4, 4, 4, 0, 16, p, 16),
                 (p, p, p, p, 4, 0, 4, 0, 0, p, 16), (p, p, p, p, 4, 1 << 15, 1 << 15, 0, 0, p, 16), (p, p, p, None, 4, 4, 4, 0, 0, p, 16)):
        assert lib.emp_ccl_seam(*args, _abi.stream_ptr()) != 0, args
    assert lib.emp_ccl_rank_roots_work_bytes(-1) == 0 and lib.emp_ccl_rank_roots_work_bytes((1 << 31) - 1) == 0
    assert lib.emp_ccl_rank_roots(p, -1, p, p, p, _abi.stream_ptr()) != 0
    assert lib.emp_ccl_lut(p, p, 16, 16, p, 16, _abi.stream_ptr()) != 0 and lib.emp_ccl_lut(p, p, -1, 16, p, 16, _abi.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert not t.any().item()


def test_rank_roots_entry_on_hand_written_forests():
    lut, count = _rank([0], 0)
    assert lut.tolist() == [0] and count == 0
    # ids 1..9: {1, 4, 9} under 1 (9 through 4), {2}, {3, 5} under 3, {6, 7, 8} under 6 (8 through 7)
    parent = [0, 1, 2, 3, 1, 3, 6, 6, 7, 4]
    lut, count = _rank(parent, 9)
    assert lut.tolist() == [0, 1, 2, 3, 1, 3, 4, 4, 4, 1] and count == 4
    lut, count = _rank(list(range(6)), 5)      # nothing united: the identity
    assert lut.tolist() == list(range(6)) and count == 5
    # more than one block of the count and rank kernels, with chains: id g hangs under g - 3, so three sets
    G = 3 * 2048 + 77
    parent = np.arange(G + 1)
    parent[4:] -= 3
    lut, count = _rank(parent, G)
    assert count == 3 and np.array_equal(lut[1:], (np.arange(G) % 3) + 1) and lut[0] == 0
    # every second id a root of its own and of its successor: ranks run through every block
    parent = np.arange(G + 1)
    parent[2::2] -= 1
    lut, count = _rank(parent, G)
    assert count == (G + 1) // 2 and np.array_equal(lut[1:], np.arange(G) // 2 + 1)


def test_lut_entry():
    import torch
    from empanada_napari_amd import _abi
    lib = _abi.load()
    rng = np.random.default_rng(8)
    n, base, G = 256 * 64 * 3 + 11, 40, 140      # more than one block, a ragged end
    ids = (rng.integers(1, 101, n) * (rng.random(n) < 0.7)).astype(np.int32)
    lut = rng.integers(1, 1000, G + 1).astype(np.int32)
    lut[0] = 0
    d_ids, d_lut = _dev(ids), _dev(lut)
    out = torch.full((n + 3,), -9, dtype=torch.int32, device='cuda')
    _abi.check(lib.emp_ccl_lut(_abi.ptr(d_ids), _abi.ptr(d_lut), base, G + 1, _abi.ptr(out), n, _abi.stream_ptr()), 'emp_ccl_lut')
    want = np.where(ids > 0, lut[base + ids], 0)
    assert np.array_equal(out.cpu().numpy()[:n], want) and (out.cpu().numpy()[n:] == -9).all()
    _abi.check(lib.emp_ccl_lut(_abi.ptr(d_ids), _abi.ptr(d_lut), base, G + 1, _abi.ptr(d_ids), n, _abi.stream_ptr()), 'emp_ccl_lut')      # in place
    assert np.array_equal(d_ids.cpu().numpy(), want)
    _abi.check(lib.emp_ccl_lut(_abi.ptr(d_ids), _abi.ptr(d_lut), base, G + 1, _abi.ptr(out), 0, _abi.stream_ptr()), 'emp_ccl_lut')      # nothing to do


# ----------------------------------------------------------------------------
# remove_boundary_labels(streamed=True)
# ----------------------------------------------------------------------------
def _border_volumes():
    pieces = CC.border_pieces()
    blobs = LC.blobs((11, 20, 24), 14, 4, np.uint32)
    return {'pieces': pieces, 'blobs': blobs}


_WANT = {}


def _want_clear(name, vol):
    if name not in _WANT:
        _WANT[name] = LC.want_clear_border(vol)
    return _WANT[name]


@pytest.mark.parametrize('name', ['pieces', 'blobs'])
def test_streamed_boundary_removal_equals_clear_border_and_the_unstreamed_call(name, tmp_path):
    import torch
    from empanada_napari_amd import labels as L, zstore
    vol = _border_volumes()[name]
    want, n_want = _want_clear(name, vol)
    if name == 'pieces':
        # 5 starts inside and reaches a face in a later slab; 6 keeps its interior piece and is not counted; 8 touches a face with
        # one voxel of a later slice; 7 is interior
        assert n_want == 2 and not (want == 5).any() and not (want == 8).any() and (want == 7).sum() == (vol == 7).sum()
        assert (want == 6).sum() == 2 * 2 * 2
    base, n_base = L.remove_boundary_labels(_dev(vol))
    assert np.array_equal(_host(base), want) and n_base == n_want
    for slab in (1, 5):
        out, n = L.remove_boundary_labels(_dev(vol), streamed=True, slab=slab)
        assert isinstance(out, torch.Tensor) and np.array_equal(_host(out), want) and n == n_want, slab
        out, n = L.remove_boundary_labels(vol, streamed=True, slab=slab)
        assert isinstance(out, np.ndarray) and out.dtype == vol.dtype and np.array_equal(out, want) and n == n_want, slab
        za = _store(tmp_path / f'in{slab}', vol, (4, 8, 8))
        zo = zstore.DirArray.create(str(tmp_path / f'out{slab}'), vol.shape, vol.dtype, (4, 8, 8))
        zc = zstore.DirArray.create(str(tmp_path / f'comp{slab}'), vol.shape, np.int32, (4, 8, 8))
        res, n = L.remove_boundary_labels(za, streamed=True, slab=slab, out=zo, components=zc)
        assert res is zo and n == n_want and np.array_equal(np.asarray(zo[...]), want), slab
        assert np.array_equal(np.asarray(zc[...]), CC.reference(vol.astype(np.int64)))      # the caller's components, written
    # in place, and components kept on the device
    d = _dev(vol)
    comps = torch.zeros(vol.shape, dtype=torch.int32, device='cuda')
    res, n = L.remove_boundary_labels(d, streamed=True, slab=3, inplace=True, components=comps)
    assert res is d and np.array_equal(_host(d), want) and n == n_want and comps.max().item() == CC.reference(vol.astype(np.int64)).max()
    own = vol.copy()
    res, n = L.remove_boundary_labels(own, streamed=True, slab=3, inplace=True)
    assert res is own and np.array_equal(own, want) and n == n_want


def test_streamed_boundary_removal_of_an_image_and_its_refusals(tmp_path):
    from empanada_napari_amd import labels as L
    img = LC.blobs((40, 56), 12, 2, np.uint16)
    want, n_want = LC.want_clear_border(img)
    for src in (_dev(img), img):
        out, n = L.remove_boundary_labels(src, streamed=True, slab=7)
        assert np.array_equal(_host(out), want) and n == n_want
    vol = CC.border_pieces()
    with pytest.raises(ValueError, match='per_slice'):
        L.remove_boundary_labels(vol, streamed=True, per_slice=True)
    with pytest.raises(TypeError, match='out='):
        L.remove_boundary_labels(vol, streamed=True, out=vol)
    with pytest.raises(ValueError, match='one slice'):
        L.remove_boundary_labels(np.broadcast_to(np.zeros((), np.int32), (4, 1 << 15, 1 << 15)), streamed=True)
    big = vol.astype(np.int64)
    big[9, 5, 5] = 1 << 33
    comps = np.full(vol.shape, -7, np.int32)
    for src in (_dev(big), big.copy()):
        with pytest.raises(ValueError, match=r'labels below 2\^31 - 1'):
            L.remove_boundary_labels(src, streamed=True, inplace=True, slab=2, components=comps)
        assert np.array_equal(_host(src), big) and (comps == -7).all()
    # the unstreamed refusal names both ways out
    with pytest.raises(ValueError, match='whole_labels=True.*streamed=True'):
        L.remove_boundary_labels(np.broadcast_to(np.zeros((), np.int32), (1024, 1024, 1024)))


# ----------------------------------------------------------------------------
# the tools
# ----------------------------------------------------------------------------
def _tool(name):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', name + '.py')
    spec = importlib.util.spec_from_file_location('_' + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_label_components_tool_and_the_streamed_boundary_flag(tmp_path, capsys):
    """tools/label_components.py and tools/clean_labels.py --boundary --streamed end to end on a small .npy and on a directory
    store: the openers, the JSON line and the file written"""
    import json
    from empanada_napari_amd import zstore
    vol = CC.border_pieces()
    want = CC.reference(vol.astype(np.int64))
    np.save(tmp_path / 'in.npy', vol)
    _store(tmp_path / 'in.zarr', vol, (4, 6, 7))
    comp, clean = _tool('label_components'), _tool('clean_labels')

    def run(mod, *argv):
        capsys.readouterr()
        res = mod.main([str(a) for a in argv])
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res      # one JSON line, what main returns
        return res
    res = run(comp, tmp_path / 'in.npy', tmp_path / 'cc.npy', '--slab', 3)
    assert res == {'shape': list(vol.shape), 'components': int(want.max()), 'slabs': 4, 'out': str(tmp_path / 'cc.npy')}
    got = np.load(tmp_path / 'cc.npy')
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert run(comp, tmp_path / 'in.zarr', tmp_path / 'cc.zarr')['components'] == int(want.max())
    zo = zstore.DirArray(str(tmp_path / 'cc.zarr'))
    assert zo.chunks == (4, 6, 7) and zo.dtype == np.int32 and np.array_equal(np.asarray(zo[...]), want)
    cleared, n_want = LC.want_clear_border(vol)
    assert run(clean, tmp_path / 'in.npy', tmp_path / 'out.npy', '--boundary', '--streamed')['labels_affected'] == n_want
    assert np.array_equal(np.load(tmp_path / 'out.npy'), cleared) and np.array_equal(np.load(tmp_path / 'in.npy'), vol)
    assert run(clean, tmp_path / 'in.zarr', tmp_path / 'out.zarr', '--boundary', '--streamed')['labels_affected'] == n_want
    assert np.array_equal(np.asarray(zstore.DirArray(str(tmp_path / 'out.zarr'))[...]), cleared)
    with pytest.raises(SystemExit) as e:
        clean.main([str(tmp_path / 'in.npy'), str(tmp_path / 'out.npy'), '--boundary', '--streamed', '--whole-labels'])
    assert e.value.code == 2
