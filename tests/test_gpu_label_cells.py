"""The table protocol the three label kernel families share (csrc/label_table.h), through their C entries themselves: a slab that
fits, a slab that cannot (overflow, and the undo that leaves the table as it was), the move into a larger table, the recount, and
finalize into buffers that are too short.  The statements are the other label tests' numpy references (unique pairs,
labels_case.want_table, measure_case.want_measures); everything is an integer, so every comparison is exact.

The shapes are the smallest at which each step can go wrong: 64 slots is the smallest legal table, slab A (2, 8, 16) holds about
twenty labels, and slab B gives every one of its 256 voxels a label of its own, none of them A's -- 256 keys cannot fit 64 slots
whatever the hash does with them.  B's labels are disjoint from A's because the box of a cell is documented as not undone."""
import ctypes as C

import numpy as np
import pytest

import labels_case as LC
import measure_case as MC

pytestmark = pytest.mark.gpu

D, H, W = 2, 8, 16
N = D * H * W
TOP = (1 << 32) - 1                 # the largest legal label of a pair; the pair (TOP, TOP) equals the table's empty marker
TOP_PAIR = (TOP << 32) | TOP
SENTINEL = 0x5a5a5a5a               # fits every column type


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()      # only the bytes matter


def _labels_a():
    return LC.runs(N, 3, np.uint32, run=5, top=30).reshape(D, H, W)      # 19 distinct values, background among them


def _labels_b():
    return (1000 + np.random.default_rng(5).permutation(N)).astype(np.uint32).reshape(D, H, W)


class Overlap:
    """slabs are (2, depth, H, W): the two sides"""
    name, prefix, slot_bytes, extra = 'overlap', 'emp_label_overlap', 16, ()

    @staticmethod
    def slab_a():
        a, b = _labels_a(), LC.runs(N, 4, np.uint32, run=5, top=2).reshape(D, H, W)
        a.reshape(-1)[10:15] = b.reshape(-1)[10:15] = TOP      # five voxels of the pair that is counted in the header
        return np.stack([a, b])

    @staticmethod
    def slab_b():
        a = _labels_b()
        b = a + 5000
        a.reshape(-1)[100:107] = b.reshape(-1)[100:107] = TOP      # seven more
        return np.stack([a, b])

    @staticmethod
    def accumulate(lib, slab, z0, total_depth, below, table, capacity, stream, ov):
        a, b = _dev(slab[0]), _dev(slab[1])
        return lib.emp_label_overlap_accumulate(_ptr(a), 4, _ptr(b), 4, slab[0].size, table, capacity, stream, ov)

    @staticmethod
    def want(vol):
        key = (vol[0].astype(np.uint64).ravel() << np.uint64(32)) | vol[1].astype(np.uint64).ravel()
        return {int(k): (int(c),) for k, c in zip(*np.unique(key, return_counts=True))}


class Table:
    """slabs are (1, depth, H, W)"""
    name, prefix, slot_bytes = 'table', 'emp_label_table', 40

    @staticmethod
    def slab_a():
        return _labels_a()[None]

    @staticmethod
    def slab_b():
        return _labels_b()[None]

    @staticmethod
    def accumulate(lib, slab, z0, total_depth, below, table, capacity, stream, ov):
        a = _dev(slab[0])
        return lib.emp_label_table_accumulate(_ptr(a), 4, z0, slab.shape[1], H, W, 0, table, capacity, stream, ov)

    @staticmethod
    def want(vol):
        labels, areas, boxes = LC.want_table(vol[0])
        boxes[:, 3:] -= 1      # the entries' boxes are inclusive
        return {int(l): (int(a), *map(int, b)) for l, a, b in zip(labels, areas, boxes)}


class Measure(Table):
    """border_faces off: a slab then has no faces but those between two of its own voxels, or one of them and the halo"""
    name, prefix, slot_bytes = 'measure', 'emp_label_measure', 136

    @staticmethod
    def accumulate(lib, slab, z0, total_depth, below, table, capacity, stream, ov):
        a, h = _dev(slab[0]), None if below is None else _dev(below)
        return lib.emp_label_measure_accumulate(_ptr(a), 4, z0, slab.shape[1], H, W, total_depth, _ptr(h), 0, 0, table, capacity, stream, ov)

    @staticmethod
    def want(vol):
        m = MC.want_measures(vol[0], border_faces=False)
        m['boxes'][:, 3:] -= 1
        rows = np.concatenate([m['areas'][:, None], m['boxes'], m['sum1'], m['sum2'], m['faces']], axis=1)
        return {int(l): tuple(map(int, r)) for l, r in zip(m['labels'], rows)}


FAMILIES = [Overlap, Table, Measure]


def _ptr(t):
    from empanada_napari_amd import _abi
    return _abi.ptr(t)


def _extra(fam):
    import torch
    return {'overlap': [], 'table': [(6, torch.int32)], 'measure': [(6, torch.int32), (9, torch.int64), (3, torch.int64)]}[fam.name]


def _entry(fam, name):
    from empanada_napari_amd import _abi
    return getattr(_abi.load(), f'{fam.prefix}_{name}')


def _new_table(fam, capacity):
    import torch
    from empanada_napari_amd import _abi
    buf = torch.empty(_entry(fam, 'work_bytes')(capacity), dtype=torch.uint8, device='cuda')
    _abi.check(_entry(fam, 'reset')(_abi.ptr(buf), capacity, _abi.stream_ptr()), 'reset')
    return buf


def _accumulate(fam, buf, capacity, slab, z0, below=None):
    """-> *h_overflow"""
    from empanada_napari_amd import _abi
    ov = C.c_int(-1)
    _abi.check(fam.accumulate(_abi.load(), slab, z0, 2 * D, below, _abi.ptr(buf), capacity, _abi.stream_ptr(), C.byref(ov)), 'accumulate')
    return ov.value


def _finalize(fam, buf, capacity, short=0):
    """(num of the counting call, num of the writing call, all rows of buffers of num rows that were pre-filled with SENTINEL as an
    int64 matrix: key, count, further columns); the writing call gets max_out = num - short"""
    import torch
    from empanada_napari_amd import _abi
    extra = _extra(fam)
    num = C.c_int64(-1)
    _abi.check(_entry(fam, 'finalize')(_abi.ptr(buf), capacity, None, None, *(None for _ in extra), 0, C.byref(num), _abi.stream_ptr()), 'finalize')
    k = num.value
    assert k > 0
    cols = [torch.full((k, 1), SENTINEL, dtype=torch.int64, device='cuda') for _ in range(2)]
    cols += [torch.full((k, c), SENTINEL, dtype=dt, device='cuda') for c, dt in extra]
    num2 = C.c_int64(-1)
    _abi.check(_entry(fam, 'finalize')(_abi.ptr(buf), capacity, *(_abi.ptr(t) for t in cols), k - short, C.byref(num2), _abi.stream_ptr()), 'finalize')
    return k, num2.value, np.concatenate([t.cpu().numpy().astype(np.int64) for t in cols], axis=1)


def _as_dict(rows):
    keys = rows[:, 0].copy().view(np.uint64)
    assert len(set(keys.tolist())) == len(keys)      # every key once
    return {int(k): tuple(map(int, r[1:])) for k, r in zip(keys, rows)}


def _cells(fam, buf, capacity):
    k, k2, rows = _finalize(fam, buf, capacity)
    assert k2 == k
    return _as_dict(rows)


@pytest.mark.parametrize('fam', FAMILIES, ids=lambda f: f.name)
def test_overflow_is_undone_and_the_grown_table_takes_the_slab(fam):
    from empanada_napari_amd import _abi
    A, B = fam.slab_a(), fam.slab_b()
    want_a, want_ab = fam.want(A), fam.want(np.concatenate([A, B], axis=1))
    assert 15 <= len(want_a) <= 64 and len(want_ab) - len(want_a) > 64
    below = A[0][-1]      # measure: the face credits B gives A's labels go through the undo as well

    small = _new_table(fam, 64)
    assert _accumulate(fam, small, 64, A, 0) == 0
    assert _cells(fam, small, 64) == want_a

    assert _accumulate(fam, small, 64, B, D, below) == 1      # by pigeonhole
    assert _cells(fam, small, 64) == want_a                   # every column of every row as before the call
    if fam is Overlap:
        assert want_a[TOP_PAIR] == (5,)

    big = _new_table(fam, 1024)
    ov = C.c_int(-1)
    _abi.check(_entry(fam, 'grow')(_abi.ptr(small), 64, _abi.ptr(big), 1024, _abi.stream_ptr(), C.byref(ov)), 'grow')
    assert ov.value == 0
    assert _cells(fam, big, 1024) == want_a
    assert _accumulate(fam, big, 1024, B, D, below) == 0
    assert _cells(fam, big, 1024) == want_ab
    if fam is Overlap:
        assert want_ab[TOP_PAIR] == (12,)

    # finalize into buffers three rows short: the count is the full one, nothing is written behind max_out
    k, k2, rows = _finalize(fam, big, 1024, short=3)
    assert k == k2 == len(want_ab)
    assert (rows[k - 3:] == SENTINEL).all()
    got = _as_dict(rows[:k - 3])
    assert len(got) == k - 3 and all(want_ab.get(key) == row for key, row in got.items())


@pytest.mark.parametrize('fam', FAMILIES, ids=lambda f: f.name)
def test_work_bytes(fam):
    work_bytes = _entry(fam, 'work_bytes')
    assert work_bytes(64) == 64 + 64 * fam.slot_bytes
    for capacity in (63, 96, 1 << 33):
        assert work_bytes(capacity) == 0
