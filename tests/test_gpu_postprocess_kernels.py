"""The kernels of csrc/postprocess.hip, each through its own C-ABI entry (emp_logits_to_prob, emp_median_slices,
emp_median_recursive, emp_instance_cells, emp_panoptic_merge) against the plain references of tests/postprocess_case.py, at the
smallest shapes that still reach each branch: the second trip of every grid-stride loop, every median kernel size, every centre
count at which the vote changes its rule or its path, the hash table of the merge beyond its capacity.  Integer outputs are
compared for equality; the probabilities keep the bound derived in tests/postprocess_case.py (printed as RATIO lines).
tests/test_postprocess_case_host.py shows on the CPU that the references reproduce the goldens and reject planted defects.
Every output buffer is pre-filled with a sentinel and carries PP.GUARD sentinel elements behind it (and in front of it where a
view is passed); work buffers are exactly *_work_bytes long, filled with 0xA5, with a guard that must survive."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import postprocess_case as PP
from oracle import postprocess as opp

pytestmark = pytest.mark.gpu

f32 = np.float32


def _abi():
    from empanada_napari_amd import _abi
    return _abi


def _lib():
    return _abi().load()


def _stream():
    return _abi().stream_ptr(torch.device('cuda:0'))


def _cuda(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()      # (a copy: the cached cases are read-only)


class Buf:
    """`front` + n + PP.GUARD elements of `fill`; .view is the n elements to write"""

    def __init__(self, n, dtype, fill, front=0):
        self.n, self.front, self.fill = int(n), front, fill
        self.t = torch.full((front + self.n + PP.GUARD,), fill, dtype=dtype, device='cuda:0')
        self.view = self.t[front:front + self.n]

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def result(self, what):
        torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        assert (a[:self.front] == self.fill).all(), f'{what}: written in front of the buffer'
        assert (a[self.front + self.n:] == self.fill).all(), f'{what}: the guard behind the buffer was written'
        return a[self.front:self.front + self.n].copy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.t == self.fill).all())


class _env:
    """an environment switch that the library reads per call"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


def _ids(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


# ----------------------------------------------------------------------------
# emp_logits_to_prob: sigmoid_kernel, softmax_kernel
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('C_', PP.PROB_CLASSES)
@pytest.mark.parametrize('shape', PP.PROB_SHAPES, ids=_ids)
def test_logits_to_prob(shape, C_):
    N, H, W = shape
    x = PP.prob_input(N, C_, H, W)
    out = Buf(x.size, torch.float32, PP.F32_SENTINEL, front=PP.GUARD)
    dx = _cuda(x)
    _abi().check(_lib().emp_logits_to_prob(_abi().ptr(dx), out.ptr(), N, C_, H, W, _stream()), 'emp_logits_to_prob')
    got = out.result('prob').reshape(x.shape)
    ref = PP.prob_ref(x)
    bound = PP.prob_bound(ref, C_)
    ratio = PP.worst_ratio(got, ref, bound)
    print(f'RATIO logits_to_prob C {C_} {N}x{H}x{W}: largest err / bound {ratio:.4f}')
    bad = PP.violations(got, ref, bound)
    assert bad == 0, f'{bad} of {ref.size} values beyond the bound, worst err / bound {ratio:.3g}'
    if C_ == 1:
        assert got[x == f32(np.inf)].tolist() == [1.0] and got[x == f32(-np.inf)].tolist() == [0.0]


def test_logits_to_prob_refuses_bad_shapes():
    out = Buf(16, torch.float32, PP.F32_SENTINEL)
    dx = _cuda(np.zeros(16, f32))
    for N, C_, H, W in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, -1)):
        assert _lib().emp_logits_to_prob(_abi().ptr(dx), out.ptr(), N, C_, H, W, _stream()) != 0
    assert out.untouched()


# ----------------------------------------------------------------------------
# emp_median_slices: median_kernel
# ----------------------------------------------------------------------------
def _median_slices(x, out):
    ks = x.shape[0]
    t = [_cuda(x[k]) for k in range(ks)]
    ptrs = (C.c_void_p * max(ks, 1))(*[a.data_ptr() for a in t])
    return _lib().emp_median_slices(ptrs, ks, out.ptr(), x.shape[1], _stream())


@pytest.mark.parametrize('count', [5, PP.BIG_COUNT])
@pytest.mark.parametrize('ks', PP.MEDIAN_KS)
def test_median_slices(ks, count):
    x = PP.median_input(ks, count)
    out = Buf(count, torch.float32, PP.F32_SENTINEL, front=PP.GUARD)
    _abi().check(_median_slices(x, out), 'emp_median_slices')
    np.testing.assert_array_equal(out.result(f'median ks {ks}'), PP.median_ref(x))


@pytest.mark.parametrize('ks', [0, 2, 4, 14, 16, 17])
def test_median_slices_refuses_even_or_oversized_ks(ks):
    x = PP.median_input(max(ks, 1), 5)
    out = Buf(5, torch.float32, PP.F32_SENTINEL)
    assert _median_slices(x[:ks] if ks else x[:0].reshape(0, 5), out) != 0
    assert out.untouched()


# ----------------------------------------------------------------------------
# emp_median_recursive: median_recursive_kernel<3 .. 15>
# ----------------------------------------------------------------------------
def _recursive(dhist, draw_ptr, n_raw, ks, n_out, dout_ptr, count):
    return _lib().emp_median_recursive(_abi().ptr(dhist), draw_ptr, n_raw, ks, n_out, dout_ptr, count, _stream())


@pytest.mark.parametrize('ks,n_out,extra,count', PP.recursive_cases(), ids=_ids)
def test_median_recursive(ks, n_out, extra, count):
    mid = (ks - 1) // 2
    n_raw = n_out + mid + extra
    x = PP.median_input(mid + n_raw, count, seed=ks + n_out)
    hist, raw = x[:mid], x[mid:]
    ref = PP.median_recursive_ref(hist, raw, ks, n_out)
    dhist, draw = _cuda(hist), _cuda(raw)
    out = Buf(n_out * count, torch.float32, PP.F32_SENTINEL, front=PP.GUARD)
    _abi().check(_recursive(dhist, _abi().ptr(draw), n_raw, ks, n_out, out.ptr(), count), 'emp_median_recursive')
    got = out.result(f'recursive ks {ks}').reshape(n_out, count)
    np.testing.assert_array_equal(got, ref)
    assert torch.equal(draw.cpu(), torch.from_numpy(raw)) and torch.equal(dhist.cpu(), torch.from_numpy(hist))
    # in place (out == raw), as the slab filter of multigpu.py calls it
    inplace = Buf(n_raw * count, torch.float32, PP.F32_SENTINEL, front=PP.GUARD)
    inplace.view.copy_(draw.reshape(-1))
    _abi().check(_recursive(dhist, inplace.ptr(), n_raw, ks, n_out, inplace.ptr(), count), 'emp_median_recursive in place')
    both = inplace.result(f'recursive in place ks {ks}').reshape(n_raw, count)
    np.testing.assert_array_equal(both[:n_out], got)
    np.testing.assert_array_equal(both[n_out:], raw[n_out:])


def test_median_recursive_refuses_bad_arguments():
    count, ks, mid, n_out = 7, 5, 2, 3
    x = PP.median_input(mid + n_out + mid, count)
    dhist, draw = _cuda(x[:mid]), _cuda(x[mid:])
    out = Buf(n_out * count, torch.float32, PP.F32_SENTINEL)
    r, o, n_raw = _abi().ptr(draw), out.ptr(), n_out + mid
    assert _recursive(dhist, r, n_raw, 4, n_out, o, count) != 0           # even
    assert _recursive(dhist, r, n_raw, 1, n_out, o, count) != 0           # no recursion at ks 1
    assert _recursive(dhist, r, n_raw, 17, n_out, o, count) != 0          # above MAX_KS
    assert _recursive(dhist, r, n_raw, ks, 0, o, count) != 0              # nothing to write
    assert _recursive(dhist, r, n_raw - 1, ks, n_out, o, count) != 0      # fewer than n_out + mid raw maps
    assert _recursive(dhist, r, n_raw, ks, n_out, o, 0) != 0              # empty maps
    assert _recursive(None, r, n_raw, ks, n_out, o, count) != 0           # the history is always read
    assert _recursive(dhist, None, n_raw, ks, n_out, o, count) != 0
    assert _recursive(dhist, r, n_raw, ks, n_out, None, count) != 0
    assert out.untouched()
    _abi().check(_recursive(dhist, r, n_raw, ks, n_out, o, count), 'emp_median_recursive')
    np.testing.assert_array_equal(out.result('recursive').reshape(n_out, count), PP.median_recursive_ref(x[:mid], x[mid:], ks, n_out))


# ----------------------------------------------------------------------------
# emp_instance_cells
# ----------------------------------------------------------------------------
def _instance_cells(ctr, off, thr, k, step, up, max_centers, grid=None):
    """-> (cells (N, h*up, w*up), centres (N, max_centers, 2), num (N,)) as numpy; every guard checked"""
    N, _, h, w = ctr.shape
    lib = _lib()
    cells = Buf(N * h * up * w * up, torch.int32, PP.I32_SENTINEL, front=PP.GUARD)
    centres = Buf(N * max_centers * 2, torch.int32, PP.I32_SENTINEL, front=PP.GUARD)
    num = Buf(N, torch.int32, PP.I32_SENTINEL, front=PP.GUARD)
    nbytes = int(lib.emp_instance_cells_work_bytes(N, h, w))
    work = Buf(nbytes, torch.uint8, PP.WORK_FILL)
    dctr, doff = _cuda(ctr), _cuda(off)
    with _env('EMP_VOTE_GRID', grid):
        _abi().check(lib.emp_instance_cells(_abi().ptr(dctr), _abi().ptr(doff), N, h, w, float(thr), int(k), int(step), int(up),
                                            cells.ptr(), centres.ptr(), num.ptr(), int(max_centers), work.ptr(), _stream()),
                     'emp_instance_cells')
    work.result('instance_cells workspace')
    return (cells.result('cells').reshape(N, h * up, w * up), centres.result('centres').reshape(N, max_centers, 2),
            num.result('num_centers'))


def _assert_centres(got, num, ref, max_centers, what):
    for n, r in enumerate(ref):
        assert int(num[n]) == r.shape[0], f'{what} image {n}: {int(num[n])} centres, reference {r.shape[0]}'      # unclamped
        kept = min(r.shape[0], max_centers)
        np.testing.assert_array_equal(got[n, :kept], r[:kept], err_msg=f'{what} image {n}')
        assert (got[n, kept:] == PP.I32_SENTINEL).all(), f'{what} image {n}: written behind the last centre'


@pytest.mark.parametrize('k', PP.NMS_KERNELS)
@pytest.mark.parametrize('shape', PP.NMS_MAPS, ids=_ids)
def test_centres(shape, k):
    """nms_mask_kernel + centers_kernel: nms_kernel 1 .. 15 (larger than the small maps), maps of 1 .. 16 383 pixels (fewer than
    32, h*w % 64 in 1..32, w == 1, h == 1, more than 256 mask words), plateaus on every border, values equal to the threshold,
    thresholds 0.25, 0 and -1, N = 3 with one all-zero image"""
    h, w = shape
    ctr = PP.nms_input(h, w)
    off = np.zeros((PP.NMS_N, 2, h, w), f32)
    for thr in (PP.NMS_THR, 0.0, -1.0):
        ref = PP.centers_ref(ctr, thr, k)
        _, got, num = _instance_cells(ctr, off, thr, k, 1, 1, h * w)
        _assert_centres(got, num, ref, h * w, f'{h}x{w} k {k} thr {thr}')
        assert int(num[1]) == 0 and (h * w < 20 or int(num[0]) > 0)


@pytest.mark.parametrize('max_centers', [1, 5])
def test_more_centres_than_max_centers(max_centers):
    """the count comes back unclamped, the first max_centers entries are the reference's first, nothing is written behind the
    buffer, and the vote uses exactly those centres"""
    h, w = 9, 11
    ctr = PP.nms_input(h, w)
    off = PP.quarter_votes(PP.NMS_N, h, w, 1, seed=9)
    cells_ref, ref = PP.cells_ref(ctr, off, 0.0, 1, 1, 2, max_centers=max_centers)
    assert ref[0].shape[0] > 20 and ref[2].shape[0] > 20 and ref[1].shape[0] == 0
    cells, got, num = _instance_cells(ctr, off, 0.0, 1, 1, 2, max_centers)
    _assert_centres(got, num, ref, max_centers, 'overflow')
    np.testing.assert_array_equal(cells, cells_ref)


def _vote(counts, h, w, step, up, grid, generic=False):
    ctr, off, ref, centres, mask = PP.vote_case(counts, h, w, step, generic)
    max_centers = max(max(counts), 1)      # exactly the largest count: the last centre is the last entry of the buffer
    cells, got, num = _instance_cells(ctr, off, 0.1, 1, step, up, max_centers, grid)
    _assert_centres(got, num, centres, max_centers, f'{counts}')
    want = opp.nearest_upsample(ref, up)
    if mask is None:
        np.testing.assert_array_equal(cells, want, err_msg=f'centres {counts} step {step} up {up} EMP_VOTE_GRID {grid}')
    else:
        m = opp.nearest_upsample(mask, up)
        bad = int(((cells != want) & ~m).sum())
        assert bad == 0, f'{bad} cells differ outside the near-tie mask ({int(mask.sum())} pixels masked)'
    return cells


@pytest.mark.parametrize('grid', [None, '0'], ids=['grid', 'scan'])
@pytest.mark.parametrize('counts,h,w', PP.VOTE_COUNT_CASES, ids=_ids)
def test_vote_at_every_centre_count_boundary(counts, h, w, grid):
    """0 | 1, 20 | 21 (argmin <-> the 1e5 start value), 191 | 192 (GRID_MIN: one image of the batch on each side), 1024 | 1025
    (CTR_TILE) and 16384 | 16385 (GRID_KMAX) centres; votes in quarters: exact ties, votes outside the map, beyond 1e5, NaN, +-inf.
    Bit for bit, with the grid (default) and with EMP_VOTE_GRID=0"""
    for step, up in ((1, 1), (4, 2)):
        cells = _vote(counts, h, w, step, up, grid)
        if max(counts) > PP.ARGMIN_MAX:
            assert (cells[-1] == 0).any() and cells[-1].max() > max(counts) // 2


@pytest.mark.parametrize('grid', [None, '0'], ids=['grid', 'scan'])
@pytest.mark.parametrize('step,up', PP.VOTE_STEP_UP, ids=_ids)
def test_vote_step_and_up(step, up, grid):
    """step in {1, 4} x up in {1, 2, 4, 8}, up != step included, on a batch of 21 and 192 centres (scan and grid)"""
    _vote((PP.ARGMIN_MAX + 1, PP.GRID_MIN), 17, 19, step, up, grid)


@pytest.mark.parametrize('grid', [None, '0'], ids=['grid', 'scan'])
@pytest.mark.parametrize('K,h,w,step', PP.VOTE_GENERIC, ids=_ids)
def test_vote_generic_offsets(K, h, w, step, grid):
    """gaussian votes on every path (argmin, scan, grid, two LDS tiles): equal to the reference outside the near-tie mask, which
    the host test caps at 1e-4 of the pixels"""
    _vote((K,), h, w, step, step, grid, generic=True)


# ----------------------------------------------------------------------------
# emp_panoptic_merge
# ----------------------------------------------------------------------------
def _merge(sem, cells, things, stuff_area, void_label, max_ids, scalar, thr=PP.MERGE_THR, divisor=1000):
    """sem / cells are passed as views that start one image into their tensors; pan is a view as well"""
    lib = _lib()
    N, C_, H, W = sem.shape
    dsem = _cuda(np.concatenate([sem[:1], sem]))[1:]
    dcells = _cuda(np.concatenate([cells[:1], cells]))[1:]
    assert dsem.is_contiguous() and dcells.is_contiguous()
    pan = Buf(N * H * W, torch.int64, PP.I64_SENTINEL, front=PP.GUARD)
    nbytes = int(lib.emp_panoptic_merge_work_bytes(N, C_, max_ids))
    work = Buf(nbytes, torch.uint8, PP.WORK_FILL)
    tl = (C.c_int32 * max(1, len(things)))(*things)
    with _env('EMP_MERGE_SCALAR', '1' if scalar else None):
        _abi().check(lib.emp_panoptic_merge(_abi().ptr(dsem), _abi().ptr(dcells), N, C_, H, W, float(thr), tl, len(things),
                                            int(divisor), int(stuff_area), int(void_label), int(max_ids), pan.ptr(), work.ptr(),
                                            _stream()), 'emp_panoptic_merge')
    work.result('merge workspace')
    return pan.result('pan').reshape(N, H, W)


@pytest.mark.parametrize('case', PP.MERGE_CASES, ids=lambda c: f'C{c[0]}-t{len(c[1])}-v{c[2]}-m{c[3]}-{c[4]}x{c[5]}')
def test_merge_against_the_reference(case):
    """scalar and vector form (planes of 33 x 31 and 5 x 7 are no multiple of 4 and take the scalar kernels either way) against
    oracle.merge_semantic_and_instance: C in {1, 2, 3, 5, 32}; thing lists [], [1], [2], [1, 2], [0, 1] and 16 classes;
    void_label 0, 255, -1; stuff_area 0, at a class count, one above, above all; max_ids 0, 1, 255, 256, 257, 600 with ids on two
    thing classes across the 256-id chunks; missing, negative and too large ids; an instance wholly on stuff pixels; an exact
    class tie; probabilities equal to confidence_thr; N = 3 with different populations"""
    C_, things, void_label, max_ids, H, W = case
    sem, cells = PP.merge_input(3, C_, H, W, things, max_ids)
    seen = set()
    for stuff_area in PP.stuff_areas(sem, things):
        ref = PP.merge_ref(sem, cells, PP.MERGE_THR, things, 1000, stuff_area, void_label, max_ids)
        for scalar in (False, True):
            got = _merge(sem, cells, things, stuff_area, void_label, max_ids, scalar)
            np.testing.assert_array_equal(got, ref, err_msg=f'stuff_area {stuff_area} EMP_MERGE_SCALAR {int(scalar)}')
        seen |= set(np.unique(ref).tolist())
    assert void_label in seen
    if things and max_ids > 1 and max(things) < max(C_, 2):
        assert any(v > 1000 for v in seen if v != void_label), 'no instance label was written'


@pytest.mark.parametrize('scalar', [False, True], ids=['vector', 'scalar'])
def test_merge_more_keys_than_the_hash_table(scalar):
    """every pixel of a 64 x 64 plane its own id (max_ids = 4096): a workgroup meets 2048 / 4096 distinct keys, the 256-entry
    table fills up and the rest take the fallback straight to the global counts"""
    sem, cells = PP.distinct_ids_input()
    for things, void_label in (([1, 2], 255), ([1], 0)):
        ref = PP.merge_ref(sem, cells, PP.MERGE_THR, things, 10000, 64, void_label, 4096)
        got = _merge(sem, cells, things, 64, void_label, 4096, scalar, divisor=10000)
        np.testing.assert_array_equal(got, ref)
        assert len(np.unique(ref)) > 1000


@pytest.mark.parametrize('shape', PP.MERGE_TRIP_SHAPES, ids=_ids)
def test_merge_write_second_trip(shape):
    """planes beyond 2048 workgroups of the write kernels: the scalar kernel's second trip (725 x 725, odd) and the vector
    kernel's (1449 x 1448); the last pixels carry an instance"""
    H, W = shape
    sem, cells = PP.merge_input(1, 2, H, W, [1], 300)
    cells[0, H - 1, W - 8:] = 299
    sem[0, :, H - 1, W - 8:] = [[0.25], [0.75]]
    ref = PP.merge_ref(sem, cells, PP.MERGE_THR, [1], 1000, 64, 255, 300)
    assert ref[0, H - 1, W - 1] > 1000
    for scalar in (False, True):
        np.testing.assert_array_equal(_merge(sem, cells, [1], 64, 255, 300, scalar), ref)


def test_merge_refuses_bad_arguments():
    sem, cells = PP.merge_input(1, 3, 8, 8, [1], 5)
    dsem, dcells = _cuda(sem), _cuda(cells)
    pan = Buf(64, torch.int64, PP.I64_SENTINEL)
    work = Buf(int(_lib().emp_panoptic_merge_work_bytes(1, 3, 5)), torch.uint8, PP.WORK_FILL)
    tl = (C.c_int32 * 17)(*range(17))

    def call(N=1, C_=3, H=8, W=8, n_things=1, max_ids=5):
        return _lib().emp_panoptic_merge(_abi().ptr(dsem), _abi().ptr(dcells), N, C_, H, W, 0.5, tl, n_things, 1000, 64, 0, max_ids,
                                         pan.ptr(), work.ptr(), _stream())
    assert call(N=0) != 0 and call(C_=0) != 0 and call(C_=33) != 0 and call(H=0) != 0 and call(max_ids=-1) != 0
    assert call(n_things=17) != 0 and call(n_things=-1) != 0
    assert pan.untouched()


# ----------------------------------------------------------------------------
# engine level
# ----------------------------------------------------------------------------
class _Fake:
    """model stand-in: the engine only asks it for its device"""

    def __init__(self):
        self._p = torch.zeros(1, device='cuda')

    def eval(self):
        return self

    def parameters(self):
        yield self._p


def _engine(coarse, k=1, thr=0.1, **kw):
    from empanada_napari_amd.engines import PanopticDeepLabRenderEngine
    return PanopticDeepLabRenderEngine(_Fake(), [1], nms_threshold=thr, nms_kernel=k, coarse_boundaries=coarse, **kw)


def test_engine_regrows_the_centre_buffer():
    """instance_cells_int with MAX_CENTERS = 8 and 30 / 5 centres: the regrow loop runs once and gives the result of the default
    bound, which is the oracle's"""
    counts, h, w = (30, 5), 17, 19
    ctr, off, ref, centres, _ = PP.vote_case(counts, h, w, 1)
    small, default = _engine(False), _engine(False)
    small.MAX_CENTERS = 8
    a, ca, na, ka = small.instance_cells_int(_cuda(ctr), _cuda(off), 1)
    b, cb, nb, kb = default.instance_cells_int(_cuda(ctr), _cuda(off), 1)
    assert ka == kb == 30 and na.cpu().tolist() == nb.cpu().tolist() == list(counts)
    assert ca.shape[1] == 32 and cb.shape[1] == default.MAX_CENTERS      # regrown to the next power of two
    np.testing.assert_array_equal(a.cpu().numpy(), ref)
    np.testing.assert_array_equal(b.cpu().numpy(), ref)
    for n, K in enumerate(counts):
        np.testing.assert_array_equal(ca[n, :K].cpu().numpy(), centres[n])
        np.testing.assert_array_equal(cb[n, :K].cpu().numpy(), centres[n])


@pytest.mark.parametrize('coarse', [True, False], ids=['coarse', 'fine'])
def test_engine_upsampling_2(coarse):
    """upsampling = 2 on either boundary mode (up = 8 at step 4, up = 2 at step 1) against oracle.get_instance_cells"""
    step = 4 if coarse else 1
    counts, h, w = (PP.ARGMIN_MAX + 1,), 17, 19
    ctr, off, _, _, _ = PP.vote_case(counts, h, w, step)
    eng = _engine(coarse)
    cells = eng.instance_cells_int(_cuda(ctr), _cuda(off), 2)[0]
    want = opp.get_instance_cells(ctr, off, 0.1, 1, coarse, 2)
    assert tuple(cells.shape) == (1, h * 2 * step, w * 2 * step) == want.shape[1:]
    np.testing.assert_array_equal(cells.cpu().numpy(), want[0].astype(np.int32))
    f = eng.get_instance_cells(_cuda(ctr), _cuda(off), 2)
    assert f.dtype == torch.float32 and np.array_equal(f.cpu().numpy(), want)


# ----------------------------------------------------------------------------
# the reference project's own outputs on the edge cases (tests/golden/postprocess_edges.npz)
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(PP.EDGE_CASES))
def test_edge_fixture_through_the_kernels(golden_dir, name):
    g = np.load(os.path.join(golden_dir, 'postprocess_edges.npz'))
    e = PP.edge_inputs(name)
    want = g[f'{name}_centers']
    K = want.shape[0]
    up = e['upsampling'] * e['step']
    cells, centres, num = _instance_cells(e['ctr'], e['off'], PP.EDGE_THR, e['k'], e['step'], up, max(K, 1))
    assert int(num[0]) == K
    np.testing.assert_array_equal(centres[0, :K], want)
    if up > 1:
        np.testing.assert_array_equal(cells[:, None], g[f'{name}_cells'])
    assert K > 0
    np.testing.assert_array_equal(cells[:, ::up, ::up], g[f'{name}_groups'])
    if name.startswith('stuff_'):
        assert int(g[f'{name}_stuff_area']) == e['stuff_area']
    if e['upsampling'] == 1:
        prob = opp.logits_to_prob(e['sem_logits'])      # logits 6 apart: no probability near a decision
        for scalar in (False, True):
            pan = _merge(prob, cells, e['things'], e['stuff_area'], e['void_label'], K, scalar, divisor=PP.EDGE_DIVISOR)
            np.testing.assert_array_equal(pan, g[f'{name}_pan'])
