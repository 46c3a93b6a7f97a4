"""csrc/pointrend.hip, its fp32 twins (csrc/ref32.hip) and the predictor (csrc/layers.hip), each through its own C-ABI entry
against the plain float64 references of tests/pointrend_case.py: up-sampling and keys, the radix select with its tie rule at its
structural edges, the zero padding of the point sampling on every border, and the fused point head against the launches it
replaces, away from the network's shape.  That each input reaches its branch is asserted on the CPU in
tests/test_pointrend_case_host.py; every tolerance is derived in tests/pointrend_case.py (module docstring), none is measured.
Every output buffer carries 64 sentinel elements behind its end, which must survive; what a kernel is meant to leave alone
inside a buffer is compared with its previous content."""
import ctypes as C

import numpy as np
import pytest
import torch

import pointrend_case as PC

pytestmark = pytest.mark.gpu

F32_SENTINEL, F16_SENTINEL, I32_SENTINEL = 12345.0, 777.0, -7777


def _abi():
    from empanada_napari_amd import _abi
    return _abi


def _stream():
    return _abi().stream_ptr(torch.device('cuda:0'))


def _cuda(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _guarded(n, dtype, fill):
    """a device buffer of n elements + PC.GUARD behind them, all set to the sentinel"""
    return torch.full((int(n) + PC.GUARD,), fill, dtype=dtype, device='cuda:0')


def _guard_intact(buf, n, fill, what):
    tail = buf[int(n):].cpu()
    assert tail.numel() == PC.GUARD and bool((tail == fill).all()), f'{what}: the guard region behind the buffer was written'


# ----------------------------------------------------------------------------
# A. upsample2x_keys
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('kind', PC.UPSAMPLE_KINDS)
@pytest.mark.parametrize('shape', PC.UPSAMPLE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_upsample2x_keys(shape, kind):
    abi = _abi()
    N, Cc, h, w = shape
    x = PC.upsample_input(kind, shape, seed=h * w + Cc)
    n_out, n_keys = N * Cc * 4 * h * w, N * 4 * h * w
    out, keys = _guarded(n_out, torch.float32, F32_SENTINEL), _guarded(n_keys, torch.int32, I32_SENTINEL)
    dx = _cuda(x)
    abi.check(abi.load().emp_pr_upsample2x_keys(abi.ptr(dx), N, Cc, h, w, abi.ptr(out), abi.ptr(keys), _stream()),
              'emp_pr_upsample2x_keys')
    torch.cuda.synchronize()
    _guard_intact(out, n_out, F32_SENTINEL, 'out')
    _guard_intact(keys, n_keys, I32_SENTINEL, 'keys')
    got = out[:n_out].cpu().numpy().reshape(N, Cc, 2 * h, 2 * w)
    err, bound = float(np.abs(got - PC.upsample_ref(x)).max()), PC.upsample_bound(x)
    print(f'upsample {shape} {kind}: max err {err:.3e}, bound {bound:.3e}')
    assert err <= bound
    k = keys[:n_keys].cpu().numpy().view(np.uint32).reshape(N, 4 * h * w)
    want = np.ascontiguousarray(PC.keys_ref(got)).view(np.uint32)        # fp32 arithmetic on the kernel's own output
    assert got.dtype == np.float32
    np.testing.assert_array_equal(k, want)
    assert not (k >> 31).any(), 'a key has its sign bit set'


# ----------------------------------------------------------------------------
# B. topk_smallest
# ----------------------------------------------------------------------------
def _work(N, plane):
    abi = _abi()
    nbytes = C.c_size_t(0)
    abi.check(abi.load().emp_pr_topk_work_bytes(N, plane, C.byref(nbytes)), 'emp_pr_topk_work_bytes')
    return _guarded(nbytes.value, torch.uint8, 0xA5), nbytes.value      # never initialised: the select must not need it


def _topk_launch(dkeys, N, plane, k, work, nbytes):
    abi = _abi()
    idx = _guarded(N * k, torch.int32, I32_SENTINEL)
    abi.check(abi.load().emp_pr_topk_smallest(abi.ptr(dkeys), N, plane, k, abi.ptr(work), nbytes, abi.ptr(idx), _stream()),
              'emp_pr_topk_smallest')
    return idx


def _check_topk(idx, keys, k, what):
    N, plane = keys.shape
    _guard_intact(idx, N * k, I32_SENTINEL, what)
    got = idx[:N * k].cpu().numpy().reshape(N, k)
    assert got.min() >= 0 and got.max() < plane, f'{what}: index out of range'
    want = PC.topk_ref(keys, k)
    for n in range(N):
        assert len(np.unique(got[n])) == k, f'{what}: image {n} lists a cell twice'
        np.testing.assert_array_equal(np.sort(got[n]), want[n], err_msg=f'{what}: image {n}')


@pytest.mark.parametrize('dist,plane', PC.topk_cases(), ids=lambda v: str(v))
def test_topk_single_image(dist, plane):
    keys = PC.topk_keys(dist, plane)[None]
    dkeys = _cuda(keys)
    work, nbytes = _work(1, plane)
    for k in PC.topk_ks(dist, keys[0]):
        idx = _topk_launch(dkeys, 1, plane, k, work, nbytes)
        torch.cuda.synchronize()
        _check_topk(idx, keys, k, f'{dist} plane {plane} k {k}')
    _guard_intact(work, nbytes, 0xA5, 'workspace')


@pytest.mark.parametrize('plane', PC.TOPK_PLANES[1:])
def test_topk_three_images_three_thresholds(plane):
    dists, keys = PC.topk_batch_keys(plane)
    dkeys = _cuda(keys)
    work, nbytes = _work(3, plane)
    ks = {1, plane - 1, plane, min(8192, plane), PC.tie_cut(dists[1], keys[1])}
    for k in sorted(k for k in ks if k is not None and 1 <= k <= plane):
        idx = _topk_launch(dkeys, 3, plane, k, work, nbytes)
        torch.cuda.synchronize()
        _check_topk(idx, keys, k, f'{dists} plane {plane} k {k}')
    _guard_intact(work, nbytes, 0xA5, 'workspace')


@pytest.mark.parametrize('plane', [4099, 530437])
def test_topk_reuses_its_workspace(plane):
    """two calls in a row on one stream and one workspace, different keys and k: the second result must be right (and the first)"""
    _, keys_a = PC.topk_batch_keys(plane)
    keys_b = np.stack([PC.topk_keys(d, plane, seed=11) for d in ('byte2', 'with_inf', 'random')])
    ka, kb = min(8192, plane - 1), PC.tie_cut('with_inf', keys_b[1])
    work, nbytes = _work(3, plane)
    da, db = _cuda(keys_a), _cuda(keys_b)
    ia = _topk_launch(da, 3, plane, ka, work, nbytes)
    ib = _topk_launch(db, 3, plane, kb, work, nbytes)
    torch.cuda.synchronize()
    _check_topk(ib, keys_b, kb, 'second call')
    _check_topk(ia, keys_a, ka, 'first call')


def test_topk_rejects_bad_arguments_without_launching():
    abi = _abi()
    lib = abi.load()
    plane = 4099
    dkeys = _cuda(PC.topk_keys('random', plane)[None])
    work, nbytes = _work(1, plane)
    idx = _guarded(plane + 1, torch.int32, I32_SENTINEL)
    for k, wb in ((plane + 1, nbytes), (100, nbytes - 1), (100, 0), (0, nbytes)):
        rc = lib.emp_pr_topk_smallest(abi.ptr(dkeys), 1, plane, k, abi.ptr(work), wb, abi.ptr(idx), _stream())
        assert rc != 0
        with pytest.raises(abi.EmpError, match='topk'):
            abi.check(rc, 'emp_pr_topk_smallest')
    torch.cuda.synchronize()
    assert bool((idx == I32_SENTINEL).all()) and bool((work == 0xA5).all()), 'a rejected call wrote something'


# ----------------------------------------------------------------------------
# C. point sampling
# ----------------------------------------------------------------------------
# (fh, fw, scale, C, feat_ld, ncls, N, index list)
SAMPLE_F16 = [
    (6, 10, 2, 8, 16, 1, 1, 'all'),
    (6, 10, 4, 128, 128, 2, 2, 'all'),
    (6, 10, 8, 256, 256, 8, 1, 'all'),
    (4, 4, 2, 264, 272, 8, 2, 'all'),          # 33 lane chunks: the lane loop runs twice
    (4, 4, 4, 256, 264, 1, 2, 'subset'),
    (4, 4, 8, 128, 128, 2, 1, 'all'),
    (6, 10, 4, 264, 264, 1, 1, 'subset'),
]
SAMPLE_F32 = [
    (6, 10, 2, 256, 256, 1, 1, 'all'),         # C % 4 == 0: the vector kernel
    (6, 10, 8, 256, 264, 8, 2, 'all'),
    (4, 4, 8, 256, 256, 2, 1, 'subset'),
    (4, 4, 4, 6, 8, 2, 2, 'all'),              # C = 6: the scalar kernel
    (4, 4, 2, 6, 6, 1, 1, 'all'),
    (6, 10, 4, 6, 8, 8, 1, 'subset'),
]


def _sample_case(case, half):
    fh, fw, scale, Cc, feat_ld, ncls, N, how = case
    H2, W2 = fh * scale, fw * scale
    feat, coarse = PC.sample_input(N, fh, fw, Cc, feat_ld, ncls, seed=Cc + scale, half=half)
    idx = PC.all_cells(N, H2, W2, seed=scale) if how == 'all' else PC.subset_cells(N, H2, W2, min(H2 * W2, 50), seed=scale)
    return feat, coarse, idx, H2, W2, PC.ld_of(Cc, ncls)


def _run_features(feat, coarse, idx, H2, W2, Cc, ld, half):
    abi = _abi()
    N, fh, fw, feat_ld = feat.shape
    ncls, P = coarse.shape[1], idx.shape[1]
    dt, fill = (torch.float16, F16_SENTINEL) if half else (torch.float32, F32_SENTINEL)
    x0, x1 = _guarded(N * P * ld, dt, fill), _guarded(N * P * ld, dt, fill)
    fn = abi.load().emp_pr_point_features_f16 if half else abi.load().emp_pr_point_features_f32
    dfeat, dcoarse, didx = _cuda(feat), _cuda(coarse), _cuda(idx)      # named: they must outlive the launch
    abi.check(fn(abi.ptr(dfeat), N, fh, fw, Cc, feat_ld, abi.ptr(dcoarse), ncls, abi.ptr(didx), P, H2, W2,
                 abi.ptr(x0), abi.ptr(x1), ld, _stream()), 'emp_pr_point_features')
    torch.cuda.synchronize()
    return x0, x1


def _check_rows(x0, x1, feat, coarse, idx, H2, W2, Cc, ld, half, what):
    R = idx.size
    fill = F16_SENTINEL if half else F32_SENTINEL
    _guard_intact(x0, R * ld, fill, what + ' x0')
    _guard_intact(x1, R * ld, fill, what + ' x1')
    r0 = x0[:R * ld].cpu().numpy().reshape(R, ld)
    r1 = x1[:R * ld].cpu().numpy().reshape(R, ld)
    ref = PC.point_rows_ref(feat, Cc, coarse, idx, H2, W2, ld)
    bound = PC.sample_bound(ref, feat, Cc, coarse, half)
    err = np.abs(r0.astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f'{what}: max err {err.max():.3e}, largest err / bound {worst:.3f}')
    assert (err <= bound).all(), f'{what}: {int((err > bound).sum())} values beyond the bound, worst err / bound {worst:.3g}'
    ncls = coarse.shape[1]
    assert (r0[:, Cc + ncls:] == 0).all(), 'pad columns must be exact zeros'
    np.testing.assert_array_equal(r1[:, Cc:].view(np.uint16 if half else np.uint32), r0[:, Cc:].view(np.uint16 if half else np.uint32),
                                  err_msg='the second buffer must carry the coarse tail and the zero pad')
    assert (r1[:, :Cc] == fill).all(), 'the feature columns of the second buffer are not the sampling kernel\'s to write'
    return r0


@pytest.mark.parametrize('case', SAMPLE_F16, ids=lambda c: '_'.join(map(str, c)))
def test_point_features_f16(case):
    feat, coarse, idx, H2, W2, ld = _sample_case(case, half=True)
    x0, x1 = _run_features(feat, coarse, idx, H2, W2, case[3], ld, half=True)
    _check_rows(x0, x1, feat, coarse, idx, H2, W2, case[3], ld, True, f'f16 {case}')


@pytest.mark.parametrize('case', SAMPLE_F32, ids=lambda c: '_'.join(map(str, c)))
def test_point_features_f32(case):
    feat, coarse, idx, H2, W2, ld = _sample_case(case, half=False)
    x0, x1 = _run_features(feat, coarse, idx, H2, W2, case[3], ld, half=False)
    _check_rows(x0, x1, feat, coarse, idx, H2, W2, case[3], ld, False, f'f32 {case}')


# ----------------------------------------------------------------------------
# D. point head
# ----------------------------------------------------------------------------
def _head_inputs(case):
    Cc, ld, num_fc, ncls, N, P, fh, fw, scale = case
    H2, W2 = fh * scale, fw * scale
    feat, coarse = PC.sample_input(N, fh, fw, Cc, Cc, ncls, seed=P + ncls, half=True)
    idx = PC.subset_cells(N, H2, W2, P, seed=num_fc)
    fc_w, fc_b, pw, pb = PC.head_weights(Cc, ld, ncls, num_fc, seed=P)
    plane = H2 * W2
    target = np.random.default_rng(P).standard_normal(N * ncls * plane).astype(np.float32)
    dev = dict(feat=_cuda(feat), coarse=_cuda(coarse), idx=_cuda(idx), fc_w=[_cuda(w) for w in fc_w], fc_b=[_cuda(b) for b in fc_b],
               pw=_cuda(pw), pb=_cuda(pb))
    return dict(feat=feat, coarse=coarse, idx=idx, fc_w=fc_w, fc_b=fc_b, pw=pw, pb=pb, H2=H2, W2=W2, plane=plane, target=target, dev=dev)


def _target(inp):
    out = _guarded(inp['target'].size, torch.float32, F32_SENTINEL)
    out[:inp['target'].size] = _cuda(inp['target'])
    return out


def _unfused(case, inp, check):
    """emp_pr_point_features_f16, emp_conv2d_nhwc_f16 per fc layer, emp_head1x1_scatter_f16 -- the launches of the network with
    EMP_FUSE_PR=0 -- checked stage by stage when ``check``"""
    from gpu_common import conv_ref
    abi = _abi()
    lib = abi.load()
    Cc, ld, num_fc, ncls, N, P, fh, fw, scale = case
    d, R = inp['dev'], N * P
    X = [_guarded(R * ld, torch.float16, F16_SENTINEL), _guarded(R * ld, torch.float16, F16_SENTINEL)]
    abi.check(lib.emp_pr_point_features_f16(abi.ptr(d['feat']), N, fh, fw, Cc, Cc, abi.ptr(d['coarse']), ncls, abi.ptr(d['idx']), P,
                                            inp['H2'], inp['W2'], abi.ptr(X[0]), abi.ptr(X[1]), ld, _stream()), 'emp_pr_point_features_f16')
    torch.cuda.synchronize()
    rows = None
    if check:
        rows = _check_rows(X[0], X[1], inp['feat'], inp['coarse'], inp['idx'], inp['H2'], inp['W2'], Cc, ld, True, f'head {case} sampling')
    cur = 0
    for f in range(num_fc):
        abi.check(lib.emp_conv2d_nhwc_f16(abi.ptr(X[cur]), 1, 1, R, ld, ld, abi.ptr(d['fc_w'][f]), abi.ptr(d['fc_b'][f]), None, None, 0,
                                          abi.ptr(X[cur ^ 1]), ld, Cc, 1, 1, 1, 0, 1, 1, 0, _stream()), 'emp_conv2d_nhwc_f16')
        torch.cuda.synchronize()
        if check:
            _guard_intact(X[cur ^ 1], R * ld, F16_SENTINEL, f'fc layer {f}')
            xin = X[cur][:R * ld].view(1, 1, R, ld)
            y = X[cur ^ 1][:R * ld].view(R, ld).float().cpu()
            ref = conv_ref(xin, torch.from_numpy(inp['fc_w'][f].astype(np.float32)).view(Cc, ld, 1, 1), torch.from_numpy(inp['fc_b'][f]),
                           relu=True).view(R, Cc)
            err = (y[:, :Cc] - ref).abs()
            assert bool((err <= 2e-3 + 2e-3 * ref.abs()).all()), f'fc layer {f}: max err {err.max():.3e}'      # the bound of test_gpu_conv.py
            assert torch.equal(y[:, Cc:], torch.from_numpy(rows[:, Cc:].astype(np.float32))), f'fc layer {f}: the coarse tail changed'
        cur ^= 1
    out = _target(inp)
    abi.check(lib.emp_head1x1_scatter_f16(abi.ptr(X[cur]), N, P, ld, ld, abi.ptr(d['pw']), abi.ptr(d['pb']), ncls, abi.ptr(out),
                                          inp['plane'], abi.ptr(d['idx']), _stream()), 'emp_head1x1_scatter_f16')
    torch.cuda.synchronize()
    if check:
        _check_scatter(out, X[cur][:R * ld].view(R, ld).cpu().numpy(), inp, N, ncls, f'head {case} predictor')
    return out


def _check_scatter(out, rows, inp, N, ncls, what):
    """the predictor on the rows the device holds, in float64, scattered into the previous content of the target"""
    n = inp['target'].size
    _guard_intact(out, n, F32_SENTINEL, what)
    got = out[:n].cpu().numpy().reshape(N, ncls, inp['plane']).astype(np.float64)
    ref, bound = PC.predictor_ref(rows, inp['pw'], inp['pb'])
    before = inp['target'].reshape(N, ncls, inp['plane'])
    want = PC.scatter_ref(before, ref, inp['idx'])
    tol = PC.scatter_ref(np.zeros_like(before), bound, inp['idx'])          # 0 wherever nothing is scattered: exact there
    err = np.abs(got - want)
    print(f'{what}: max err {err.max():.3e}, largest err / bound {float((err / np.maximum(tol, 1e-300)).max()):.3f}')
    assert (err <= tol).all(), f'{what}: {int((err > tol).sum())} cells beyond the bound or changed outside the index list'


def _fused(case, inp):
    abi = _abi()
    Cc, ld, num_fc, ncls, N, P, fh, fw, scale = case
    d = inp['dev']
    out = _target(inp)
    wp = (C.c_void_p * num_fc)(*[t.data_ptr() for t in d['fc_w']])
    bp = (C.c_void_p * num_fc)(*[t.data_ptr() for t in d['fc_b']])
    abi.check(abi.load().emp_pr_point_head(abi.ptr(d['feat']), N, fh, fw, Cc, Cc, abi.ptr(d['coarse']), ncls, abi.ptr(d['idx']), P, inp['H2'],
                                           inp['W2'], wp, bp, num_fc, ld, abi.ptr(d['pw']), abi.ptr(d['pb']), abi.ptr(out), inp['plane'],
                                           _stream()), 'emp_pr_point_head')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('case', PC.HEAD_CASES, ids=PC.head_case_id)
def test_point_head_fused_is_bit_identical_to_the_checked_chain(case):
    abi = _abi()
    assert abi.load().emp_pr_point_head_supported(case[0], case[1], case[3], case[2]) == 1
    inp = _head_inputs(case)
    chain = _unfused(case, inp, check=True)
    fused = _fused(case, inp)
    diff = int((chain.view(torch.int32) != fused.view(torch.int32)).sum())
    assert diff == 0, f'{diff} of {chain.numel()} values differ between the fused head and the launches it replaces'


@pytest.mark.parametrize('shape', PC.HEAD_UNSUPPORTED, ids=lambda s: 'C%d_ld%d_cls%d_fc%d' % s)
def test_point_head_rejects_unsupported_shapes(shape):
    abi = _abi()
    lib = abi.load()
    Cc, ld, ncls, num_fc = shape
    assert lib.emp_pr_point_head_supported(Cc, ld, ncls, num_fc) == 0
    z = torch.zeros(4096, dtype=torch.float32, device='cuda:0')
    out = _guarded(64, torch.float32, F32_SENTINEL)
    ptrs = (C.c_void_p * 8)(*[z.data_ptr()] * 8)
    zi = z.int()
    rc = lib.emp_pr_point_head(abi.ptr(z), 1, 2, 2, Cc, Cc, abi.ptr(z), ncls, abi.ptr(zi), 4, 4, 4, ptrs, ptrs, num_fc, ld, abi.ptr(z),
                               abi.ptr(z), abi.ptr(out), 16, _stream())
    assert rc != 0
    with pytest.raises(abi.EmpError, match='unsupported shape'):
        abi.check(rc, 'emp_pr_point_head')
    torch.cuda.synchronize()
    assert bool((out == F32_SENTINEL).all())


# (fh, fw, scale, C, feat_ld, ncls, N, P)
TWIN_CASES = [(6, 10, 4, 256, 256, 3, 2, 100), (4, 4, 8, 6, 8, 2, 1, 300), (6, 10, 2, 256, 264, 8, 1, 120)]


@pytest.mark.parametrize('case', TWIN_CASES, ids=lambda c: '_'.join(map(str, c)))
def test_fp32_twin_sampling_then_predictor(case):
    """emp_pr_point_features_f32 followed by emp_head1x1_scatter_f32 (the fp32 mode's launches): the rows against the float64
    sampling, the scattered logits against the float64 predictor on the rows the device holds"""
    abi = _abi()
    fh, fw, scale, Cc, feat_ld, ncls, N, P = case
    H2, W2 = fh * scale, fw * scale
    ld, plane = PC.ld_of(Cc, ncls), H2 * W2
    feat, coarse = PC.sample_input(N, fh, fw, Cc, feat_ld, ncls, seed=P, half=False)
    idx = PC.subset_cells(N, H2, W2, P, seed=Cc)
    x0, x1 = _run_features(feat, coarse, idx, H2, W2, Cc, ld, half=False)
    rows = _check_rows(x0, x1, feat, coarse, idx, H2, W2, Cc, ld, False, f'twin {case} sampling')
    rng = np.random.default_rng(P)
    pw = np.zeros((ncls, ld), np.float32)
    pw[:, :Cc + ncls] = rng.standard_normal((ncls, Cc + ncls)) / np.sqrt(Cc + ncls)
    pb = rng.standard_normal(ncls).astype(np.float32)
    inp = dict(target=rng.standard_normal(N * ncls * plane).astype(np.float32), plane=plane, idx=idx, pw=pw, pb=pb)
    out = _target(inp)
    dpw, dpb, didx = _cuda(pw), _cuda(pb), _cuda(idx)
    abi.check(abi.load().emp_head1x1_scatter_f32(abi.ptr(x0), N, P, ld, ld, abi.ptr(dpw), abi.ptr(dpb), ncls, abi.ptr(out), plane,
                                                 abi.ptr(didx), _stream()), 'emp_head1x1_scatter_f32')
    torch.cuda.synchronize()
    _check_scatter(out, rows, inp, N, ncls, f'twin {case} predictor')
