"""The network's glue kernels -- csrc/layers.hip, csrc/stem.hip, their fp32 twins in csrc/ref32.hip, avgpool_hl32 of
csrc/conv16x3p.hip -- each through its own emp_op_* entry against the plain float64 references of tests/layers_case.py, at the
smallest shapes at which each kernel can still go wrong: partial tiles, one pixel into the next tile, every remainder loop, the
valid-region masking of all six stems, both resize kernels of each precision bit for bit against each other.  Every tolerance
is a bound derived in tests/layers_case.py (module docstring), none is measured; tests/test_layers_case_host.py shows on the CPU
that an emulation of each kernel keeps its bound and that one with a defect does not.  Every output buffer is wider than what is
written (row stride > C where the launcher takes one, three rows and 64 elements behind the end), pre-filled with a sentinel
that must survive outside the written slice; inputs live in a channel slice of a wider buffer where the launcher takes a stride,
followed by rows of +inf that no kernel may read."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import layers_case as LC
import pointrend_case as PC

pytestmark = pytest.mark.gpu

F16, F32, HL32 = LC.F16, LC.F32, LC.HL32
TORCH_OF = {F16: torch.float16, F32: torch.float32}
FILL_OF = {F16: LC.F16_SENTINEL, F32: LC.F32_SENTINEL}
PAD_OF = {F16: 8, F32: 4}      # channels a lane moves at once: strides are multiples of it
EXTRA_ROWS = 3
PREC_ID = {F16: 'f16', F32: 'f32', HL32: 'hl32'}.get


def _abi():
    from empanada_napari_amd import _abi
    return _abi


def _stream():
    return _abi().stream_ptr(torch.device('cuda:0'))


def _cuda(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def _ptr(t, offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + offset * t.element_size())


def _call(name, *args):
    abi = _abi()
    abi.check(getattr(abi.load(), name)(*args), name)


class Out:
    """a sentinel-filled device buffer of (rows + EXTRA_ROWS) x ld elements + LC.GUARD, of which rows x C are to be written"""

    def __init__(self, rows, C_, ld, dtype, fill):
        self.rows, self.C, self.ld, self.fill = int(rows), C_, ld, fill
        self.t = torch.full(((self.rows + EXTRA_ROWS) * ld + LC.GUARD,), fill, dtype=dtype, device='cuda:0')

    def result(self, what):
        """the written slice; asserts that everything around it still holds the sentinel"""
        torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        body = a[:(self.rows + EXTRA_ROWS) * self.ld].reshape(self.rows + EXTRA_ROWS, self.ld)
        assert (a[body.size:] == self.fill).all() and (body[self.rows:] == self.fill).all(), f'{what}: written behind the last row'
        assert (body[:self.rows, self.C:] == self.fill).all(), f'{what}: written outside the channel slice'
        return body[:self.rows, :self.C].copy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.t == self.fill).all())


def _out(rows, C_, prec, ld=None):
    return Out(rows, C_, ld or C_, TORCH_OF[prec], FILL_OF[prec])


def _report(what, got, ref, bound):
    ratio = LC.worst_ratio(got, ref, bound)
    print(f'RATIO {what}: largest err / bound {ratio:.4f}')
    bad = LC.violations(got, ref, bound)
    assert bad == 0, f'{what}: {bad} of {ref.size} values beyond the bound, worst err / bound {ratio:.3g}'


# ----------------------------------------------------------------------------
# stems
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stem_case(k, C_, shape, dtype):
    H, W, vh, vw = shape
    seed = 1000 * k + 10 * (H + W + vh + vw) + dtype
    img = LC.stem_image(dtype, LC.STEM_N, vh, vw, seed)
    w, b = LC.stem_weights(k, C_, seed)
    return img, w, b, LC.stem_ref(img, dtype, H, W, w, b, k)


def _run_stem(entry, k, C_, shape, dtype, prec, out_ld=None):
    H, W, vh, vw = shape
    img, w, b, _ = _stem_case(k, C_, shape, dtype)
    sub, mul = LC.NORMALISE[dtype]
    div = 4 if entry == 'emp_op_stem_pool' else 2
    out = _out(LC.STEM_N * (H // div) * (W // div), C_, prec, out_ld)
    dimg, dw, db = _cuda(img), _cuda(w), _cuda(b)
    args = [_ptr(dimg), dtype, float(sub), float(mul), LC.STEM_N, H, W, vh, vw, _ptr(dw), _ptr(db)]
    args += [C_, _ptr(out.t), out.ld] if entry == 'emp_op_stem3x3s2' else [_ptr(out.t)]
    _call(entry, *args, prec, _stream())
    return out.result(f'{entry} {shape}').reshape(LC.STEM_N, H // div, W // div, C_)


@pytest.mark.parametrize('prec', [F16, F32], ids=PREC_ID)
@pytest.mark.parametrize('dtype', LC.STEM_DTYPES, ids=['f32', 'u8', 'u16'].__getitem__)
@pytest.mark.parametrize('shape', LC.STEM7_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_stem7x7(shape, dtype, prec):
    ref, S, T = _stem_case(7, 64, shape, dtype)[3]
    got = _run_stem('emp_op_stem7x7', 7, 64, shape, dtype, prec)
    _report(f'stem7x7 {PREC_ID(prec)}', got, ref, LC.stem_conv_bound(ref, S, T, 7, prec, False))


@pytest.mark.parametrize('prec', [F16, F32], ids=PREC_ID)
@pytest.mark.parametrize('dtype', LC.STEM_DTYPES, ids=['f32', 'u8', 'u16'].__getitem__)
@pytest.mark.parametrize('shape', LC.STEM_POOL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_stem_pool(shape, dtype, prec):
    ref, S, T = _stem_case(7, 64, shape, dtype)[3]
    pref, pbound = LC.stem_pool_ref_bound(ref, S, T, prec)
    got = _run_stem('emp_op_stem_pool', 7, 64, shape, dtype, prec)
    _report(f'stem_pool {PREC_ID(prec)}', got, pref, pbound)
    # fused against unfused: the max-pool of what the VALU stem stores, within the two stems' bounds added
    conv = _run_stem('emp_op_stem7x7', 7, 64, shape, dtype, prec)
    both = pbound + LC.maxpool_ref(LC.stem_conv_bound(ref, S, T, 7, prec, False), pad=0.0)
    _report(f'stem_pool against max-pool(stem7x7) {PREC_ID(prec)}', got, LC.maxpool_ref(conv).astype(np.float64), both)


@pytest.mark.parametrize('prec', [F16, F32], ids=PREC_ID)
@pytest.mark.parametrize('dtype', LC.STEM_DTYPES, ids=['f32', 'u8', 'u16'].__getitem__)
@pytest.mark.parametrize('C_', LC.STEM3_C)
@pytest.mark.parametrize('shape', LC.STEM3_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_stem3x3s2(shape, C_, dtype, prec):
    ref, S, T = _stem_case(3, C_, shape, dtype)[3]
    got = _run_stem('emp_op_stem3x3s2', 3, C_, shape, dtype, prec, out_ld=C_ + 2 * PAD_OF[prec])
    _report(f'stem3x3s2 {PREC_ID(prec)}', got, ref, LC.stem_conv_bound(ref, S, T, 3, prec, False))


# ----------------------------------------------------------------------------
# max-pool: exact
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('negative', [False, True], ids=['signed', 'all_negative'])
@pytest.mark.parametrize('prec', [F16, F32], ids=PREC_ID)
@pytest.mark.parametrize('hw', LC.MAXPOOL_HW, ids=lambda s: 'x'.join(map(str, s)))
def test_maxpool_is_exact(hw, prec, negative):
    H, W = hw
    for C_ in LC.MAXPOOL_C[prec]:
        x = LC.signed_map((LC.MAXPOOL_N, H, W, C_), prec, H * W + C_, negative=negative)
        out = _out(LC.MAXPOOL_N * (H // 2) * (W // 2), C_, prec)
        dx = _cuda(x)
        _call('emp_op_maxpool3x3s2', _ptr(dx), LC.MAXPOOL_N, H, W, C_, _ptr(out.t), prec, _stream())
        got = out.result(f'maxpool {hw} C={C_}')
        np.testing.assert_array_equal(got.reshape(-1), LC.maxpool_ref(x).reshape(-1), err_msg=f'C={C_}')


# ----------------------------------------------------------------------------
# fuse_combine
# ----------------------------------------------------------------------------
def _fuse_cases():
    return [(mode, H, W) for mode in (0, 1) for H, W in LC.FUSE_OUT_HW[mode]]


@pytest.mark.parametrize('layout', ['f16', 'f16_hi_lo', 'f32'])
@pytest.mark.parametrize('case', _fuse_cases(), ids=lambda c: 'mode%d_%dx%d' % c)
def test_fuse_combine(case, layout):
    mode, H, W = case
    prec = F32 if layout == 'f32' else F16
    for C_ in LC.FUSE_C:
        for with_c in (True, False):
            for neg in ((False, True) if mode == 1 else (False,)):
                a, b, c, coef = LC.fuse_inputs(mode, H, W, C_, prec, 7 * H + W + C_ + mode, negative_a=neg)
                if not with_c:
                    c = None
                ref, A = LC.fuse_ref(a, b, c, coef, mode)
                rows = LC.FUSE_N * H * W
                ld = {'f16': C_ + 8, 'f16_hi_lo': 2 * C_, 'f32': C_}[layout]
                out = _out(rows, C_ if layout != 'f16_hi_lo' else 2 * C_, prec, ld)
                da, db, dc = _cuda(a), _cuda(b), (None if c is None else _cuda(c))
                lo_ptr = _ptr(out.t, C_) if layout == 'f16_hi_lo' else None      # the network's layout: out_lo = out + C
                _call('emp_op_fuse_combine', _ptr(da), _ptr(db), _ptr(dc), float(coef[0]), float(coef[1]), float(coef[2]), mode, LC.FUSE_N,
                      H, W, C_, _ptr(out.t), lo_ptr, 0 if layout == 'f32' else ld, prec, _stream())
                what = f'fuse_combine {layout} mode {mode}'
                got = out.result(f'{what} C={C_} c={with_c}').reshape(LC.FUSE_N, H, W, -1)
                e = LC.fuse_e32(A)
                _report(what, got[..., :C_], ref, LC.half_bound(ref, e) if prec == F16 else e)
                if layout == 'f16_hi_lo':
                    hi, lo = got[..., :C_], got[..., C_:]
                    _report(what + ' pair', hi.astype(np.float64) + lo.astype(np.float64), ref, LC.fuse_pair_bound(ref, A))
                    assert LC.pair_inconsistent(hi, lo) == 0, 'hi is not the fp16 rounding of hi + lo'


@pytest.mark.parametrize('prec', [F16, F32], ids=PREC_ID)
@pytest.mark.parametrize('case', _fuse_cases(), ids=lambda c: 'mode%d_%dx%d' % c)
def test_fuse_resize_part_is_exact(case, prec):
    """ca = 1, cb = 0 and b = 0: the output is the nearest / max resize of a itself, bit for bit"""
    mode, H, W = case
    for C_ in LC.FUSE_C:
        a, b, _, _ = LC.fuse_inputs(mode, H, W, C_, prec, H + W + C_, negative_a=(mode == 1))
        out = _out(LC.FUSE_N * H * W, C_, prec)
        da, db = _cuda(a), _cuda(np.zeros_like(b))
        _call('emp_op_fuse_combine', _ptr(da), _ptr(db), None, 1.0, 0.0, 0.0, mode, LC.FUSE_N, H, W, C_, _ptr(out.t), None, 0, prec, _stream())
        got = out.result(f'fuse resize mode {mode}')
        np.testing.assert_array_equal(got.reshape(-1), LC.fuse_resize(a, mode).reshape(-1))


# ----------------------------------------------------------------------------
# bilinear NHWC
# ----------------------------------------------------------------------------
def _bilinear(x, H, W, prec, variant=0, what='bilinear'):
    """x (N,h,w,C) in the kernel's type -> the (N,H,W,C) output, through a channel slice of a wider input and output"""
    N, h, w, C_ = x.shape
    pad = PAD_OF[prec]
    buf = LC.slice_buffer(x, C_ + pad, prec, 5, w + 2)
    out = _out(N * H * W, C_, prec, C_ + 2 * pad)
    dbuf = _cuda(buf)
    _call('emp_op_bilinear_ac_nhwc', _ptr(dbuf), N, h, w, C_, C_ + pad, _ptr(out.t), H, W, C_ + 2 * pad, prec, variant, _stream())
    return out.result(f'{what} {x.shape} -> {H}x{W}').reshape(N, H, W, C_)


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


@pytest.mark.parametrize('part', [0, 1], ids=['rows', 'columns'])
@pytest.mark.parametrize('prec', [F16, F32], ids=PREC_ID)
def test_bilinear_sweep(prec, part):
    sweep = LC.bilinear_sweep()
    half = 9 * 33
    worst, C_ = 0.0, PAD_OF[prec]
    for h, w, H, W in (sweep[:half] if part == 0 else sweep[half:]):
        x = LC.signed_map((LC.BILINEAR_N, h, w, C_), prec, h * w + H + W)
        got = _bilinear(x, H, W, prec)
        ref = LC.bilinear_ref(x, H, W)
        bound = LC.bilinear_bound(x, ref, H, W, prec)
        bad = LC.violations(got, ref, bound)
        assert bad == 0, f'{h}x{w} -> {H}x{W}: {bad} values beyond the bound, worst err / bound {LC.worst_ratio(got, ref, bound):.3g}'
        worst = max(worst, LC.worst_ratio(got, ref, bound))
        if (h, w) == (H, W):
            np.testing.assert_array_equal(_bits(got), _bits(x), err_msg=f'identity {h}x{w}')
    print(f'RATIO bilinear nhwc {PREC_ID(prec)}: largest err / bound {worst:.4f}')


@pytest.mark.parametrize('case', LC.BILINEAR_UP4_F16, ids=lambda c: 'C%d_%dx%d_%dx%d' % c)
def test_bilinear_f16_four_pixel_kernel_is_bit_identical(case):
    C_, h, w, H, W = case
    x = LC.signed_map((LC.BILINEAR_N, h, w, C_), F16, h * w + H + W)
    one = _bilinear(x, H, W, F16, variant=1)
    four = _bilinear(x, H, W, F16, variant=2)
    auto = _bilinear(x, H, W, F16, variant=0)
    ref = LC.bilinear_ref(x, H, W)
    _report('bilinear nhwc f16 (one-pixel kernel)', one, ref, LC.bilinear_bound(x, ref, H, W, F16))
    np.testing.assert_array_equal(_bits(four), _bits(one), err_msg='four-pixel kernel against one-pixel kernel')
    np.testing.assert_array_equal(_bits(auto), _bits(one), err_msg='dispatcher against one-pixel kernel')


@pytest.mark.parametrize('case', LC.BILINEAR_X4_F32, ids=lambda c: 'C%d_%dx%d_%dx%d' % c)
def test_bilinear_f32_four_column_kernel_is_bit_identical(case, monkeypatch):
    C_, h, w, H, W = case
    x = LC.signed_map((LC.BILINEAR_N, h, w, C_), F32, h * w + H + W)
    four = _bilinear(x, H, W, F32)
    monkeypatch.setenv('EMP_BILINEAR32_X4', '0')
    one = _bilinear(x, H, W, F32)
    monkeypatch.delenv('EMP_BILINEAR32_X4')
    ref = LC.bilinear_ref(x, H, W)
    _report('bilinear nhwc f32 (one-column kernel)', one, ref, LC.bilinear_bound(x, ref, H, W, F32))
    np.testing.assert_array_equal(_bits(four), _bits(one))


@pytest.mark.parametrize('case', LC.BILINEAR_UP4_REFUSED, ids=lambda c: 'C%d_%dx%d_%dx%d' % c)
def test_bilinear_f16_four_pixel_kernel_refuses_what_it_cannot_take(case):
    abi = _abi()
    C_, h, w, H, W = case
    x = LC.signed_map((1, h, w, C_), F16, 3)
    out = _out(H * W, C_, F16)
    dx = _cuda(x)
    rc = abi.load().emp_op_bilinear_ac_nhwc(_ptr(dx), 1, h, w, C_, C_, _ptr(out.t), H, W, C_, F16, 2, _stream())
    assert rc != 0
    with pytest.raises(abi.EmpError, match='four-pixel'):
        abi.check(rc, 'emp_op_bilinear_ac_nhwc')
    assert out.untouched()
    got = _bilinear(x, H, W, F16)      # the dispatcher takes the one-pixel kernel
    ref = LC.bilinear_ref(x, H, W)
    _report('bilinear nhwc f16 (dispatcher)', got, ref, LC.bilinear_bound(x, ref, H, W, F16))
    np.testing.assert_array_equal(_bits(got), _bits(_bilinear(x, H, W, F16, variant=1)))


@pytest.mark.parametrize('case', LC.BILINEAR_IDLE, ids=lambda c: 'C%d_%dx%d_%dx%d' % c)
def test_bilinear_f16_idle_threads(case):
    C_, h, w, H, W = case
    x = LC.signed_map((LC.BILINEAR_N, h, w, C_), F16, h * w + H + W)
    got = _bilinear(x, H, W, F16)
    ref = LC.bilinear_ref(x, H, W)
    _report('bilinear nhwc f16 (C = 48)', got, ref, LC.bilinear_bound(x, ref, H, W, F16))
    np.testing.assert_array_equal(_bits(got), _bits(_bilinear(x, H, W, F16, variant=1)))


@pytest.mark.parametrize('prec', [F16, F32], ids=PREC_ID)
def test_bilinear_same_size_is_a_strided_copy(prec):
    C_, h, w, H, W = LC.BILINEAR_SAME
    x = LC.signed_map((LC.BILINEAR_N, h, w, C_), prec, 11)
    x.reshape(-1)[:2] = (0.0, 6.0e-8 if prec == F16 else 1.0e-30)      # a zero and a tiny value (an fp16 subnormal)
    np.testing.assert_array_equal(_bits(_bilinear(x, H, W, prec)), _bits(x))


@pytest.mark.parametrize('case', LC.BILINEAR_NCHW, ids=lambda c: 'x%d_%dx%d_nc%d' % (c[0], c[1][0], c[1][1], c[2]))
def test_bilinear_nchw_f32(case):
    scale, (h, w), NC = case
    x = LC.signed_map((NC, h, w, 1), F32, scale + h + NC)
    H, W = h * scale, w * scale
    out = _out(NC * H, W, F32)
    dx = _cuda(x)
    _call('emp_op_bilinear_ac_nchw_f32', _ptr(dx), NC, h, w, _ptr(out.t), scale, _stream())
    got = out.result(f'bilinear nchw {case}').reshape(NC, H, W, 1)
    ref = LC.bilinear_ref(x, H, W)
    _report('bilinear nchw f32', got, ref, LC.bilinear_bound(x, ref, H, W, F32))


# ----------------------------------------------------------------------------
# global average pool
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('prec', [F16, F32, HL32], ids=PREC_ID)
def test_avgpool(prec):
    abi = _abi()
    worst = 0.0
    for HW in LC.AVG_HW[prec]:
        for C_ in LC.AVG_C[prec]:
            N, ld = LC.AVG_N, C_ + LC.AVG_PAD[prec]
            x = LC.avg_input(N, HW, C_, prec, HW + C_)
            ref, bound = LC.avgpool_ref_bound(x, prec)
            dbuf = _cuda(LC.slice_buffer(x, ld, F32 if prec == HL32 else prec, 5, 2))
            work, nbytes = None, C.c_size_t(0)
            abi.check(abi.load().emp_op_avgpool_work_bytes(N, C_, prec, C.byref(nbytes)), 'emp_op_avgpool_work_bytes')
            assert (nbytes.value > 0) == (prec == F16)
            if prec == F16:
                work = torch.full((nbytes.value + LC.GUARD,), 0xA5, dtype=torch.uint8, device='cuda:0')      # never initialised
            if prec == HL32:      # the plane region's format, made by the library itself; what it does not write stays +inf
                hl = torch.full(((N * HW + 2) * 2 * ld,), float('inf'), dtype=torch.float16, device='cuda:0')
                _call('emp_hl32_from_f32', _ptr(dbuf), _ptr(hl), N * HW, C_, ld, ld, _stream())
                src = hl
            else:
                src = dbuf
            out = _out(N, C_, F32)
            _call('emp_op_avgpool', _ptr(src), N, HW, C_, ld, _ptr(out.t), _ptr(work), nbytes.value, prec, _stream())
            got = out.result(f'avgpool {PREC_ID(prec)} HW={HW} C={C_}')
            bad = LC.violations(got, ref, bound)
            assert bad == 0, f'HW={HW} C={C_}: {bad} values beyond the bound, worst err / bound {LC.worst_ratio(got, ref, bound):.3g}'
            worst = max(worst, LC.worst_ratio(got, ref, bound))
            if work is not None:
                assert bool((work[nbytes.value:] == 0xA5).all()), 'written behind the scratch buffer'
    print(f'RATIO avgpool {PREC_ID(prec)}: largest err / bound {worst:.4f}')


# ----------------------------------------------------------------------------
# gemv
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('K', LC.GEMV_K)
def test_gemv(K):
    worst = 0.0
    for N, Cout in LC.GEMV_NC:
        x, w, b = LC.gemv_inputs(N, K, Cout, K + Cout)
        dx, dw, db = _cuda(x), _cuda(w), _cuda(b)
        for bias in (b, None):
            for relu in (1, 0):
                out = _out(N, Cout, F32)
                _call('emp_op_gemv', _ptr(dx), N, K, _ptr(dw), _ptr(db) if bias is not None else None, Cout, relu, _ptr(out.t), _stream())
                got = out.result(f'gemv K={K} N={N} Cout={Cout}')
                ref, bound = LC.gemv_ref_bound(x, w, bias, relu)
                bad = LC.violations(got, ref, bound)
                assert bad == 0, f'N={N} Cout={Cout} bias={bias is not None} relu={relu}: {bad} values beyond the bound'
                worst = max(worst, LC.worst_ratio(got, ref, bound))
    print(f'RATIO gemv f32: largest err / bound {worst:.4f}')


# ----------------------------------------------------------------------------
# gate
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('prec', [F16, F32], ids=PREC_ID)
@pytest.mark.parametrize('rows', LC.GATE_ROWS)
def test_gate_mul(rows, prec):
    pad = PAD_OF[prec]
    for C_ in LC.GATE_C[prec]:
        x, g = LC.gate_inputs(rows, C_, prec, rows + C_)
        xb = LC.slice_buffer(x, C_ + pad, prec, 1, EXTRA_ROWS, guard_fill=FILL_OF[prec])
        gb = LC.slice_buffer(g, C_ + 2 * pad, prec, 2, EXTRA_ROWS, guard_fill=FILL_OF[prec])
        dx, dg = _cuda(xb), _cuda(gb)
        _call('emp_op_gate_mul', _ptr(dx), C_ + pad, _ptr(dg), C_ + 2 * pad, rows, C_, prec, _stream())
        torch.cuda.synchronize()
        ax, ag = dx.cpu().numpy(), dg.cpu().numpy()
        owned, before, other, other_before = (ag, gb, ax, xb) if prec == F16 else (ax, xb, ag, gb)
        np.testing.assert_array_equal(_bits(other), _bits(other_before), err_msg='the operand the kernel does not own changed')
        np.testing.assert_array_equal(_bits(owned[rows:]), _bits(before[rows:]), err_msg='written behind the last row')
        np.testing.assert_array_equal(_bits(owned[:, C_:]), _bits(before[:, C_:]), err_msg='written outside the channel slice')
        got = owned[:rows, :C_]
        ref, bound = LC.gate_ref_bound(x, g, prec)
        assert np.isfinite(got).all()
        _report(f'gate_mul {PREC_ID(prec)}', got, ref, bound)
        o, xx = got.reshape(-1), x.reshape(-1)
        assert o[0] == xx[0] and o[2] == xx[2], 'a gate of +30 / +90 must pass x through exactly'
        assert o[3] == 0 and (prec == F32 or o[1] == 0), 'a gate of -90 (fp16: -30 too) must give exactly 0'


# ----------------------------------------------------------------------------
# depthwise fp32: strip against plain against float64
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('case', LC.DW32_CASES, ids=lambda c: 'k%d_%dx%d_C%d' % c)
def test_dwconv_f32_strip_against_plain(case, monkeypatch):
    K, H, W, C_ = case
    x = LC.signed_map((LC.DW32_N, H, W, C_), F32, K + W)
    w = (LC.signed_map((K * K, C_), F32, K) / K).astype(np.float32)
    dbuf, dw = _cuda(LC.slice_buffer(x, C_ + 4, F32, 5, W + 2)), _cuda(w)

    def run():
        out = _out(LC.DW32_N * H * W, C_, F32, C_ + 8)
        _call('emp_op_dwconv_nhwc_f32', _ptr(dbuf), LC.DW32_N, H, W, C_, C_ + 4, _ptr(dw), K, _ptr(out.t), C_ + 8, _stream())
        return out.result(f'dwconv32 {case}').reshape(x.shape)
    default = run()
    monkeypatch.setenv('EMP_DW32_STRIP', '0')
    plain = run()
    monkeypatch.delenv('EMP_DW32_STRIP')
    ref, bound = LC.dw_ref_bound(x, w, K)
    _report('dwconv f32 (plain kernel)', plain, ref, bound)
    np.testing.assert_array_equal(_bits(default), _bits(plain), err_msg='strip kernel against plain kernel')


# ----------------------------------------------------------------------------
# head1x1 without a scatter index
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('half', [True, False], ids=['f16', 'f32'])
def test_head1x1_without_scatter_index(half):
    N, P, K, ld, ncls, plane = 2, 37, 72, 80, 3, 41
    rng = np.random.default_rng(K)
    rows = rng.standard_normal((N * P, ld)).astype(np.float16 if half else np.float32)
    pw = (rng.standard_normal((ncls, K)) / np.sqrt(K)).astype(np.float32)
    pb = rng.standard_normal(ncls).astype(np.float32)
    target = rng.standard_normal((N, ncls, plane)).astype(np.float32)
    out = torch.full((target.size + LC.GUARD,), LC.F32_SENTINEL, dtype=torch.float32, device='cuda:0')
    out[:target.size] = _cuda(target).reshape(-1)
    drows, dpw, dpb = _cuda(rows), _cuda(pw), _cuda(pb)
    _call('emp_head1x1_scatter_f16' if half else 'emp_head1x1_scatter_f32', _ptr(drows), N, P, K, ld, _ptr(dpw), _ptr(dpb), ncls, _ptr(out),
          plane, None, _stream())
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert (a[target.size:] == LC.F32_SENTINEL).all()
    got = a[:target.size].reshape(N, ncls, plane)
    np.testing.assert_array_equal(got[:, :, P:], target[:, :, P:], err_msg='cells behind the last row changed')
    ref, bound = PC.predictor_ref(rows[:, :K], pw, pb)
    _report('head1x1 without index ' + ('f16' if half else 'f32'), got[:, :, :P].transpose(0, 2, 1).reshape(N * P, ncls), ref, bound)


# ----------------------------------------------------------------------------
# argument checks: every EMP_REQUIRE of the wrapped launchers, once through its entry
# ----------------------------------------------------------------------------
def _bad_calls(z, out):
    """(what, entry, args, message): z a zeroed scratch buffer every input pointer may point at, out the sentinel-filled output"""
    Z, O = _ptr(z), _ptr(out)

    def stem(entry, H=8, W=8, vh=8, vw=8, dtype=LC.IMG_U8, prec=F16, C_=8, ld=16, N=1):
        tail = [C_, O, ld] if entry == 'emp_op_stem3x3s2' else [O]
        return [Z, dtype, 0.5, 2.0, N, H, W, vh, vw, Z, Z] + tail + [prec]

    def fuse(mode=0, H=4, W=4, C_=8, lo=None, ld=8, prec=F16, a=Z):
        return [a, Z, None, 0.5, 0.5, 0.0, mode, 1, H, W, C_, O, lo, ld, prec]

    def bil(C_=8, in_ld=8, out_ld=8, prec=F16, variant=0, h=2, w=2, H=4, W=4, N=1):
        return [Z, N, h, w, C_, in_ld, O, H, W, out_ld, prec, variant]

    def avg(HW=4, C_=32, ld=32, prec=F16, work=Z, wb=1 << 16, N=1):
        return [Z, N, HW, C_, ld, O, work, wb, prec]

    def gate(C_=8, x_ld=8, g_ld=8, prec=F16, rows=2):
        return [O, x_ld, O, g_ld, rows, C_, prec]
    calls = []
    for entry in ('emp_op_stem7x7', 'emp_op_stem_pool', 'emp_op_stem3x3s2'):
        for prec in (F16, F32):
            calls += [(f'{entry} {PREC_ID(prec)} odd H', entry, stem(entry, H=6 if 'pool' in entry else 7, vh=6, prec=prec), 'stem'),
                      (f'{entry} {PREC_ID(prec)} odd W', entry, stem(entry, W=6 if 'pool' in entry else 7, vw=6, prec=prec), 'stem'),
                      (f'{entry} {PREC_ID(prec)} dtype', entry, stem(entry, dtype=3, prec=prec), 'dtype'),
                      (f'{entry} {PREC_ID(prec)} vh > H', entry, stem(entry, vh=9, prec=prec), 'valid size'),
                      (f'{entry} {PREC_ID(prec)} vw > W', entry, stem(entry, vw=9, prec=prec), 'valid size'),
                      (f'{entry} {PREC_ID(prec)} empty image', entry, stem(entry, vh=0, prec=prec), 'valid size'),
                      (f'{entry} {PREC_ID(prec)} N = 0', entry, stem(entry, N=0, prec=prec), 'valid size')]
        calls += [(f'{entry} prec', entry, stem(entry, prec=2), 'prec')]
    calls += [('stem3x3 f16 C % 8', 'emp_op_stem3x3s2', stem('emp_op_stem3x3s2', C_=12), 'bad shape'),
              ('stem3x3 f32 C % 4', 'emp_op_stem3x3s2', stem('emp_op_stem3x3s2', C_=6, prec=F32), 'bad shape'),
              ('stem3x3 f16 out_ld < C', 'emp_op_stem3x3s2', stem('emp_op_stem3x3s2', C_=16, ld=8), 'bad shape'),
              ('stem3x3 f16 out_ld % 8', 'emp_op_stem3x3s2', stem('emp_op_stem3x3s2', ld=12), 'bad shape'),
              ('stem3x3 f32 out_ld < C', 'emp_op_stem3x3s2', stem('emp_op_stem3x3s2', C_=16, ld=8, prec=F32), 'bad shape'),
              ('maxpool f16 C % 8', 'emp_op_maxpool3x3s2', [Z, 1, 4, 4, 12, O, F16], 'maxpool'),
              ('maxpool f32 C % 4', 'emp_op_maxpool3x3s2', [Z, 1, 4, 4, 6, O, F32], 'maxpool'),
              ('maxpool f16 odd H', 'emp_op_maxpool3x3s2', [Z, 1, 3, 4, 8, O, F16], 'maxpool'),
              ('maxpool f32 odd W', 'emp_op_maxpool3x3s2', [Z, 1, 4, 3, 8, O, F32], 'maxpool'),
              ('maxpool null', 'emp_op_maxpool3x3s2', [None, 1, 4, 4, 8, O, F16], 'null'),
              ('maxpool prec', 'emp_op_maxpool3x3s2', [Z, 1, 4, 4, 8, O, 7], 'prec'),
              ('fuse C % 8', 'emp_op_fuse_combine', fuse(C_=12, ld=16), 'fuse_combine'),
              ('fuse mode', 'emp_op_fuse_combine', fuse(mode=2), 'fuse_combine'),
              ('fuse out_ld < C', 'emp_op_fuse_combine', fuse(C_=16, ld=8), 'output stride'),
              ('fuse out_ld % 8', 'emp_op_fuse_combine', fuse(ld=12), 'output stride'),
              ('fuse mode 0 odd H', 'emp_op_fuse_combine', fuse(H=3), 'even'),
              ('fuse f32 mode', 'emp_op_fuse_combine', fuse(mode=-1, prec=F32), 'mode'),
              ('fuse f32 mode 0 odd W', 'emp_op_fuse_combine', fuse(W=5, prec=F32), 'even'),
              ('fuse f32 lo', 'emp_op_fuse_combine', fuse(lo=O, prec=F32), 'no lo part'),
              ('fuse null a', 'emp_op_fuse_combine', fuse(a=None), 'null'),
              ('bilinear f16 C % 8', 'emp_op_bilinear_ac_nhwc', bil(C_=12, in_ld=16, out_ld=16), 'multiples of 8'),
              ('bilinear f16 in_ld % 8', 'emp_op_bilinear_ac_nhwc', bil(in_ld=12), 'multiples of 8'),
              ('bilinear f16 out_ld < C', 'emp_op_bilinear_ac_nhwc', bil(C_=16, in_ld=16, out_ld=8), 'geometry'),
              ('bilinear f16 C > 2048', 'emp_op_bilinear_ac_nhwc', bil(C_=2056, in_ld=2056, out_ld=2056), '2048'),
              ('bilinear f16 variant', 'emp_op_bilinear_ac_nhwc', bil(variant=3), 'variant'),
              ('bilinear f16 h = 0', 'emp_op_bilinear_ac_nhwc', bil(h=0), 'geometry'),
              ('bilinear f32 C % 4', 'emp_op_bilinear_ac_nhwc', bil(C_=6, prec=F32), 'multiples of 4'),
              ('bilinear f32 variant', 'emp_op_bilinear_ac_nhwc', bil(prec=F32, variant=1), 'variant'),
              ('bilinear f32 W = 0', 'emp_op_bilinear_ac_nhwc', bil(prec=F32, W=0), 'geometry'),
              ('bilinear nchw NC = 0', 'emp_op_bilinear_ac_nchw_f32', [Z, 0, 2, 2, O, 2], 'bad arguments'),
              ('bilinear nchw scale 0', 'emp_op_bilinear_ac_nchw_f32', [Z, 1, 2, 2, O, 0], 'bad arguments'),
              ('bilinear nchw null', 'emp_op_bilinear_ac_nchw_f32', [None, 1, 2, 2, O, 2], 'bad arguments'),
              ('avgpool f16 C % 8', 'emp_op_avgpool', avg(C_=12), 'multiple of 8'),
              ('avgpool f16 HW = 0', 'emp_op_avgpool', avg(HW=0), 'avgpool'),
              ('avgpool f16 in_ld < C', 'emp_op_avgpool', avg(ld=16), 'avgpool'),
              ('avgpool f16 no scratch', 'emp_op_avgpool', avg(work=None), 'scratch'),
              ('avgpool f16 small scratch', 'emp_op_avgpool', avg(wb=16 * 32 * 4 - 1), 'scratch'),
              ('avgpool f32 HW = 0', 'emp_op_avgpool', avg(HW=0, prec=F32), 'avgpool32'),
              ('avgpool f32 in_ld < C', 'emp_op_avgpool', avg(ld=16, prec=F32), 'avgpool32'),
              ('avgpool hl32 C % 32', 'emp_op_avgpool', avg(C_=16, prec=HL32), 'avgpool_hl32'),
              ('avgpool N = 0', 'emp_op_avgpool', avg(N=0), 'geometry'),
              ('avgpool prec', 'emp_op_avgpool', avg(prec=3), 'prec'),
              ('gemv K = 0', 'emp_op_gemv', [Z, 1, 0, Z, Z, 1, 0, O], 'gemv'),
              ('gemv Cout = 0', 'emp_op_gemv', [Z, 1, 8, Z, Z, 0, 0, O], 'gemv'),
              ('gemv null', 'emp_op_gemv', [Z, 1, 8, None, Z, 1, 0, O], 'gemv'),
              ('gate f16 C % 8', 'emp_op_gate_mul', gate(C_=12, x_ld=16, g_ld=16), 'gate_mul'),
              ('gate f16 x_ld < C', 'emp_op_gate_mul', gate(C_=16, g_ld=16), 'gate_mul'),
              ('gate f32 C % 4', 'emp_op_gate_mul', gate(C_=6, prec=F32), 'gate_mul32'),
              ('gate f32 g_ld < C', 'emp_op_gate_mul', gate(C_=16, x_ld=16, prec=F32), 'gate_mul32'),
              ('gate rows = 0', 'emp_op_gate_mul', gate(rows=0), 'gate_mul'),
              ('dwconv32 C % 4', 'emp_op_dwconv_nhwc_f32', [Z, 1, 4, 4, 6, 8, Z, 3, O, 8], 'dwconv32'),
              ('dwconv32 K = 4', 'emp_op_dwconv_nhwc_f32', [Z, 1, 4, 4, 8, 8, Z, 4, O, 8], 'dwconv32'),
              ('dwconv32 out_ld < C', 'emp_op_dwconv_nhwc_f32', [Z, 1, 4, 4, 8, 8, Z, 3, O, 4], 'dwconv32'),
              ('head1x1 K > 512', 'emp_head1x1_scatter_f16', [Z, 1, 4, 520, 520, Z, Z, 1, O, 4, None], 'head1x1'),
              ('head1x1 K % 8', 'emp_head1x1_scatter_f16', [Z, 1, 4, 12, 16, Z, Z, 1, O, 4, None], 'head1x1')]
    return calls


def test_bad_arguments_launch_nothing():
    abi = _abi()
    lib = abi.load()
    z = torch.zeros(1 << 16, dtype=torch.float32, device='cuda:0')
    out = torch.full((1 << 16,), LC.F32_SENTINEL, dtype=torch.float32, device='cuda:0')
    calls = _bad_calls(z, out)
    assert len({c[0] for c in calls}) == len(calls)
    for what, entry, args, message in calls:
        rc = getattr(lib, entry)(*args, _stream())
        assert rc != 0, f'{what}: accepted'
        with pytest.raises(abi.EmpError, match=message):
            abi.check(rc, what)
    torch.cuda.synchronize()
    assert bool((out == LC.F32_SENTINEL).all()), 'a rejected call wrote something'
    nbytes = C.c_size_t(7)
    assert lib.emp_op_avgpool_work_bytes(0, 8, F16, C.byref(nbytes)) != 0 and lib.emp_op_avgpool_work_bytes(1, 8, 9, C.byref(nbytes)) != 0
    assert nbytes.value == 7
