"""The references, bounds and inputs of tests/layers_case.py, checked on the CPU alone -- the proof that the GPU tests of
tests/test_gpu_layer_kernels.py can fail.  Per operator:

1. a numpy emulation of the kernel's arithmetic (fp32 in the kernel's order of operations, fp16 rounding where the kernel rounds)
   stays within the derived bound of the float64 reference on every generated case: the bound is derived correctly and the
   reference keeps it;
2. the same emulation with ONE defect exceeds the bound on at least one generated case of that operator: a kernel with that defect
   cannot pass on the GPU;
3. the float64 references agree with torch-CPU's own operators in double where torch has one.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layers_case as LC

f32, f16, f64 = np.float32, np.float16, np.float64


def fma32(a, b, c):
    """fmaf: the product of two fp32 values is exact in double, one rounding of the sum"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def unwritten(out, mutant, fill):
    """the 'last column / row left unwritten' defects on an (N,H,W,C) output"""
    if mutant == 'last_col_unwritten':
        out[:, :, -1] = fill
    if mutant == 'last_row_unwritten':
        out[:, -1] = fill
    return out


# ----------------------------------------------------------------------------
# stems
# ----------------------------------------------------------------------------
def emu_stem(img, dtype, H, W, w, b, k, prec, mfma, pool, mutant=None):
    N, vh, vw = img.shape
    sub, mul = LC.NORMALISE[dtype]
    p = k // 2

    def norm(raw):
        return raw if dtype == LC.IMG_F32 else (raw - sub) * mul      # two fp32 roundings

    raw = img.astype(f32)
    x = np.zeros((N, H, W), f32)
    ring = f32(0)
    if mutant == 'raw_zero_outside_valid':      # padded to H x W BEFORE the normalisation
        x[:, :vh, :vw] = raw
        x = norm(x)
    else:
        x[:, :vh, :vw] = norm(raw)
        if mutant == 'raw_zero_outside_image':  # the convolution's own padding normalised like a pixel
            ring = norm(f32(0))
    xp = np.pad(x, ((0, 0), (p, p), (p, p)), constant_values=ring)
    Ho, Wo = H // 2, W // 2
    acc = np.zeros((N, Ho, Wo, w.shape[1]), f32)

    def tap(src, ky, kx):
        return src[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2, None]
    if not mfma:
        for ky in range(k):
            for kx in range(k):
                acc = fma32(tap(xp, ky, kx), w[ky * k + kx], acc)
    else:
        xh = xp.astype(f16)
        xl = (xp - xh.astype(f32)).astype(f16)
        wh = w.astype(f16)
        wl = (w - wh.astype(f32)).astype(f16)
        for ks in range(2):      # one MFMA per product and tap group: exact products, the sum rounded once
            for a, bb in ((wl, xh), (wh, xl), (wh, xh)):
                s = np.zeros(acc.shape, f64)
                for ky in range(4 * ks, min(4 * ks + 4, k)):
                    for kx in range(k):
                        s += tap(bb, ky, kx).astype(f64) * a[ky * k + kx].astype(f64)
                acc = (acc.astype(f64) + s).astype(f32)
    v = acc if mutant == 'bias_skipped' else acc + b
    if mutant != 'relu_skipped':
        v = np.maximum(v, f32(0))
    if prec == LC.F16:
        v = v.astype(f16)
    if pool:
        v = LC.maxpool_ref(v)
    return unwritten(v.copy(), mutant, LC.F16_SENTINEL if prec == LC.F16 else LC.F32_SENTINEL)


# (name, k, mfma, pool, shapes, channel counts)
STEMS = [('stem7x7', 7, False, False, LC.STEM7_SHAPES, [64]), ('stem_pool', 7, True, True, LC.STEM_POOL_SHAPES, [64]),
         ('stem3x3s2', 3, False, False, LC.STEM3_SHAPES, LC.STEM3_C)]
STEM_MUTANTS = ['raw_zero_outside_valid', 'raw_zero_outside_image', 'bias_skipped', 'relu_skipped', 'last_col_unwritten',
                'last_row_unwritten']


def stem_cases(name):
    _, k, mfma, pool, shapes, Cs = next(s for s in STEMS if s[0] == name)
    for i, (H, W, vh, vw) in enumerate(shapes):
        for dtype in LC.STEM_DTYPES:
            C = Cs[i % len(Cs)]
            yield k, mfma, pool, H, W, vh, vw, dtype, C, 100 * i + dtype


def stem_check(name, prec, mutant=None):
    bad = 0
    for k, mfma, pool, H, W, vh, vw, dtype, C, seed in stem_cases(name):
        img = LC.stem_image(dtype, LC.STEM_N, vh, vw, seed)
        w, b = LC.stem_weights(k, C, seed)
        ref, S, T = LC.stem_ref(img, dtype, H, W, w, b, k)
        if pool:
            ref, bound = LC.stem_pool_ref_bound(ref, S, T, prec)
        else:
            bound = LC.stem_conv_bound(ref, S, T, k, prec, mfma)
        bad += LC.violations(emu_stem(img, dtype, H, W, w, b, k, prec, mfma, pool, mutant), ref, bound)
    return bad


@pytest.mark.parametrize('prec', [LC.F16, LC.F32])
@pytest.mark.parametrize('name', [s[0] for s in STEMS])
def test_stem_emulation_keeps_the_bound(name, prec):
    assert stem_check(name, prec) == 0


@pytest.mark.parametrize('mutant', STEM_MUTANTS)
@pytest.mark.parametrize('prec', [LC.F16, LC.F32])
@pytest.mark.parametrize('name', [s[0] for s in STEMS])
def test_stem_mutant_exceeds_the_bound(name, prec, mutant):
    assert stem_check(name, prec, mutant) > 0


def test_stem_cases_have_what_the_mutants_need():
    for name, _, _, _, shapes, _ in STEMS:
        assert any(vh == H - 1 or vw == W - 1 for H, W, vh, vw in shapes), name      # one pixel short of the padded size
    for dtype in (LC.IMG_U8, LC.IMG_U16):
        sub, mul = LC.NORMALISE[dtype]
        assert abs((0 - float(sub)) * float(mul)) > 1.0      # raw 0 is far from normalised 0
    assert (LC.stem_weights(7, 64, 0)[1] < -0.5).sum() >= 21


def test_stem_reference_is_torch_conv2d():
    for name, k, _, pool, shapes, Cs in STEMS:
        H, W, vh, vw = shapes[-2]
        img = LC.stem_image(LC.IMG_U8, 2, vh, vw, 3)
        w, b = LC.stem_weights(k, Cs[0], 3)
        ref = LC.stem_ref(img, LC.IMG_U8, H, W, w, b, k)[0]
        x = torch.zeros(2, 1, H, W, dtype=torch.float64)
        x[:, 0, :vh, :vw] = torch.from_numpy(LC.normalise(img, LC.IMG_U8))
        wt = torch.from_numpy(w.astype(f64)).t().reshape(-1, 1, k, k)
        y = F.relu(F.conv2d(x, wt, torch.from_numpy(b.astype(f64)), stride=2, padding=k // 2))
        if pool:
            ref, y = LC.maxpool_ref(ref), F.max_pool2d(y, 3, 2, 1)
        np.testing.assert_allclose(ref, y.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)


# ----------------------------------------------------------------------------
# max-pool
# ----------------------------------------------------------------------------
def emu_maxpool(x, mutant=None):
    out = LC.maxpool_ref(x, pad=0.0 if mutant == 'pad_zero' else -np.inf)
    return unwritten(out.copy(), mutant, 777.0)


def maxpool_inputs(prec):
    for H, W in LC.MAXPOOL_HW:
        for C in LC.MAXPOOL_C[prec]:
            for neg in (False, True):
                yield LC.signed_map((LC.MAXPOOL_N, H, W, C), prec, H * W + C, negative=neg)


@pytest.mark.parametrize('prec', [LC.F16, LC.F32])
@pytest.mark.parametrize('mutant', ['pad_zero', 'last_col_unwritten', 'last_row_unwritten'])
def test_maxpool_mutant_differs(prec, mutant):
    assert any((emu_maxpool(x, mutant) != LC.maxpool_ref(x)).any() for x in maxpool_inputs(prec))
    if mutant == 'pad_zero':      # every all-negative map shows it, in every border window
        for x in maxpool_inputs(prec):
            if (x < 0).all():
                diff = emu_maxpool(x, mutant) != LC.maxpool_ref(x)
                assert diff[:, 0].all() and diff[:, :, 0].all()


def test_maxpool_reference_is_torch_max_pool2d():
    for x in maxpool_inputs(LC.F32):
        y = F.max_pool2d(torch.from_numpy(x.astype(f64)).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy()
        np.testing.assert_array_equal(LC.maxpool_ref(x).astype(f64), y)


# ----------------------------------------------------------------------------
# fuse_combine
# ----------------------------------------------------------------------------
def emu_fuse(a, b, c, coef, mode, prec, mutant=None):
    """-> (out, lo): lo = fp16(v - hi) for the fp16 kernel, None for the fp32 one"""
    N, H, W, C = b.shape
    if mode == 0 and mutant == 'mode0_no_shift':      # a[y][x] of the half-size map: runs into the rows below
        n, y, x = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing='ij')
        flat = a.reshape(-1, C)
        ra = flat[((n * (H // 2) + y) * (W // 2) + x) % flat.shape[0]]
    elif mode == 1 and mutant == 'pad_zero':
        ra = LC.maxpool_ref(a, pad=0.0)
    else:
        ra = LC.fuse_resize(a, mode)
    v = coef[0] * ra.astype(f32) + coef[1] * b.astype(f32)
    if c is not None and mutant != 'cc_dropped':
        v = v + coef[2] * c.astype(f32)
    fill = LC.F16_SENTINEL if prec == LC.F16 else LC.F32_SENTINEL
    if prec == LC.F32:
        return unwritten(v.copy(), mutant, fill), None
    hi = v.astype(f16)
    lo = (v - hi.astype(f32)).astype(f16)
    return unwritten(hi.copy(), mutant, fill), lo


def fuse_cases(prec):
    for mode in (0, 1):
        for H, W in LC.FUSE_OUT_HW[mode]:
            for C in LC.FUSE_C:
                for with_c in (True, False):
                    for neg in ((False, True) if mode == 1 else (False,)):
                        a, b, c, coef = LC.fuse_inputs(mode, H, W, C, prec, 7 * H + W + C + mode, negative_a=neg)
                        yield mode, a, b, (c if with_c else None), coef


def fuse_check(prec, mutant=None):
    bad = 0
    for mode, a, b, c, coef in fuse_cases(prec):
        ref, A = LC.fuse_ref(a, b, c, coef, mode)
        out, lo = emu_fuse(a, b, c, coef, mode, prec, mutant)
        e = LC.fuse_e32(A)
        bad += LC.violations(out, ref, LC.half_bound(ref, e) if prec == LC.F16 else e)
        if lo is not None and mutant is None:
            pair = out.astype(f64) + lo.astype(f64)
            bad += LC.violations(pair, ref, LC.fuse_pair_bound(ref, A))
            bad += LC.pair_inconsistent(out, lo)
    return bad


@pytest.mark.parametrize('prec', [LC.F16, LC.F32])
def test_fuse_emulation_keeps_the_bound(prec):
    assert fuse_check(prec) == 0


@pytest.mark.parametrize('mutant', ['mode0_no_shift', 'cc_dropped', 'pad_zero', 'last_col_unwritten', 'last_row_unwritten'])
@pytest.mark.parametrize('prec', [LC.F16, LC.F32])
def test_fuse_mutant_exceeds_the_bound(prec, mutant):
    assert fuse_check(prec, mutant) > 0


def test_fuse_pair_bound_is_tighter_than_fp16():
    ref = np.array([1.0])
    assert LC.fuse_pair_bound(ref, ref)[0] < 0.01 * LC.half_bound(ref, LC.fuse_e32(ref))[0]
    for mode, a, b, c, coef in fuse_cases(LC.F16):
        assert (coef > 0).all() and 0.99 < coef.sum() < 1.0


# ----------------------------------------------------------------------------
# bilinear
# ----------------------------------------------------------------------------
def emu_bilinear(buf, N, h, w, C, H, W, mutant=None, explicit_fma=True):
    """on the flat (rows + guard, in_ld) buffer of LC.slice_buffer, fp32 coordinates and the kernels' expression; the result in
    fp32 (the fp16 kernel rounds it once more)"""
    def axis(n_in, n_out):
        o = np.arange(n_out, dtype=f32)
        if mutant == 'align_corners_false':
            f = np.maximum((o + f32(0.5)) * f32(n_in / n_out) - f32(0.5), f32(0))
        else:
            s = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
            f = s * o
        i0 = f.astype(np.int64)
        i1 = i0 + 1 if mutant == 'clamp_dropped' else i0 + (i0 < n_in - 1)
        lo = f - i0.astype(f32)
        return i0, i1, lo, f32(1) - lo
    y0, y1, ly, hy = axis(h, H)
    x0, x1, lx, hx = axis(w, W)
    n = np.arange(N)[:, None, None]

    def at(yy, xx):
        return buf[(n * h + yy[None, :, None]) * w + xx[None, None, :], :C].astype(f32)
    lx, hx = (t[None, None, :, None] for t in (lx, hx))
    ly, hy = (t[None, :, None, None] for t in (ly, hy))
    with np.errstate(invalid='ignore'):
        if explicit_fma:
            t0, t1 = fma32(lx, at(y0, x1), hx * at(y0, x0)), fma32(lx, at(y1, x1), hx * at(y1, x0))
            out = fma32(ly, t1, hy * t0)
        else:
            out = hy * (hx * at(y0, x0) + lx * at(y0, x1)) + ly * (hx * at(y1, x0) + lx * at(y1, x1))
    return unwritten(out.copy(), mutant, f32(777.0))


def bilinear_shapes():
    shapes = [(8, h, w, H, W) for h, w, H, W in LC.bilinear_sweep()]
    return shapes + LC.BILINEAR_UP4_F16 + LC.BILINEAR_UP4_REFUSED + LC.BILINEAR_IDLE + [LC.BILINEAR_SAME]


def bilinear_check(prec, mutant=None, shapes=None):
    bad = 0
    for C, h, w, H, W in (shapes or bilinear_shapes()):
        C = min(C, 16)      # the arithmetic does not depend on the channel count
        x = LC.signed_map((LC.BILINEAR_N, h, w, C), prec, h * w + H + W)
        buf = LC.slice_buffer(x, C + 8, prec, 5, w + 2)
        ref = LC.bilinear_ref(x, H, W)
        out = emu_bilinear(buf, LC.BILINEAR_N, h, w, C, H, W, mutant, explicit_fma=prec == LC.F16)
        if prec == LC.F16:
            with np.errstate(invalid='ignore', over='ignore'):
                out = out.astype(f16)
        bad += LC.violations(out, ref, LC.bilinear_bound(x, ref, H, W, prec))
    return bad


@pytest.mark.parametrize('prec', [LC.F16, LC.F32])
def test_bilinear_emulation_keeps_the_bound(prec):
    assert bilinear_check(prec) == 0


@pytest.mark.parametrize('mutant', ['align_corners_false', 'clamp_dropped', 'last_col_unwritten', 'last_row_unwritten'])
@pytest.mark.parametrize('prec', [LC.F16, LC.F32])
def test_bilinear_mutant_exceeds_the_bound(prec, mutant):
    assert bilinear_check(prec, mutant) > 0


def test_bilinear_same_size_is_a_copy_in_the_emulation():
    C, h, w, H, W = LC.BILINEAR_SAME
    x = LC.signed_map((2, h, w, C), LC.F16, 1)
    out = emu_bilinear(LC.slice_buffer(x, C + 8, LC.F16, 5, w + 2), 2, h, w, C, H, W).astype(f16)
    np.testing.assert_array_equal(out.view(np.uint16), x.view(np.uint16))


def test_bilinear_sweep_and_kernel_shapes():
    sw = LC.bilinear_sweep()
    assert len(sw) == 2 * 9 * 33 + 9
    assert any(h > H for h, w, H, W in sw) and any(H == 1 and h > 1 for h, w, H, W in sw) and any(W == 1 and w > 1 for h, w, H, W in sw)
    assert any(h == 1 and H > 1 for h, w, H, W in sw) and any((h, w) == (H, W) for h, w, H, W in sw)
    for C, h, w, H, W in LC.BILINEAR_UP4_F16:
        assert LC.up4_preconditions(C, w, W)
    assert not any(LC.up4_preconditions(C, w, W) for C, h, w, H, W in LC.BILINEAR_UP4_REFUSED)
    C, h, w, H, W = LC.BILINEAR_UP4_F16[0]
    assert 256 // (C // 8) == 1                                   # one four-pixel group per block iteration
    C, h, w, H, W = LC.BILINEAR_UP4_F16[2]
    assert (W // 4) % (256 // (C // 8)) != 0                      # a ragged last segment
    C, h, w, H, W = LC.BILINEAR_UP4_F16[3]
    assert W == 4 * (256 // (C // 8))                             # exactly at the threshold
    for C, h, w, H, W in LC.BILINEAR_X4_F32:
        assert W % 4 == 0 and W >= 4 * w
    for C, h, w, H, W in LC.BILINEAR_IDLE:
        assert 256 % (C // 8) != 0 and 256 // (C // 8) == 42 and W % 42 != 0


def test_bilinear_reference_is_torch_interpolate():
    for C, h, w, H, W in [(8, h, w, H, W) for h, w, H, W in LC.bilinear_sweep()[::7]] + LC.BILINEAR_IDLE:
        x = LC.signed_map((2, h, w, 4), LC.F32, h + w + H + W)
        y = F.interpolate(torch.from_numpy(x.astype(f64)).permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=True)
        np.testing.assert_allclose(LC.bilinear_ref(x, H, W), y.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-13)


# ----------------------------------------------------------------------------
# average pool
# ----------------------------------------------------------------------------
def dropped_from(HW, prec):
    """first pixel of what the 'last pixel segment dropped' defect loses: the last non-empty segment of the fp16 kernel, the
    remainder loop (or the last round of the waves) of the others"""
    if prec == LC.F16:
        per = -(-HW // 16)
        return ((HW - 1) // per) * per
    return (HW // 64) * 64 if HW % 64 else HW - 16


def emu_avgpool(x, prec, mutant=None):
    """x (N,HW,C) in the kernel's input type -> (N,C) fp32, in the kernel's order of additions"""
    N, HW, C = x.shape
    if prec == LC.HL32:
        hi = x.astype(f16)
        x = hi.astype(f32) + (x - hi.astype(f32)).astype(f16).astype(f32)
    x = x.astype(f32)
    end = max(dropped_from(HW, prec), 0) if mutant == 'last_segment_dropped' else HW
    z = np.zeros((N, C), f32)
    if prec == LC.F16:
        per = -(-HW // 16)
        t = z
        for seg in range(16):
            p0, p1 = seg * per, min(HW, seg * per + per)
            r = z
            for lane in range(8):
                s = z
                for p in range(p0 + lane, min(p1, end), 8):
                    s = s + x[:, p]
                r = r + s
            t = t + r
        total = t
    else:
        parts = []
        for q in range(16):
            s = [z, z, z, z]
            if prec == LC.F32:
                p = q
                while p + 48 < HW:
                    for j in range(4):
                        if p + 16 * j < end:
                            s[j] = s[j] + x[:, p + 16 * j]
                    p += 64
                while p < HW:
                    if p < end:
                        s[0] = s[0] + x[:, p]
                    p += 16
            else:
                for k, p in enumerate(range(q, HW, 16)):
                    if p < end:
                        s[k & 3] = s[k & 3] + x[:, p]
            parts.append((s[0] + s[1]) + (s[2] + s[3]))
        if prec == LC.F32:
            total = z
            for q in range(16):
                total = total + parts[q]
        else:
            st = 8
            while st >= 1:
                for q in range(st):
                    parts[q] = parts[q] + parts[q + st]
                st //= 2
            total = parts[0]
    count = -(-HW // 16) * 16 if mutant == 'padded_count' else HW
    return total * (f32(1) / f32(count)) if prec == LC.F16 else total / f32(count)


def avg_check(prec, mutant=None):
    bad = 0
    for HW in LC.AVG_HW[prec]:
        for C in LC.AVG_C[prec][:2]:
            x = LC.avg_input(LC.AVG_N, HW, min(C, 40), prec, HW + C)
            ref, bound = LC.avgpool_ref_bound(x, prec)
            bad += LC.violations(emu_avgpool(x, prec, mutant), ref, bound)
    return bad


@pytest.mark.parametrize('prec', [LC.F16, LC.F32, LC.HL32])
def test_avgpool_emulation_keeps_the_bound(prec):
    assert avg_check(prec) == 0


@pytest.mark.parametrize('mutant', ['padded_count', 'last_segment_dropped'])
@pytest.mark.parametrize('prec', [LC.F16, LC.F32, LC.HL32])
def test_avgpool_mutant_exceeds_the_bound(prec, mutant):
    assert avg_check(prec, mutant) > 0


def test_avgpool_reference_is_torch_adaptive_avg_pool2d():
    x = LC.avg_input(2, 15, 8, LC.F32, 0)
    y = F.adaptive_avg_pool2d(torch.from_numpy(x.astype(f64)).reshape(2, 3, 5, 8).permute(0, 3, 1, 2), 1).reshape(2, 8).numpy()
    np.testing.assert_allclose(LC.avgpool_ref_bound(x, LC.F32)[0], y, rtol=0, atol=1e-14)


# ----------------------------------------------------------------------------
# gemv
# ----------------------------------------------------------------------------
def emu_gemv(x, w, b, relu, mutant=None):
    N, K = x.shape
    Kend = (K // 64) * 64 if mutant == 'tail_dropped' else K
    s = np.zeros((N, w.shape[0], 64), f32)
    for k in range(Kend):
        s[:, :, k % 64] = fma32(x[:, None, k], w[None, :, k], s[:, :, k % 64])
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, np.arange(64) ^ o]
    out = s[:, :, 0]
    if b is not None and mutant != 'bias_skipped':
        out = out + b
    if relu and mutant != 'relu_skipped':
        out = np.maximum(out, f32(0))
    return out


def gemv_check(mutant=None):
    bad = 0
    for K in LC.GEMV_K:
        for N, Cout in LC.GEMV_NC:
            x, w, b = LC.gemv_inputs(N, K, Cout, K + Cout)
            for bias in (b, None):
                for relu in (1, 0):
                    ref, bound = LC.gemv_ref_bound(x, w, bias, relu)
                    bad += LC.violations(emu_gemv(x, w, bias, relu, mutant), ref, bound)
    return bad


def test_gemv_emulation_keeps_the_bound():
    assert gemv_check() == 0


@pytest.mark.parametrize('mutant', ['tail_dropped', 'bias_skipped', 'relu_skipped'])
def test_gemv_mutant_exceeds_the_bound(mutant):
    assert gemv_check(mutant) > 0


# ----------------------------------------------------------------------------
# gate
# ----------------------------------------------------------------------------
def emu_gate(x, g, prec, mutant=None):
    a, b = (g, x) if mutant == 'sigmoid_of_x_times_g' else (x, g)
    with np.errstate(over='ignore'):
        out = a.astype(f32) * (f32(1) / (f32(1) + np.exp(-b.astype(f32))))
    return out.astype(f16) if prec == LC.F16 else out


def gate_check(prec, mutant=None):
    bad = 0
    for rows in LC.GATE_ROWS:
        for C in LC.GATE_C[prec]:
            x, g = LC.gate_inputs(rows, C, prec, rows + C)
            ref, bound = LC.gate_ref_bound(x, g, prec)
            out = emu_gate(x, g, prec, mutant)
            bad += LC.violations(out, ref, bound)
            if mutant is None:      # the extremes: +30 and +90 give x itself, -90 gives 0 (and -30 in fp16)
                o, xx = out.reshape(-1), x.reshape(-1)
                bad += int(o[0] != xx[0]) + int(o[2] != xx[2]) + int(o[3] != 0) + int(prec == LC.F16 and o[1] != 0)
                bad += int(not np.isfinite(out).all())
    return bad


@pytest.mark.parametrize('prec', [LC.F16, LC.F32])
def test_gate_emulation_keeps_the_bound(prec):
    assert gate_check(prec) == 0


@pytest.mark.parametrize('prec', [LC.F16, LC.F32])
def test_gate_mutant_exceeds_the_bound(prec):
    assert gate_check(prec, 'sigmoid_of_x_times_g') > 0


# ----------------------------------------------------------------------------
# depthwise fp32
# ----------------------------------------------------------------------------
def test_depthwise_emulation_keeps_the_bound_and_matches_torch():
    assert any(W % 8 == 0 for _, _, W, _ in LC.DW32_CASES) and any(W % 8 for _, _, W, _ in LC.DW32_CASES)
    for K, H, W, C in LC.DW32_CASES:
        x = LC.signed_map((LC.DW32_N, H, W, C), LC.F32, K + W)
        w = (LC.signed_map((K * K, C), LC.F32, K) / K).astype(f32)
        ref, bound = LC.dw_ref_bound(x, w, K)
        xp = np.pad(x, ((0, 0), (K // 2, K // 2), (K // 2, K // 2), (0, 0)))
        acc = np.zeros_like(x)
        for ky in range(K):
            for kx in range(K):
                acc = fma32(xp[:, ky:ky + H, kx:kx + W], w[ky * K + kx], acc)
        assert LC.violations(acc, ref, bound) == 0
        assert LC.violations(np.zeros_like(x), ref, bound) > 0
        wt = torch.from_numpy(w.astype(f64)).t().reshape(C, 1, K, K)
        y = F.conv2d(torch.from_numpy(x.astype(f64)).permute(0, 3, 1, 2), wt, padding=K // 2, groups=C).permute(0, 2, 3, 1).numpy()
        np.testing.assert_allclose(ref, y, rtol=0, atol=1e-12)
