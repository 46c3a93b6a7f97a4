"""Inputs, the kernel's arithmetic emulated on the CPU, plain float64 references and derived per-element error bounds of the
operand-range tests of the `fp16x3` family (tests/test_x3_range_case_host.py, tests/test_gpu_x3_range.py): csrc/conv16x3.hip,
csrc/conv16x3p.hip and csrc/sepconv_x3.hip through their C ABI entries.  numpy in float64 / float32 / float16; no GPU.

Every convolution is brought to its GEMM view (M pixels x K) . (Cout x K), K walked tap-major as the kernels walk it, and every
bound is PER OUTPUT ELEMENT.  U = 2^-24 is the unit round-off of fp32.

* the split (split, u).  hi = fp16(x), lo = fp16(x - hi).  |x - hi| <= 2^-11 |x| and x - hi is exact in fp32; lo rounds it to
  within 2^-11 |x - hi| <= 2^-22 |x| where lo is a normal fp16, and to within 2^-25 (half the subnormal step) where it is not:
  u(x) = max(2^-22 |x|, 2^-25).  Nothing is ever off by more than |x| itself (below 2^-25 the pair is zero and the error IS |x|;
  an exact zero -- the padding of a convolution -- has no error), so u is capped at |x|.  The relative 2^-22 holds for
  2^-3 <= |x| < 65520 (lo normal, hi finite); below 2^-3 the bound is the absolute 2^-25; at and above 65520 hi is infinite.
* the product.  w x is replaced by w_lo x_hi + w_hi x_lo + w_hi x_hi.  With x = hi + lo + dx, |dx| <= u(x), the difference is
  dx w + x dw - dx dw + x_lo w_lo:  u(x)|w| + |x|u(w) + u(x)u(w)  and the dropped term |x_lo||w_lo| <= 2^-11|x| 2^-11|w|.
* the accumulation.  The fp16 x fp16 products are exact in fp32.  Per 32-channel step three MFMA results enter the fp32
  accumulator; inside an MFMA the order is not documented.  On any path a term passes at most K additions inside the MFMAs and
  3 ceil(K / 32) between them, each rounding a partial sum bounded by S = |x| . |w|:  (K + 3 ceil(K / 32)) U S.
* the epilogue.  Bias, per-image bias and residual are one fp32 addition each: one U of A = S + |b| + |b_n| + |r| (plus the
  error so far) each.  ReLU is 1-Lipschitz and exact.  SiLU is t / (1 + __expf(-t)): __expf is exp2 of the rounded product
  t log2(e) (the argument off by U |t| log2(e), i.e. a relative U |t| ln 2 log2 e = U |t| of the result, plus the 1 ulp of
  v_exp_f32), the sum 1 + e (U), the division (within 2.5 ulp: 5 U), together below (9 + |t|) U |silu(t)|, asserted as
  (13 + |t|) U |silu(t)| for the second-order terms (+ 2^-126 for a flushed subnormal result; below t = -87 the fp32 e^-t
  overflows and the quotient is -0 instead of a value below 1e-35: the whole value is allowed); SiLU's slope is at most 1.0999, so an error e before it is 1.1 e after.
  An hl32 output adds u(result).  The fused head is an fp32 dot product over the Cout activations: the activations' bound
  through |head_w|, the products (U each) and at most Cout additions of partial sums bounded by |head_w| . |act| + |head_b|.
* the depthwise half of the separable block is an fp32 fmaf chain from 0 over the k*k taps: the pointwise operand d is off by
  at most k*k U sum |tap x| (25 U for every case: k <= 5) before it is split; the split term is u() of the float64 value.

worst_bound adds all of this up and can never be exceeded by a correct kernel.  rss_bound is the root of the sum of squares of the
same maximum roundings (every rounding taken at its maximum, but independent in sign):
    u(x)^2 . w^2 + x^2 . u(w)^2 + (2^-22 x)^2 . w^2 + 2^-48 (x^2 . w^2)(3 ceil(K / 32) + 32)
(3 ceil(K/32) roundings between the MFMAs and 32 inside one, each of a partial sum whose size is the root sum square of the
terms), plus the epilogue terms as above, linearly.  A uniform rounding has a standard deviation of max / sqrt(3): a correct
kernel stays within 3 of this bound on every draw used here (test_x3_range_case_host.py asserts it of the emulation; the largest
ratio measured is 2.7), and the GPU tests accept 6 -- twice that, about ten standard deviations.  Neither factor is fitted to a
kernel.

Families of inputs (FAMILIES), each a function of (case, seed):
* exact_* : operands a + b 2^-12 with a in +-{1, 2} (or 0), b in {0, sign a}, so that hi = a and lo = b 2^-12 exactly; integer
  bias, residual and head.  Every term the kernel adds is a multiple of one quantum q (1 without a lo half, 2^-12 with one) and
  the sum of the terms' magnitudes stays below 2^24 q (exact_expected), so every partial sum in any order is exact in fp32: the
  result is the float64 result BIT FOR BIT -- minus exactly sum w_lo x_lo where both operands carry a lo half (exact_xw), which
  pins that the kernel drops that term.  Operands are sparse enough for the magnitude condition at the case's K.
* ladder_dnE / ladder_upE : randn operands (clipped at 4 sigma) with one exponent per input channel, x[..., c] *= 2^e_c,
  w[:, c] *= 2^-e_c, e_c uniform in [-E, 0] / [0, E]: the float64 result keeps unit scale while the operands leave it.  Where
  2^E times four sigma would leave fp16's range -- where the contract ends -- the exponent is capped: activations at 2^13 (up),
  weights at floor(log2(65000 sqrt(K) / 4)) (down).
* top : ladder(0) with 1 % of the activations at +-65504 and +-65519 (the largest fp32 values whose hi is finite); weights
  (depthwise taps in the separable block) x 2^-4 so that every sum and every hl32 output stays inside fp16's range.
* tiny : activations at 2^-14 randn -- the bottom of fp16's normal range, every lo half subnormal or zero -- with 1 % of the
  entries at each of +-2^-14, +-2^-24, +-2^-25, +-2^-26 and -0.0; weights x 2^12.

Planted defects of the emulation (VARIANTS): `flush` (fp16 subnormals of all four halves read as zero), `drop_wl` / `drop_xl`
(one cross product missing), `hi_twice` (the x operand's lo half zero in every second K step, the first included: one of two staging buffers
holding hi twice)."""
import functools
import math

import numpy as np

U = 2.0 ** -24
Q12 = 2.0 ** -12
SILU_LIP = 1.1
MIN16 = 2.0 ** -14           # the smallest normal fp16
VARIANTS = ('flush', 'drop_wl', 'drop_xl', 'hi_twice')
EXACT = ('exact_0', 'exact_x', 'exact_w', 'exact_xw')
LADDER_E = (0, 4, 8, 12, 16)
LADDERS = tuple(f'ladder_{d}{E}' for E in LADDER_E for d in ('dn', 'up'))
FAMILIES = EXACT + LADDERS + ('top', 'tiny')
CVT_FAMILIES = LADDERS + ('top', 'tiny')
RSS_HOST, RSS_GPU = 3.0, 6.0


# ----------------------------------------------------------------------------
# the split
# ----------------------------------------------------------------------------
def split(t):
    """fp32 -> (hi, lo) fp16, bit for bit what split_store / store4 / emp_hl32_from_f32 compute"""
    t = np.asarray(t, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        hi = t.astype(np.float16)
        lo = (t - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def pair_value(t):
    """hi + lo in fp32 (exact: both halves lie inside t's own 24-bit window)"""
    hi, lo = split(t)
    return hi.astype(np.float32) + lo.astype(np.float32)


def u(t):
    a = np.abs(np.asarray(t, np.float64))
    return np.minimum(np.maximum(2.0 ** -22 * a, 2.0 ** -25), a)


# ----------------------------------------------------------------------------
# cases: the smallest shapes that reach each kernel's code paths (N = 1)
# ----------------------------------------------------------------------------
def _c(id, kernel, H, W, Cin, Cout, k=1, stride=1, pad=0, dil=1, act=1, res='', bias_n=False, out_fmt=0, **kw):
    d = dict(id=id, kernel=kernel, N=1, H=H, W=W, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=pad, dil=dil, act=act, res=res,
             bias_n=bias_n, out_fmt=out_fmt, wmode=0, Cin2=0, head_c=0, groups=1, cin_g=0, ksplit=False)
    d.update(kw)
    return d


CASES = [
    # emp_conv2d_nhwc_f16x3
    _c('nhwc_1x1_k16', 'nhwc', 9, 11, 16, 40),                                          # K = 16: one half-filled step
    _c('nhwc_3x3_k144', 'nhwc', 9, 11, 16, 40, 3, 1, 1),                                # a 32-step straddles two taps
    _c('nhwc_s2_res', 'nhwc', 10, 12, 48, 96, 3, 2, 1, res='f32'),
    _c('nhwc_dil4_silu', 'nhwc', 12, 12, 64, 128, 3, 1, 4, 4, act=2),
    _c('nhwc_grouped', 'nhwc', 9, 11, 32, 24, 3, 1, 1, groups=3, cin_g=24),             # Cin = Cin16 of a group, Cout per group
    # emp_conv2d_nhwc_f16x3_ex
    *[_c(f'ex_k1152_w{m}', 'ex', 12, 12, 128, 136, 3, 1, 1, bias_n=True, wmode=m) for m in (0, 1, 2)],      # the split-role kernel
    *[_c(f'ex_k1040_w{m}', 'ex', 12, 12, 1040, 128, wmode=m) for m in (0, 1, 2)],       # two-buffer kernel, K tail of 16
    _c('ex_splitk', 'ex', 16, 16, 256, 256, 3, 1, 1, wmode=5),
    _c('ex_in2', 'ex', 10, 14, 64, 256, wmode=1, Cin2=64),
    _c('ex_head1', 'ex', 9, 11, 128, 256, wmode=1, head_c=1),
    _c('ex_head2', 'ex', 9, 11, 128, 256, wmode=1, head_c=2),
    _c('ex_hl32out', 'ex', 10, 12, 64, 256, wmode=1, out_fmt=1),
    # emp_conv2d_hl32_f16x3 (+ _ksplit)
    _c('hl32_k288', 'hl32', 12, 12, 32, 256, 3, 1, 1),
    _c('hl32_k128', 'hl32', 10, 10, 128, 256, res='hl32', bias_n=True, act=2),          # K = 128: the minimum
    _c('hl32_ksplit', 'hl32', 16, 16, 512, 256, 3, 1, 2, 2, res='f32', out_fmt=1, ksplit=True),
    # emp_sepconv_x3_nhwc_f32
    _c('sep_k5_64', 'sep', 8, 16, 64, 128, 5, act=0),
    _c('sep_k3_silu', 'sep', 9, 13, 128, 128, 3, act=2),
    _c('sep_k5_head2', 'sep', 8, 16, 256, 256, 5, head_c=2),
]
CASE = {c['id']: c for c in CASES}
KERNELS = ('nhwc', 'ex', 'hl32', 'sep')
CVT_SHAPE, CVT_LD = (37, 96), 128


def out_hw(c):
    if c['kernel'] == 'sep':
        return c['H'], c['W']
    e = c['dil'] * (c['k'] - 1) + 1
    return (c['H'] + 2 * c['pad'] - e) // c['stride'] + 1, (c['W'] + 2 * c['pad'] - e) // c['stride'] + 1


def total_cout(c):
    return c['Cout'] * c['groups']


def k_of(c):
    """the K of one output's dot product"""
    if c['kernel'] == 'sep':
        return c['Cin']
    return c['k'] * c['k'] * c['Cin'] + c['Cin2']


def x_channels(c):
    return (c['groups'] - 1) * c['cin_g'] + c['Cin'] if c['groups'] > 1 else c['Cin']


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
def _randn(rng, shape):
    return np.clip(rng.standard_normal(shape), -4.0, 4.0)


def _seed(c, family):
    return 1000 * [k['id'] for k in CASES].index(c['id']) + FAMILIES.index(family)


def ladder_exponents(family, K, n, rng):
    """one exponent per input channel; the caps keep four sigma inside fp16's range (module docstring)"""
    E = int(family[9:])
    if family[7:9] == 'dn':
        E = min(E, int(math.floor(math.log2(65000.0 * math.sqrt(K) / 4.0))))
        return rng.integers(-E, 1, n)
    return rng.integers(0, min(E, 13) + 1, n)


def _exact_operand(rng, shape, p, with_lo):
    a = rng.choice([-2.0, -1.0, 1.0, 2.0], shape) * (rng.random(shape) < p)
    b = np.sign(a) * rng.integers(0, 2, shape) if with_lo else 0.0
    return a + b * Q12


def _ints(rng, shape, m=3):
    return rng.integers(-m, m + 1, shape).astype(np.float64)


def build(c, family):
    """-> dict of fp32 arrays in the layouts the C ABI takes: x (N,H,W,C); w (Cout_total, k*k, Cin) tap-major (sep: dw (k*k, C),
    pw (Cout, C)); w2 (Cout, Cin2), x2; b; bn (N, Cout); r (N,Ho,Wo,Cout) -- for res 'hl32' the fp32 map the hl32 map is made
    from; hw (head_c, Cout), hb"""
    rng = np.random.default_rng(_seed(c, family))
    N, H, W, Cin, k = c['N'], c['H'], c['W'], c['Cin'], c['k']
    Ho, Wo = out_hw(c)
    Co, K, Cx = total_cout(c), k_of(c), x_channels(c)
    sep = c['kernel'] == 'sep'
    p = {}
    if family in EXACT:
        xl, wl = family in ('exact_x', 'exact_xw'), family in ('exact_w', 'exact_xw')
        dens = min(1.0, math.sqrt(700.0 / (2.25 * K)))
        p['x'] = _exact_operand(rng, (N, H, W, Cx), dens, xl)
        if sep:      # one tap of +-1 per channel: the depthwise value is a shifted +-x, exactly
            dw = np.zeros((k * k, Cin))
            dw[rng.integers(0, k * k, Cin), np.arange(Cin)] = rng.choice([-1.0, 1.0], Cin)
            p['dw'] = dw
            p['pw'] = _exact_operand(rng, (Co, Cin), dens, wl)
        else:
            p['w'] = _exact_operand(rng, (Co, k * k, Cin), dens, wl)
        if c['Cin2']:
            p['x2'] = _exact_operand(rng, (N, H, W, c['Cin2']), dens, xl)
            p['w2'] = _exact_operand(rng, (Co, c['Cin2']), dens, wl)
        p['b'] = _ints(rng, (Co,))
        if c['bias_n']:
            p['bn'] = _ints(rng, (N, Co))
        if c['res']:
            p['r'] = _ints(rng, (N, Ho, Wo, Co))
        if c['head_c']:
            p['hw'] = _ints(rng, (c['head_c'], Co), 1) * (rng.random((c['head_c'], Co)) < 0.125)
            p['hb'] = _ints(rng, (c['head_c'],))
    else:
        x = _randn(rng, (N, H, W, Cx))
        ws = 1.0
        if family.startswith('ladder'):
            e = ladder_exponents(family, K, Cx, rng)
        else:
            e = np.zeros(Cx, np.int64)
        if family == 'top':
            sel = rng.random(x.shape)
            vals = np.array([65504.0, -65504.0, 65519.0, -65519.0])
            x = np.where(sel < 0.01, vals[rng.integers(0, 4, x.shape)], x)
            ws = 2.0 ** -4
        if family == 'tiny':
            x = x * MIN16
            sel, sgn = rng.random(x.shape), rng.choice([-1.0, 1.0], x.shape)
            for i, v in enumerate((2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -26)):
                x = np.where((sel >= 0.01 * i) & (sel < 0.01 * (i + 1)), sgn * v, x)
            x = np.where((sel >= 0.04) & (sel < 0.05), -0.0, x)
            ws = 2.0 ** 12
        p['x'] = x * 2.0 ** e
        if sep:
            p['dw'] = _randn(rng, (k * k, Cin)) / k * (ws if family == 'top' else 1.0)
            p['pw'] = _randn(rng, (Co, Cin)) / math.sqrt(Cin) * 2.0 ** -e * (1.0 if family == 'top' else ws)
        else:
            w = _randn(rng, (Co, k * k, Cin)) / math.sqrt(K) * ws
            for g in range(c['groups']):
                rows = slice(g * c['Cout'], (g + 1) * c['Cout'])
                w[rows] *= 2.0 ** -e[g * c['cin_g']:g * c['cin_g'] + Cin]
            if c['groups'] > 1:
                w[:, :, c['cin_g']:] = 0.0      # the padding of a group's channels to a multiple of 16
            p['w'] = w
        if c['Cin2']:
            e2 = ladder_exponents(family, K, c['Cin2'], rng) if family.startswith('ladder') else np.zeros(c['Cin2'], np.int64)
            x2 = _randn(rng, (N, H, W, c['Cin2']))
            if family == 'tiny':
                x2 = x2 * MIN16
            p['x2'] = x2 * 2.0 ** e2
            p['w2'] = _randn(rng, (Co, c['Cin2'])) / math.sqrt(K) * ws * 2.0 ** -e2
        p['b'] = _randn(rng, (Co,))
        if c['bias_n']:
            p['bn'] = _randn(rng, (N, Co))
        if c['res']:
            p['r'] = _randn(rng, (N, Ho, Wo, Co))
        if c['head_c']:
            p['hw'] = _randn(rng, (c['head_c'], Co)) / math.sqrt(Co)
            p['hb'] = _randn(rng, (c['head_c'],))
    return {n: np.ascontiguousarray(v, dtype=np.float32) for n, v in p.items()}


def build_cvt(family):
    """the (37, 96) map of the hl32 conversion tests"""
    rng = np.random.default_rng(7000 + FAMILIES.index(family))
    x = _randn(rng, CVT_SHAPE)
    if family.startswith('ladder'):
        x = x * 2.0 ** ladder_exponents(family, 1 << 20, CVT_SHAPE[1], rng)
    elif family == 'top':
        x = np.where(rng.random(x.shape) < 0.04, np.array([65504.0, -65504.0, 65519.0, -65519.0])[rng.integers(0, 4, x.shape)], x)
    else:
        x = x * MIN16
        sel, sgn = rng.random(x.shape), rng.choice([-1.0, 1.0], x.shape)
        for i, v in enumerate((2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -26, 2.0 ** -27)):
            x = np.where((sel >= 0.03 * i) & (sel < 0.03 * (i + 1)), sgn * v, x)
        x = np.where((sel >= 0.15) & (sel < 0.18), -0.0, x)
    return np.ascontiguousarray(x, dtype=np.float32)


# ----------------------------------------------------------------------------
# the GEMM view
# ----------------------------------------------------------------------------
def im2col(x, k, stride, pad, dil):
    """(N,H,W,C) -> (N*Ho*Wo, k*k*C), tap-major (ky, kx, c), zero padding"""
    N, H, W, C = x.shape
    e = dil * (k - 1) + 1
    Ho, Wo = (H + 2 * pad - e) // stride + 1, (W + 2 * pad - e) // stride + 1
    xp = np.zeros((N, H + 2 * pad, W + 2 * pad, C), x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    cols = [xp[:, ky * dil:ky * dil + stride * (Ho - 1) + 1:stride, kx * dil:kx * dil + stride * (Wo - 1) + 1:stride]
            for ky in range(k) for kx in range(k)]
    return np.concatenate(cols, axis=-1).reshape(N * Ho * Wo, k * k * C)


def depthwise(x, dw, k, dtype):
    """(N,H,W,C) x (k*k, C) taps, pad k // 2 -> value, sum |tap x|, sum (tap x)^2.  dtype float32: the kernel's fmaf chain from 0
    (ky-major, kx-minor); float64: the reference"""
    N, H, W, C = x.shape
    cols = im2col(np.asarray(x, np.float64), k, 1, k // 2, 1).reshape(N * H * W, k * k, C)
    terms = cols * np.asarray(dw, np.float64)[None]
    if dtype == np.float64:
        return terms.sum(1), np.abs(terms).sum(1), (terms ** 2).sum(1)
    acc = np.zeros((N * H * W, C), np.float32)
    for t in range(k * k):      # fp32 x fp32 is exact in float64; one rounding per tap
        acc = (acc.astype(np.float64) + terms[:, t]).astype(np.float32)
    return acc, None, None


def gemm_blocks(c, p, dtype=np.float64):
    """-> list of (X (M, K), W (Cout_block, K), ex, ex2): the blocks' outputs lie side by side along Cout.  ex / ex2: a further
    error of the x operand before its split (the depthwise chain), maximum and squared-rss; None otherwise"""
    f = lambda a: np.asarray(a, dtype)
    if c['kernel'] == 'sep':
        d, s1, s2 = depthwise(p['x'], p['dw'], c['k'], dtype)
        if dtype == np.float64:
            n = c['k'] * c['k']
            return [(d, f(p['pw']), n * U * s1, n * U * U * s2)]
        return [(d, f(p['pw']), None, None)]
    out = []
    for g in range(c['groups']):
        x = p['x'][..., g * c['cin_g']:g * c['cin_g'] + c['Cin']] if c['groups'] > 1 else p['x']
        X = im2col(f(x), c['k'], c['stride'], c['pad'], c['dil'])
        Wm = f(p['w'][g * c['Cout']:(g + 1) * c['Cout']]).reshape(c['Cout'], -1)
        if c['Cin2']:
            X = np.concatenate([X, f(p['x2']).reshape(-1, c['Cin2'])], 1)
            Wm = np.concatenate([Wm, f(p['w2'])], 1)
        out.append((X, Wm, None, None))
    return out


def _rows(c, p, name):
    """bias_n / residual as (M, Cout) float64 (the residual as the kernel sees it: hi + lo of an hl32 map)"""
    M = c['N'] * out_hw(c)[0] * out_hw(c)[1]
    if name == 'bn':
        return np.repeat(np.asarray(p['bn'], np.float64), M // c['N'], axis=0)
    r = pair_value(p['r']) if c['res'] == 'hl32' else p['r']
    return np.asarray(r, np.float64).reshape(M, -1)


def _silu(t):
    return t / (1.0 + np.exp(-t))


# ----------------------------------------------------------------------------
# reference and bounds
# ----------------------------------------------------------------------------
def reference(c, p, halves=None):
    """-> dict(ref, worst, rss) per output element, (M, Cout) -- (M, head_c) with a fused head.  halves: fp16-round the operands
    once (the plain fp16 product the mode must NOT be): ref only"""
    refs, worsts, rss2s, Ss = [], [], [], []
    for X, Wm, ex, ex2 in gemm_blocks(c, p):
        if halves:
            refs.append(X.astype(np.float16).astype(np.float64) @ Wm.astype(np.float16).astype(np.float64).T)
            continue
        K = X.shape[1]
        steps = (K + 31) // 32
        aX, aW, uX, uW = np.abs(X), np.abs(Wm), u(X), u(Wm)
        uX2 = uX ** 2
        if ex is not None:
            uX, uX2 = uX + ex, uX2 + ex2
        S = aX @ aW.T
        X2, W2 = X * X, Wm * Wm
        S2 = X2 @ W2.T
        refs.append(X @ Wm.T)
        worsts.append(uX @ aW.T + aX @ uW.T + uX @ uW.T + 2.0 ** -22 * S + (K + 3 * steps) * U * S)
        rss2s.append(uX2 @ W2.T + X2 @ (uW ** 2).T + 2.0 ** -44 * S2 + 2.0 ** -48 * (3 * steps + 32) * S2)
        Ss.append(S)
    t = np.concatenate(refs, 1) + np.asarray(p['b'], np.float64)[None]
    if halves:
        worst = rss = A = np.zeros_like(t)
    else:
        worst, rss, A = np.concatenate(worsts, 1), np.sqrt(np.concatenate(rss2s, 1)), np.concatenate(Ss, 1)
    A = A + np.abs(p['b'])[None]
    n_ep = 1
    for name, on in (('bn', c['bias_n']), ('r', bool(c['res']))):
        if on:
            v = _rows(c, p, name)
            t, A, n_ep = t + v, A + np.abs(v), n_ep + 1
    ep = n_ep * U * (A + worst)
    worst, rss = worst + ep, rss + ep
    if c['act'] == 1:
        out = np.maximum(t, 0.0)
    elif c['act'] == 2:
        with np.errstate(over='ignore'):
            out = _silu(t)
        ea = (13.0 + np.abs(t)) * U * np.abs(out) + 2.0 ** -126 + np.where(t < -87.0, np.abs(out), 0.0)
        worst, rss = SILU_LIP * worst + ea, SILU_LIP * rss + ea
    else:
        out = t
    if c['out_fmt']:
        e = u(np.abs(out) + worst)
        worst, rss = worst + e, rss + e
    if c['head_c']:
        hw, hb = np.asarray(p['hw'], np.float64), np.asarray(p['hb'], np.float64)
        n = out.shape[1] + 2
        Ah = (np.abs(out) + worst) @ np.abs(hw).T + np.abs(hb)[None]
        worst = worst @ np.abs(hw).T + n * U * Ah
        rss = np.sqrt((rss ** 2) @ (hw ** 2).T + n * U * U * ((out ** 2) @ (hw ** 2).T)) + U * np.abs(hb)[None]
        out = out @ hw.T + hb[None]
    if halves:
        return dict(ref=out)
    return dict(ref=out, worst=worst, rss=rss)


@functools.lru_cache(maxsize=None)
def case_reference(case_id, family):
    """(inputs, reference) of a listed case, computed once per process and not to be modified"""
    c = CASE[case_id]
    p = build(c, family)
    return p, reference(c, p)


def ratios(got, r):
    """(worst ratio against worst_bound, worst ratio against rss_bound, max|err| / max|ref|); NaN / inf count as inf"""
    err = np.abs(np.asarray(got, np.float64) - r['ref'])
    if not np.isfinite(err).all():
        return float('inf'), float('inf'), float('inf')
    tiny = 1e-300
    return (float((err / np.maximum(r['worst'], tiny)).max()), float((err / np.maximum(r['rss'], tiny)).max()),
            float(err.max() / max(float(np.abs(r['ref']).max()), tiny)))


# ----------------------------------------------------------------------------
# the kernel's arithmetic, emulated
# ----------------------------------------------------------------------------
def _flush(h):
    return np.where(np.abs(h) < MIN16, np.float32(0.0), h)


def emulate_gemm(X, Wm, variant=None):
    """(M, K) x (Cout, K) fp32 -> fp32 accumulator: per 32-channel step w_lo x_hi, then w_hi x_lo, then w_hi x_hi"""
    xh, xl = (h.astype(np.float32) for h in split(X))
    wh, wl = (h.astype(np.float32) for h in split(Wm))
    if variant == 'flush':
        xh, xl, wh, wl = _flush(xh), _flush(xl), _flush(wh), _flush(wl)
    acc = np.zeros((X.shape[0], Wm.shape[0]), np.float32)
    for i, k0 in enumerate(range(0, X.shape[1], 32)):
        s = slice(k0, k0 + 32)
        if variant != 'drop_wl':
            acc = acc + xh[:, s] @ wl[:, s].T
        if variant != 'drop_xl' and not (variant == 'hi_twice' and i % 2 == 0):
            acc = acc + xl[:, s] @ wh[:, s].T
        acc = acc + xh[:, s] @ wh[:, s].T
    return acc


def emulate(c, p, variant=None):
    """the listed case as the kernel computes it, fp32 epilogue included -> (M, Cout | head_c) fp32"""
    t = np.concatenate([emulate_gemm(X, Wm, variant) for X, Wm, _, _ in gemm_blocks(c, p, np.float32)], 1)
    t = t + p['b'][None]
    if c['bias_n']:
        t = t + _rows(c, p, 'bn').astype(np.float32)
    if c['res']:
        t = t + _rows(c, p, 'r').astype(np.float32)
    if c['act'] == 1:
        t = np.maximum(t, np.float32(0.0))
    elif c['act'] == 2:
        with np.errstate(over='ignore'):
            t = (t / (np.float32(1.0) + np.exp(-t))).astype(np.float32)
    if c['out_fmt']:
        t = pair_value(t)
    if c['head_c']:
        t = t @ p['hw'].T + p['hb'][None]
    return t.astype(np.float32)


# ----------------------------------------------------------------------------
# the exact family
# ----------------------------------------------------------------------------
def exact_expected(c, p):
    """-> (expected float64 (M, Cout | head_c), tolerance, q, largest sum of |terms|).  Asserts what makes the expectation exact:
    hi and lo are the integer and the 2^-12 parts and every term is a multiple of q; the caller compares the magnitude with
    2^24 q.  The tolerance is 0 (bit for bit) unless the case ends in SiLU: then SiLU's own rounding of an exact argument (module
    docstring), and the split of that value for an hl32 output."""
    refs, mags, q = [], [], 1.0
    for X, Wm, _, _ in gemm_blocks(c, p):
        halves = []
        for v in (X, Wm):
            hi, lo = (h.astype(np.float64) for h in split(v))
            assert np.array_equal(hi + lo, v), 'the pair does not hold the operand exactly'
            assert np.array_equal(hi, np.trunc(v)), 'hi is not the integer part'
            assert np.array_equal(lo / Q12, np.round(lo / Q12)), 'lo is not a multiple of 2^-12'
            if lo.any():
                q = Q12
            halves += [hi, lo]
        xh, xl, wh, wl = halves
        refs.append(X @ Wm.T - xl @ wl.T)      # integers + multiples of 2^-12 below 2^12: exact in float64
        mags.append(np.abs(xh) @ np.abs(wh).T + np.abs(xh) @ np.abs(wl).T + np.abs(xl) @ np.abs(wh).T)
    t, mag = np.concatenate(refs, 1), np.concatenate(mags, 1)
    for name, on in (('b', True), ('bn', c['bias_n']), ('r', bool(c['res']))):
        if on:
            v = np.asarray(p['b'], np.float64)[None] if name == 'b' else _rows(c, p, name)
            assert np.array_equal(v, np.round(v))
            t, mag = t + v, mag + np.abs(v)
    worst = float(mag.max())
    tol = np.zeros_like(t)
    if c['act'] == 1:
        t = np.maximum(t, 0.0)
    elif c['act'] == 2:
        with np.errstate(over='ignore'):
            arg, t = t, _silu(t)
        tol = (13.0 + np.abs(arg)) * U * np.abs(t) + 2.0 ** -126 + np.where(arg < -87.0, np.abs(t), 0.0)
    if c['out_fmt']:      # the exact fp32 value, split (a 24-bit value need not fit the pair)
        if c['act'] == 2:
            tol = tol + u(np.abs(t) + tol)
        else:
            t = pair_value(t.astype(np.float32)).astype(np.float64)
    if c['head_c']:
        assert c['act'] == 1
        hw, hb = np.asarray(p['hw'], np.float64), np.asarray(p['hb'], np.float64)
        assert np.array_equal(hw, np.round(hw)) and np.array_equal(hb, np.round(hb))
        worst = max(worst, float((np.abs(t) @ np.abs(hw).T + np.abs(hb)[None]).max()))
        t = t @ hw.T + hb[None]
    return t, tol, q, worst


# ----------------------------------------------------------------------------
# network level: move the bottlenecks' inner maps along the exponent ladder without changing the function
# ----------------------------------------------------------------------------
def rescale_bottlenecks(P, E, seed=0, up=False, aspp=True):
    """Folded parameter dict -> a dict of the SAME function whose inner maps sit at other magnitudes: the output channel c of every
    encoder.layer*.*.conv1 / conv2 (weight row and bias) is multiplied by 2^e_c and the matching input channel of the following
    conv2 / conv3 divided by it, e_c uniform in [-E, 0] (up: [0, E]).  ReLU commutes with a positive scale and a power of two is
    exact in fp32, so an fp32 forward is unchanged bit for bit (test_x3_range_case_host.py).  aspp: the same for the four
    convolution branches of every ASPP and the matching column blocks of aspp.project.0 (the pooled branch stays)."""
    rng = np.random.default_rng(seed)
    Q = {k: (np.array(w, copy=True), np.array(b, copy=True)) for k, (w, b) in P.items()}

    def move(name, nxt, col0=0):
        w, b = Q[name]
        e = rng.integers(0, E + 1, w.shape[0]) if up else rng.integers(-E, 1, w.shape[0])
        s = (2.0 ** e).astype(np.float32)
        Q[name] = (w * s.reshape(-1, *([1] * (w.ndim - 1))), b * s)
        w2, b2 = Q[nxt]
        w2 = w2.copy()
        w2[:, col0:col0 + len(s)] /= s.reshape(1, -1, *([1] * (w2.ndim - 2)))
        Q[nxt] = (w2, b2)

    for name in list(P):
        if name.startswith('encoder.layer') and name.endswith(('.conv1', '.conv2')):
            move(name, name[:-1] + str(int(name[-1]) + 1))
        elif aspp and '.aspp.convs.' in name and name.endswith('.0'):      # convs.0.0 .. convs.3.0 (the pooled branch ends in .1)
            pre, i = name.split('.aspp.convs.')[0], int(name.split('.aspp.convs.')[1][0])
            move(name, pre + '.aspp.project.0', i * P[name][0].shape[0])
    return Q


def rescaled_names(P, aspp=True):
    a, b = rescale_bottlenecks(P, 0, 0, False, aspp), rescale_bottlenecks(P, 1, 0, True, aspp)
    return [k for k in P if not np.array_equal(a[k][0], b[k][0])]
