"""Inputs, the kernels' arithmetic emulated on the CPU, plain float64 references and derived per-element error bounds of the
operand-range tests of the fp16 engine's convolutions (tests/test_f16_range_case_host.py, tests/test_gpu_f16_range.py):
csrc/conv_igemm.hip (also as the grouped kernel), conv_igemm256.hip, conv_igemm_s64.hip, conv3x3c64.hip, sepconv.hip and the
dwconv of layers.hip, through their C ABI entries.  numpy in float64 / float32 / float16; no GPU.  The structure is that of
tests/x3_range_case.py (im2col, U, SILU_LIP and the factors RSS_HOST / RSS_GPU come from there); what differs:

* the operands ARE fp16 values (made in float64, rounded once) and the reference is float64 arithmetic on those same values:
  there is no input-rounding term.  fp16 x fp16 is exact in fp32.
* the accumulation.  One 16x16x32 MFMA per 32-channel step enters the fp32 accumulator; the order inside an MFMA is not
  documented.  A term passes at most K additions inside MFMAs and ceil(K / 32) between them, each rounding a partial sum bounded
  by S = |x| . |w|:  worst (K + ceil(K / 32)) U S;  rss 2^-48 (x^2 . w^2)(ceil(K / 32) + 32).  K includes Cin2 of a second source
  (and the zero-weight pad columns of a group: they add exact zeros).
* the epilogue, as read in every kernel that has one -- conv_igemm.hip (the LDS-transposed and the direct one), conv_igemm256.hip
  (wave_epilogue, wave_epilogue_b2b), conv_igemm_s64.hip, conv3x3c64.hip (bias only), the mma role of sepconv.hip (bias only) --
  is the same everywhere:  v = acc + bias (a null bias adds 0.0);  v += bias_n;  v += (float)residual;  v = act(v);  store
  (half)v.  One fp32 addition each (one U of A = S + |b| + |b_n| + |r| plus the error so far), the fp16 residual converts exactly,
  ReLU is exact, SiLU = v / (1 + __expf(-v)) as derived in x3_range_case: (13 + |t|) U |silu(t)| + 2^-126, slope <= 1.1.
* the store is ONE rounding to fp16: h(v) = max(2^-11 |v|, 2^-25) below 65520, +-inf from 65520 on (torch's .half(), the oracle's
  Fp16Emu.r16).  With E the accumulated fp32 error (worst, or RSS rss capped at worst) an element is accepted when
  |got - y64| <= E + h(|y64| + E).  The inf rule is on t, the value the kernel rounds (y64 after the activation):
  t - E >= 65520: got must be +inf;  t + E <= -65520: -inf;  |t| + E < 65520: finite and inside the bound;  in between either
  (at most 1 % of a case's elements, and none outside the `over` family: asserted of the float64 reference on the CPU).
* the separable block: the depthwise half is an fp32 fmaf chain from 0 over the taps, ky-major (k*k U sum |tap x|), rounded to
  fp16 as the pointwise operand -- one more h() -- and both go through |pw|.  Head mode keeps y in fp32 (no store rounding) and
  adds an fp32 dot product over Cout: fmaf chains per mma wave (32 couts each), then head_store adds the waves' shares to the head
  bias one by one -- Cout / 32 roundings at the bias's magnitude.  emp_dwconv_nhwc_f16 alone is the chain and one store.
* the fused next conv (wave_epilogue_b2b) consumes the finished fp16 tile: next_out is held to the plain bound of a 1x1 ReLU
  convolution whose x is the `out` the kernel returned (next_reference).

The factors 3 (host) and 6 (GPU) on rss are x3_range_case's and were NOT refitted for this family.

Families (FAMILIES), each a function of (case, seed):
* exact : sparse +-1 / +-2 operands, integer bias / residual / head, the sum of the terms' magnitudes at most 2048
  (exact_expected asserts it): every partial sum in any order is an integer that fp32 AND fp16 hold, the result is the float64
  result bit for bit (a case that ends in SiLU: SiLU's own rounding of the exact argument, then the store).  Pins the index
  arithmetic of the shuffle, the split stores, the group strides, the second source's stride.
* ladder_dnE / ladder_upE, E in {0, 4, 8, 12}: randn (4 sigma) with one exponent per input channel on x and its inverse on w's
  column, x3_range_case's caps (never reached at E <= 12).  Going up the weights reach fp16's subnormals and stay: the MFMA reads
  them as values.
* top : 1 % of the activations at +-65504, weights (the depthwise taps of a separable block) x 2^-4: every sum stays in range.
* tiny : activations 2^-14 randn with 1 % each at +-2^-14, +-2^-24, -0.0; weights x 2^-4; bias, per-image bias, residual and
  next bias at 2^-18: most outputs are fp16 subnormals, which reference and store keep.
* over : ladder_up0 with about 2 % of the couts' biases at +-3 x 65520 and 2 % of the residual at +-65504: outputs beyond
  +-2 x 65520 must be +-inf of the right sign (0 behind a ReLU, -0 behind SiLU), never NaN and never 65504, while 65504 + O(1)
  must stay finite.  (A fused-next case pushes one cout up and the others down: its tile then holds one +inf per pixel, next_out
  is +inf or 0 by the sign of that weight, never inf - inf.)

Planted defects of the emulation (VARIANTS, has_feature): flush_in (subnormal operands read as zero), flush_out (subnormal
results stored as zero), round_twice (rounded to fp16 before the residual and again after), bias16 (bias and per-image bias
rounded to fp16), saturate (overflow stored as +-65504), acc16 (the accumulator rounded to fp16 after every K-walk group of 256
channels).  bias16 and acc16 are planted in the implicit-GEMM entries only: in the separable block the depthwise operand's own
fp16 rounding, 2^-11 |d| through |pw| (rss about 5e-4 at unit scale), is larger than either (2^-12 |b| and 2^-12 |acc|, about
2e-4) -- the bound is honest there and cannot tell them apart."""
import functools
import math

import numpy as np

from x3_range_case import RSS_GPU, RSS_HOST, SILU_LIP, U, depthwise, im2col, ladder_exponents  # noqa: F401

MIN16 = 2.0 ** -14
INF16 = 65520.0              # the smallest magnitude that rounds to inf
VARIANTS = ('flush_in', 'flush_out', 'round_twice', 'bias16', 'saturate', 'acc16')
LADDER_E = (0, 4, 8, 12)
LADDERS = tuple(f'ladder_{d}{E}' for E in LADDER_E for d in ('dn', 'up'))
FAMILIES = ('exact',) + LADDERS + ('top', 'tiny', 'over')
DEFECT_FAMILIES = {'flush_in': ('tiny',), 'flush_out': ('tiny',), 'saturate': ('over',), 'round_twice': LADDERS, 'bias16': LADDERS,
                   'acc16': LADDERS}
EXACT_MAG = 2048.0
HEAD_WAVE_COUTS = 32         # couts per mma wave of sepconv.hip (16 MT, MT = 2): the shares head_store adds to the head bias
KWALK = 256                  # channels per K-walk group (conv_igemm.hip: 4 slabs of 64; the other tiles: 8 of 32)


def h(v):
    return np.maximum(2.0 ** -11 * np.abs(v), 2.0 ** -25)


def r16(v):
    """one rounding to fp16 (inf from 65520 on), returned as float32"""
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(v, np.float32).astype(np.float16).astype(np.float32)


# ----------------------------------------------------------------------------
# cases: the smallest shapes that reach each path.  variants: the `variant` word of the entry (the `tile` of the grouped one)
# ----------------------------------------------------------------------------
def _c(id, entry, H, W, Cin, Cout, k=1, stride=1, pad=0, dil=1, act=1, variants=(0,), **kw):
    d = dict(id=id, entry=entry, N=1, H=H, W=W, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=pad, dil=dil, act=act, res=False,
             bias_n=False, Cin2=0, H2=0, W2=0, stride2=1, ps=0, split=0, split3=0, next=0, groups=1, gw=0, head_c=0,
             variants=tuple(variants))
    d.update(kw)
    return d


_TILES = tuple(s + 16 * t for t in (1, 2, 3) for s in (1, 2, 3))
_T3 = (19, 35, 51)
PACKED = 1 << 20

CASES = [
    # emp_conv2d_nhwc_f16
    _c('c1x1_40', 'nhwc', 9, 11, 64, 40, variants=_TILES + (112,)),
    _c('c3x3_72', 'nhwc', 9, 11, 64, 72, 3, 1, 1, variants=_TILES + (112,)),
    _c('c3x3_c64', 'nhwc', 9, 20, 64, 64, 3, 1, 1, variants=(96, 19)),
    _c('s2_res', 'nhwc', 10, 12, 128, 96, 3, 2, 1, act=0, res=True, variants=(19, 35, 51, 112)),
    _c('dil4_silu', 'nhwc', 12, 12, 64, 128, 3, 1, 4, 4, act=2, variants=(19, 51, 83, 112)),
    _c('k4608_bn', 'nhwc', 12, 12, 512, 128, 3, 1, 1, N=2, bias_n=True, variants=(19, 83, 112, (2 << 8) + 19)),
    _c('t256_res', 'nhwc', 1, 300, 128, 256, res=True, variants=(64, 64 | PACKED, 83)),
    _c('t256_dil2_silu', 'nhwc', 12, 12, 256, 256, 3, 1, 2, 2, act=2, variants=(64, 83, 19)),
    # emp_conv1x1_dual_nhwc_f16
    _c('dual', 'dual', 9, 7, 64, 256, Cin2=128, H2=17, W2=13, stride2=2, variants=(19, 51, 64, 83, 112)),
    # emp_conv2d_nhwc_f16_ex
    _c('ps', 'ex', 7, 9, 128, 128, ps=32, variants=_T3),
    _c('ps_in2', 'ex', 7, 9, 64, 128, ps=32, Cin2=64, H2=7, W2=9, variants=_T3),
    _c('split2', 'ex', 9, 11, 64, 176, split=128, variants=_T3),
    _c('split3', 'ex', 9, 11, 64, 112, split=64, split3=96, variants=_T3),
    _c('split256', 'ex', 1, 300, 128, 512, split=256, variants=(64,)),
    _c('next', 'ex', 224, 224, 64, 256, res=True, next=64, variants=(0,)),
    _c('next_in2', 'ex', 224, 224, 64, 256, res=True, next=64, Cin2=64, H2=224, W2=224, variants=(0,)),
    # emp_conv2d_grouped_nhwc_f16: Cin = the slab a group reads, gw = its width (input and output), row = (groups - 1) gw + Cin + 8
    _c('g56', 'grouped', 9, 11, 64, 56, 3, 1, 1, groups=3, gw=56, variants=(0, 1, 2)),
    _c('g72_s2_silu', 'grouped', 10, 12, 128, 72, 3, 2, 1, act=2, groups=2, gw=72, variants=(0, 1, 2)),
    # the separable family
    _c('dw5', 'dw', 9, 13, 128, 128, 5, act=0),
    _c('dw3', 'dw', 9, 13, 128, 128, 3, act=0),
    _c('sep5_128', 'sep', 8, 16, 128, 128, 5),
    _c('sep5_head1', 'sep', 8, 16, 256, 256, 5, head_c=1),
    _c('sep5_head2', 'sep', 8, 16, 256, 256, 5, head_c=2),
    _c('sep3_silu', 'sep', 9, 13, 128, 128, 3, act=2),
]
CASE = {c['id']: c for c in CASES}
ENTRIES = ('nhwc', 'dual', 'ex', 'grouped', 'dw', 'sep')


def is_gemm(c):
    return c['entry'] in ('nhwc', 'dual', 'ex', 'grouped')


def store16(c):
    return not c['head_c']


def has_feature(c, variant):
    """does the case run the code the planted defect touches (module docstring)"""
    if variant == 'flush_out':
        return store16(c)
    if variant == 'saturate':      # (the dwconv has no epilogue operand that could push an output over)
        return store16(c) and c['entry'] != 'dw'
    if variant == 'round_twice':
        return c['res']
    if variant in ('bias16', 'acc16'):
        return is_gemm(c)
    return True


def out_hw(c):
    if not is_gemm(c):
        return c['H'], c['W']
    e = c['dil'] * (c['k'] - 1) + 1
    return (c['H'] + 2 * c['pad'] - e) // c['stride'] + 1, (c['W'] + 2 * c['pad'] - e) // c['stride'] + 1


def total_cout(c):
    return c['Cout'] * c['groups']


def x_channels(c):
    return (c['groups'] - 1) * c['gw'] + c['Cin'] + 8 if c['groups'] > 1 else c['Cin']


def k_of(c):
    return c['Cin'] if c['entry'] in ('sep', 'dw') else c['k'] * c['k'] * c['Cin'] + c['Cin2']


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
def _randn(rng, shape):
    return np.clip(rng.standard_normal(shape), -4.0, 4.0)


def _ints(rng, shape, m=3):
    return rng.integers(-m, m + 1, shape).astype(np.float64)


def _sparse(rng, shape, p):
    return rng.choice([-2.0, -1.0, 1.0, 2.0], shape) * (rng.random(shape) < p)


def _seed(c, family):
    return 1000 * [k['id'] for k in CASES].index(c['id']) + FAMILIES.index(family) + 77


def over_channels(c):
    """(couts pushed up, couts pushed down) of the `over` family"""
    Co = total_cout(c)
    n = max(2, int(round(0.02 * Co)))
    idx = (np.arange(n) * 37 + 5) % Co
    if c['next']:
        return idx[:1], idx[1:]
    return idx[0::2], idx[1::2]


def build(c, family):
    """-> dict of arrays in the layouts the C ABI takes: fp16 x (N,H,W,Cx), w (Cout_total, k*k, Cin) tap-major (a group's pad
    columns zero), x2 (N,H2,W2,Cin2), w2 (Cout, Cin2), r (N,Ho,Wo,Cout), nw (next, Cout), dw (k*k, C), pw (Cout, C); fp32 b, bn
    (N, Cout), nb, hw (head_c, Cout), hb"""
    rng = np.random.default_rng(_seed(c, family))
    N, H, W, Cin, k = c['N'], c['H'], c['W'], c['Cin'], c['k']
    Ho, Wo = out_hw(c)
    Co, K, Cx, G, gw = total_cout(c), k_of(c), x_channels(c), c['groups'], c['gw']
    sep = not is_gemm(c)
    p = {}
    if family == 'exact':
        dens = min(1.0, math.sqrt(560.0 / (2.25 * K)))
        p['x'] = _sparse(rng, (N, H, W, Cx), dens)
        if sep:      # one tap of +-1 per channel: the depthwise value is a shifted +-x, exactly
            dw = np.zeros((k * k, Cin))
            dw[rng.integers(0, k * k, Cin), np.arange(Cin)] = rng.choice([-1.0, 1.0], Cin)
            p['dw'] = dw
            p['pw'] = _sparse(rng, (Co, Cin), dens)
        else:
            p['w'] = _sparse(rng, (Co, k * k, Cin), dens)
            if G > 1:
                p['w'][:, :, gw:] = 0.0
        if c['Cin2']:
            p['x2'] = _sparse(rng, (N, c['H2'], c['W2'], c['Cin2']), dens)
            p['w2'] = _sparse(rng, (Co, c['Cin2']), dens)
        p['b'] = _ints(rng, (Co,))
        if c['bias_n']:
            p['bn'] = _ints(rng, (N, Co))
        if c['res']:
            p['r'] = _ints(rng, (N, Ho, Wo, Co))
        if c['next']:
            p['nw'] = _sparse(rng, (c['next'], Co), 4.0 / Co)
            p['nb'] = _ints(rng, (c['next'],))
        if c['head_c']:
            p['hw'] = _ints(rng, (c['head_c'], Co), 1) * (rng.random((c['head_c'], Co)) < 0.125)
            p['hb'] = _ints(rng, (c['head_c'],))
    else:
        x = _randn(rng, (N, H, W, Cx))
        e = ladder_exponents(family, K, Cx, rng) if family.startswith('ladder') else np.zeros(Cx, np.int64)
        ws = es = 1.0            # scale of the weights; of the epilogue operands
        if family == 'top':
            x = np.where(rng.random(x.shape) < 0.01, rng.choice([65504.0, -65504.0], x.shape), x)
            ws = 2.0 ** -4
        if family == 'tiny':
            x = x * MIN16
            sel, sgn = rng.random(x.shape), rng.choice([-1.0, 1.0], x.shape)
            for i, v in enumerate((2.0 ** -14, 2.0 ** -24)):
                x = np.where((sel >= 0.01 * i) & (sel < 0.01 * (i + 1)), sgn * v, x)
            x = np.where((sel >= 0.02) & (sel < 0.03), -0.0, x)
            ws, es = 2.0 ** -4, 2.0 ** -18
        p['x'] = x * 2.0 ** e
        if sep:
            p['dw'] = _randn(rng, (k * k, Cin)) / k * (ws if family == 'top' else 1.0)
            p['pw'] = _randn(rng, (Co, Cin)) / math.sqrt(Cin) * 2.0 ** -e * (1.0 if family == 'top' else ws)
        else:
            w = _randn(rng, (Co, k * k, Cin)) / math.sqrt(k * k * (gw or Cin) + c['Cin2']) * ws
            for g in range(G):
                w[g * c['Cout']:(g + 1) * c['Cout']] *= 2.0 ** -e[g * gw:g * gw + Cin]
            if G > 1:
                w[:, :, gw:] = 0.0      # the pad columns of a group's slab: they meet the neighbour group's channels
            p['w'] = w
        if c['Cin2']:
            e2 = ladder_exponents(family, K, c['Cin2'], rng) if family.startswith('ladder') else np.zeros(c['Cin2'], np.int64)
            x2 = _randn(rng, (N, c['H2'], c['W2'], c['Cin2']))
            if family == 'tiny':
                x2 = x2 * MIN16
            p['x2'] = x2 * 2.0 ** e2
            p['w2'] = _randn(rng, (Co, c['Cin2'])) / math.sqrt(K) * ws * 2.0 ** -e2
        b = _randn(rng, (Co,)) * es
        if family == 'over':
            up, dn = over_channels(c)
            b[up], b[dn] = 3.0 * INF16, -3.0 * INF16
        p['b'] = b
        if c['bias_n']:
            p['bn'] = _randn(rng, (N, Co)) * es
        if c['res']:
            r = _randn(rng, (N, Ho, Wo, Co)) * es
            if family == 'over':
                r = np.where(rng.random(r.shape) < 0.02, rng.choice([65504.0, -65504.0], r.shape), r)
            p['r'] = r
        if c['next']:
            p['nw'] = _randn(rng, (c['next'], Co)) / math.sqrt(Co)
            p['nb'] = _randn(rng, (c['next'],)) * es
        if c['head_c']:
            p['hw'] = _randn(rng, (c['head_c'], Co)) / math.sqrt(Co)
            p['hb'] = _randn(rng, (c['head_c'],))
    f32 = ('b', 'bn', 'nb', 'hw', 'hb')
    with np.errstate(over='raise'):
        return {n: np.ascontiguousarray(v, dtype=np.float32 if n in f32 else np.float16) for n, v in p.items()}


# ----------------------------------------------------------------------------
# the GEMM view
# ----------------------------------------------------------------------------
def second_source(c, p, dtype):
    s = c['stride2']
    Ho, Wo = out_hw(c)
    return np.asarray(p['x2'], dtype)[:, ::s, ::s][:, :Ho, :Wo].reshape(-1, c['Cin2'])


def gemm_blocks(c, p, dtype=np.float64):
    """-> list of (X (M, K), W (Cout_block, K), group id per column): the blocks' outputs lie side by side along Cout; the group
    id is the K-walk group of a column (the second source continues the last one)"""
    f = lambda a: np.asarray(a, dtype)
    out = []
    for g in range(c['groups']):
        x = p['x'][..., g * c['gw']:g * c['gw'] + c['Cin']] if c['groups'] > 1 else p['x']
        X = im2col(f(x), c['k'], c['stride'], c['pad'], c['dil'])
        Wm = f(p['w'][g * c['Cout']:(g + 1) * c['Cout']]).reshape(c['Cout'], -1)
        grp = np.tile(np.arange(c['Cin']) // KWALK, c['k'] * c['k'])
        if c['Cin2']:
            X = np.concatenate([X, second_source(c, p, dtype)], 1)
            Wm = np.concatenate([Wm, f(p['w2'])], 1)
            grp = np.concatenate([grp, np.full(c['Cin2'], grp.max())])
        out.append((X, Wm, grp))
    return out


def _rows(c, p, name):
    M = c['N'] * out_hw(c)[0] * out_hw(c)[1]
    if name == 'bn':
        return np.repeat(np.asarray(p['bn'], np.float64), M // c['N'], axis=0)
    return np.asarray(p['r'], np.float64).reshape(M, -1)


def _silu(t):
    with np.errstate(over='ignore'):
        return t / (1.0 + np.exp(-t))


# ----------------------------------------------------------------------------
# reference and bounds
# ----------------------------------------------------------------------------
def _gemm_bound(X, Wm, ex=None, ex2=None):
    """float64 product and the accumulation terms; ex / ex2: a further error of the x operand (maximum, squared rss)"""
    K = X.shape[1]
    steps = (K + 31) // 32
    with np.errstate(invalid='ignore', over='ignore'):
        aX = np.abs(X) + (ex if ex is not None else 0.0)
        S = aX @ np.abs(Wm).T
        S2 = (aX * aX) @ (Wm * Wm).T
        ref = X @ Wm.T
    worst = (K + steps) * U * S
    rss2 = 2.0 ** -48 * (steps + 32) * S2
    if ex is not None:
        worst, rss2 = worst + ex @ np.abs(Wm).T, rss2 + ex2 @ (Wm * Wm).T
    return ref, worst, rss2, S


@np.errstate(invalid='ignore', over='ignore')      # (inf - inf of the bounds next to an infinite reference value)
def _epilogue(t, worst, rss, A, adds, act, to16, head=None, wave_couts=HEAD_WAVE_COUTS):
    """adds: the (M, Cout) float64 operands of the fp32 additions, in the kernels' order -> dict(ref, worst, rss, store16).
    wave_couts: couts per mma wave of the kernel whose head this is (sepp_range_case passes sepconv_precise.hip's)"""
    for v in adds:
        t, A = t + v, A + np.abs(v)
    ep = len(adds) * U * (A + worst)
    worst, rss = worst + ep, rss + ep
    nf = ~np.isfinite(t)            # (a fused-next tile of the `over` family holds +inf: the value is then exact)
    worst, rss = np.where(nf, 0.0, worst), np.where(nf, 0.0, rss)
    if act == 1:
        out = np.maximum(t, 0.0)
    elif act == 2:
        out = _silu(t)
        ea = (13.0 + np.abs(t)) * U * np.abs(out) + 2.0 ** -126 + np.where(t < -87.0, np.abs(out), 0.0)
        worst, rss = SILU_LIP * worst + ea, SILU_LIP * rss + ea
    else:
        out = t
    if head is not None:
        hw, hb = (np.asarray(v, np.float64) for v in head)
        n = out.shape[1] + 2
        Ah = (np.abs(out) + worst) @ np.abs(hw).T + np.abs(hb)[None]
        worst = worst @ np.abs(hw).T + n * U * Ah
        # head_store starts from the head bias and adds the mma waves' shares (HEAD_WAVE_COUTS couts each) one by one: that many
        # roundings of a partial sum bounded by |hb| + |y| . |hw|, not one (the x3 module's form, `+ U |hb|`, has one)
        nw = out.shape[1] // wave_couts
        rss = (np.sqrt((rss ** 2) @ (hw ** 2).T + n * U * U * ((out ** 2) @ (hw ** 2).T))
               + math.sqrt(nw) * U * (np.abs(hb)[None] + np.abs(out) @ np.abs(hw).T))
        out = out @ hw.T + hb[None]
    return dict(ref=out, worst=worst, rss=np.minimum(rss, worst), store16=to16)


def reference(c, p):
    """-> dict(ref, worst, rss, store16) per output element: (M, Cout_total), (M, head_c) with a fused head.  worst / rss are the
    accumulated fp32 error E BEFORE the store; accept() adds the store's rounding"""
    if c['entry'] in ('dw', 'sep'):
        kk = c['k'] * c['k']
        d, s1, s2 = depthwise(p['x'], p['dw'], c['k'], np.float64)
        e_dw, e_dw2 = kk * U * s1, kk * U * U * s2
        if c['entry'] == 'dw':
            return dict(ref=d, worst=e_dw, rss=np.minimum(np.sqrt(e_dw2), e_dw), store16=True)
        r = h(np.abs(d) + e_dw)
        ref, worst, rss2, S = _gemm_bound(d, np.asarray(p['pw'], np.float64), e_dw + r, e_dw2 + r * r)
        head = (p['hw'], p['hb']) if c['head_c'] else None
        return _epilogue(ref, worst, np.sqrt(rss2), S, [np.asarray(p['b'], np.float64)[None]], c['act'], store16(c), head)
    parts = [_gemm_bound(X, Wm) for X, Wm, _ in gemm_blocks(c, p)]
    ref, worst, rss2, S = (np.concatenate([q[i] for q in parts], 1) for i in range(4))
    adds = [np.asarray(p['b'], np.float64)[None] + np.zeros_like(ref)]
    if c['bias_n']:
        adds.append(_rows(c, p, 'bn'))
    if c['res']:
        adds.append(_rows(c, p, 'r'))
    return _epilogue(ref, worst, np.sqrt(rss2), S, adds, c['act'], True)


def next_reference(c, p, out16):
    """the fused next conv on the tile the kernel returned: a 1x1 ReLU convolution of out16 (M, Cout) fp16"""
    ref, worst, rss2, S = _gemm_bound(np.asarray(out16, np.float64), np.asarray(p['nw'], np.float64))
    return _epilogue(ref, worst, np.sqrt(rss2), S, [np.asarray(p['nb'], np.float64)[None] + np.zeros_like(ref)], 1, True)


@functools.lru_cache(maxsize=None)
def case_reference(case_id, family):
    """(inputs, reference) of a listed case, computed once per process and not to be modified"""
    c = CASE[case_id]
    p = build(c, family)
    return p, reference(c, p)


# ----------------------------------------------------------------------------
# acceptance
# ----------------------------------------------------------------------------
def _bound(r, E):
    return E + h(np.abs(r['ref']) + E) if r['store16'] else E


def accept(got, r, factor):
    """per-element acceptance (module docstring) -> (ok (bool array), ambiguous (bool array): the band where inf and finite are
    both right).  factor: on rss (RSS_HOST / RSS_GPU); E = min(factor rss, worst)"""
    got = np.asarray(got, np.float64)
    t = r['ref']
    E = np.minimum(factor * r['rss'], r['worst'])
    with np.errstate(invalid='ignore'):
        inside = np.isfinite(got) & (np.abs(got - t) <= _bound(r, E))
        if not r['store16']:
            return inside, np.zeros(t.shape, bool)
        pinf, ninf = t - E >= INF16, t + E <= -INF16
        fin = np.abs(t) + E < INF16
    amb = ~(pinf | ninf | fin)
    ok = np.where(pinf, got == np.inf, np.where(ninf, got == -np.inf,
                  np.where(fin, inside, inside | (np.isinf(got) & (np.sign(got) == np.sign(t))))))
    return ok, amb


def ratios(got, r):
    """(f_worst, f_rss, max|err| / max|ref|) over the elements that must be finite: f is the factor on E at which the element
    would just be accepted, |err| = f E + h(|y| + f E) solved for f -- so f_worst <= 1 and f_rss <= factor is the acceptance"""
    got = np.asarray(got, np.float64)
    t = r['ref']
    with np.errstate(invalid='ignore'):
        m = np.isfinite(t) & (np.abs(t) + r['worst'] < INF16 if r['store16'] else np.isfinite(t))
    if not np.isfinite(got[m]).all():
        return float('inf'), float('inf'), float('inf')
    err = np.abs(got[m] - t[m])

    def f(E):
        E = np.maximum(E[m], 1e-300)
        if not r['store16']:
            return float((err / E).max())
        a = (err - 2.0 ** -11 * np.abs(t[m])) / (E * (1.0 + 2.0 ** -11))
        b = (err - 2.0 ** -25) / E
        return float(np.maximum(np.minimum(a, b), 0.0).max())
    return f(r['worst']), f(r['rss']), float(err.max() / max(float(np.abs(t[m]).max()), 1e-300))


# ----------------------------------------------------------------------------
# the kernels' arithmetic, emulated
# ----------------------------------------------------------------------------
def _flush(v):
    return np.where(np.abs(v) < MIN16, np.float32(0.0), v).astype(np.float32)


def emulate_gemm(X, Wm, grp, variant=None):
    """(M, K) x (Cout, K) fp16 values in fp32 -> the fp32 accumulator: one product per 32-channel step, K-walk groups in order"""
    if variant == 'flush_in':
        X, Wm = _flush(X), _flush(Wm)
    acc = np.zeros((X.shape[0], Wm.shape[0]), np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for g in range(int(grp.max()) + 1):
            cols = np.nonzero(grp == g)[0]
            for k0 in range(0, len(cols), 32):
                s = cols[k0:k0 + 32]
                acc = acc + X[:, s] @ Wm[:, s].T
            if variant == 'acc16':
                acc = r16(acc)
    return acc


def _finish(t, adds, res, act, variant, to16, head=None):
    with np.errstate(invalid='ignore', over='ignore'):
        for v in adds:
            t = t + (r16(v) if variant == 'bias16' else np.asarray(v, np.float32))
        if res is not None:
            if variant == 'round_twice':
                t = r16(t)
            t = t + np.asarray(res, np.float32)
        if act == 1:
            t = np.maximum(t, np.float32(0.0))
        elif act == 2:
            t = (t / (np.float32(1.0) + np.exp(-t))).astype(np.float32)
        if head is not None:      # head_store: the bias, then the waves' shares in order
            v = np.broadcast_to(np.asarray(head[1], np.float32)[None], (t.shape[0], len(head[1])))
            for c0 in range(0, t.shape[1], HEAD_WAVE_COUTS):
                v = v + t[:, c0:c0 + HEAD_WAVE_COUTS] @ head[0][:, c0:c0 + HEAD_WAVE_COUTS].T
            return v.astype(np.float32)
        if not to16:
            return t
        o = r16(t)
        if variant == 'saturate':
            o = np.where(np.isinf(o), np.sign(o) * np.float32(65504.0), o)
        if variant == 'flush_out':
            o = _flush(o)
    return o.astype(np.float16)


def emulate(c, p, variant=None):
    """the listed case as the kernel computes it -> (M, Cout_total) fp16, (M, head_c) fp32 with a head; a fused-next case gives
    (out, next_out)"""
    if c['entry'] in ('dw', 'sep'):
        x, dw = np.asarray(p['x'], np.float32), np.asarray(p['dw'], np.float32)
        if variant == 'flush_in':
            x, dw = _flush(x), _flush(dw)
        d, _, _ = depthwise(x, dw, c['k'], np.float32)
        if c['entry'] == 'dw':
            return _finish(d, [], None, 0, variant, True)
        acc = emulate_gemm(r16(d), np.asarray(p['pw'], np.float32), np.zeros(c['Cin'], np.int64), variant)
        head = (p['hw'], p['hb']) if c['head_c'] else None
        return _finish(acc, [p['b'][None]], None, c['act'], variant, store16(c), head)
    acc = np.concatenate([emulate_gemm(X, Wm, grp, variant) for X, Wm, grp in gemm_blocks(c, p, np.float32)], 1)
    adds = [p['b'][None]] + ([_rows(c, p, 'bn')] if c['bias_n'] else [])
    out = _finish(acc, adds, _rows(c, p, 'r') if c['res'] else None, c['act'], variant, True)
    if not c['next']:
        return out
    acc = emulate_gemm(out.astype(np.float32), np.asarray(p['nw'], np.float32), np.zeros(out.shape[1], np.int64), variant)
    return out, _finish(acc, [p['nb'][None]], None, 1, variant, True)


# ----------------------------------------------------------------------------
# the exact family
# ----------------------------------------------------------------------------
def exact_expected(c, p):
    """-> (float64 result (M, Cout_total | head_c), the same for next_out or None, largest sum of |terms|).  Asserts what makes
    the expectation exact: integer operands and every sum of magnitudes <= 2048 (a head's fp32 sum: 2^24).  Behind SiLU the
    result is not an integer: reference()'s bound then holds SiLU's rounding of the exact argument"""
    def ints(*vs):
        for v in vs:
            assert np.array_equal(np.asarray(v, np.float64), np.round(np.asarray(v, np.float64)))
    if c['entry'] in ('dw', 'sep'):
        ints(p['x'], p['dw'])
        d, s1, _ = depthwise(p['x'], p['dw'], c['k'], np.float64)
        assert s1.max() <= 2.0
        if c['entry'] == 'dw':
            return d, None, float(s1.max())
        blocks = [(d, np.asarray(p['pw'], np.float64))]
    else:
        blocks = [(X, Wm) for X, Wm, _ in gemm_blocks(c, p)]
    t = np.concatenate([X @ Wm.T for X, Wm in blocks], 1)
    mag = np.concatenate([np.abs(X) @ np.abs(Wm).T for X, Wm in blocks], 1)
    for X, Wm in blocks:
        ints(X, Wm)
    for name, on in (('b', True), ('bn', c['bias_n']), ('r', c['res'])):
        if on:
            v = np.asarray(p['b'], np.float64)[None] if name == 'b' else _rows(c, p, name)
            ints(v)
            t, mag = t + v, mag + np.abs(v)
    worst = float(mag.max())
    assert worst <= EXACT_MAG, worst
    t = np.maximum(t, 0.0) if c['act'] == 1 else _silu(t) if c['act'] == 2 else t
    nxt = None
    if c['next']:
        nw, nb = np.asarray(p['nw'], np.float64), np.asarray(p['nb'], np.float64)
        ints(nw, nb)
        m2 = float((np.abs(t) @ np.abs(nw).T + np.abs(nb)[None]).max())
        assert m2 <= EXACT_MAG, m2
        nxt = np.maximum(t @ nw.T + nb[None], 0.0)
    if c['head_c']:
        hw, hb = np.asarray(p['hw'], np.float64), np.asarray(p['hb'], np.float64)
        ints(hw, hb)
        assert float((np.abs(t) @ np.abs(hw).T + np.abs(hb)[None]).max()) < 2.0 ** 24
        t = t @ hw.T + hb[None]
    return t, nxt, worst


def exact_mismatches(c, got, want, r):
    """number of elements that are not the exact result (behind SiLU: not inside SiLU's own bound)"""
    if c['act'] == 2:
        return int((~accept(got, r, RSS_GPU)[0]).sum())
    return int((np.asarray(got, np.float64) != want).sum())
