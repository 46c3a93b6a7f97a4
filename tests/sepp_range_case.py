"""Inputs, the kernel's arithmetic emulated on the CPU, a plain float64 reference and derived per-element error bounds of the
operand-range tests of the precise separable block (tests/test_sepp_range_case_host.py, tests/test_gpu_sepp_range.py):
csrc/sepconv_precise.hip through emp_sepconvp_nhwc_f16 / emp_sepconvp_ws_nhwc_f16 and the three pack entries.  numpy in float64 /
float32 / float16; no GPU.  The method is that of tests/x3_range_case.py and tests/f16_range_case.py (U, SILU_LIP, the factors
RSS_HOST / RSS_GPU, depthwise, im2col, ladder_exponents come from the first; h, r16, INF16, MIN16, EXACT_MAG, the activation / head
terms (_epilogue) and the acceptance rule with its inf band (accept, ratios) from the second).  What is this kernel's own:

* the reference is float64 arithmetic on the operands the kernel holds: fp16 activations, fp32 taps (NOT fp16 values), pointwise
  weights rounded once to fp16 -- for the weight-split form (WS) the float64 sum of fp16(w) and fp16(w - fp16(w)), as
  sepconvp_pack_pw_kernel makes them (w - fp16(w) is exact in fp32) -- and fp32 bias, head weights and head bias.
* depthwise: an fp32 fma chain from 0 over the k*k taps, ky-major / kx-minor (the kernel walks input rows r and, per row, ky with
  y = r - ky: for one output row ky ascends with r).  fp16 x fp32 products are exact inside the fma.  k*k roundings of partial sums
  bounded by s = sum |tap x|:  e_dw = k*k U s  (rss: k*k U^2 sum (tap x)^2).
* the split (split_hi_lo, sepconv_common.h): hi = cvt_pkrtz(d), lo = cvt_pkrtz(d - hi), BOTH round toward zero; d - hi is exact in
  fp32.  With e = floor(log2 |d|): hi keeps the 11 leading bits, the rest r = d - hi has the sign of d and |r| < 2^(e-10); lo keeps
  the 11 leading bits of r, so the pair is short of d by less than 2^(e-21) where lo is a normal fp16 (|r| >= 2^-14) and by less than
  2^-24, the subnormal step, where it is not (below 2^-14 hi itself is a multiple of 2^-24 and lo is zero; below 2^-24 the pair is
  zero):      u(d) = max(2^-21 2^floor(log2 |d|), 2^-24), capped at |d|.
  The issue's form has 2^-20; the code gives 2^-21: 22 bits, not the header's 21, from |d| = 2^-3 up (2^(e-21) >= 2^-24), an absolute
  2^-24 below.  The error has the sign of -d: these are truncations, one-sided, NOT zero-mean roundings, so the term enters rss at
  its worst-case value, linearly:  sum |w| u(d).  (Nothing smaller is claimed; it is 1e-3 of the store's rounding at unit scale.)
  Round toward zero does not overflow by IEEE's rule: from 65520 on hi = +-65504 and lo carries the rest, to within lo's own step
  2^(floor(log2(|d| - 65504)) - 10) <= 32, up to a total of 65504 + 65504 = 131008; beyond that the value would be clamped.  u()
  follows that rule up to 131008; `dover` is the family that asks the hardware.
* GEMM: fp16 x fp16 products are exact in fp32.  The accumulators start from the bias; per 32-channel k-step the MFMAs are w*hi,
  w*lo and, WS, w_lo*hi: m = 2 (3) per step.  A term passes at most m K additions inside MFMAs and m ceil(K / 32) between them, each
  rounding a partial sum bounded by A = |b| + (|w| + |w_lo|) . |d|:  worst (m K + m ceil(K/32)) U A;  rss 2^-48 (m ceil(K/32) + 32)
  (|b| + sqrt(d^2 . w^2))^2.  There is no epilogue addition: the bias is inside the partial sums.
* WS computes (w + w_lo)(hi + lo) - w_lo lo: the dropped term is sum |w_lo| |lo|, |lo| < 2^-10 |d| (|d| - 65504 beyond 65536),
  carried linearly in both bounds.
* epilogue: act (ReLU exact, SiLU as in x3_range_case), then ONE store rounding h().  Head mode: no store rounding; head_plane_sums
  is an fmaf chain over the wave's couts, head_store adds the NMW = 4 mma waves' shares to the head bias one by one.  An mma wave
  holds 16 MT couts: 32 at Cout = 128 (MT = 2) and 64 at Cout = 256 (MT = 4) -- four shares either way, not Cout / 32 as in
  sepconv.hip (eight waves): f16_range_case's head term is used with wave_couts = Cout / 4.

Acceptance is f16_range_case's: |got - y64| <= E + h(|y64| + E), E = min(worst, RSS rss), the factors 3 (host) and 6 (GPU) are
x3_range_case's and were not refitted.

Families (FAMILIES; families_of(case)), each a function of (case, seed):
* exact : sparse +-1 / +-2 activations, one tap of +-1 per channel at a random position, sparse +-1 / +-2 weights, integer bias and
  head; sum of magnitudes <= 2048 (exact_expected asserts it).  The result is the float64 result bit for bit (behind SiLU: within
  SiLU's own rounding and the store).  Pins which tap is which, the halo indexing at ragged edges, the swizzled B-tile addressing
  and the packers' fragment order.
* ladder_dnE / ladder_upE, E in {0, 4, 8, 12}: one exponent per input channel on x, its inverse on that channel's pointwise column
  (the depthwise half is per channel, so the float64 result keeps its scale); ladder_exponents and its caps.
* top : 1 % of the activations at +-65504, taps x 2^-4: every |d| stays below 65504 (asserted of the reference on the CPU).
* tiny : activations 2^-14 randn with 1 % each at +-2^-14, +-2^-24 and -0.0; pointwise weights x 2^-4, bias 2^-18: most hi halves
  are subnormal and every lo half is subnormal or zero.
* over : ladder_up0 with about 2 % of the couts' biases at +-3 x 65520: outputs beyond +-2 x 65520 must be +-inf of the right sign
  (0 behind ReLU, -0 behind SiLU), never NaN and never 65504.  Not for head cases.
* dover : 1 % of the activations at +-65504, ONE tap per channel of magnitude in [1.1, 1.6] and the others x 2^-4, pointwise weights
  x 2^-4: about 1 % of |d| lies in (65520, 131008 - 4096), nothing beyond, every output finite (all asserted of the reference).

Planted defects of the emulation (VARIANTS, DEFECT_FAMILIES, has_feature): no_lo (the operand is hi only), lo_every_second_kstep,
flush_pair (subnormal hi / lo read as zero), taps16 (taps rounded to fp16), ws_no_third (w_lo*hi missing), saturate_store (overflow
stored as +-65504), bias_last (bias rounded to fp16 and added after the GEMM).  The five that are planted on the ladders are not
listed for ladder_dn12, and bias_last not for ladder_dn8 either: there a twelfth of the channels carries depthwise values near
2^-12 (2^-8), where the pair's absolute floor 2^-24 IS fp16's own step, against pointwise columns of 2^12 (2^8).  The bound's
honest split term, sum |w| 2^-24 over those channels -- one-sided, hence linear in K -- is then as large as what hi alone, fp16 taps
or a missing w_lo leave on the unit-scale channels (2^-11 per term, summed at random: sqrt(K)), and at dn8 as large as 2^-12 |b|
through a head: correct arithmetic and the defect cannot be told apart (0 elements outside on p5_512 and on the head cases)."""
import functools
import math

import numpy as np

from x3_range_case import RSS_GPU, RSS_HOST, SILU_LIP, U, depthwise, im2col, ladder_exponents  # noqa: F401
import f16_range_case as fc
from f16_range_case import EXACT_MAG, INF16, MIN16, accept, h, r16, ratios  # noqa: F401

VARIANTS = ('no_lo', 'lo_every_second_kstep', 'flush_pair', 'taps16', 'ws_no_third', 'saturate_store', 'bias_last')
LADDER_E = (0, 4, 8, 12)
LADDERS = tuple(f'ladder_{d}{E}' for E in LADDER_E for d in ('dn', 'up'))
FAMILIES = ('exact',) + LADDERS + ('top', 'tiny', 'over', 'dover')
OVERFLOW_FAMILIES = ('over',)      # where the either-inf-or-finite band may hold elements at all
_TO_DN8 = tuple(f for f in LADDERS if f != 'ladder_dn12')
DEFECT_FAMILIES = {'no_lo': _TO_DN8 + ('top',), 'lo_every_second_kstep': _TO_DN8, 'flush_pair': ('tiny',), 'taps16': _TO_DN8,
                   'ws_no_third': _TO_DN8, 'saturate_store': ('over',),
                   'bias_last': tuple(f for f in _TO_DN8 if f != 'ladder_dn8')}
MAX16 = 65504.0
PAIR_MAX = 2 * MAX16         # 131008: what hi + lo can hold
DOVER_MARGIN = 4096.0
NMW = 4                      # mma waves of sepconv_precise.hip (SC_NMW): the shares head_store adds to the head bias
GRID = 256                   # persistent_grid(): one workgroup per CU, rounded down to a multiple of 8; an MI355X has 256 CUs
TILE_H, TILE_W = 8, 16


# ----------------------------------------------------------------------------
# cases: the smallest shapes that reach each path
# ----------------------------------------------------------------------------
def multi_shape(N, grid=GRID):
    """the smallest H x W (in pixels) at which a workgroup takes two tiles: tile_of(1) of workgroup 0 is 8 * (grid / 8) = grid, so
    N * tiles_x * tiles_y > grid; ragged in both directions"""
    best = None
    for ty in range(1, grid + 2):
        tx = -(-(grid // N + 1) // ty)
        H, W = (ty - 1) * TILE_H + 1, (tx - 1) * TILE_W + 1
        if best is None or H * W < best[0] * best[1]:
            best = (H, W)
    return best


def _c(id, ks, H, W, C, Cout, act, head=0, ws=False, in_ld=0, N=1, entry=None):
    return dict(id=id, ks=ks, N=N, H=H, W=W, C=C, in_ld=in_ld or C, Cout=Cout, act=act, head_c=head, ws=ws,
                entry=entry or ('head' if head else 'ws' if ws else f'p{ks}'))


CASES = [
    _c('p5_128', 5, 9, 17, 128, 128, 1),
    _c('p5_ld', 5, 9, 17, 192, 256, 0, in_ld=200),      # in_ld % 8 == 0 is the launcher's 16-byte rule
    _c('p5_512', 5, 8, 16, 512, 256, 1),
    _c('p5_silu', 5, 9, 17, 128, 128, 2),
    _c('p5_head1', 5, 9, 17, 256, 256, 1, head=1),
    _c('p5_head2', 5, 8, 16, 256, 256, 1, head=2),
    _c('p3_silu', 3, 9, 17, 128, 128, 2),
    _c('p3_256', 3, 9, 17, 256, 256, 1),
    _c('ws5_128', 5, 9, 17, 128, 128, 1, ws=True),
    _c('ws3_silu', 3, 9, 17, 128, 128, 2, ws=True),
    _c('ws5_head1', 5, 9, 17, 128, 128, 1, head=1, ws=True),
    _c('multi', 5, *multi_shape(2), 128, 128, 1, N=2),
]
CASE = {c['id']: c for c in CASES}
ENTRIES = ('p5', 'p3', 'ws', 'head')


def families_of(c):
    if c['id'] == 'multi':
        return ('exact', 'ladder_dn0')
    return tuple(f for f in FAMILIES if not (f == 'over' and c['head_c']))


def has_feature(c, variant):
    if variant == 'ws_no_third':
        return c['ws']
    if variant == 'saturate_store':
        return not c['head_c']
    return True


def defect_families(c, variant):
    return tuple(f for f in DEFECT_FAMILIES[variant] if f in families_of(c))


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
def _seed(c, family):
    return 1000 * [k['id'] for k in CASES].index(c['id']) + FAMILIES.index(family) + 4242


def over_channels(c):
    n = max(2, int(round(0.02 * c['Cout'])))
    idx = (np.arange(n) * 37 + 5) % c['Cout']
    return idx[0::2], idx[1::2]


def build(c, family):
    """-> dict of arrays in the layouts the C ABI takes: fp16 x (N,H,W,in_ld) (channels from C on are not the kernel's to read);
    fp32 dw (k*k, C), pw (Cout, C) -- the packers' inputs --, b, hw (head_c, Cout), hb"""
    rng = np.random.default_rng(_seed(c, family))
    N, H, W, C, ld, k, Co, hc = c['N'], c['H'], c['W'], c['C'], c['in_ld'], c['ks'], c['Cout'], c['head_c']
    p = {}
    if family == 'exact':
        dens = min(1.0, math.sqrt(560.0 / (2.25 * C)))
        p['x'] = fc._sparse(rng, (N, H, W, ld), dens)
        dw = np.zeros((k * k, C))
        dw[rng.integers(0, k * k, C), np.arange(C)] = rng.choice([-1.0, 1.0], C)
        p['dw'] = dw
        p['pw'] = fc._sparse(rng, (Co, C), dens)
        p['b'] = fc._ints(rng, (Co,))
        if hc:
            p['hw'] = fc._ints(rng, (hc, Co), 1) * (rng.random((hc, Co)) < 0.125)
            p['hb'] = fc._ints(rng, (hc,))
    else:
        x = fc._randn(rng, (N, H, W, ld))
        e = np.zeros(ld, np.int64)
        if family.startswith('ladder'):
            e[:C] = ladder_exponents(family, C, C, rng)
        ts = ws = es = 1.0            # scale of the taps; of the pointwise weights; of the bias
        if family in ('top', 'dover'):
            x = np.where(rng.random(x.shape) < 0.01, rng.choice([MAX16, -MAX16], x.shape), x)
            ts = 2.0 ** -4
        if family == 'tiny':
            x = x * MIN16
            sel, sgn = rng.random(x.shape), rng.choice([-1.0, 1.0], x.shape)
            for i, v in enumerate((2.0 ** -14, 2.0 ** -24)):
                x = np.where((sel >= 0.01 * i) & (sel < 0.01 * (i + 1)), sgn * v, x)
            x = np.where((sel >= 0.02) & (sel < 0.03), -0.0, x)
            ws, es = 2.0 ** -4, 2.0 ** -18
        p['x'] = x * 2.0 ** e
        dw = fc._randn(rng, (k * k, C)) / k * ts
        if family == 'dover':
            ws = 2.0 ** -4
            dw[rng.integers(0, k * k, C), np.arange(C)] = rng.choice([-1.0, 1.0], C) * rng.uniform(1.1, 1.6, C)
        p['dw'] = dw
        p['pw'] = fc._randn(rng, (Co, C)) / math.sqrt(C) * ws * 2.0 ** -e[:C]
        b = fc._randn(rng, (Co,)) * es
        if family == 'over':
            up, dn = over_channels(c)
            b[up], b[dn] = 3.0 * INF16, -3.0 * INF16
        p['b'] = b
        if hc:
            p['hw'] = fc._randn(rng, (hc, Co)) / math.sqrt(Co)
            p['hb'] = fc._randn(rng, (hc,))
    with np.errstate(over='raise'):
        return {n: np.ascontiguousarray(v, dtype=np.float16 if n == 'x' else np.float32) for n, v in p.items()}


def weights(c, p, dtype=np.float64):
    """the pointwise weights as the kernel holds them: (fp16(w), WS: fp16(w - fp16(w)), else zeros), as `dtype`"""
    w = np.asarray(p['pw'], np.float32)
    hi = w.astype(np.float16)
    lo = (w - hi.astype(np.float32)).astype(np.float16) if c['ws'] else np.zeros_like(hi)
    return hi.astype(dtype), lo.astype(dtype)


# ----------------------------------------------------------------------------
# the split
# ----------------------------------------------------------------------------
def rtz16(v):
    """fp32 -> fp16, round toward zero by IEEE's rule (overflow gives +-65504): the nearest fp16, stepped back where it is larger"""
    v = np.asarray(v, np.float32)
    with np.errstate(over='ignore'):
        t = v.astype(np.float16)
    t = np.where(np.isinf(t) & np.isfinite(v), np.copysign(np.float16(MAX16), t), t).astype(np.float16)
    back = np.abs(t.astype(np.float32)) > np.abs(v)
    return np.where(back, np.nextafter(t, np.float16(0.0)), t).astype(np.float16)


def split_rtz(d):
    """fp32 -> (hi, lo) fp16 as split_hi_lo computes them"""
    d = np.asarray(d, np.float32)
    hi = rtz16(d)
    return hi, rtz16(d - hi.astype(np.float32))


def u_pair(a):
    """how far hi + lo can be short of a value of magnitude a (module docstring)"""
    a = np.asarray(a, np.float64)
    e = np.floor(np.log2(np.maximum(a, 1e-300)))
    low = np.maximum(2.0 ** -21 * 2.0 ** e, 2.0 ** -24)
    high = 2.0 ** -10 * 2.0 ** np.floor(np.log2(np.maximum(a - MAX16, 32.0)))
    return np.minimum(np.where(a < 65536.0, low, high), a)


def lo_mag(a):
    """the largest |lo| of a value of magnitude a"""
    return np.where(a < 65536.0, 2.0 ** -10 * a, a - MAX16)


# ----------------------------------------------------------------------------
# reference and bounds
# ----------------------------------------------------------------------------
def depthwise64(c, p):
    """-> d, e_dw, e_dw^2 (rss): (M, C) float64"""
    kk = c['ks'] * c['ks']
    d, s1, s2 = depthwise(p['x'][..., :c['C']], p['dw'], c['ks'], np.float64)
    return d, kk * U * s1, kk * U * U * s2


@np.errstate(invalid='ignore', over='ignore')
def reference(c, p):
    """-> dict(ref, worst, rss, store16) per output element: (M, Cout), (M, head_c) in head mode.  worst / rss are the accumulated
    fp32 error E BEFORE the store; accept() adds the store's rounding"""
    d, e_dw, e_dw2 = depthwise64(c, p)
    wh, wl = weights(c, p)
    w, aw = wh + wl, np.abs(wh) + np.abs(wl)
    b = np.asarray(p['b'], np.float64)[None]
    K = c['C']
    steps, m = (K + 31) // 32, 3 if c['ws'] else 2
    a = np.abs(d) + e_dw
    lin = u_pair(a) @ np.abs(w).T + (lo_mag(a) @ np.abs(wl).T if c['ws'] else 0.0)
    A = np.abs(b) + a @ aw.T
    worst = e_dw @ np.abs(w).T + lin + (m * K + m * steps) * U * A
    rss = np.sqrt(e_dw2 @ (w * w).T + 2.0 ** -48 * (m * steps + 32) * (np.abs(b) + np.sqrt((a * a) @ (aw * aw).T)) ** 2) + lin
    head = (p['hw'], p['hb']) if c['head_c'] else None
    return fc._epilogue(d @ w.T + b, worst, rss, A, [], c['act'], not c['head_c'], head, wave_couts=c['Cout'] // NMW)


@functools.lru_cache(maxsize=None)
def case_reference(case_id, family, N=None):
    """(case, inputs, reference) of a listed case (N: with another batch size), computed once per process and not to be modified"""
    c = CASE[case_id] if N is None else dict(CASE[case_id], N=N)
    p = build(c, family)
    return c, p, reference(c, p)


# ----------------------------------------------------------------------------
# the kernel's arithmetic, emulated
# ----------------------------------------------------------------------------
def _flush(v):
    return np.where(np.abs(v) < MIN16, np.float32(0.0), v).astype(np.float32)


def emulate(c, p, variant=None):
    """the listed case as the kernel computes it -> (M, Cout) fp16, (M, head_c) fp32 in head mode"""
    C, Co = c['C'], c['Cout']
    dw = r16(p['dw']) if variant == 'taps16' else np.asarray(p['dw'], np.float32)
    d, _, _ = depthwise(np.asarray(p['x'][..., :C], np.float32), dw, c['ks'], np.float32)
    hi, lo = (v.astype(np.float32) for v in split_rtz(d))
    if variant == 'flush_pair':
        hi, lo = _flush(hi), _flush(lo)
    if variant == 'no_lo':
        lo = np.zeros_like(lo)
    wh, wl = weights(c, p, np.float32)
    b = np.asarray(p['b'], np.float32)[None]
    with np.errstate(invalid='ignore', over='ignore'):
        t = np.zeros((d.shape[0], Co), np.float32) + (np.float32(0.0) if variant == 'bias_last' else b)
        for i, k0 in enumerate(range(0, C, 32)):
            s = slice(k0, k0 + 32)
            t = t + hi[:, s] @ wh[:, s].T
            if not (variant == 'lo_every_second_kstep' and i % 2 == 0):
                t = t + lo[:, s] @ wh[:, s].T
            if c['ws'] and variant != 'ws_no_third':
                t = t + hi[:, s] @ wl[:, s].T
        if variant == 'bias_last':
            t = t + r16(b)
        if c['act'] == 1:
            t = np.maximum(t, np.float32(0.0))
        elif c['act'] == 2:
            t = (t / (np.float32(1.0) + np.exp(-t))).astype(np.float32)
        if c['head_c']:      # head_store: the head bias, then the four waves' shares in order
            hw = np.asarray(p['hw'], np.float32)
            v = np.broadcast_to(np.asarray(p['hb'], np.float32)[None], (t.shape[0], c['head_c']))
            for c0 in range(0, Co, Co // NMW):
                v = v + t[:, c0:c0 + Co // NMW] @ hw[:, c0:c0 + Co // NMW].T
            return v.astype(np.float32)
        o = r16(t)
        if variant == 'saturate_store':
            o = np.where(np.isinf(o), np.sign(o) * np.float32(MAX16), o)
    return o.astype(np.float16)


# ----------------------------------------------------------------------------
# the exact family
# ----------------------------------------------------------------------------
def exact_expected(c, p):
    """-> (float64 result (M, Cout | head_c), tolerance before the store, largest sum of |terms|).  Asserts what makes the
    expectation exact: integer operands, one tap per channel, every sum of magnitudes <= 2048 (the head's fp32 sum: 2^24).  The
    tolerance is 0 unless the case ends in SiLU: then SiLU's own rounding of the exact argument"""
    for n in ('x', 'dw', 'pw', 'b') + (('hw', 'hb') if c['head_c'] else ()):
        v = np.asarray(p[n], np.float64)
        assert np.array_equal(v, np.round(v)), n
    d, s1, _ = depthwise(p['x'][..., :c['C']], p['dw'], c['ks'], np.float64)
    assert s1.max() <= 2.0
    w = np.asarray(p['pw'], np.float64)
    b = np.asarray(p['b'], np.float64)[None]
    t = d @ w.T + b
    mag = float((np.abs(d) @ np.abs(w).T + np.abs(b)).max())
    assert mag <= EXACT_MAG, mag
    tol = np.zeros_like(t)
    if c['act'] == 1:
        t = np.maximum(t, 0.0)
    elif c['act'] == 2:
        arg, t = t, fc._silu(t)
        tol = (13.0 + np.abs(arg)) * U * np.abs(t) + 2.0 ** -126 + np.where(arg < -87.0, np.abs(t), 0.0)
    if c['head_c']:
        assert c['act'] == 1
        hw, hb = np.asarray(p['hw'], np.float64), np.asarray(p['hb'], np.float64)
        assert float((np.abs(t) @ np.abs(hw).T + np.abs(hb)[None]).max()) < 2.0 ** 24
        t = t @ hw.T + hb[None]
    return t, tol, mag


def exact_mismatches(c, got, want, tol):
    """number of elements that are not the exact result (behind SiLU: outside SiLU's own rounding and the one store)"""
    got = np.asarray(got, np.float64)
    if c['act'] == 2:
        return int((~(np.abs(got - want) <= tol + h(np.abs(want) + tol))).sum())
    return int((got != want).sum())


# ----------------------------------------------------------------------------
# the fp16 pair the kernel exists to beat: emp_dwconv_nhwc_f16 + emp_conv2d_nhwc_f16 on taps and weights rounded to fp16
# ----------------------------------------------------------------------------
def pair_case(c):
    """the case as f16_range_case's `sep` entry describes it (fp16 taps, the depthwise result rounded to fp16)"""
    return dict(fc.CASE['sep5_128'], id=c['id'], H=c['H'], W=c['W'], N=c['N'], Cin=c['C'], Cout=c['Cout'], k=c['ks'], act=c['act'], head_c=0)


@functools.lru_cache(maxsize=None)
def pair_advantage(case_id, family):
    """What the derived bounds say about `closer to y64 than the pair`, with no kernel run.  The pair computes on fp16(taps): its
    float64 reference differs from y64 by the KNOWN D = y64(taps16) - y64, and its output lies within B_pair (f16_range_case's
    bound at factor 6, store included) of that reference, so |pair - y64| >= |D| - B_pair per element; the precise kernel lies
    within B (this module's bound at factor 6, store included) of y64.  -> (rms of max(|D| - B_pair, 0), rms of B): the first
    above the second is the bounds implying a smaller rms error for the precise kernel."""
    c, p, r = case_reference(case_id, family)
    assert not c['head_c'] and not c['ws']
    q = dict(x=np.ascontiguousarray(p['x'][..., :c['C']]), dw=p['dw'].astype(np.float16), pw=p['pw'].astype(np.float16), b=p['b'])
    rp = fc.reference(pair_case(c), q)
    Ep, E = np.minimum(RSS_GPU * rp['rss'], rp['worst']), np.minimum(RSS_GPU * r['rss'], r['worst'])
    Bp, B = Ep + h(np.abs(rp['ref']) + Ep), E + h(np.abs(r['ref']) + E)
    low = np.maximum(np.abs(rp['ref'] - r['ref']) - Bp, 0.0)
    return float(np.sqrt((low ** 2).mean())), float(np.sqrt((B ** 2).mean()))
