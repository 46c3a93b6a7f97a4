"""Inputs, plain float64 references and derived error bounds of the glue-layer tests (tests/test_layers_case_host.py,
tests/test_gpu_layer_kernels.py): the non-GEMM kernels of csrc/layers.hip, the fused stem of csrc/stem.hip, their fp32 twins in
csrc/ref32.hip and avgpool_hl32 of csrc/conv16x3p.hip, each called through its own emp_op_* entry.  numpy / torch-CPU in float64;
no GPU.  The references are written from the operators' definitions (encoders/resnet.py conv1 + bn1 + relu + maxpool,
regnet.py stem, bifpn.py fast-normalised fusion, F.interpolate(align_corners=True), AdaptiveAvgPool2d(1), x * sigmoid(g));
test_layers_case_host.py holds them against torch's own operators in double.

Every tolerance is derived from the arithmetic the kernel is documented to perform, never from its output.
U = 2^-24 is the unit round-off of fp32 (one rounding of a value v costs at most U |v|), UH = 2^-11 that of fp16.

* storing fp16 (half_bound).  A value t = ref + e, |e| <= e32, rounded to nearest fp16 moves by at most half an ulp: UH |t| for a
  normal result, 2^-25 (half the subnormal step) below 2^-14:  e16 = e32 + UH (|ref| + e32) + 2^-25.
* exact operators: max-pool (both precisions), the nearest / max part of fuse_combine, a same-size resize (s = (h-1)/(h-1) = 1,
  f = ox, l = 0: 1 * (1 * v + 0 * v') + 0 * (..) = v), the operand gate_mul does not own, four-column against one-column
  resize, strip against plain depthwise: compared bit for bit.
* VALU stems (stem7x7, stem3x3s2; stem_valu_e32).  x = (raw - sub) * mul rounds twice (raw is an integer below 2^16: exact), so
  every product |w x| carries 2 U; the K = k*k taps are one fmaf chain (one rounding per tap, each of a partial sum bounded by
  S = sum |w||x| + |b|: K U S in any order); the bias add rounds once.  (K + 3) U S, asserted as (K + 4) U S for the
  second-order terms.  ReLU is 1-Lipschitz and keeps the bound.
* MFMA stems (stem_pool, both precisions; stem_mfma_e32).  Both operands leave as fp16 hi + lo: hi = fp16(v) is off by at most
  UH |v|, lo = fp16(v - hi) by UH of that -- 2^-22 |v| -- or by 2^-25 where v - hi is an fp16 subnormal (every lo part of the
  taps, |w| ~ 1/7, is).  The product w x is replaced by wh xh + wh xl + wl xh: what is missing is wl xl (<= 2^-22 |w||x|) and
  the two residues (<= (2^-22 |w| + 2^-25) |x| and the same with w and x swapped): 3 * 2^-22 |w||x| + 2^-25 (|w| + |x|) per tap
  -- the "~2^-21" of stem.hip.  The fp16 x fp16 products are exact in fp32; they are summed in fp32 in an order the matrix pipe
  does not document: 2 tap groups x 3 products x 32 addends = 192 addends, so at most 192 roundings of partial sums bounded by
  S on any path (the worst case of a chain; a tree has fewer).  With the normalisation (2 U) and the bias (U), and one more for the
  second-order terms:  (196 U + 3 * 2^-22) S + 2^-25 T,  T = sum over the taps of |w| + |x|.
  The fp16 kernel rounds the conv tile to fp16 before the pool (rounding is monotone: the max of the rounded values is the
  rounded max); |max a_i - max b_i| <= max |a_i - b_i|, so a pooled output is bounded by the largest bound in its window.
* fuse_combine (fuse_e32).  The resized operand is exact.  v = ca ra + cb b (+ cc c): the first product passes through its own
  rounding and two sums, the others through fewer: 3 U A, A = |ca ra| + |cb b| + |cc c|; asserted as 4 U A (second order).
  The hi / lo pair: hi = fp16(v) exactly, so hi is within half_bound of the reference and |lo| is at most half an ulp of hi
  (pair_inconsistent; fp16(hi + lo) == hi itself cannot be asked: lo is rounded too, and where that lands hi + lo on the
  midpoint of two fp16 values the tie may break the other way); v - hi is exact in fp32 and lo = fp16(v - hi) is off by UH |v - hi| <= 2^-22 |v|, or 2^-25 below the fp16
  subnormal floor:  e_pair = e32 + 2^-22 (|ref| + e32) + 2^-25.
* bilinear, align_corners=True (bilinear_e32).  s = (h-1)/(H-1) and f = s * o round once each: the source coordinate is off by
  at most 2 U f (f <= h - 1 < 2^22, so floor(f) never leaves the map).  l = f - floor(f) is exact.  The interpolant is
  continuous and piecewise linear in each coordinate with slope at most 2 M, M = max|map| (so landing on the other side of an
  integer changes nothing beyond this): 4 U (fy + fx) M from the two coordinates.  The weights 1 - l round once (half an ulp of
  a value <= 1: U / 2 each, U M over the four corners); on every path from a corner to the result there are four roundings
  (product, inner sum, outer product, outer sum; an fma only removes one), each of a convex combination bounded by M: 4 U M.
      e32 = (4 (fy + fx) + 5) U M, asserted with 6 for the second-order terms; it grows with the source side as f does.
* average pool (avgpool_depth).  A sum of fp32 terms: every rounding on the path of a term is of a partial sum bounded by
  sum |x|, so the error is at most depth * U * sum|x| / HW, depth = the longest chain of additions in the kernel's fixed order
  (+ the final scaling).  fp16 kernel: 16 segments of per = ceil(HW / 16) pixels, 8 pixel lanes each summing ceil(per / 8) terms,
  the 8 lanes in a chain, the 16 segments in a chain, inv = 1 / HW (one rounding) and the product: ceil(per / 8) + 8 + 16 + 2.
  fp32 kernel: 16 waves x 4 partial sums of ceil(HW / 64) terms (+ up to 3 of the remainder loop), a pair tree (2), a chain of 16
  and the division: ceil(HW / 64) + 3 + 2 + 16 + 1.  hl32 kernel: hi + lo (1), ceil(HW / 64) terms per partial sum, the pair
  tree (2), a four-level tree over the waves and the division: 1 + ceil(HW / 64) + 2 + 4 + 1 -- against the mean of the fp32 map
  the hl32 map was made from, which the split reproduces to 2^-22 |x| + 2^-25 per element.
* gemv (gemv_depth).  A lane chains ceil(K / 64) fmaf, six butterfly additions join the lanes, the bias add rounds once:
  (ceil(K / 64) + 7) U (sum |x||w| + |b|).
* gate (gate_e32).  x / (1 + exp(-g)) in fp32: exp within 2 ulp (4 U relative; it enters 1 / (1 + e) damped by e / (1 + e) < 1),
  the sum 1 + e (U), the division within 2.5 ulp (5 U), the product (U): 11 U |ref|, asserted as 12 U |ref|, + 2^-126 where the
  result is an fp32 subnormal that may be flushed.  exp(-90) = 0 and exp(-30) < U make the gate exactly x; exp(90) = inf makes it
  exactly 0: asserted as equalities.
* depthwise fp32 (dw_e32): one fmaf chain of K*K taps from 0: K*K U sum |w||x|.
* the fp32 mode's convolution (conv32_ref_bound; csrc/ref32.hip conv32_kernel).  Both operands are fp32 and enter the exact fp32
  matrix pipe as they are: no operand error.  v_mfma_f32_32x32x2_f32 is an fmaf chain per output: K = KH KW Cin16 steps (the
  padding's products are exact zeros), every step rounding a partial sum bounded by S = |x| . |w|, so on any path a term passes
  at most K roundings:  worst = K U S.  Taken independent in sign, K roundings each of a partial sum whose size is the root sum
  square of the terms:  rss = U sqrt(K) sqrt(x^2 . w^2).  The epilogue is x3_range_case's, the same code: bias, per-image bias
  and residual one addition each, U (S + |b| + |b_n| + |r| + error so far) each; ReLU keeps the bound; SiLU is
  t / (1 + __expf(-t)): 1.1 times the error before it plus (13 + |t|) U |silu(t)| + 2^-126.  A head's partial sums in ascending
  order and its bias (head_finish_bound): tiles + 1 additions, (tiles + 1) U (sum |part| + |b|).
  A correct kernel never exceeds `worst`; test_graph32_case_host.py holds a float32 evaluation of the same sums, in ascending
  and in a shuffled order, to 3 of `rss` (x3_range_case.RSS_HOST) and the GPU tests accept min(worst, 6 rss) (RSS_GPU) --
  the factors of the fp16x3 bounds, not refitted.
  (head1x1 on the fp32 graph is pointrend_case.predictor_ref's bound: a K-term fp32 dot product in any order and the bias add.)
"""
import numpy as np

import x3_range_case as x3

U = 2.0 ** -24
UH = 2.0 ** -11
SUB16 = 2.0 ** -25           # half the step of the fp16 subnormals
TINY32 = 2.0 ** -126         # the smallest normal fp32
GUARD = 64                   # sentinel elements behind every output buffer
F16, F32, HL32 = 0, 1, 2     # emp_op_prec
IMG_F32, IMG_U8, IMG_U16 = 0, 1, 2
F32_SENTINEL, F16_SENTINEL = 12345.0, 777.0

NP_OF = {F16: np.float16, F32: np.float32}


def half_bound(ref, e32):
    return e32 + UH * (np.abs(ref) + e32) + SUB16


def violations(got, ref, bound):
    """number of values that are not within the bound (a NaN counts)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    return int((~(err <= bound)).sum())


def worst_ratio(got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    if np.isnan(err).any():
        return float('inf')
    return float((err / np.maximum(bound, 1e-300)).max())


# ----------------------------------------------------------------------------
# max-pool 3x3 / 2, pad 1 with -inf  (also the 'down' resize of the fusion and the stem's pool)
# ----------------------------------------------------------------------------
def maxpool_ref(x, pad=-np.inf):
    """(N,H,W,C) -> (N,H/2,W/2,C), H, W even; in x's dtype (a max is exact)"""
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    xp = np.full((N, H + 2, W + 2, C), pad, dtype=x.dtype)
    xp[:, 1:-1, 1:-1] = x
    out = np.full((N, Ho, Wo, C), -np.inf, dtype=x.dtype)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, xp[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2])
    return out


MAXPOOL_HW = [(2, 2), (6, 10), (34, 18)]
MAXPOOL_C = {F16: [8, 24, 64], F32: [4, 12, 8, 24, 64]}
MAXPOOL_N = 3


def signed_map(shape, prec, seed, negative=False):
    """O(1) signed values in the kernel's storage type; negative: every value below zero (a pad of 0 would win every window)"""
    x = np.random.default_rng(seed).standard_normal(shape)
    if negative:
        x = -np.abs(x) - 0.25
    return x.astype(NP_OF[prec])


# ----------------------------------------------------------------------------
# stems
# ----------------------------------------------------------------------------
# (H, W, vh, vw): padded and valid size
STEM_POOL_SHAPES = [(16, 16, 16, 16), (48, 80, 48, 80), (36, 68, 36, 68), (48, 64, 37, 50), (36, 68, 33, 65), (16, 16, 15, 16)]
STEM7_SHAPES = [(2, 2, 2, 2), (34, 66, 34, 66), (48, 80, 48, 80), (34, 66, 29, 66), (48, 80, 48, 79)]
STEM3_SHAPES = [(2, 2, 2, 2), (6, 10, 6, 10), (34, 18, 34, 18), (34, 18, 33, 18), (6, 10, 6, 9)]
STEM3_C = [8, 32, 40]
STEM_DTYPES = [IMG_U8, IMG_U16, IMG_F32]
STEM_N = 2
NORMALISE = {IMG_U8: (np.float32(127.3), np.float32(1 / 58.4)), IMG_U16: (np.float32(32000.7), np.float32(1 / 15000.3)),
             IMG_F32: (np.float32(0.37), np.float32(1.7))}      # float input is NOT normalised: sub / mul must be ignored


def stem_image(dtype, N, vh, vw, seed):
    rng = np.random.default_rng(seed)
    if dtype == IMG_U8:
        return rng.integers(0, 256, (N, vh, vw)).astype(np.uint8)
    if dtype == IMG_U16:
        return rng.integers(0, 65536, (N, vh, vw)).astype(np.uint16)
    return rng.standard_normal((N, vh, vw)).astype(np.float32)


def stem_weights(k, C, seed):
    """taps (k*k, C) ~ N(0, 1) / k, biases with every third one below -0.5 so that ReLU clamps there"""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((k * k, C)) / k).astype(np.float32)
    b = (0.5 * rng.standard_normal(C)).astype(np.float32)
    b[::3] = -np.abs(b[::3]) - 0.5
    return w, b


def normalise(img, dtype):
    x = img.astype(np.float64)
    if dtype == IMG_F32:
        return x
    sub, mul = NORMALISE[dtype]
    return (x - float(sub)) * float(mul)


def conv_s2(x, w, k):
    """(N,H,W) float64, taps (k*k, C) -> (N,H/2,W/2,C): stride 2, zero padding k // 2"""
    p = k // 2
    N, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    xp = np.pad(x, ((0, 0), (p, p), (p, p)))
    out = np.zeros((N, Ho, Wo, w.shape[1]))
    for ky in range(k):
        for kx in range(k):
            out += xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2, None] * w[ky * k + kx]
    return out


def stem_ref(img, dtype, H, W, w, b, k):
    """conv (k x k, stride 2, pad k // 2) + bias + ReLU of the image normalised, THEN zero-padded to H x W.  Returns the
    reference, S = sum |w||x| + |b| and T = sum over the taps of |w| + |x| (the bounds' ingredients), all (N,H/2,W/2,C)."""
    N, vh, vw = img.shape
    x = np.zeros((N, H, W))
    x[:, :vh, :vw] = normalise(img, dtype)
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    ref = np.maximum(conv_s2(x, w64, k) + b64, 0.0)
    S = conv_s2(np.abs(x), np.abs(w64), k) + np.abs(b64)
    T = conv_s2(np.abs(x), np.ones_like(w64), k) + np.abs(w64).sum(0)
    return ref, S, T


def stem_valu_e32(S, k):
    return (k * k + 4) * U * S


def stem_mfma_e32(S, T):
    return (196 * U + 3 * 2.0 ** -22) * S + 2.0 ** -25 * T


def stem_conv_bound(ref, S, T, k, prec, mfma):
    e = stem_mfma_e32(S, T) if mfma else stem_valu_e32(S, k)
    return half_bound(ref, e) if prec == F16 else e


def stem_pool_ref_bound(ref, S, T, prec):
    """the fused stem: max-pool of the conv reference; bound = the largest conv bound in the window"""
    return maxpool_ref(ref), maxpool_ref(stem_conv_bound(ref, S, T, 7, prec, True), pad=0.0)


# ----------------------------------------------------------------------------
# fuse_combine
# ----------------------------------------------------------------------------
FUSE_OUT_HW = {0: [(2, 2), (4, 6), (18, 34)], 1: [(1, 1), (3, 5), (17, 9)]}
FUSE_C = [8, 40]
FUSE_N = 2


def fuse_inputs(mode, H, W, C, prec, seed, negative_a=False):
    ah, aw = (H // 2, W // 2) if mode == 0 else (2 * H, 2 * W)
    a = signed_map((FUSE_N, ah, aw, C), prec, seed, negative=negative_a)
    b = signed_map((FUSE_N, H, W, C), prec, seed + 1)
    c = signed_map((FUSE_N, H, W, C), prec, seed + 2)
    wts = np.random.default_rng(seed + 3).uniform(0.2, 1.0, 3)
    coef = (wts / (wts.sum() + 1e-4)).astype(np.float32)      # fast-normalised fusion: positive, summing to just under 1
    return a, b, c, coef


def fuse_resize(a, mode):
    """mode 0: nearest x2 of a; mode 1: 3x3 / 2 max-pool of a.  Exact, in a's dtype."""
    if mode == 0:
        return a.repeat(2, axis=1).repeat(2, axis=2)
    return maxpool_ref(a)


def fuse_ref(a, b, c, coef, mode):
    """-> (reference, A = sum of the absolute terms), float64; c may be None"""
    ra = fuse_resize(a, mode).astype(np.float64)
    terms = [float(coef[0]) * ra, float(coef[1]) * b.astype(np.float64)]
    if c is not None:
        terms.append(float(coef[2]) * c.astype(np.float64))
    return sum(terms), sum(np.abs(t) for t in terms)


def fuse_e32(A):
    return 4 * U * A


def pair_inconsistent(hi, lo):
    """number of pairs whose lo part is more than half an ulp of hi: hi would not be the fp16 rounding of hi + lo"""
    return int((np.abs(lo.astype(np.float64)) > 0.5 * np.spacing(np.abs(hi)).astype(np.float64)).sum())


def fuse_pair_bound(ref, A):
    e = fuse_e32(A)
    return e + 2.0 ** -22 * (np.abs(ref) + e) + SUB16


# ----------------------------------------------------------------------------
# bilinear, align_corners=True
# ----------------------------------------------------------------------------
def _axis(n_in, n_out):
    f = np.arange(n_out) * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    i0 = np.minimum(np.floor(f).astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), f - i0


def bilinear_ref(x, H, W):
    """(N,h,w,C) -> (N,H,W,C), float64: output (oy, ox) samples the source at (oy (h-1)/(H-1), ox (w-1)/(W-1)) -- the corners of
    the two maps coincide -- bilinearly between the four neighbours, the upper one clamped to the map (scale 0 when H or W is 1)"""
    x64 = np.asarray(x, np.float64)
    y0, y1, ly = _axis(x.shape[1], H)
    x0, x1, lx = _axis(x.shape[2], W)
    lx, ly = lx[None, None, :, None], ly[None, :, None, None]
    top = x64[:, y0][:, :, x0] * (1 - lx) + x64[:, y0][:, :, x1] * lx
    bot = x64[:, y1][:, :, x0] * (1 - lx) + x64[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def bilinear_e32(x, H, W):
    """(H, W, 1) array: (4 (fy + fx) + 6) U M"""
    h, w = x.shape[1:3]
    M = float(np.abs(x.astype(np.float64)).max())
    fy = np.arange(H) * ((h - 1) / (H - 1) if H > 1 else 0.0)
    fx = np.arange(W) * ((w - 1) / (W - 1) if W > 1 else 0.0)
    return ((4 * (fy[:, None] + fx[None, :]) + 6) * U * M)[:, :, None]


def bilinear_bound(x, ref, H, W, prec):
    e = bilinear_e32(x, H, W)
    return half_bound(ref, e) if prec == F16 else e + 0 * ref


def bilinear_sweep():
    """(h, w, H, W): source side 1..9 x output side 1..33 in rows with a fixed column ratio (3 -> 7), the same in columns with a
    fixed row ratio, and the nine square identities: down-scaling, H = 1 and W = 1 (scale 0), h = 1 and identity are all in it"""
    rows = [(s, 3, o, 7) for s in range(1, 10) for o in range(1, 34)]
    cols = [(3, s, 7, o) for s in range(1, 10) for o in range(1, 34)]
    return rows + cols + [(s, s, s, s) for s in range(1, 10)]


# the four-pixel kernels at their smallest reachable shapes: (C, h, w, H, W)
# C = 64 has 32 four-pixel groups per block iteration, so the kernel needs W >= 128: 4 x 32 -> 16 x 128 is its smallest shape; the
# transposed 32 x 4 -> 128 x 16 does not meet W >= 4 ppb and goes to the one-pixel kernel (BILINEAR_UP4_REFUSED)
BILINEAR_UP4_F16 = [(2048, 2, 2, 8, 8), (256, 8, 8, 32, 32), (256, 8, 8, 32, 36), (64, 4, 32, 16, 128)]
BILINEAR_X4_F32 = [(4, 2, 2, 8, 8), (12, 5, 7, 17, 28)]
BILINEAR_UP4_REFUSED = [(8, 2, 2, 8, 8), (64, 32, 4, 128, 16), (256, 8, 8, 32, 34), (256, 16, 16, 32, 32)]      # W < 4 ppb (twice); W % 4; 3 sx >= 1
BILINEAR_IDLE = [(48, 5, 11, 7, 43), (48, 5, 30, 7, 100)]      # 256 % (C / 8) != 0: 42 pixels per block iteration, 4 idle threads
BILINEAR_SAME = (16, 7, 5, 7, 5)
BILINEAR_NCHW = [(scale, hw, nc) for scale in (4, 2) for hw in ((1, 1), (3, 5), (16, 16)) for nc in (1, 3, 6)]
BILINEAR_N = 2


def up4_preconditions(C, w, W):
    """the dispatcher's rule for the four-pixel fp16 kernel, in the launcher's own fp32 arithmetic"""
    ppb = 256 // (C // 8)
    sx = np.float32(w - 1) / np.float32(W - 1) if W > 1 else np.float32(0)
    return W % 4 == 0 and bool(np.float32(3) * sx < np.float32(1)) and W >= 4 * ppb


def slice_buffer(x, ld, prec, seed, guard_rows, guard_fill=np.inf):
    """x (..., C) placed in the first C channels of rows `ld` wide; the other channels carry finite noise, and guard_rows rows of
    guard_fill follow the last one: an index that runs off the end of the map reads them.  -> (rows + guard_rows, ld)"""
    C = x.shape[-1]
    rows = x.reshape(-1, C)
    buf = np.random.default_rng(seed).standard_normal((rows.shape[0] + guard_rows, ld)).astype(x.dtype)
    buf[:rows.shape[0], :C] = rows
    buf[rows.shape[0]:] = guard_fill
    return buf


# ----------------------------------------------------------------------------
# global average pool
# ----------------------------------------------------------------------------
AVG_HW = {F16: [1, 4, 15, 16, 17, 100, 257], F32: [1, 15, 16, 17, 63, 64, 65, 113], HL32: [1, 15, 16, 17, 63, 64, 65, 113]}
AVG_C = {F16: [8, 264, 512], F32: [4, 72, 128], HL32: [32, 96]}
AVG_PAD = {F16: 8, F32: 4, HL32: 32}      # in_ld = C + pad
AVG_N = 2


def avg_input(N, HW, C, prec, seed):
    """(N, HW, C) with mean 1.5: a dropped pixel or a wrong divisor is far outside the bound"""
    x = 1.5 + np.random.default_rng(seed).standard_normal((N, HW, C))
    return x.astype(np.float16 if prec == F16 else np.float32)


def avgpool_depth(HW, prec):
    if prec == F16:
        per = -(-HW // 16)
        return -(-per // 8) + 8 + 16 + 2
    if prec == F32:
        return -(-HW // 64) + 3 + 2 + 16 + 1
    return 1 + -(-HW // 64) + 2 + 4 + 1


def avgpool_ref_bound(x, prec):
    x64 = x.astype(np.float64)
    ref, mean_abs = x64.mean(1), np.abs(x64).mean(1)
    bound = avgpool_depth(x.shape[1], prec) * U * mean_abs
    if prec == HL32:
        bound = bound + 2.0 ** -22 * mean_abs + SUB16
    return ref, bound


# ----------------------------------------------------------------------------
# gemv
# ----------------------------------------------------------------------------
GEMV_K = [1, 63, 64, 65, 2048]
GEMV_NC = [(1, 1), (1, 5), (3, 7), (2, 256)]


def gemv_inputs(N, K, Cout, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, K)).astype(np.float32)
    w = (rng.standard_normal((Cout, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    return x, w, b


def gemv_ref_bound(x, w, b, relu):
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    ref, S = x64 @ w64.T, np.abs(x64) @ np.abs(w64).T
    if b is not None:
        ref, S = ref + b.astype(np.float64), S + np.abs(b.astype(np.float64))
    if relu:
        ref = np.maximum(ref, 0.0)
    return ref, (-(-x.shape[1] // 64) + 7) * U * S


# ----------------------------------------------------------------------------
# gate
# ----------------------------------------------------------------------------
GATE_ROWS = [1, 33, 1000]
GATE_C = {F16: [8, 40], F32: [4, 12]}
GATE_EXTREMES = (30.0, -30.0, 90.0, -90.0)


def gate_inputs(rows, C, prec, seed):
    """x, g (rows, C); the first four elements of g are +-30 and +-90 (x there is +-1.25: away from zero)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, C))
    g = 3.0 * rng.standard_normal((rows, C))
    g.reshape(-1)[:4] = GATE_EXTREMES
    x.reshape(-1)[:4] = (1.25, -1.25, -1.25, 1.25)
    return x.astype(NP_OF[prec]), g.astype(NP_OF[prec])


def gate_ref_bound(x, g, prec):
    ref = x.astype(np.float64) / (1.0 + np.exp(-g.astype(np.float64)))
    e = 12 * U * np.abs(ref) + TINY32
    return ref, (half_bound(ref, e) if prec == F16 else e)


# ----------------------------------------------------------------------------
# depthwise fp32
# ----------------------------------------------------------------------------
DW32_CASES = [(5, 6, 16, 8), (5, 6, 13, 8), (3, 5, 8, 12), (3, 5, 9, 4)]      # (K, H, W, C): W % 8 == 0 reaches the strip kernel
DW32_N = 2


def dw_ref_bound(x, w, K):
    """x (N,H,W,C), taps (K*K, C): stride 1, zero padding K // 2"""
    P = K // 2
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    N, H, W, C = x.shape

    def conv(xx, ww):
        xp = np.pad(xx, ((0, 0), (P, P), (P, P), (0, 0)))
        out = np.zeros_like(xx)
        for ky in range(K):
            for kx in range(K):
                out += xp[:, ky:ky + H, kx:kx + W] * ww[ky * K + kx]
        return out
    return conv(x64, w64), K * K * U * conv(np.abs(x64), np.abs(w64))


# ----------------------------------------------------------------------------
# the fp32 mode's convolution (conv32_kernel) and the fused head's finish
# ----------------------------------------------------------------------------
def conv32_ref_bound(c, p):
    """A case dict and operands in x3_range_case's layouts (x3_range_case._c / build: x (N,H,W,C), w (Cout, k*k, Cin) tap-major,
    b, bn, r; groups as there) -> dict(ref, worst, rss), (M, Cout) float64: the module docstring's bound of conv32_kernel"""
    refs, worsts, rsss, Ss = [], [], [], []
    for X, Wm, _, _ in x3.gemm_blocks(c, p):
        K = X.shape[1]
        S = np.abs(X) @ np.abs(Wm).T
        refs.append(X @ Wm.T)
        worsts.append(K * U * S)
        rsss.append(U * np.sqrt(K) * np.sqrt((X * X) @ (Wm * Wm).T))
        Ss.append(S)
    t = np.concatenate(refs, 1) + np.asarray(p['b'], np.float64)[None]
    worst, rss, A = np.concatenate(worsts, 1), np.concatenate(rsss, 1), np.concatenate(Ss, 1) + np.abs(p['b'])[None]
    n_ep = 1
    for name, on in (('bn', c['bias_n']), ('r', bool(c['res']))):
        if on:
            v = x3._rows(c, p, name)
            t, A, n_ep = t + v, A + np.abs(v), n_ep + 1
    ep = n_ep * U * (A + worst)
    worst, rss = worst + ep, rss + ep
    if c['act'] == 1:
        out = np.maximum(t, 0.0)
    elif c['act'] == 2:
        with np.errstate(over='ignore'):
            out = x3._silu(t)
        ea = (13.0 + np.abs(t)) * U * np.abs(out) + TINY32 + np.where(t < -87.0, np.abs(out), 0.0)
        worst, rss = x3.SILU_LIP * worst + ea, x3.SILU_LIP * rss + ea
    else:
        out = t
    return dict(ref=out, worst=worst, rss=rss)


def conv32_emulate(c, p, order=None, rows=None, cols=None):
    """the same sums in float32, one rounding per term in the K order `order` (a permutation of K; None: ascending, the
    kernel's), then the fp32 epilogue -> float32, (M, Cout) or its sub-matrix rows x cols (index arrays).  fp32 x fp32 is exact
    in float64, so the float64 product rounded once with the running sum is an fmaf.  One group only."""
    (X, Wm, _, _), = x3.gemm_blocks(c, p)
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows)
    cols = np.arange(Wm.shape[0]) if cols is None else np.asarray(cols)
    X, Wm = X[rows], Wm[cols]
    acc = np.zeros((len(rows), len(cols)), np.float32)
    for k in (range(X.shape[1]) if order is None else order):
        acc = (acc.astype(np.float64) + X[:, k:k + 1] * Wm[None, :, k]).astype(np.float32)
    t = acc + np.asarray(p['b'], np.float32)[None, cols]
    if c['bias_n']:
        t = t + x3._rows(c, p, 'bn').astype(np.float32)[np.ix_(rows, cols)]
    if c['res']:
        t = t + x3._rows(c, p, 'r').astype(np.float32)[np.ix_(rows, cols)]
    if c['act'] == 1:
        t = np.maximum(t, np.float32(0.0))
    elif c['act'] == 2:
        with np.errstate(over='ignore'):
            t = (t / (np.float32(1.0) + np.exp(-t))).astype(np.float32)
    return t.astype(np.float32)


def head_finish_ref_bound(part, b):
    """part (tiles, M, C) as the kernel reads it, b (C) -> (reference (M, C), bound): tiles additions from the bias"""
    part, b = np.asarray(part, np.float64), np.asarray(b, np.float64)
    return part.sum(0) + b[None], (part.shape[0] + 1) * U * (np.abs(part).sum(0) + np.abs(b)[None])
