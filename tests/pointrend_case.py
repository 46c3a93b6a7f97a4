"""Inputs and plain references of the PointRend kernels' tests (tests/test_pointrend_case_host.py,
tests/test_gpu_pointrend_kernels.py): csrc/pointrend.hip, its fp32 twins in csrc/ref32.hip and the predictor of csrc/layers.hip,
each called through its own C-ABI entry.  numpy / torch-CPU in float64; no GPU.  Written from the semantics of
oracle/pdl_model.py (calculate_uncertainty, uncertain_points_on_grid, point_sample, point_head_forward), which
test_pointrend_case_host.py holds these references against on tie-free inputs.

Every tolerance below is derived from the arithmetic the kernel is documented to perform, never from its output.
U = 2^-24 is the unit round-off of fp32 (one rounding of a value v costs at most U |v|), UH = 2^-11 that of fp16.

* up-sampling (upsample_bound).  The x2 bilinear weights are 0, 0.25, 0.75 or 1: exact.  An output is
  hy (hx a + lx b) + ly (hx c + lx d): every input passes through at most five roundings (product, inner sum, outer product,
  outer sum, and one more where a product and a sum are not contracted into an fma), each of a term bounded by max|in| because
  the weights are convex.  Five roundings: 5 U max|in|; asserted as 8 U max|in|.
* keys.  Recomputed in np.float32 from the kernel's own up-sampled output they must be bit-equal: |v| is exact and top1 - top2 is
  one fp32 subtraction of two of the stored values.
* selection.  Integer: exact.
* point sampling (sample_bound).  The cell centre is computed in fp32 as point_rend.py:131-135 does; the kernel may contract
  step * i + 0.5 step into an fma, which moves the coordinate by at most two roundings of a value below 1: U.  Then
  g = 2c - 1 (error 2U carried, + U/2), g + 1 (+ U), times the map size S = fw or fh (carried error times S, + one rounding of
  a value <= 2S: 2SU), minus 1 (+ 2SU), halved (exact): the sample position is off by at most
  0.5 (S (2 + 0.5 + 1) + 2S + 2S) U < 4 S U.  The bilinear interpolant with zero padding is continuous in the position (so a
  floor() that lands on the other side of an integer changes nothing beyond this) with slope at most 2 M per axis, M = max|map|:
  16 max(fh, fw) U M from the two coordinates.  The weights: 1 - l (U/2) and a product (U/2 relative) each, four of them: at most
  6 U M; the four-term fmaf chain rounds four partial sums bounded by M: 4 U M.
      e32 = (16 max(fh, fw) + 10) U M.
  The f16 kernel then rounds once to fp16: UH (|ref| + e32) for a normal result, half the subnormal step (2^-25) below 2^-14;
  asserted with the whole step, 2^-24:
      e16 = e32 + UH (|ref| + e32) + 2^-24.
* predictor (predictor_ref).  A dot product of K terms accumulated in fp32 in any order is within K U sum|x||w| of the exact one
  (fma or not, tree or chain); the bias add rounds once more: U (|ref| + K U sum|x||w|).
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
UH = 2.0 ** -11
CHUNK = 2048                 # keys per workgroup of the select / compact passes (pointrend.hip)
SCAN_ROUND = 256             # chunks per round of compact_scan_kernel
GRID_CAP = 4096 * 256        # threads of the capped grid of upsample2x_keys_kernel
TILE = 256                   # points per tile of the fused point head
HEAD_GRID = 256              # workgroups of the fused point head: more tiles than this and its tile loop runs twice
KEY_MAX = 0x7f800000         # +inf: the largest key the select is specified for
GUARD = 64                   # sentinel elements behind every output buffer


# ----------------------------------------------------------------------------
# A. up-sampling and keys
# ----------------------------------------------------------------------------
UPSAMPLE_SHAPES = [(2, 1, 1, 1), (1, 1, 1, 9), (2, 1, 5, 7), (1, 2, 5, 7), (2, 4, 6, 10), (1, 8, 3, 3), (1, 1, 16, 16),
                   (1, 1, 520, 520)]
UPSAMPLE_KINDS = ('gauss', 'tied', 'const')


def upsample_input(kind, shape, seed=0):
    """(N, C, h, w) float32 logits.  'gauss': 4 * N(0, 1).  'tied': class 1 repeats class 0 over the left half of the map (the
    whole map when it is one column wide) and the pair is lifted above every other class there, so that the two largest logits
    of an up-sampled cell are exactly equal; class C-1 repeats class C-2 on the right half without being lifted; with one
    class the left half is zero.  'const': one value per class."""
    N, C, h, w = shape
    rng = np.random.default_rng(seed)
    x = (4.0 * rng.standard_normal(shape)).astype(np.float32)
    if kind == 'tied':
        half = max(1, w // 2)
        if C > 1:
            x[:, 0, :, :half] = np.abs(x[:, 0, :, :half]) + 20.0
            x[:, 1, :, :half] = x[:, 0, :, :half]
            if C > 2:
                x[:, C - 1, :, half:] = x[:, C - 2, :, half:]
        else:
            x[:, 0, :, :half] = 0.0      # one class: a region of zero logits, whose key must be +0
    elif kind == 'const':
        x[:] = (1.5 - 0.25 * np.arange(C, dtype=np.float32))[None, :, None, None]
    return x


def upsample_ref(x):
    """F.interpolate(scale_factor=2, bilinear, align_corners=False) in float64."""
    return F.interpolate(torch.from_numpy(np.asarray(x)).double(), scale_factor=2, mode='bilinear', align_corners=False).numpy()


def upsample_bound(x):
    return 8.0 * U * float(np.abs(x).max())


def keys_ref(v):
    """(N, C, H, W) -> (N, H*W) in v's own dtype: |v0| for one class, top1 - top2 otherwise (the negated uncertainty of
    point_rend.py:11-31: the smaller the key, the less certain the cell)."""
    v = np.asarray(v)
    N, C = v.shape[:2]
    if C == 1:
        return np.abs(v[:, 0]).reshape(N, -1)
    s = np.sort(v, axis=1)
    return (s[:, -1] - s[:, -2]).reshape(N, -1)


# ----------------------------------------------------------------------------
# B. selection
# ----------------------------------------------------------------------------
TOPK_PLANES = [1, 7, 100, 2048, 2049, 4099, 16384, 530437]
TOPK_DISTS = ('all_equal', 'all_zero', 'two_valued', 'random', 'byte0', 'byte1', 'byte2', 'byte3', 'straddle', 'with_inf')
BYTE_BASE = 0x3A4B5C6D
STRADDLE_T = np.float32(1.5).view(np.uint32)
STRADDLE_TAKEN = 140         # tied keys the straddle case's cutting k takes


def straddle_positions(plane):
    """the tied group of the 'straddle' keys: 336 cells across the boundary of chunks 0 | 1 and 11 across that of chunks 1 | 2"""
    assert plane >= 2 * CHUNK + 3
    return np.concatenate([np.arange(CHUNK - 40, CHUNK + 296), np.arange(2 * CHUNK - 8, 2 * CHUNK + 3)])


def topk_dists(plane):
    if plane == 1:
        return ('all_equal', 'all_zero', 'random')
    return tuple(d for d in TOPK_DISTS if d != 'straddle' or plane >= 2 * CHUNK + 3)


def topk_keys(dist, plane, seed=0):
    """(plane,) uint32 keys, all <= KEY_MAX (fp32 bit patterns of non-negative values)."""
    rng = np.random.default_rng([seed, plane, TOPK_DISTS.index(dist)])
    if dist == 'all_equal':
        return np.full(plane, np.float32(1.0).view(np.uint32), np.uint32)
    if dist == 'all_zero':
        return np.zeros(plane, np.uint32)
    if dist == 'two_valued':
        return np.where(rng.random(plane) < 0.4, np.float32(0.25).view(np.uint32), np.float32(3.0).view(np.uint32)).astype(np.uint32)
    if dist == 'random':
        return np.abs(4.0 * rng.standard_normal(plane)).astype(np.float32).view(np.uint32)
    if dist.startswith('byte'):
        b = int(dist[4])
        v = rng.integers(0, 0x7f if b == 3 else 0x100, plane).astype(np.uint32)      # byte 3 stays below 0x7f: finite
        return ((BYTE_BASE & ~(0xff << (8 * b))) | (v << np.uint32(8 * b))).astype(np.uint32)
    if dist == 'straddle':
        keys = (2.0 + rng.random(plane)).astype(np.float32)                          # [2, 3): above the tied value
        small = rng.choice(plane, size=plane // 16, replace=False)
        keys[small] = rng.random(len(small)).astype(np.float32)                      # [0, 1): below it
        keys[straddle_positions(plane)] = np.float32(1.5)
        return keys.view(np.uint32)
    if dist == 'with_inf':
        keys = np.abs(4.0 * rng.standard_normal(plane)).astype(np.float32)
        keys[rng.choice(plane, size=max(2, plane // 8), replace=False)] = np.inf
        return keys.view(np.uint32)
    raise ValueError(dist)


def tie_cut(dist, keys):
    """a k that takes some but not all of a group of equal keys, or None"""
    plane = len(keys)
    if dist == 'straddle':
        return int((keys < STRADDLE_T).sum()) + STRADDLE_TAKEN
    if dist == 'with_inf':
        n_inf = int((keys == KEY_MAX).sum())
        return plane - n_inf + n_inf // 2 if n_inf >= 2 else None
    vals, counts = np.unique(keys, return_counts=True)
    if counts.max() < 2:
        return None
    t = vals[np.argmax(counts)]
    return int((keys < t).sum()) + int(counts.max()) // 2


def topk_ks(dist, keys):
    plane = len(keys)
    ks = {1, plane - 1, plane, min(8192, plane), tie_cut(dist, keys)}
    return sorted(k for k in ks if k is not None and 1 <= k <= plane)


def topk_cases():
    """every (dist, plane) pair of the single-image sweep"""
    return [(d, p) for p in TOPK_PLANES for d in topk_dists(p)]


BATCH_DISTS = ('random', 'two_valued', 'byte1')      # N = 3: one distribution, so one threshold, per image


def topk_batch_keys(plane):
    dists = [d if d in topk_dists(plane) else 'random' for d in BATCH_DISTS]
    if plane >= 2 * CHUNK + 3:
        dists[1] = 'straddle'
    return dists, np.stack([topk_keys(d, plane, seed=7 + i) for i, d in enumerate(dists)])


def topk_ref(keys, k):
    """(N, plane) -> (N, k) sorted indices of the k smallest keys per image: every key below the k-th smallest value and, of the
    cells equal to it, those with the lowest index -- which is what a stable argsort lists first."""
    keys = np.atleast_2d(keys)
    return np.stack([np.sort(np.argsort(row, kind='stable')[:k]) for row in keys]).astype(np.int64)


def select_threshold(keys, k):
    """the four radix passes of launch_topk_smallest on one image: (T, krem, bytes) -- the k-th smallest key, how many of the keys
    equal to it are taken, and for each pass the number of candidate keys that entered it"""
    prefix, krem, entered = 0, int(k), []
    for p in range(4):
        shift = 24 - 8 * p
        himask = 0 if p == 0 else (0xffffffff << (shift + 8)) & 0xffffffff
        cand = keys[(keys & np.uint32(himask)) == np.uint32(prefix)]
        entered.append(len(cand))
        hist = np.bincount(((cand >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256)
        ex = np.cumsum(hist) - hist
        hit = np.nonzero((hist > 0) & (ex < krem) & (krem <= ex + hist))[0]
        assert len(hit) == 1, 'exactly one bucket holds the k-th key'
        prefix |= int(hit[0]) << shift
        krem -= int(ex[hit[0]])
    return prefix, krem, entered


def scan_rounds(plane):
    nb = -(-plane // CHUNK)
    return nb, -(-nb // SCAN_ROUND)


def select_model(keys, k):
    """CPU model of launch_topk_smallest on one image: radix select of the threshold, then the ORDERED compaction -- per-chunk
    counts of keys below / equal to the threshold, their exclusive scan in rounds of 256 chunks with carries, and every selected
    cell written at its chunk's offset plus its rank inside the chunk; of the equal keys only ranks below krem are written."""
    plane = len(keys)
    if k == plane:
        return np.arange(plane, dtype=np.int64)
    T, krem, _ = select_threshold(keys, k)
    nless = k - krem
    nb, _ = scan_rounds(plane)
    chunk = np.arange(plane) // CHUNK
    out = np.full(k, -1, np.int64)
    for flag, base, limit in ((keys < np.uint32(T), 0, nless), (keys == np.uint32(T), nless, krem)):
        cnt = np.bincount(chunk[flag], minlength=nb)
        off, carry = np.zeros(nb, np.int64), 0
        for b0 in range(0, nb, SCAN_ROUND):
            c = cnt[b0:b0 + SCAN_ROUND]
            off[b0:b0 + SCAN_ROUND] = carry + np.cumsum(c) - c
            carry += int(c.sum())
        g = np.cumsum(flag) - flag                                   # rank among the flagged cells of the whole plane
        pos = off[chunk] + (g - g[chunk * CHUNK])                    # chunk offset + rank inside the chunk
        take = flag & (pos < limit)
        assert flag.sum() >= limit and len(np.unique(pos[take])) == limit
        out[base + pos[take]] = np.nonzero(take)[0]
    assert (out >= 0).all()
    return np.sort(out)


# ----------------------------------------------------------------------------
# C. point sampling
# ----------------------------------------------------------------------------
def ld_of(C, ncls):
    """row length of the point rows as the network computes it: C + ncls rounded up to 64"""
    return (C + ncls + 63) // 64 * 64


def all_cells(N, H2, W2, seed=0):
    """every cell of the grid per image, shuffled: all borders and corners are sampled"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(H2 * W2) for _ in range(N)]).astype(np.int32)


def border_cells(H2, W2):
    corners = [0, W2 - 1, (H2 - 1) * W2, H2 * W2 - 1]
    edges = [W2 // 2, (H2 - 1) * W2 + W2 // 2, (H2 // 2) * W2, (H2 // 2) * W2 + W2 - 1]
    return list(dict.fromkeys(corners + edges))


def subset_cells(N, H2, W2, P, seed=0):
    """P distinct cells per image in random order: the four corners, one cell of each edge, the rest drawn at random"""
    rng = np.random.default_rng(seed)
    fixed = border_cells(H2, W2)
    assert len(fixed) <= P <= H2 * W2
    rest = np.setdiff1d(np.arange(H2 * W2), fixed)
    return np.stack([rng.permutation(np.concatenate([fixed, rng.choice(rest, size=P - len(fixed), replace=False)]))
                     for _ in range(N)]).astype(np.int32)


def sample_input(N, fh, fw, C, feat_ld, ncls, seed=0, half=True):
    """NHWC features (N, fh, fw, feat_ld), rounded to fp16 for the f16 kernel, with junk in the channels [C, feat_ld) that no
    kernel may read into its output, and NCHW fp32 coarse logits (N, ncls, fh, fw)"""
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((N, fh, fw, feat_ld)).astype(np.float32)
    feat[..., C:] = 1000.0
    if half:
        feat = feat.astype(np.float16)
    coarse = (4.0 * rng.standard_normal((N, ncls, fh, fw))).astype(np.float32)
    return feat, coarse


def point_coords(idx, H2, W2):
    """cell index -> (x, y) in [0, 1]^2, in fp32 exactly as point_rend.py:131-135 computes it"""
    idx = torch.from_numpy(np.asarray(idx).astype(np.int64))
    h_step, w_step = 1.0 / float(H2), 1.0 / float(W2)
    coords = torch.zeros(idx.shape[0], idx.shape[1], 2, dtype=torch.float)
    coords[:, :, 0] = 0.5 * w_step + w_step * (idx % W2).float()
    coords[:, :, 1] = 0.5 * h_step + h_step * torch.div(idx, W2, rounding_mode='floor').float()
    return coords


def point_sample_ref(maps, coords):
    """point_sample (point_rend.py:33-60) in float64: maps (N, C, h, w), coords (N, P, 2) fp32 -> (N, C, P)"""
    m = torch.from_numpy(np.asarray(maps, dtype=np.float64))
    grid = 2.0 * coords.double().unsqueeze(2) - 1.0
    return F.grid_sample(m, grid, mode='bilinear', padding_mode='zeros', align_corners=False).squeeze(3).numpy()


def point_rows_ref(feat, C, coarse, idx, H2, W2, ld):
    """the (N*P, ld) rows [C features | ncls coarse | zeros] in float64, from the operands as stored"""
    N, P = idx.shape
    ncls = coarse.shape[1]
    coords = point_coords(idx, H2, W2)
    f = point_sample_ref(np.asarray(feat, dtype=np.float64)[..., :C].transpose(0, 3, 1, 2), coords)      # (N, C, P)
    c = point_sample_ref(coarse, coords)
    rows = np.zeros((N * P, ld), np.float64)
    rows[:, :C] = f.transpose(0, 2, 1).reshape(N * P, C)
    rows[:, C:C + ncls] = c.transpose(0, 2, 1).reshape(N * P, ncls)
    return rows


def sample_bound(rows_ref, feat, C, coarse, half):
    """element-wise bound of |kernel - rows_ref| (derivation: module docstring); the pad columns get 0: they must be exact"""
    fh, fw = coarse.shape[2:]
    ncls = coarse.shape[1]
    k = (16.0 * max(fh, fw) + 10.0) * U
    e = np.zeros_like(rows_ref)
    e[:, :C] = k * float(np.abs(np.asarray(feat, dtype=np.float64)[..., :C]).max())
    e[:, C:C + ncls] = k * float(np.abs(coarse).max())
    if half:
        live = np.zeros_like(rows_ref, dtype=bool)
        live[:, :C + ncls] = True
        e = np.where(live, e + UH * (np.abs(rows_ref) + e) + 2.0 ** -24, 0.0)
    return e


# ----------------------------------------------------------------------------
# D. point head
# ----------------------------------------------------------------------------
def predictor_ref(rows, w, b):
    """rows (R, K), w (ncls, K), b (ncls) -> (float64 logits (R, ncls), element-wise bound of an fp32 accumulation)"""
    rows, w = np.asarray(rows, dtype=np.float64), np.asarray(w, dtype=np.float64)
    ref = rows @ w.T + np.asarray(b, dtype=np.float64)
    acc = rows.shape[1] * U * (np.abs(rows) @ np.abs(w).T)
    return ref, acc + U * (np.abs(ref) + acc)


def scatter_ref(target, logits, idx):
    """target (N, ncls, plane) with logits (N*P, ncls) written at idx (N, P); everything else keeps its content"""
    out = np.array(target, dtype=np.float64)
    N, P = idx.shape
    lg = np.asarray(logits).reshape(N, P, -1)
    for n in range(N):
        out[n][:, idx[n]] = lg[n].T
    return out


def head_weights(C, ld, ncls, num_fc, seed=0):
    """fc layers (C, ld) fp16 + (C,) fp32 bias and the predictor (ncls, ld) fp32 + (ncls,) bias; the columns [C + ncls, ld) of
    every weight are zero, as the network packs them"""
    rng = np.random.default_rng([seed, C, ncls, num_fc])
    fc_w, fc_b = [], []
    for _ in range(num_fc):
        w = np.zeros((C, ld), np.float32)
        w[:, :C + ncls] = rng.standard_normal((C, C + ncls)) * np.sqrt(2.0 / (C + ncls))
        fc_w.append(w.astype(np.float16))
        fc_b.append((0.1 * rng.standard_normal(C)).astype(np.float32))
    pw = np.zeros((ncls, ld), np.float32)
    pw[:, :C + ncls] = rng.standard_normal((ncls, C + ncls)) * np.sqrt(1.0 / (C + ncls))
    pb = (0.1 * rng.standard_normal(ncls)).astype(np.float32)
    return fc_w, fc_b, pw, pb


def point_head_ref(fine, coarse, fc_w, fc_b, pw, pb):
    """point_head_forward (point_rend.py:181-188) in float64: fine (R, C), coarse (R, ncls), fc weights (C, C + ncls), predictor
    (ncls, C + ncls) -> (logits (R, ncls), bound of an fp32 evaluation of the same chain: per layer the incoming error through
    |W|, the accumulation bound of predictor_ref and one rounding of the result; ReLU does not grow an error)"""
    coarse = np.asarray(coarse, dtype=np.float64)

    def layer(x, err, w, b):
        w = np.asarray(w, dtype=np.float64)
        y = x @ w.T + np.asarray(b, dtype=np.float64)
        acc = x.shape[1] * U * (np.abs(x) @ np.abs(w).T)
        return y, err @ np.abs(w).T + acc + U * (np.abs(y) + acc)

    x = np.concatenate([np.asarray(fine, dtype=np.float64), coarse], axis=1)
    err = np.zeros_like(x)
    for w, b in zip(fc_w, fc_b):
        y, ey = layer(x, err, w, b)
        x = np.concatenate([np.maximum(y, 0.0), coarse], axis=1)
        err = np.concatenate([ey, np.zeros_like(coarse)], axis=1)
    return layer(x, err, pw, pb)


# (C, ld, num_fc, ncls, N, P, fh, fw, scale): every (C, ld), num_fc, ncls and point count of the fused head at least once;
# N * P = 100 is one partial tile, 257 a full tile and a tile of one live row, 9 * 8192 = 288 tiles on a grid of 256
HEAD_CASES = [
    (256, 320, 3, 1, 1, 100, 6, 10, 4),
    (256, 320, 1, 3, 1, 256, 6, 10, 4),
    (256, 320, 4, 8, 1, 257, 6, 10, 4),
    (256, 320, 3, 3, 3, 8192, 24, 40, 4),
    (256, 320, 3, 1, 9, 8192, 24, 40, 4),
    (128, 192, 3, 3, 1, 100, 4, 4, 8),
    (128, 192, 1, 8, 1, 257, 6, 10, 4),
    (128, 192, 4, 1, 1, 256, 6, 10, 8),
    (128, 192, 3, 8, 3, 8192, 24, 40, 4),
    (128, 192, 1, 3, 9, 8192, 24, 40, 4),
]
HEAD_UNSUPPORTED = [(64, 128, 1, 3), (256, 320, 9, 3), (256, 320, 1, 5)]      # (C, ld, ncls, num_fc)


def head_case_id(c):
    return 'C%d_fc%d_cls%d_%dx%d' % (c[0], c[2], c[3], c[4], c[5])


def head_tiles(N, P):
    return -(-(N * P) // TILE)
