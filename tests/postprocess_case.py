"""Inputs, plain references and bounds for the direct tests of csrc/postprocess.hip (tests/test_postprocess_case_host.py,
tests/test_gpu_postprocess_kernels.py, the edge fixture of oracle/gen_golden.py).  No GPU, no torch.

The references are those of oracle/postprocess.py (which reproduces the reference project on tests/golden/postprocess.npz,
median3d.npz and postprocess_edges.npz), wrapped where the kernels' interface differs: batches, int32 cells, `up`, the clamp of
the centre count to `max_centers`, ids outside 1..max_ids.  Everything integer is compared for equality.

Bound of the probabilities (derived, not measured)
--------------------------------------------------
u = 2^-24 is the unit roundoff of fp32.  The device library documents expf at no more than 1 ulp, i.e. a relative error of at
most 2u; an fp32 add and the correctly rounded divide (build flag of the file) err by at most u each.

  sigmoid   r = 1 / (1 + e),  e = expf(-x).  The error 2u of e reaches 1 + e damped by e / (1 + e) < 1; the add and the
            divide add u each:  |r' - r| <= (2u + u + u) r = 4u r  to first order.
  softmax   r_c = e_c / s,  e_c = expf(fl32(x_c - max)),  s = e_0 + ... + e_{C-1}.  The reference evaluates exp at the SAME
            fp32-rounded argument, so the subtraction costs nothing.  Numerator 2u; every term of the sum 2u, and since all
            terms are positive the C - 1 additions add (C - 1) u to the relative error of s; the divide u:
            |r'_c - r_c| <= (2u + 2u + (C - 1) u + u) r_c = (C + 4) u r_c  to first order.

Second-order terms are below (C + 4)^2 u^2 < 2^-38 relative for C <= 32: a factor (1 + 2^-12) on the bound covers them with room.
Results, numerators or terms below FLT_MIN may be flushed to zero or carry an absolute error of a subnormal ulp; the largest
term of the sum is expf(0) = 1, so s >= 1 and any such error reaches the result as less than FLT_MIN absolute: the floor.  expf
overflows (e = inf, r = 0) only where 1 / (1 + e) < 2^-128 < FLT_MIN.

Voting: which inputs must match bit for bit
-------------------------------------------
Votes that are multiples of 0.25 with |dy|, |dx| < 1024 have at most 13 significant bits, so dy * dy is exact in fp32 and
dx * dx + dy * dy is exact in float64: the oracle's fused multiply-add (emulated through float64) rounds once, exactly like the
device's, and two centres at the same rounded distance are at the same true distance.  A vote of 3e5 leaves that range, but its
fl32(dy * dy) is the same correctly rounded product on both sides and fits float64 next to dx * dx without a second rounding.
Generic (gaussian) votes could differ where the float64 emulation double-rounds (~2^-29 per element) AND the two nearest
centres, or the nearest and the 1e5 start value, are closer than the fp32 evaluation resolves; `near_tie_mask` excludes the
pixels whose two smallest float64 distances differ by no more than 2^-20 of the smaller (32 ulp of fp32, against an evaluation
error of about 2 ulp) or whose best distance lies within that margin of 1e5.  At most NEAR_TIE_CAP of the pixels may be excluded.
"""
import functools
import os
import re

import numpy as np

from oracle import postprocess as opp

f32 = np.float32
U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)

# mirrored from csrc/postprocess.hip; source_constants() reads them out of the source and the host test compares
MAX_KS = 15                  # largest median kernel
CTR_TILE = 1024              # centres per LDS tile of the scan
GRID_MIN, GRID_KMAX = 192, 16384      # centre counts between which the grid path votes
MERGE_VEC_GROUPS = 4         # groups of 4 pixels per thread of the vector count kernel: 4096 pixels per workgroup
ARGMIN_MAX = 20              # up to 20 centres: argmin (always an index); above: start value 1e5
HASH_SIZE = 256              # entries of the count kernels' LDS hash table
LAUNCH_CAP, BLOCK = 4096, 256         # grid-stride kernels: at most 4096 workgroups of 256
ONE_TRIP = LAUNCH_CAP * BLOCK         # 1 048 576 elements: one more runs the second trip of the loop
BIG_COUNT = ONE_TRIP + 37
MERGE_SCALAR_PIXELS, MERGE_VEC_PIXELS = BLOCK * 8, BLOCK * 4 * MERGE_VEC_GROUPS

GUARD = 64                   # sentinel elements around every output buffer
F32_SENTINEL, I32_SENTINEL, I64_SENTINEL, WORK_FILL = 12345.0, -7777, -777777, 0xA5

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'empanada-napari_amd', 'csrc', 'postprocess.hip')


def source_constants(path=SOURCE):
    src = open(path).read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(set(m)) == 1, f'{pattern!r}: {m}'
        return m[0]

    cap = one(r'inline int grid_for\(int64_t total, int per_block = (\d+), int cap = (\d+) \* (\d+)\)')
    return {
        'MAX_KS': int(one(r'constexpr int MAX_KS = (\d+);')),
        'CTR_TILE': int(one(r'constexpr int CTR_TILE = (\d+);')),
        'GRID_MIN': int(one(r'constexpr int GRID_MIN = (\d+),')),
        'GRID_KMAX': int(one(r'GRID_KMAX = (\d+),')),
        'MERGE_VEC_GROUPS': int(one(r'constexpr int MERGE_VEC_GROUPS = (\d+);')),
        'ARGMIN_MAX': int(one(r'float best = \(K > (\d+)\) \? 1e5f : INFINITY;')),
        'ARGMIN_MAX_first': int(one(r'const bool first = \(K <= (\d+)\)')),
        'HASH_SIZE': int(one(r'__shared__ int tkey\[(\d+)\];')),
        'HASH_PROBES': int(one(r'for \(int probe = 0; probe < (\d+) && !done; \+\+probe\)')),
        'BLOCK': int(cap[0]),
        'LAUNCH_CAP': int(cap[1]) * int(cap[2]),
    }


# ----------------------------------------------------------------------------
# medians
# ----------------------------------------------------------------------------
def median_ref(x):
    """x (ks, ...) -> the middle order statistic over axis 0"""
    return np.sort(x, axis=0)[(x.shape[0] - 1) // 2]


def median_recursive_ref(hist, raw, ks, n_out):
    """hist (mid, count) filtered maps before the run, raw (n_raw, count): out[j] is the middle order statistic of the last
    mid outputs (seeded by hist) and raw[j .. j+mid] -- the recursion itself"""
    mid = (ks - 1) // 2
    assert hist.shape[0] == mid and raw.shape[0] >= n_out + mid
    filtered = [h for h in hist]
    for j in range(n_out):
        window = np.stack(filtered[len(filtered) - mid:] + [raw[j + k] for k in range(mid + 1)])
        assert window.shape[0] == ks
        filtered.append(np.sort(window, axis=0)[mid])
    return np.stack(filtered[mid:])


def median_stack_ref(stack, ks):
    """a whole stack (n, count) as the 3-D engine filters it: the first and the last mid slices stay raw"""
    mid = (ks - 1) // 2
    n = stack.shape[0]
    if mid == 0 or n <= 2 * mid:
        return stack.copy()
    body = median_recursive_ref(stack[:mid], stack[mid:], ks, n - 2 * mid)
    return np.concatenate([stack[:mid], body, stack[n - mid:]])


def median_input(ks, count, seed=0):
    """(ks, count) float32 with ties across slices: a third of the pixels draw from five values"""
    rng = np.random.default_rng([seed, ks, count % 1000])
    x = rng.standard_normal((ks, count)).astype(f32)
    tied = rng.integers(0, 5, (ks, count)).astype(f32)
    sel = rng.random(count) < 0.33
    x[:, sel] = tied[:, sel]
    x[:, :min(3, count)] = x[0, :min(3, count)]      # every slice equal
    return x


MEDIAN_KS = tuple(range(1, MAX_KS + 1, 2))
RECURSIVE_KS = tuple(range(3, MAX_KS + 1, 2))


def recursive_cases():
    """(ks, n_out, extra raw maps, count): every ks x n_out in {1, 2, mid, mid + 3} x n_raw - n_out - mid in {0, 2} at count 7;
    the count past one trip of the grid-stride loop at ks 3 and 15 only"""
    cases = []
    for ks in RECURSIVE_KS:
        mid = (ks - 1) // 2
        for n_out in sorted({1, 2, mid, mid + 3}):
            for extra in (0, 2):
                cases.append((ks, n_out, extra, 7))
    cases += [(3, 2, 2, BIG_COUNT), (15, 2, 0, BIG_COUNT)]
    return cases


# ----------------------------------------------------------------------------
# probabilities
# ----------------------------------------------------------------------------
def prob_ref(x):
    """float64 reference of emp_logits_to_prob on (N, C, H, W) float32 logits; the softmax at the fp32-rounded argument"""
    x = np.asarray(x, f32)
    with np.errstate(over='ignore'):
        if x.shape[1] == 1:
            return 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
        a = (x - x.max(axis=1, keepdims=True)).astype(f32).astype(np.float64)
        e = np.exp(a)
        return e / e.sum(axis=1, keepdims=True)


def prob_bound(ref, C_):
    rel = (4 if C_ == 1 else C_ + 4) * U * (1 + 2.0 ** -12)
    return rel * np.abs(ref) + FLT_MIN


def violations(got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    return int((~(err <= bound)).sum())


def worst_ratio(got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    if np.isnan(err).any():
        return float('inf')
    return float((err / bound).max())


PROB_SHAPES = [(2, 3, 5), (1, 1, BIG_COUNT)]      # (N, H, W): a tiny map; one row past the first trip of the loop
PROB_CLASSES = (1, 2, 5)


def prob_input(N, C_, H, W, seed=0):
    rng = np.random.default_rng([seed, N, C_, H, W])
    x = (rng.standard_normal((N, C_, H, W)) * 6).astype(f32)
    flat = x.reshape(N, C_, -1)
    if C_ == 1:
        edge = np.array([88, -88, 104, -104, np.inf, -np.inf, 0, -0.0, 1e-30, 16.5, -16.5, 87.5, -87.5], f32)
        flat[0, 0, :len(edge)] = edge
        flat[-1, 0, -2:] = [-88, 88]      # and on the last elements: the second trip at the large shape
    else:
        flat[0, C_ - 1, ::3] -= 200.0      # one class plane far below the others: its exponential underflows
        flat[0, 0, 1] = flat[0, 1, 1]      # equal logits
        flat[-1, :, -1] = np.linspace(-90, 3, C_)
    return x


# ----------------------------------------------------------------------------
# centres
# ----------------------------------------------------------------------------
def centers_ref(ctr, thr, k):
    """ctr (N, 1, h, w) -> per image the (K, 2) int64 (y, x) centres of oracle.find_instance_center, row-major"""
    return [opp.find_instance_center(ctr[n:n + 1], thr, k) for n in range(ctr.shape[0])]


NMS_KERNELS = (1, 2, 3, 4, 5, 7, 15)
NMS_MAPS = [(1, 1), (1, 40), (40, 1), (5, 6), (7, 9), (8, 8), (5, 13), (9, 11), (127, 129)]
NMS_THR = 0.25               # exactly representable; the maps hold values equal to it
NMS_N = 3


def nms_input(h, w, seed=0):
    """(3, 1, h, w) heat maps on a grid of sixteenths (so that equal values and plateaus abound): plateaus touching every
    border and every corner, values exactly equal to NMS_THR, zeros and negative values; image 1 is all zero"""
    rng = np.random.default_rng([seed, h, w])
    x = (rng.integers(-2, 17, (NMS_N, 1, h, w)) / 16.0).astype(f32)
    x[rng.random(x.shape) < 0.5] = 0.0
    x[rng.random(x.shape) < 0.1] = NMS_THR
    top = f32(1.0)
    for img in (x[0, 0], x[2, 0]):
        img[0, :min(w, 3)] = top                   # plateau on the top-left corner
        img[h - 1, max(0, w - 2):] = top           # bottom-right corner
        img[max(0, h - 3):, 0] = top               # left border, bottom-left corner
        img[:min(h, 2), w - 1] = top               # right border, top-right corner
        img[h // 2, w // 2] = NMS_THR              # equal to the threshold
    x[1] = 0.0
    return x


def exact_centres_map(N, h, w, counts, seed=0):
    """(N, 1, h, w) heat map with exactly counts[n] pixels at 0.5 .. 0.9 and the rest 0: nms_kernel = 1 keeps each of them"""
    rng = np.random.default_rng([seed, h, w] + list(counts))
    x = np.zeros((N, 1, h, w), f32)
    for n, K in enumerate(counts):
        where = rng.choice(h * w, size=K, replace=False)
        x[n, 0].reshape(-1)[where] = (0.5 + 0.4 * rng.random(K)).astype(f32)
    return x


# ----------------------------------------------------------------------------
# voting
# ----------------------------------------------------------------------------
VOTE_CHUNK = 1 << 19         # pixels x centres per block of the distance matrix (stays in the cache)


def _vote_geometry(centres, off, step):
    off = np.asarray(off, f32)
    h, w = off.shape[1:]
    ys = (np.arange(h, dtype=f32) * f32(step)).astype(f32)
    xs = (np.arange(w, dtype=f32) * f32(step)).astype(f32)
    ly = (ys[:, None] + off[0]).astype(f32).reshape(-1)
    lx = (xs[None, :] + off[1]).astype(f32).reshape(-1)
    c = (f32(step) * centres.astype(f32)).astype(f32)
    return ly, lx, c


def vote_ref(centres, off, step):
    """oracle.group_pixels for one image -- centres (K, 2) int (y, x), off (2, h, w) fp32 -> (h, w) int64 ids -- as blocks of a
    pixels x centres matrix of the oracle's fp32 distances (the arithmetic of opp._norm2) instead of a loop over the centres: the first minimum
    is the lowest index among equals (the oracle's strict '<' in index order), up to ARGMIN_MAX centres always an index, above
    only a distance below 1e5.  tests/test_postprocess_case_host.py holds it against group_pixels itself."""
    K = centres.shape[0]
    assert K > 0
    ly, lx, c = _vote_geometry(centres, off, step)
    ids = np.zeros(ly.size, np.int64)
    rows = max(1, VOTE_CHUNK // K)
    cy, cx = np.ascontiguousarray(c[None, :, 0]), np.ascontiguousarray(c[None, :, 1])
    with np.errstate(invalid='ignore', over='ignore'):
        for p0 in range(0, ly.size, rows):
            sl = slice(p0, p0 + rows)
            # opp._norm2 term by term, in place: fl32(dy * dy); dx * dx + that in float64 (the emulated fma); fl32; fl32 sqrt
            dy2 = cy - ly[sl, None]
            np.multiply(dy2, dy2, out=dy2)
            s = (cx - lx[sl, None]).astype(np.float64)
            np.multiply(s, s, out=s)
            s += dy2
            d = s.astype(f32)
            np.sqrt(d, out=d)
            d[np.isnan(d)] = np.inf      # a NaN distance is never below anything
            first = np.argmin(d, axis=1)
            if K <= ARGMIN_MAX:
                ids[sl] = first + 1      # all NaN / inf: index 0, as argmin (and the oracle's forced first update)
            else:
                ids[sl] = np.where(d[np.arange(d.shape[0]), first] < f32(1e5), first + 1, 0)
    return ids.reshape(off.shape[1:])


def near_tie_mask(centres, off, step):
    """(h, w) bool: pixels whose nearest centre the fp32 evaluation may not resolve (module docstring)"""
    K = centres.shape[0]
    ly, lx, c = _vote_geometry(centres, off, step)
    mask = np.zeros(ly.size, bool)
    margin = 2.0 ** -20
    rows = max(1, VOTE_CHUNK // K)
    with np.errstate(invalid='ignore', over='ignore'):
        for p0 in range(0, ly.size, rows):
            sl = slice(p0, p0 + rows)
            dy = (c[None, :, 0] - ly[sl, None]).astype(f32).astype(np.float64)
            dx = (c[None, :, 1] - lx[sl, None]).astype(f32).astype(np.float64)
            d = np.sqrt(dy * dy + dx * dx)
            if K > 1:
                two = np.partition(d, 1, axis=1)[:, :2]
                mask[sl] |= (two[:, 1] - two[:, 0]) <= margin * two[:, 0]
            best = d.min(axis=1)
            if K > ARGMIN_MAX:
                mask[sl] |= np.abs(best - 1e5) <= margin * 1e5
            mask[sl] |= ~np.isfinite(best)
    return mask.reshape(off.shape[1:])


NEAR_TIE_CAP = 1e-4


def cells_ref(ctr, off, thr, k, step, up, max_centers=None):
    """emp_instance_cells on (N, 1, h, w) / (N, 2, h, w): per image the oracle's centres, the vote over the first
    min(K, max_centers) of them, int32, every cell repeated up x up -> (cells (N, h*up, w*up) int32, list of centres)"""
    N, _, h, w = ctr.shape
    centres = centers_ref(ctr, thr, k)
    cells = np.zeros((N, h * up, w * up), np.int32)
    for n in range(N):
        used = centres[n] if max_centers is None else centres[n][:max_centers]
        if used.shape[0]:
            cells[n] = opp.nearest_upsample(vote_ref(used, off[n], step).astype(np.int32), up)
    return cells, centres


def quarter_votes(N, h, w, step, seed=0, special=True):
    """(N, 2, h, w) votes in multiples of 0.25 (exact ties, bit-for-bit inputs): most within +-12 cells, a band pointing outside
    the map, and with `special` one vote beyond 1e5 and NaN / +inf / -inf votes"""
    rng = np.random.default_rng([seed, N, h, w, step])
    off = (rng.integers(-48 * step, 48 * step + 1, (N, 2, h, w)) / 4.0).astype(f32)
    off[:, :, ::5, ::3] = np.round(off[:, :, ::5, ::3])      # whole cells: pixels equidistant from several centres
    off[:, 0, h - 1, :] = 300.0       # below the map
    off[:, 1, :, 0] = -250.25         # left of it
    if special and h * w >= 12:
        flat = off.reshape(N, 2, -1)
        flat[:, 0, 1] = 3.0e5
        flat[:, 1, 2] = -3.0e5
        flat[:, 0, 3] = np.nan
        flat[:, 1, 4] = np.inf
        flat[:, 0, 5] = -np.inf
        flat[N - 1, :, 6] = np.nan
    return off


def gaussian_votes(N, h, w, step, sigma, seed=0):
    rng = np.random.default_rng([seed, N, h, w, step, 77])
    return (rng.standard_normal((N, 2, h, w)) * sigma * step).astype(f32)


# (centre counts per image, h, w): maps just large enough, more than one workgroup of 256 pixels each
VOTE_COUNT_CASES = [
    ((0, 1), 17, 19), ((20, 21), 17, 19),                     # argmin <-> 1e5 start value
    ((GRID_MIN - 1, GRID_MIN), 17, 19),                       # scan <-> grid; one image of the batch on each side
    ((CTR_TILE, CTR_TILE + 1), 33, 35),                       # one <-> two LDS tiles
    ((GRID_KMAX, GRID_KMAX + 1), 130, 130),                   # grid <-> back to the scan
]
VOTE_STEP_UP = [(1, 1), (1, 2), (1, 4), (1, 8), (4, 1), (4, 2), (4, 4), (4, 8)]
VOTE_GENERIC = [(15, 17, 19, 1), (25, 17, 19, 4), (300, 40, 37, 1), (1100, 40, 37, 4), (5000, 80, 80, 1)]   # (K, h, w, step)


@functools.lru_cache(maxsize=None)
def vote_case(counts, h, w, step, generic=False):
    """inputs and the up = 1 reference of one voting case, computed once: (ctr, off, cells (N, h, w) int32, centres, mask)"""
    N = len(counts)
    ctr = exact_centres_map(N, h, w, counts, seed=step)
    off = gaussian_votes(N, h, w, step, 6.0) if generic else quarter_votes(N, h, w, step)
    cells, centres = cells_ref(ctr, off, 0.1, 1, step, 1)
    assert [c.shape[0] for c in centres] == list(counts)
    mask = None
    if generic:
        mask = np.stack([near_tie_mask(centres[n], off[n], step) if counts[n] else np.zeros((h, w), bool) for n in range(N)])
    for a in (ctr, off, cells):
        a.setflags(write=False)
    return ctr, off, cells, centres, mask


# ----------------------------------------------------------------------------
# merge
# ----------------------------------------------------------------------------
def merge_ref(sem, cells, thr, things, divisor, stuff_area, void_label, max_ids):
    """emp_panoptic_merge on sem (N, C, H, W) probabilities and cells (N, H, W) int32: per image
    oracle.merge_semantic_and_instance on the harden_seg output; an id outside 1 .. max_ids is no instance, and (as
    get_panoptic_seg does) an id counts only on pixels of a thing class"""
    N = sem.shape[0]
    out = []
    for n in range(N):
        hard = opp.harden_seg(sem[n:n + 1], thr)[0]
        ids = cells[n].astype(np.int64)[None]
        ids = np.where((ids > 0) & (ids <= max_ids), ids, 0)
        thing = np.isin(hard, list(things)) if len(things) else np.zeros(hard.shape, bool)
        out.append(merge_semantic_and_instance_fast(hard, np.where(thing, ids, 0), divisor, things, stuff_area, void_label)[0])
    return np.stack(out)


def merge_semantic_and_instance_fast(sem_seg, ins_seg, divisor, things, stuff_area, void_label):
    """oracle.merge_semantic_and_instance with the loop over instances replaced by one (id, class) table -- identical output
    (the host test compares the two); the 4096-id plane would otherwise take 4096 passes"""
    sem_seg, ins_seg = np.asarray(sem_seg, np.int64), np.asarray(ins_seg, np.int64)
    pan = np.zeros_like(sem_seg) + void_label
    ncls = int(max([sem_seg.max()] + list(things))) + 1
    thing = np.isin(sem_seg, list(things)) if len(things) else np.zeros(sem_seg.shape, bool)
    live = thing & (ins_seg > 0)
    table = np.zeros((int(ins_seg.max()) + 1, ncls), np.int64)
    np.add.at(table, (ins_seg[live], sem_seg[live]), 1)
    new = np.full(table.shape[0], -1, np.int64)
    tracker = {}
    for i in np.nonzero(table.sum(axis=1))[0]:
        c = int(np.argmax(table[i]))      # first maximum: ties -> smallest class
        tracker[c] = tracker.get(c, 0) + 1
        new[i] = c * divisor + tracker[c]
    pan[live] = new[ins_seg[live]]
    for c in np.unique(sem_seg):
        if int(c) in things:
            continue
        smask = (sem_seg == c) & ~(ins_seg > 0)
        if int(smask.sum()) >= stuff_area:
            pan[smask] = c * divisor
    return pan


MERGE_THR = 0.5


def merge_input(N, C_, H, W, things, max_ids, seed=0):
    """sem (N, C, H, W) probabilities on a grid of 1/64 and cells (N, H, W) int32, different populations per image.
    Ids lie in blocks of 2 x 3 pixels and run from -3 to max_ids + 40 with gaps (every id divisible by 7 is missing); the
    class planes put ids on at least two thing classes, make whole instances lie on stuff pixels, give one instance an exact
    class tie, and hold probabilities exactly equal to MERGE_THR and exact ties between planes."""
    rng = np.random.default_rng([seed, N, C_, H, W, max_ids] + list(things))
    sem = (rng.integers(0, 65, (N, C_, H, W)) / 64.0).astype(f32)
    if C_ == 1:
        sem[rng.random(sem.shape) < 0.15] = MERGE_THR
    else:
        # smooth class regions: stripes of the classes, so that instances mostly sit inside one class
        yy, xx = np.mgrid[0:H, 0:W]
        for n in range(N):
            region = ((yy // 5 + xx // 7 + n) % C_)
            for c in range(C_):
                sem[n, c][region == c] += 1.0
        tie = rng.random((N, H, W)) < 0.1
        m = sem.max(axis=1)
        for c in (0, min(1, C_ - 1)):
            sem[:, c][tie] = m[tie]              # exact ties between planes 0 and 1 at the maximum: the lower class wins
    bh, bw = -(-H // 2), -(-W // 3)
    blocks = rng.integers(-3, max_ids + 41, (N, bh, bw))
    blocks[blocks % 7 == 0] = 0
    blocks[rng.random(blocks.shape) < 0.2] = 0
    if N > 1:
        blocks[1] = np.where(rng.random((bh, bw)) < 0.7, 0, blocks[1])      # a sparse image
    cells = np.ascontiguousarray(np.repeat(np.repeat(blocks, 2, axis=1), 3, axis=2)[:, :H, :W].astype(np.int32))
    cells[N - 1, H - 1, W - 1], cells[N - 1, H - 1, W - 2] = -2, max_ids + 7      # outside 1 .. max_ids: no instance
    stuff = [c for c in range(max(C_, 2)) if c not in things]
    if max_ids >= 3 and H >= 8 and W >= 8:
        cells[0][(cells[0] == 2) | (cells[0] == 3)] = 0
        if things and stuff:
            cells[0, 0:2, 0:3] = 2                               # id 2 wholly on stuff pixels: no number, void or stuff label
            _set_class(sem, 0, slice(0, 2), slice(0, 3), stuff[0])
        live = [t for t in things if t < max(C_, 2)]
        if len(live) >= 2:
            cells[0, 4:6, 0:4] = 3                               # id 3: four pixels of each of two thing classes
            _set_class(sem, 0, slice(4, 6), slice(0, 2), live[1])
            _set_class(sem, 0, slice(4, 6), slice(2, 4), live[0])
    return sem, cells


def _set_class(sem, n, ys, xs, c):
    if sem.shape[1] == 1:
        sem[n, 0, ys, xs] = 1.0 if c == 1 else 0.0
    else:
        sem[n, :, ys, xs] = 0.0
        sem[n, c, ys, xs] = 2.0


def merge_features(sem, cells, things, max_ids):
    """which of the merge's corner cases an input holds (the host test asserts them case by case)"""
    found = set()
    for n in range(sem.shape[0]):
        hard = opp.harden_seg(sem[n:n + 1], MERGE_THR)[0, 0]
        ids = cells[n]
        if (ids > max_ids).any():
            found.add('id_above_max')
        if (ids < 0).any():
            found.add('negative_id')
        ok = (ids > 0) & (ids <= max_ids)
        thing = np.isin(hard, list(things)) if len(things) else np.zeros(hard.shape, bool)
        present = set(np.unique(ids[ok]).tolist())
        if present and len(present) < max(present):
            found.add('missing_ids')
        classes = {}
        for i in present:
            v, c = np.unique(hard[(ids == i) & thing], return_counts=True)
            if v.size == 0:
                found.add('all_stuff_instance')
                continue
            if (c == c.max()).sum() > 1:
                found.add('class_tie')
            classes.setdefault(int(v[np.argmax(c)]), []).append(i)
        big = [c for c, l in classes.items() if any(i <= HASH_SIZE for i in l) and any(i > HASH_SIZE for i in l)]
        if len(big) >= 2:
            found.add('two_classes_carry_over_chunks')
    if sem.shape[1] == 1 and (sem == f32(MERGE_THR)).any():
        found.add('prob_equals_thr')
    return found


def distinct_ids_input(H=64, W=64, C_=3):
    """every pixel of the plane its own id (max_ids = H * W): a workgroup of the count kernels sees 2048 / 4096 distinct keys,
    far beyond the HASH_SIZE entries of its table"""
    rng = np.random.default_rng(4096)
    sem = (rng.integers(0, 65, (1, C_, H, W)) / 64.0).astype(f32)
    cells = rng.permutation(H * W).astype(np.int32).reshape(1, H, W) + 1
    return sem, cells


def stuff_counts(sem, things, n=0):
    """{class: pixels} of the stuff classes of image n"""
    hard = opp.harden_seg(sem[n:n + 1], MERGE_THR)[0]
    return {int(c): int((hard == c).sum()) for c in np.unique(hard) if int(c) not in things}


THINGS16 = list(range(1, 32, 2))      # 16 thing classes of C = 32
MERGE_CASES = [      # (C, things, void_label, max_ids, H, W)
    (1, [1], 0, 256, 33, 31),
    (1, [], 255, 255, 33, 31),
    (1, [2], -1, 1, 8, 8),
    (2, [1], 255, 257, 33, 31),
    (2, [0, 1], 0, 600, 64, 64),
    (3, [2], 255, 0, 33, 31),
    (3, [1, 2], -1, 600, 64, 64),
    (3, [1, 2], 255, 600, 33, 31),
    (5, [1, 2], 255, 257, 40, 52),
    (5, [], 0, 255, 5, 7),
    (32, THINGS16, 255, 600, 64, 64),
    (32, THINGS16, -1, 256, 33, 31),
]


# the two write kernels stride over at most 2048 workgroups: the scalar one makes a second trip from 524 289 pixels, the
# vector one (4 pixels per lane) from 2 097 153.  725 x 725 is odd (scalar kernels either way), 1449 x 1448 a multiple of 4.
MERGE_WRITE_CAP = 2048
MERGE_TRIP_SHAPES = [(725, 725), (1449, 1448)]


def stuff_areas(sem, things):
    """0, exactly one stuff class's count, one above it, above every count (plane + 1)"""
    counts = stuff_counts(sem, things)
    plane = sem.shape[-1] * sem.shape[-2]
    if not counts:
        return [0, plane + 1]
    c = sorted(counts.values())[len(counts) // 2]
    return [0, c, c + 1, plane + 1]


# ----------------------------------------------------------------------------
# the edge fixture: tests/golden/postprocess_edges.npz holds the reference project's outputs on these inputs
# ----------------------------------------------------------------------------
EDGE_CASES = {      # name: (H, W, coarse, C, things, void_label, nms_kernel, exact centre count or None, upsampling, stuff_area)
    'void255': (24, 28, False, 1, [1], 255, 3, None, 1, 2000),      # class 0 below stuff_area: void
    'things2': (24, 28, False, 4, [2], 255, 3, None, 1, 64),
    'things12': (24, 28, False, 4, [1, 2], 255, 3, None, 1, 64),
    'stuff_at': (24, 28, False, 4, [1, 2], 255, 3, None, 1, 'at'),
    'stuff_above': (24, 28, False, 4, [1, 2], 255, 3, None, 1, 'above'),
    'nms1': (24, 28, False, 1, [1], 0, 1, None, 1, 64),
    'nms5': (48, 48, True, 1, [1], 0, 5, None, 1, 64),
    'k20': (24, 28, False, 1, [1], 0, 1, 20, 1, 64),
    'k21': (24, 28, False, 1, [1], 0, 1, 21, 1, 64),
    'up2_coarse': (32, 32, True, 1, [1], 0, 3, None, 2, 64),
    'up2_fine': (16, 20, False, 1, [1], 0, 3, None, 2, 64),
}
EDGE_THR, EDGE_DIVISOR = 0.1, 1000


def edge_inputs(name):
    """-> dict(sem_logits (1, C, H, W), ctr (1, 1, h, w), off (1, 2, h, w), stuff_area, ...); logits are multiples of 0.25 with
    the winning class 6 above the rest, so that no probability lies near a decision"""
    H, W, coarse, C_, things, void_label, k, K, upsampling, stuff_area = EDGE_CASES[name]
    step = 4 if coarse else 1
    h, w = H // step, W // step
    seed = sorted({n.split('_')[0] for n in EDGE_CASES}).index(name.split('_')[0])      # stuff_at / stuff_above: one input
    rng = np.random.default_rng([2024, seed])
    yy, xx = np.mgrid[0:H, 0:W]
    logits = (rng.integers(-4, 5, (1, C_, H, W)) / 4.0).astype(f32)
    if C_ == 1:
        logits[0, 0] += np.where((yy // 6 + xx // 9) % 2 == 0, 6.0, -6.0).astype(f32)
    else:
        region = (yy // 6 + xx // 9) % (C_ - 1)
        region[:3, :5] = C_ - 1      # the last (stuff) class: one patch of 15 pixels, below the default stuff_area
        for c in range(C_):
            logits[0, c][region == c] += 6.0
    if K is None:
        ctr = (rng.integers(0, 17, (1, 1, h, w)) / 16.0).astype(f32)
        ctr[rng.random(ctr.shape) < 0.6] = 0.0
        ctr[0, 0, 1:3, 1:3] = 1.0      # a plateau
    else:
        ctr = exact_centres_map(1, h, w, [K], seed=seed)
    off = quarter_votes(1, h, w, step, seed=seed, special=False)
    if stuff_area in ('at', 'above'):
        counts = stuff_counts(opp.logits_to_prob(logits), things)
        stuff_area = min(counts.values()) + (stuff_area == 'above')
    return dict(sem_logits=logits, ctr=ctr, off=off, coarse=coarse, step=step, things=things, void_label=void_label, k=k,
                upsampling=upsampling, stuff_area=int(stuff_area), C=C_)


def edge_oracle(name):
    """the oracle's outputs in the fixture's layout: centres, groups, the up-sampled cells and (upsampling 1) the panoptic map"""
    e = edge_inputs(name)
    out = {}
    centres = opp.find_instance_center(e['ctr'], EDGE_THR, e['k'])
    out['centers'] = centres
    if centres.shape[0]:
        out['groups'] = opp.group_pixels(centres, e['off'], step=e['step'])
    cells = opp.get_instance_cells(e['ctr'], e['off'], EDGE_THR, e['k'], e['coarse'], e['upsampling'])
    if e['upsampling'] * e['step'] > 1:      # (otherwise the cells are the groups)
        out['cells'] = cells.astype(np.int32)
    if e['upsampling'] == 1:
        hard = opp.harden_seg(opp.logits_to_prob(e['sem_logits']), MERGE_THR)[0]
        out['pan'] = opp.get_panoptic_seg(hard, cells, e['things'], EDGE_DIVISOR, e['stuff_area'], e['void_label'])
    return out
