"""Inputs and a numpy model of the two-read select of csrc/pointrend.hip (launch_topk_smallest without EMP_TOPK_LEGACY) and the
inputs of the panoptic merge's A/B test (tests/test_select_merge_case_host.py, tests/test_gpu_select_merge_ab.py).  No GPU.

The select histograms the SEL_BITS bits below the sign bit of every key, finds the bin B that holds the k-th smallest key,
selects every key of a lower bin outright and resolves the exact threshold among the keys of bin B alone -- unless that bin
holds more than SEL_CAP keys of the image, in which case the image refines the threshold with two more histogram levels over
all of its keys.  Both constants mirror csrc/pointrend.hip; the host test reads them out of the source and fails if they differ.
"""
import numpy as np

import pointrend_case as PC

SEL_BITS = 12                # width of the leading digit: bits 30..19 of the key
SEL_CAP = 8192               # keys of the threshold bin that an image may send to its candidate buffer
SEL_SHIFT = 31 - SEL_BITS
LEVELS = ((SEL_SHIFT, SEL_BITS), (SEL_SHIFT - 12, 12), (0, SEL_SHIFT - 12))      # (shift, bits) of the three histogram levels


def digit(keys):
    return (np.asarray(keys, np.uint32) >> np.uint32(SEL_SHIFT)).astype(np.int64)


def threshold_bin(keys, k):
    """(B, krem, pop): the bin of the leading digit that holds the k-th smallest key, how many keys are still to take from it
    and how many it holds"""
    hist = np.bincount(digit(keys), minlength=1 << SEL_BITS)
    ex = np.cumsum(hist) - hist
    hit = np.nonzero((hist > 0) & (ex < k) & (k <= ex + hist))[0]
    assert len(hit) == 1
    b = int(hit[0])
    return b, int(k - ex[b]), int(hist[b])


def path_of(keys, k):
    """'identity' (k == plane: no select runs), 'fast' or 'overflow'"""
    if k == len(keys):
        return 'identity'
    return 'overflow' if threshold_bin(keys, k)[2] > SEL_CAP else 'fast'


def ordered_ref(keys, k):
    """the output array element for element: every index whose key is below the k-th value, ascending, then the lowest
    indices among the keys equal to it, ascending; k == plane is the identity branch, which lists every cell in order"""
    keys = np.asarray(keys, np.uint32)
    if k == len(keys):
        return np.arange(k, dtype=np.int64)
    t = np.sort(keys, kind='stable')[k - 1]
    less = np.nonzero(keys < t)[0]
    ties = np.nonzero(keys == t)[0][:k - len(less)]
    return np.concatenate([less, ties]).astype(np.int64)


def select2_model(keys, k):
    """numpy model of the two-read select on one image: the ordered output array and the path taken"""
    keys = np.asarray(keys, np.uint32)
    plane = len(keys)
    if k == plane:
        return np.arange(plane, dtype=np.int64), 'identity'
    b, krem, pop = threshold_bin(keys, k)
    if pop <= SEL_CAP:
        # candidate pass: masks by digit; resolve: bisection on the candidates (in any order: they arrive through an atomic)
        less = digit(keys) < b
        cand = np.nonzero(digit(keys) == b)[0]
        ck = keys[cand]
        t = np.uint32(b << SEL_SHIFT)
        for bit in range(SEL_SHIFT - 1, -1, -1):
            trial = np.uint32(int(t) | (1 << bit))
            if int((ck < trial).sum()) < krem:
                t = trial
        krem -= int((ck < t).sum())
        less[cand[ck < t]] = True
        eq = np.zeros(plane, bool)
        eq[cand[ck == t]] = True
        path = 'fast'
    else:
        prefix = b << SEL_SHIFT
        for shift, bits in LEVELS[1:]:
            himask = (0xffffffff << (shift + bits)) & 0xffffffff
            sub = keys[(keys & np.uint32(himask)) == np.uint32(prefix)]
            hist = np.bincount(((sub >> np.uint32(shift)) & np.uint32((1 << bits) - 1)).astype(np.int64), minlength=1 << bits)
            ex = np.cumsum(hist) - hist
            hit = np.nonzero((hist > 0) & (ex < krem) & (krem <= ex + hist))[0]
            assert len(hit) == 1
            prefix |= int(hit[0]) << shift
            krem -= int(ex[hit[0]])
        t = np.uint32(prefix)
        less, eq = keys < t, keys == t
        path = 'overflow'
    nless = k - krem
    assert int(less.sum()) == nless and int(eq.sum()) >= krem >= 1
    return np.concatenate([np.nonzero(less)[0], np.nonzero(eq)[0][:krem]]).astype(np.int64), path


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
def select_ks(dist, keys):
    """k in {1, the tie cut, min(8192, plane), plane - 1}"""
    plane = len(keys)
    ks = {1, PC.tie_cut(dist, keys), min(8192, plane), plane - 1}
    return sorted(k for k in ks if k is not None and 1 <= k <= plane)


BOUNDARY_PLANE = 40003       # odd, so that the second and third image of a batch start off a 16-byte boundary
BOUNDARY_BIN_V = 7           # value of bits 23..19 in the threshold bin


def boundary_keys(n_cand, seed=0):
    """the 'byte2' construction (BYTE_BASE with bits 23..16 drawn at random: 32 bins of the leading digit, 3 bits inside a
    bin) with exactly n_cand keys in the bin BOUNDARY_BIN_V, and a k whose k-th key lies in that bin and cuts a tied group"""
    rng = np.random.default_rng([seed, n_cand])
    plane = BOUNDARY_PLANE
    hi = rng.integers(0, 31, plane)
    hi = np.where(hi >= BOUNDARY_BIN_V, hi + 1, hi)            # every 5-bit value but BOUNDARY_BIN_V
    where = rng.choice(plane, size=n_cand, replace=False)
    hi[where] = BOUNDARY_BIN_V
    v = ((hi << 3) | rng.integers(0, 8, plane)).astype(np.uint32)
    keys = ((PC.BYTE_BASE & ~(0xff << 16)) | (v << np.uint32(16))).astype(np.uint32)
    k = int((hi < BOUNDARY_BIN_V).sum()) + n_cand // 2
    return keys, k


MIXED_PLANES = (16384, 530437)
MIXED_DISTS = ('random', 'all_equal', 'byte3')      # the middle image overflows, its neighbours do not


def mixed_batch(plane):
    return np.stack([PC.topk_keys(d, plane, seed=3 + i) for i, d in enumerate(MIXED_DISTS)])


# merge: (H, W) x C x max_ids; N = 3 passed as a view that starts one image into a larger tensor
MERGE_SHAPES = [(5, 7), (33, 31), (64, 64)]
MERGE_CLASSES = (1, 3)
MERGE_MAX_IDS = (0, 300)
MERGE_N = 3


def merge_input(H, W, C, max_ids, seed=0):
    """sem (N + 1, C, H, W) float32 probabilities and cells (N + 1, H, W) int32 (the test passes [1:]): ids in blocks of 4 x 6
    pixels from 0 (no instance) to max_ids + 40 (above the table: treated as none), exact ties between the class planes, and
    one class that is rare in image 1 and frequent in image 2 so that stuff_area falls on both sides of a class count"""
    rng = np.random.default_rng([seed, H, W, C, max_ids])
    N = MERGE_N + 1
    sem = rng.random((N, C, H, W)).astype(np.float32)
    if C > 1:
        sem[:, 1][sem[:, 0] > 0.8] = sem[:, 0][sem[:, 0] > 0.8]      # ties between planes 0 and 1: the lower class wins
        sem[2, C - 1] *= 0.05                                         # class C-1 nearly absent in the view's image 1
        sem[3, C - 1] += 0.5                                          # and dominant in its image 2
    blocks = rng.integers(0, max_ids + 41, (N, -(-H // 4), -(-W // 6)))
    blocks[rng.random(blocks.shape) < 0.3] = 0
    cells = np.repeat(np.repeat(blocks, 4, axis=1), 6, axis=2)[:, :H, :W].astype(np.int32)
    return sem, np.ascontiguousarray(cells)
