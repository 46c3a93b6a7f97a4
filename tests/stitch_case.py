"""Inputs and references of the stitching kernels' tests (tests/test_stitch_case_host.py, tests/test_gpu_stitch_kernels.py):
csrc/sparse.hip's connected components, run extraction, run fills and cross morphology, at the sizes where their chunk scans take
a second pass and their capped grids take a second step.  numpy / scipy only; everything is integer, every comparison exact.

* components: ``oracle.sparse.label_nd`` (scipy.ndimage.label per value + raster renumbering, pinned in test_oracle_sparse.py);
  for the exhaustive batches ``components_batch`` below (min-index propagation over equal-valued 8-neighbours)
* runs:       on the raveled array, a start is ``f != 0 and f != f_prev``, an end is ``f != 0 and f != f_next``
* fill:       index arrays built with np.repeat, assigned instance after instance (later instances overwrite)
* morphology: scipy.ndimage.grey_erosion / grey_dilation with the 3-D cross, mode 'reflect' (as oracle.sparse.erode / dilate)

The generators are seeded and return int64 arrays."""
import numpy as np
from scipy import ndimage as ndi

i64 = np.int64
CHUNK = 2048                 # pixels per chunk of the two chunk scans (sparse.hip)
SCAN_PASS = 256 * CHUNK      # first pixel index whose chunk is scanned in a second pass (524 288)
GRID_CAP = 4096 * 256        # first element index reached by the second step of a capped grid-stride loop (1 048 576)
DIV = 1000                   # label divisor of the two-class maps: class 1 = [1000, 2000), class 2 = [2000, 3000)
TWO_CLASS = (1001, 1002, 1003, 2001, 2002)


# ----------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------
def plant(arr, lo, count, value):
    """``count`` isolated elements of ``value`` with raveled index >= lo, in place: each sits in the middle of a cleared 3^n
    neighbourhood on one row (rows are the last axis) that lies entirely behind ``lo``, three columns apart."""
    w = arr.shape[-1]
    rows = arr.reshape(-1, w)
    y = -(-int(lo) // w) + 1
    assert 3 * count <= w + 1 and y + 1 < rows.shape[0], 'no room for the planted elements'
    lead = arr.shape[:-1]
    cy = np.unravel_index(y, lead)
    for k in range(count):
        x = 3 * k + 1 if 3 * k + 1 < w else w - 1
        box = tuple(slice(max(0, c - 1), c + 2) for c in cy) + (slice(max(0, x - 1), x + 2),)
        arr[box] = 0
        arr[cy + (x,)] = value
    return arr


def blobs(shape, n, holes, seed=0, values=TWO_CLASS, planted=None):
    """n random boxes (2-D or 3-D) of a few distinct ids, so that same-id pieces touch and split, with a fraction ``holes`` of
    the elements cleared (the _label_image / _label_volume of test_gpu_sparse.py).  ``planted = (lo, count)``: ``count``
    isolated elements of values[0] with raveled index >= lo (see plant)."""
    rng = np.random.default_rng(seed)
    out = np.zeros(shape, i64)
    div = (2,) + (3,) * (len(shape) - 1) if len(shape) == 3 else (3,) * len(shape)
    for _ in range(n):
        at = [int(rng.integers(0, s)) for s in shape]
        ext = [int(rng.integers(1, s // d + 2)) for s, d in zip(shape, div)]
        out[tuple(slice(a, a + e) for a, e in zip(at, ext))] = values[int(rng.integers(0, len(values)))]
    out[rng.random(shape) < holes] = 0
    if planted is not None:
        plant(out, planted[0], planted[1], values[0])
    return out


def noise(shape, values=(0, 1, 2), seed=0, p=None, planted=None):
    """i.i.d. elements of ``values`` (probabilities ``p``): the percolation regime, thousands of ragged components"""
    rng = np.random.default_rng(seed)
    out = np.asarray(values, i64)[rng.choice(len(values), size=shape, p=p)]
    if planted is not None:
        plant(out, planted[0], planted[1], [v for v in values if v != 0][0])
    return out


def serpentine(H, W):
    """one one-pixel-wide path: every other row full, joined alternately at the right and the left end"""
    a = np.zeros((H, W), i64)
    a[0::2] = 1
    for y in range(1, H, 2):
        a[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    return a


def spiral(H, W):
    """one one-pixel-wide rectangular spiral from the top-left corner inwards, one empty pixel between its arms"""
    a = np.zeros((H, W), i64)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = 1

    def free(yy, xx, ddy, ddx):
        ny, nx = yy + ddy, xx + ddx
        if not (0 <= ny < H and 0 <= nx < W) or a[ny, nx]:
            return False
        by, bx = ny + ddy, nx + ddx
        return not (0 <= by < H and 0 <= bx < W and a[by, bx])

    while True:
        if not free(y, x, dy, dx):
            dy, dx = dx, -dy                       # turn right
            if not free(y, x, dy, dx):
                return a
        y, x = y + dy, x + dx
        a[y, x] = 1


def two_spirals(H, W):
    """the spiral (label 1) and the gap between its arms (label 2): two interleaved spirals that touch all along and must stay
    two components"""
    return np.where(spiral(H, W) == 1, 1, 2).astype(i64)


def comb(H, W):
    """one-pixel teeth in every other column that meet only in the spine, the LAST row: each tooth starts as a component of
    its own in row 0"""
    a = np.zeros((H, W), i64)
    a[:, 0::2] = 1
    a[H - 1] = 1
    return a


def staircase(H, W, amp=16):
    """one pixel per row, its column a triangle wave of amplitude ``amp``: diagonal links only, up-left and up-right in turn"""
    assert W > 1
    amp = min(amp, W - 1)
    y = np.arange(H)
    t = y % (2 * amp)
    a = np.zeros((H, W), i64)
    a[y, np.where(t <= amp, t, 2 * amp - t)] = 1
    return a


ADVERSARIAL = (('serpentine', serpentine, 1), ('spiral', spiral, 1), ('comb', comb, 1), ('two_spirals', two_spirals, 2),
               ('staircase', staircase, 1))


def vertical_line(H, W):
    a = np.zeros((H, W), i64)
    a[:, W // 2] = 1
    return a


def with_junk(img, lo, hi, seed=0):
    """an int64 copy whose background holds values that the range [lo, hi) must read as background: negative ones, other classes,
    values >= 2^31 and values whose low 32 bits lie inside the range"""
    rng = np.random.default_rng(seed)
    junk = np.array([0, 0, 0, -5, -lo - 1, lo - 1, hi, hi + 7, (1 << 31) + lo + 1, (1 << 32) + lo + 1, (1 << 40) + lo + 2], i64)
    out = np.array(img, i64)
    bg = out == 0
    out[bg] = junk[rng.integers(0, len(junk), size=int(bg.sum()))]
    return out


# ----------------------------------------------------------------------------
# exhaustive sets
# ----------------------------------------------------------------------------
def _digits(n_images, base, cells):
    k = np.arange(n_images, dtype=i64)[:, None]
    return (k // base ** np.arange(cells, dtype=i64)[None, :]) % base


def all_3x3():
    """all 3^9 images over {0, 1, 2}: every 8-neighbourhood of two labels and background"""
    return _digits(3 ** 9, 3, 9).reshape(-1, 3, 3)


def all_binary_3x5():
    """all 2^15 binary 3 x 5 images: every pixel of the middle row sees up, up-left, up-right, left and right with a further
    column on either side"""
    return _digits(2 ** 15, 2, 15).reshape(-1, 3, 5)


def mosaic_2x2x2():
    """all 3^8 volumes over {0, 1, 2} in one (2, 242, 242) volume, 81 x 81 tiles with one zero voxel between neighbours"""
    cubes = _digits(3 ** 8, 3, 8).reshape(81, 81, 2, 2, 2)
    out = np.zeros((2, 81 * 3, 81 * 3), i64)
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                out[dz, dy::3, dx::3] = cubes[:, :, dz, dy, dx]
    return np.ascontiguousarray(out[:, :-1, :-1])


# ----------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------
def components_batch(imgs):
    """(N, H, W) -> (components (N, H, W), counts (N,)): every non-zero pixel starts as its linear index and takes the minimum
    over its equal-valued 8-neighbours until nothing changes; the fixed points are numbered in raster order"""
    imgs = np.asarray(imgs, i64)
    N, H, W = imgs.shape
    big = H * W
    own = np.broadcast_to(np.arange(big, dtype=i64).reshape(H, W), imgs.shape)
    live = imgs != 0
    idx = np.where(live, own, big)
    vpad = np.pad(imgs, ((0, 0), (1, 1), (1, 1)), constant_values=0)
    while True:
        ipad = np.pad(idx, ((0, 0), (1, 1), (1, 1)), constant_values=big)
        new = idx
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if dy == 1 and dx == 1:
                    continue
                same = live & (vpad[:, dy:dy + H, dx:dx + W] == imgs)
                new = np.where(same, np.minimum(new, ipad[:, dy:dy + H, dx:dx + W]), new)
        if np.array_equal(new, idx):
            break
        idx = new
    root = (live & (idx == own)).reshape(N, big)
    rank = np.cumsum(root, axis=1)
    flat = np.minimum(idx.reshape(N, big), big - 1)
    out = np.where(live.reshape(N, big), np.take_along_axis(rank, flat, axis=1), 0)
    return out.reshape(N, H, W).astype(i64), root.sum(axis=1).astype(i64)


def runs_ref(img):
    """(n, 3) int64 {start, length, label} of the raveled array, in raster order"""
    f = np.asarray(img, i64).reshape(-1)
    prev = np.concatenate([[0], f[:-1]])
    nxt = np.concatenate([f[1:], [0]])
    s = np.flatnonzero((f != 0) & (f != prev))
    e = np.flatnonzero((f != 0) & (f != nxt))
    return np.stack([s, e + 1 - s, f[s]], axis=1).astype(i64).reshape(-1, 3)


def in_range(img, lo, hi):
    img = np.asarray(img, i64)
    return np.where((img >= lo) & (img < hi), img, 0)


def run_indices(starts, runs):
    starts, runs = np.asarray(starts, i64), np.asarray(runs, i64)
    first = np.cumsum(runs) - runs
    return np.repeat(starts - first, runs) + np.arange(int(runs.sum()), dtype=i64)


def fill_ref(volume, instances):
    """numpy_fill_instances without the loop over runs: instance after instance, later ones overwrite"""
    flat = volume.reshape(-1)
    for iid, a in instances.items():
        flat[run_indices(a['starts'], a['runs'])] = iid
    return volume


def cross_morph_ref(vol, op):
    """op 0: grey erosion, op 1: grey dilation with the 3-D cross, border mode 'reflect'"""
    fn = ndi.grey_dilation if op else ndi.grey_erosion
    return fn(np.asarray(vol, i64), footprint=ndi.generate_binary_structure(3, 1), mode='reflect')


def first_indices(components):
    """raveled index of each component's first element, in label order 1..K"""
    flat = np.asarray(components).reshape(-1)
    ids, first = np.unique(flat, return_index=True)
    return first[ids != 0]


def force_connected_ref(pan, thing_list, label_divisor):
    """oracle.sparse.force_connected_pan with its per-pixel union-find replaced by oracle.sparse.label_nd (the same
    skimage.measure.label statement, vectorised); the two are compared in test_stitch_case_host.py"""
    from oracle import sparse as osp
    pan = np.array(pan, i64)
    for label in thing_list:
        lo = label * label_divisor
        cc = osp.label_nd(in_range(pan, lo, lo + label_divisor))
        pan[cc > 0] = cc[cc > 0] + lo
    return pan


def rle_seg_ref(pan, labels, label_divisor, thing_list):
    """oracle.sparse.pan_seg_to_rle_seg (force_connected=True) without its per-pixel and per-label loops: components from
    label_nd, runs from runs_ref, boxes from the pixel coordinates; compared with it in test_stitch_case_host.py"""
    from oracle import sparse as osp
    pan = np.asarray(pan, i64)
    H, W = pan.shape
    seg = {}
    for label in labels:
        lo = label * label_divisor
        inst = in_range(pan, lo, lo + label_divisor)
        if label in thing_list:
            inst = osp.label_nd(inst)
            inst[inst > 0] += lo
        r = runs_ref(inst)
        r = r[np.argsort(r[:, 2], kind='stable')]
        ys, xs = np.nonzero(inst)
        v = inst[ys, xs]
        ids = np.unique(v)
        k = np.searchsorted(ids, v)
        lo_y, lo_x = np.full(len(ids), H), np.full(len(ids), W)
        hi_y, hi_x = np.full(len(ids), -1), np.full(len(ids), -1)
        np.minimum.at(lo_y, k, ys), np.minimum.at(lo_x, k, xs), np.maximum.at(hi_y, k, ys), np.maximum.at(hi_x, k, xs)
        cut = np.searchsorted(r[:, 2], ids, side='left').tolist() + [len(r)]
        seg[label] = {int(i): {'box': (int(lo_y[n]), int(lo_x[n]), int(hi_y[n]) + 1, int(hi_x[n]) + 1),
                               'starts': r[cut[n]:cut[n + 1], 0], 'runs': r[cut[n]:cut[n + 1], 1]}
                      for n, i in enumerate(ids)}
    return seg


# ----------------------------------------------------------------------------
# the cases whose preconditions test_stitch_case_host.py asserts
# ----------------------------------------------------------------------------
def full(shape, value=1001):
    return np.full(shape, value, i64)


SWEEP_2D = ((1, 1), (1, 64), (1, 65), (64, 1), (300, 1), (2, 63), (5, 64), (7, 65), (70, 67), (33, 255), (9, 257), (3, 2049))
SWEEP_3D = ((1, 1, 1), (1, 1, 130), (1, 70, 67), (70, 1, 67), (67, 70, 1), (2, 3, 2049))


def sweep_images(shape):
    """the three images of a geometry-sweep shape: noise, blobs, one label filling the image"""
    seed = shape[0] * 10007 + shape[1]
    return np.stack([noise(shape, (0, 1001, 1002), seed), blobs(shape, 12, 0.15, seed, values=(1001, 1002, 1003)), full(shape)])


def sweep_volumes(shape):
    seed = shape[0] * 10007 + shape[1] * 101 + shape[2]
    return [noise(shape, (0, 1001, 1002), seed), blobs(shape, 14, 0.2, seed, values=(1001, 1002, 1003))]


def multipass_513():
    """(2, 513, 1031): 259 chunks per image (two scan passes); image 0 is densely covered (more than 65 536 runs), image 1
    sparsely (fewer); both have isolated pixels behind SCAN_PASS"""
    shape = (513, 1031)
    return np.stack([blobs(shape, 600, 0.15, 21, planted=(SCAN_PASS, 12)), blobs(shape, 40, 0.15, 22, planted=(SCAN_PASS, 12))])


def multipass_1025():
    """(1, 1025, 1031): 517 chunks (three scan passes), isolated pixels behind GRID_CAP"""
    return blobs((1025, 1031), 160, 0.15, 23, planted=(GRID_CAP, 12))[None]


VOLUME_SHAPE = (5, 461, 467)


def strided_volume():
    """1 076 435 voxels of 3 / 4 / 0 at 35 % / 20 % / 45 %, isolated voxels behind GRID_CAP"""
    return noise(VOLUME_SHAPE, (3, 4, 0), 31, p=(0.35, 0.20, 0.45), planted=(GRID_CAP, 12))


def max_runs_batch():
    """(3, 8, 256) with 2, 3 and 700 runs: max_runs 1 overflows in all images, 4 in one, 1000 in none"""
    out = np.zeros((3, 8 * 256), i64)
    out[0, [5, 900]] = 4
    out[1, [0, 7, 2047]] = 5
    out[2, 0:1400:2] = 6
    return out.reshape(3, 8, 256)


def boundary_runs():
    """(2, 5, 2048) built from runs that start or end exactly at thread (8), chunk (2048) and image boundaries"""
    hw = 5 * CHUNK
    spans = [[(0, 8, 3), (8, 16, 4), (16, 24, 4), (2040, 2048, 5), (2048, 2056, 5), (4093, 4096, 6), (4096, 4100, 7),
              (6143, 6145, 8), (8184, 8192, 9), (8192, 8193, 1), (8199, 8200, 1), (8200, 8208, 2), (hw - 8, hw, 9)],
             [(0, 1, 9), (7, 9, 9), (2047, 2049, 3), (2049, 4096, 4), (4096, 6144, 4), (6144, 6152, 5), (hw - 1, hw, 5)]]
    out = np.zeros((2, hw), i64)
    for n, img in enumerate(spans):
        for a, b, v in img:
            out[n, a:b] = v
    return out.reshape(2, 5, CHUNK)


def fill_runs(n_runs=40000, seed=0):
    """``n_runs`` non-overlapping runs of lengths 1, 63, 64, 65 (and 5000 for every 1000th) with gaps of 0..3 -> (starts, lens,
    vals, size); vals stay below 256 so that every element size holds them"""
    rng = np.random.default_rng(seed)
    lens = np.array([1, 63, 64, 65], i64)[rng.integers(0, 4, size=n_runs)]
    lens[::1000] = 5000
    gaps = rng.integers(0, 4, size=n_runs).astype(i64)
    starts = np.cumsum(lens + gaps) - lens
    vals = rng.integers(1, 256, size=n_runs).astype(i64)
    order = rng.permutation(n_runs)                 # the kernel takes the runs in any order
    return starts[order], lens[order], vals[order], int(starts.max() + 5000 + 3)


def overlapping_instances(shape, n_runs=10000, seed=0):
    """four instances of ``n_runs`` runs each over the same volume: they overlap each other heavily"""
    rng = np.random.default_rng(seed)
    size = int(np.prod(shape))
    inst = {}
    for k in (7, 3, 12, 5):
        s = np.sort(rng.choice(size - 200, size=n_runs, replace=False)).astype(i64)
        r = rng.integers(1, 200, size=n_runs).astype(i64)
        e = np.minimum(s + r, np.append(s[1:], size))
        inst[k] = {'box': (0, 0, 0) + tuple(shape), 'starts': s, 'runs': e - s}
    return inst
