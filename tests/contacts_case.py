"""The statements the Contact Labels tests compare against, in numpy (tests/test_contacts_case_host.py,
tests/test_gpu_label_contacts.py).  Everything raw is an integer: every comparison is exact.

* want_contacts:           per half-direction one shifted compare of the array against itself, the differing pairs keyed
                           min << 32 | max, np.unique and np.add.at into the 13 (an image: 4) columns
* want_contacts_per_pair:  the definition pair by pair with boolean masks, for tiny volumes
* model_contacts:          the same table the way the kernel forms it -- every pair from its later voxel in the raveled slab, a
                           halo slice below a slab -- with one rule at a time broken on request, to show that the cases of the
                           device test notice each of them
* face_size / crofton:     the derived quantities restated
There is no counterpart in the reference plugin and skimage (skimage.graph.RAG) is not available: nothing is pinned against it."""
import numpy as np

import shape_case as SC

MASK = np.uint64(0xffffffff)


def _pairs_of(vol, d):
    """(p, p + d) for every p with both ends in the array"""
    lo = tuple(slice(max(0, -v), vol.shape[a] - max(0, v)) for a, v in enumerate(d))
    hi = tuple(slice(max(0, v), vol.shape[a] - max(0, -v)) for a, v in enumerate(d))
    return vol[lo], vol[hi]


def _table(keys, cols, ndirs):
    """rows sorted by key from one (key, column) per counted voxel pair"""
    uniq, inv = np.unique(keys, return_inverse=True)
    pairs = np.zeros((len(uniq), ndirs), np.int64)
    np.add.at(pairs, (inv.reshape(-1), cols), 1)
    return {'a': (uniq >> np.uint64(32)).astype(np.int64), 'b': (uniq & MASK).astype(np.int64), 'pairs': pairs}


def want_contacts(vol, background=False):
    """dict(a, b, pairs) of one array of non-negative labels below 2^32, rows sorted by (a, b)"""
    u = np.asarray(vol).astype(np.uint64)
    dirs = SC.half_dirs(u.ndim)
    keys, cols = [], []
    for k, d in enumerate(dirs):
        p, q = _pairs_of(u, d)
        m = p != q
        if not background:
            m &= (p != 0) & (q != 0)
        p, q = p[m], q[m]
        keys.append((np.minimum(p, q) << np.uint64(32)) | np.maximum(p, q))
        cols.append(np.full(len(p), k, np.int64))
    return _table(np.concatenate(keys), np.concatenate(cols), len(dirs))


def want_contacts_per_pair(vol, background=False):
    """the definition, a pass per pair of labels and direction"""
    vol = np.asarray(vol)
    dirs = SC.half_dirs(vol.ndim)
    labels = [int(v) for v in np.unique(vol) if background or v != 0]
    rows = []
    for i, a in enumerate(labels):
        for b in labels[i + 1:]:
            n = []
            for d in dirs:
                p, q = _pairs_of(vol, d)
                n.append(int(np.count_nonzero(((p == a) & (q == b)) | ((p == b) & (q == a)))))
            if sum(n) > 0:
                rows.append((a, b, n))
    return {'a': np.array([r[0] for r in rows], np.int64), 'b': np.array([r[1] for r in rows], np.int64),
            'pairs': np.array([r[2] for r in rows], np.int64).reshape(len(rows), len(dirs))}


# ----------------------------------------------------------------------------
# the kernel's rules, one at a time breakable
# ----------------------------------------------------------------------------
DEFECTS = ('diagonal_wraps_into_neighbouring_row', 'seam_pairs_dropped', 'seam_pairs_counted_twice', 'stale_halo', 'key_not_symmetrised',
           'background_pairs_entered')


def model_contacts(vol, background=False, slab=None, defect=None):
    """want_contacts of a 3-D array by the kernel's rules; ``defect``: one of DEFECTS, or None"""
    assert defect is None or defect in DEFECTS
    u = np.asarray(vol).astype(np.uint64)
    D, H, W = u.shape
    HW = H * W
    slab = D if slab is None else slab
    dirs = SC.half_dirs(3)
    guard = np.zeros(W + 2, np.uint64)
    keys, cols = [], []
    for z0 in range(0, D, slab):
        z1 = min(D, z0 + slab)
        if z0 == 0:
            halo = np.zeros(HW, np.uint64)      # there is no slice below
        elif defect == 'stale_halo':      # the slice that was there a slab ago
            halo = u[z0 - 1 - slab].reshape(-1) if z0 - 1 - slab >= 0 else np.zeros(HW, np.uint64)
        else:
            halo = u[z0 - 1].reshape(-1)
        own = u[z0:z1].reshape(-1)
        buf = np.concatenate([guard, halo, own, guard])      # the raveled slab with the slice below it in front
        base = len(guard) + HW
        i = np.arange(own.size)
        z, y, x = z0 + i // HW, i // W % H, i % W
        for k, (dz, dy, dx) in enumerate(dirs):
            # the voxel is the LATER end: its partner is p - d, read from the raveled slab, counted where its coordinates lie in the array
            inside = (y - dy >= 0) & (y - dy < H) & (z - dz >= 0)
            if defect != 'diagonal_wraps_into_neighbouring_row':
                inside &= (x - dx >= 0) & (x - dx < W)
            nb = buf[base + i - dz * HW - dy * W - dx]
            m = inside & (nb != own)
            if not background and defect != 'background_pairs_entered':
                m &= (nb != 0) & (own != 0)
            seam = (z == z0) & (dz == 1) & (z0 > 0)      # the pairs across the slab's lower border: from the halo, by this slab only
            if defect == 'seam_pairs_dropped':
                m &= ~seam
            reps = 2 if defect == 'seam_pairs_counted_twice' else 1      # ... and once more by the slab below, from its side
            for sel in [m] + [m & seam] * (reps - 1):
                p, q = own[sel], nb[sel]
                if defect == 'key_not_symmetrised':
                    keys.append((p << np.uint64(32)) | q)
                else:
                    keys.append((np.minimum(p, q) << np.uint64(32)) | np.maximum(p, q))
                cols.append(np.full(len(p), k, np.int64))
    return _table(np.concatenate(keys), np.concatenate(cols), 13)


def same(got, want):
    return all(got[f].shape == want[f].shape and np.array_equal(got[f], want[f]) for f in ('a', 'b', 'pairs'))


# ----------------------------------------------------------------------------
# the derived quantities, restated
# ----------------------------------------------------------------------------
def face_size(pairs, spacing):
    """the pairs along the axes (z, y, x order) times the physical size of the voxel face between them"""
    pairs = np.asarray(pairs, np.float64)
    nd = 3 if pairs.shape[1] == 13 else 2
    sp = np.asarray(spacing, np.float64)
    return sum(pairs[:, c] * np.prod(sp) / sp[ax] for ax, c in enumerate(SC.AXIS_COLUMNS[nd]))


def crofton(pairs, spacing):
    """2 sum c N v / |d| (an image: pi / 2 in place of 2): shape_case's estimator on the pair counts"""
    return SC.crofton(pairs, spacing)


def plane_ratio(normal, spacing=(1, 1, 1)):
    """What the estimator gives for a unit area of an unbounded plane with this normal: the lattice lines of direction d_k, one per
    v / |d_k| of perpendicular area, cross it |n . u_k| |d_k| / v times, so the estimate is 2 sum_k c_k |n . u_k| -- 1 where the
    weighted directions average |cos| as the sphere does.  It depends on the direction weights only."""
    sp = np.asarray(spacing, np.float64)
    n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    d = np.array(SC.half_dirs(3), np.float64) * sp
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    return float(2.0 * np.sum(SC.weights(sp, 3) * np.abs(u @ n)))


# ----------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------
def all_distinct(shape, dtype=np.uint32):
    """every voxel another label, 1 .. size in a fixed shuffled order: every pair in the array is a row of its own"""
    n = int(np.prod(shape))
    return (1 + np.random.default_rng(5).permutation(n)).astype(dtype).reshape(shape)


def distinct_rows(shape):
    """the number of pairs in an array: sum_k prod_i (n_i - |d_k,i|)"""
    return sum(int(np.prod([s - abs(v) for s, v in zip(shape, d)])) for d in SC.half_dirs(len(shape)))


def half_spaces(shape=(6, 5, 7), c=3):
    """label 1 below z = c, label 2 from there on"""
    vol = np.ones(shape, np.uint8)
    vol[c:] = 2
    return vol


def diagonal_halves(n=48):
    """two labels split by the plane through the centre of an n^3 cube with normal (1, 1, 1)"""
    z, y, x = np.indices((n, n, n))
    return (1 + (2 * (z + y + x) > 3 * (n - 1))).astype(np.uint8)


def hexagon_area(n):
    """of the section of an n^3 cube by the plane through its centre with normal (1, 1, 1): a regular hexagon of side n / sqrt 2"""
    return 3.0 * np.sqrt(3.0) / 4.0 * n * n


def check(m, want, shape):
    """a LabelContacts against want_contacts' dict"""
    assert m.shape == tuple(shape)
    for f in ('a', 'b', 'pairs'):
        got = getattr(m, f)
        assert got.shape == want[f].shape and np.array_equal(got, want[f]), (f, got[got != want[f]][:8], want[f][got != want[f]][:8])
    assert np.array_equal(m.counts, want['pairs'].sum(axis=1)) and (m.counts > 0).all()
