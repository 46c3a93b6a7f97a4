"""Inputs, reference and a numpy emulation for the slab-by-slab connected components (tests/test_components_case_host.py,
tests/test_gpu_label_components.py).  Everything is integer: every comparison is exact.

* reference:  ``oracle.sparse.label_nd`` -- scipy.ndimage.label per value with the full structure, the components numbered in
              raster order of their first elements (skimage.measure.label's documented behaviour, restated);
* emulation:  ``slab_components``: the algorithm of ``labels.label_components`` in numpy -- ``label_nd`` per slab, provisional ids
              offset by a running base, unions across every seam over the 9 neighbours of equal value with the smaller id as
              root, the roots ranked in id order, a LUT per slab.  ``defect=`` plants one mistake, so that the tests can show that
              the cases tell a wrong implementation from a right one.
* cases:      ``cases()``: name -> array; no volume larger than 12 x 16 x 24 (the capacity case, 16 x 32 x 32, and the 40 x 56
              image apart)."""
import numpy as np

from oracle import sparse as osparse

SLABS = (1, 2, 3, 5)      # and the whole depth
DEFECTS = ('no_diagonals', 'no_value_test', 'local_order', 'no_base', 'stale_halo')


def reference(arr):
    return osparse.label_nd(np.asarray(arr)).astype(np.int32)


def as_volume(arr):
    """an image (R, W) as the slab stream sees it: R slices of one row"""
    arr = np.asarray(arr)
    return arr.reshape(arr.shape[0], 1, arr.shape[1]) if arr.ndim == 2 else arr


def seam_unions(pv, pid, cv, cid, base_prev, base_cur, diagonals=True, value_test=True, shortcut=False):
    """the pairs (a, b) of provisional ids that the seam between two slices unites: emp_ccl_seam restated.  ``shortcut``: as the
    kernel does it, a voxel whose partner straight below matches issues that union only"""
    H, W = cv.shape
    pairs = []
    for y, x in zip(*np.nonzero(cid)):
        if shortcut and pid[y, x] != 0 and pv[y, x] == cv[y, x]:
            pairs.append((base_cur + int(cid[y, x]), base_prev + int(pid[y, x])))
            continue
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if not diagonals and (dy or dx):
                    continue
                yy, xx = y + dy, x + dx
                if not (0 <= yy < H and 0 <= xx < W) or pid[yy, xx] == 0:
                    continue
                if value_test and pv[yy, xx] != cv[y, x]:
                    continue
                pairs.append((base_cur + int(cid[y, x]), base_prev + int(pid[yy, xx])))
    return pairs


class Forest:
    """union-find over ids 1..G; ``smallest_root=False`` makes the larger id the root of a union"""

    def __init__(self, smallest_root=True):
        self.parent = [0]
        self.smallest_root = smallest_root

    def extend(self, k):
        self.parent += range(len(self.parent), len(self.parent) + k)

    def find(self, a):
        while self.parent[a] != a:
            a = self.parent[a]
        return a

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return
        if (a < b) == self.smallest_root:
            a, b = b, a
        self.parent[a] = b      # a > b: the smaller id is the root (the defect: the larger one)

    def lut(self):
        """(lut, count): lut[g] = the 1-based rank of g's root among the roots in id order; lut[0] = 0"""
        G = len(self.parent) - 1
        roots = [g for g in range(1, G + 1) if self.parent[g] == g]
        rank = {r: i for i, r in enumerate(roots, start=1)}
        return np.asarray([0] + [rank[self.find(g)] for g in range(1, G + 1)], np.int64), len(roots)


def slab_components(arr, slab, defect=None):
    """the slab algorithm on the host -> (components int32, count)"""
    assert defect is None or defect in DEFECTS
    vol = as_volume(arr)
    D = vol.shape[0]
    bounds = [(z, min(D, z + slab)) for z in range(0, D, slab)]
    forest = Forest(smallest_root=defect != 'local_order')
    local, bases, G = [], [], 0
    halo_vals = halo_ids = None
    for k, (z0, z1) in enumerate(bounds):
        ids = osparse.label_nd(vol[z0:z1])
        K = int(ids.max()) if ids.size else 0
        forest.extend(K)
        if k > 0:
            for a, b in seam_unions(halo_vals, halo_ids, vol[z0], ids[0], bases[-1], G, diagonals=defect != 'no_diagonals',
                                    value_test=defect != 'no_value_test'):
                forest.union(a, b)
        local.append(ids)
        bases.append(G)
        G += K
        if defect != 'stale_halo' or k == 0:      # the defect keeps the first slab's last slice for every seam
            halo_vals, halo_ids = vol[z1 - 1], ids[-1]
    lut, count = forest.lut()
    out = np.zeros(vol.shape, np.int32)
    for (z0, z1), ids, base in zip(bounds, local, bases):
        out[z0:z1] = np.where(ids > 0, lut[(0 if defect == 'no_base' else base) + ids], 0)
    return out.reshape(np.asarray(arr).shape), count


# ----------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------
def random_volume(seed, shape=(7, 6, 9), values=3, density=0.45):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, values + 1, shape) * (rng.random(shape) < density)).astype(np.int32)


def capacity_volume():
    """16 x 32 x 32 with isolated voxels on a lattice of pitch 2 in every second slice and more beside: thousands of components,
    so that a union-find that starts with a few entries doubles many times"""
    v = np.zeros((16, 32, 32), np.int32)
    v[::2, ::2, ::2] = 1
    v[1::4, 1::4, :] = 2      # rods that join nothing of value 1
    return v


def seam_pairs(shape=(2, 5, 7)):
    """per seam offset (dy, dx) two-voxel volumes: one voxel in slice 1, its partner in slice 0 at the offset, for the voxel in the
    interior, in every corner and on every edge of the slice as far as the partner stays inside"""
    _, H, W = shape
    spots = [(y, x) for y in (0, H // 2, H - 1) for x in (0, W // 2, W - 1)]
    out = {}
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            for y, x in spots:
                if 0 <= y + dy < H and 0 <= x + dx < W:
                    v = np.zeros(shape, np.int32)
                    v[1, y, x] = v[0, y + dy, x + dx] = 5
                    out[f'pair{dy:+d}{dx:+d}_at{y}_{x}'] = v
    return out


def touching_values():
    """equal and unequal values face to face, edge to edge and corner to corner across the seam z = 1 | 2"""
    v = np.zeros((4, 6, 12), np.int32)
    v[1, 1, 1], v[2, 1, 1] = 3, 3      # equal, straight: one component
    v[1, 1, 4], v[2, 1, 4] = 3, 4      # unequal, straight: two
    v[1, 3, 7], v[2, 4, 8] = 2, 2      # equal, corner to corner: one
    v[1, 3, 10], v[2, 4, 11] = 2, 1      # unequal, corner to corner: two
    v[0:2, 5, 0:3] = 6
    v[2:4, 5, 2:5] = 7      # two plates that overlap in x: never one
    return v


def u_shape():
    """two arms that start in slice 0 and meet only in the last slice: two local components of the early slabs, one in the end"""
    v = np.zeros((7, 5, 9), np.int32)
    v[:, 2, 1] = 4
    v[:, 2, 7] = 4
    v[6, 2, 1:8] = 4
    v[0, 0, 0] = 4      # and a piece of the same value that stays apart
    return v


def serpent():
    """one component that winds through every slice several times: it leaves a slab and comes back, and every seam has unions that
    only a chain through later slabs completes"""
    D, H, W = 9, 7, 11
    v = np.zeros((D, H, W), np.int32)
    for i, x in enumerate(range(0, W, 2)):
        v[:, 3, x] = 9
        v[D - 1 if i % 2 == 0 else 0, 3, x:min(W, x + 3)] = 9
    v[4, 0, :] = 9      # a bar of the same value that touches nothing
    return v


def late_first_voxel():
    """numbering: component A starts in slice 0 at a late raster position, B starts earlier in raster order but is joined to its
    first voxel only through slice 2, and C lies in between"""
    v = np.zeros((4, 6, 8), np.int32)
    v[0, 4, 6] = 1      # A
    v[0, 1, 1] = 2      # B's first voxel
    v[1, 1, 1] = 2
    v[2, 1, 1:6] = 2
    v[1, 1, 5] = 2      # in slab 1 of slab size 1 a piece of its own with a higher local number than C's
    v[1, 0, 3] = 3      # C: between B's two pieces in raster order of slice 1
    v[3, 5, 0] = 1
    return v


def background_slab():
    v = random_volume(11, (9, 6, 9))
    v[3:6] = 0
    return v


def border_pieces():
    """for clear_border: label 5 touches a face only in a later slab than the one it starts in; label 6 has one border piece and
    one interior piece; label 7 is interior"""
    v = np.zeros((10, 12, 14), np.uint16)
    v[2:10, 5, 5] = 5      # starts inside, runs to the last slice
    v[0:2, 1:3, 1:3] = 6      # at a face
    v[4:6, 7:9, 8:10] = 6      # inside: stays, so label 6 is not removed
    v[3:5, 2:4, 9:12] = 7
    v[6, 10, 1:13] = 8      # inside
    v[7, 11, 6] = 8      # ... but this voxel of the same component lies on the face y = 11
    return v


def image():
    rng = np.random.default_rng(5)
    return (rng.integers(1, 4, (40, 56)) * (rng.random((40, 56)) < 0.5)).astype(np.int32)


def cases():
    out = {f'random{s}': random_volume(s) for s in range(4)}
    out['random_12x16x24'] = random_volume(9, (12, 16, 24))
    out.update(seam_pairs())
    out.update(touching=touching_values(), u=u_shape(), serpent=serpent(), late=late_first_voxel(), background_slab=background_slab(),
               empty=np.zeros((5, 4, 6), np.int32), full=np.full((5, 4, 6), 3, np.int32), border=border_pieces().astype(np.int32),
               image=image())
    return out


_REF = {}


def cached_reference(name, arr):
    """the reference of a named case, computed once and handed out read-only"""
    if name not in _REF:
        ref = reference(arr)
        ref.setflags(write=False)
        _REF[name] = ref
    return _REF[name]
