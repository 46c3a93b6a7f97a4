"""The statements the Shape Labels tests compare against, in numpy (tests/test_shape_case_host.py, tests/test_gpu_shape_labels.py).
Everything raw is an integer: every comparison is exact.

* intercepts / euler_closed / euler_open:  the definitions, per mask: shifted compares on the padded mask, and the cell counts of
                    the cubical complex (V - E + F - C) by OR (closed cubes: full connectivity) and by AND (face connectivity)
* want_shapes:      the same per label of a whole array at once: shifted compares with np.bincount on both labels of a pair, and
                    per kind of cell the sorted stack of the voxels that touch it, its distinct non-zero values credited
* model_shapes:     the same table the way the kernel forms it -- every pair from its later voxel in the raveled slab, a halo
                    slice below a slab, the border as a closed form per voxel, one vertex per voxel and the vertices of the high
                    faces from the voxels at the last index -- with one rule at a time broken on request, to show that the cases
                    of the device test notice each of them
* crofton / weights: the derived quantities restated (scipy's spherical Voronoi cells; a quadrature on the sphere to check them)
* the case generators of the device test"""
import itertools

import numpy as np

import labels_case as LC


def half_dirs(nd):
    """first non-zero component +1, lexicographic"""
    return [d for d in itertools.product((-1, 0, 1), repeat=nd) if any(d) and next(v for v in d if v) > 0]


AXIS_COLUMNS = {3: (8, 2, 0), 2: (2, 0)}      # the columns of the axis directions, in the order of measure_labels' faces


# ----------------------------------------------------------------------------
# the definitions, per mask
# ----------------------------------------------------------------------------
def intercepts(mask, d, border_faces=True):
    """#{p in M : p + d not in M} + #{p in M : p - d not in M}; without border_faces only pairs inside the array count"""
    mask = np.asarray(mask, dtype=bool)
    if border_faces:
        m = np.pad(mask, 1)
        ax = tuple(range(m.ndim))
        return sum(int(np.count_nonzero(m & ~np.roll(m, tuple(-s * v for v in d), ax))) for s in (1, -1))
    lo = tuple(slice(max(0, -v), mask.shape[a] - max(0, v)) for a, v in enumerate(d))      # p with p + d inside
    hi = tuple(slice(max(0, v), mask.shape[a] - max(0, -v)) for a, v in enumerate(d))      # p + d
    p, q = mask[lo], mask[hi]
    return int(np.count_nonzero(p & ~q)) + int(np.count_nonzero(q & ~p))


def euler_closed(mask):
    """chi of the union of the closed voxel cubes: a cell belongs to the mask if any voxel that touches it does"""
    m = np.pad(np.asarray(mask).astype(bool), 1)
    nd, chi = m.ndim, 0
    for j in range(nd + 1):
        for axes in itertools.combinations(range(nd), j):
            u = m.copy()
            for a in axes:
                u = u | np.roll(u, 1, axis=a)
            chi += (-1) ** (nd - j) * int(np.count_nonzero(u))
    return chi


def euler_open(mask):
    """voxels - face pairs + 2 x 2 quads - 2 x 2 x 2 octets inside the mask"""
    m = np.pad(np.asarray(mask).astype(bool), 1)
    nd, chi = m.ndim, 0
    for j in range(nd + 1):
        for axes in itertools.combinations(range(nd), j):
            u = m.copy()
            for a in axes:
                u = u & np.roll(u, 1, axis=a)
            chi += (-1) ** j * int(np.count_nonzero(u))
    return chi


def want_shapes_per_mask(vol, border_faces=True):
    """the table of one array from the definitions, a pass per label and direction"""
    vol = np.asarray(vol)
    labels = np.unique(vol)
    labels = labels[labels != 0]
    dirs = half_dirs(vol.ndim)
    return {'labels': labels.astype(np.int64), 'areas': np.array([np.count_nonzero(vol == l) for l in labels], np.int64),
            'intercepts': np.array([[intercepts(vol == l, d, border_faces) for d in dirs] for l in labels], np.int64).reshape(len(labels), len(dirs)),
            'euler': np.array([[euler_closed(vol == l), euler_open(vol == l)] for l in labels], np.int64).reshape(len(labels), 2)}


# ----------------------------------------------------------------------------
# the same per label, vectorised
# ----------------------------------------------------------------------------
def _indexed(vol):
    """(labels with 0 in front, the array as indices into them: 0 is the background)"""
    labels, inv = np.unique(vol, return_inverse=True)
    inv = inv.reshape(vol.shape).astype(np.int64)
    if labels[0] != 0:
        labels, inv = np.concatenate([[0], labels]), inv + 1
    return labels, inv


def want_shapes(vol, border_faces=True):
    """dict(labels, areas, intercepts, euler) of one array, labels ascending, background 0 left out"""
    vol = np.asarray(vol)
    nd = vol.ndim
    labels, idx = _indexed(vol)
    k = len(labels)
    dirs = half_dirs(nd)
    icpt = np.zeros((k, len(dirs)), np.int64)
    padded = np.pad(idx, 1, constant_values=-1)      # -1: outside the array
    for j, d in enumerate(dirs):
        lo = tuple(slice(1, -1) if v == 0 else (slice(0, -1) if v > 0 else slice(1, None)) for v in d)
        hi = tuple(slice(1, -1) if v == 0 else (slice(1, None) if v > 0 else slice(0, -1)) for v in d)
        p, q = padded[lo], padded[hi]      # every pair (p, p + d) with at least one end in the array
        differ = p != q
        if not border_faces:
            differ &= (p >= 0) & (q >= 0)
        for side in (p, q):
            icpt[:, j] += np.bincount(side[differ & (side >= 0)], minlength=k)
    euler = np.zeros((k, 2), np.int64)
    m = np.pad(idx, 1)
    for j in range(nd + 1):
        for axes in itertools.combinations(range(nd), j):
            stack = [m]
            for a in axes:
                stack = stack + [np.roll(s, 1, axis=a) for s in stack]
            s = np.sort(np.stack(stack).reshape(len(stack), -1), axis=0)      # the 2^j voxels of every cell
            new = np.concatenate([s[:1] != 0, (s[1:] != s[:-1]) & (s[1:] != 0)])      # its distinct non-zero values
            euler[:, 0] += (-1) ** (nd - j) * np.bincount(s[new], minlength=k)
            whole = (s[0] == s[-1]) & (s[0] != 0)      # all of one label
            euler[:, 1] += (-1) ** j * np.bincount(s[0][whole], minlength=k)
    areas = np.bincount(idx.reshape(-1), minlength=k).astype(np.int64)
    return {'labels': labels[1:].astype(np.int64), 'areas': areas[1:], 'intercepts': icpt[1:], 'euler': euler[1:]}


def want_shapes_per_slice(vol, border_faces=True):
    """the same per image of a stack, with a leading `slices` column: a Python loop of want_shapes"""
    parts = [want_shapes(vol[z], border_faces) for z in range(vol.shape[0])]
    out = {f: np.concatenate([p[f] for p in parts]) for f in parts[0]}
    out['slices'] = np.concatenate([np.full(len(p['labels']), z, np.int64) for z, p in enumerate(parts)])
    return out


# ----------------------------------------------------------------------------
# the kernel's rules, one at a time breakable
# ----------------------------------------------------------------------------
DEFECTS = ('diagonal_wraps_into_neighbouring_row', 'seam_diagonal_pairs_dropped', 'stale_halo', 'high_face_cells_skipped',
           'high_face_cells_in_every_slab', 'one_side_credited', 'euler_across_slices_per_slice')


def vertex_chi(m, nd, closed):
    """What a vertex adds to the Euler number of a label that occupies the voxels m around it: bit t (one bit per axis, the last
    axis lowest) is the voxel vertex - t.  The vertex owns, per subset of the axes, the cell that leads from it towards lower
    indices along them; closed: the cell counts if any voxel that touches it (every axis of the subset set in t) is of the label;
    open: the block that the voxel `all bits set` spans towards higher indices along the subset counts if all of it is."""
    full, chi = (1 << nd) - 1, 0
    for axes in range(full + 1):
        dim = bin(axes).count('1')
        if closed:
            hit = any((m >> t) & 1 for t in range(full + 1) if t & axes == axes)
        else:
            hit = all((m >> t) & 1 for t in range(full + 1) if t | axes == full)
        chi += (-1) ** dim * int(hit)
    return chi


_CHI = {(nd, closed): np.array([vertex_chi(m, nd, closed) for m in range(1 << (1 << nd))], np.int64) for nd in (2, 3) for closed in (True, False)}


def model_shapes(vol, border_faces=True, per_slice=False, slab=None, defect=None):
    """want_shapes (per_slice: want_shapes_per_slice) of a 3-D array by the kernel's rules; ``defect``: one of DEFECTS, or None"""
    vol = np.asarray(vol)
    D, H, W = vol.shape
    assert defect is None or defect in DEFECTS
    labels, idx = _indexed(vol)
    k = len(labels)
    HW = H * W
    slab = D if slab is None else slab
    nkeys = D * k if per_slice else k
    areas = np.zeros(nkeys, np.int64)
    icpt = np.zeros((nkeys, 13), np.int64)
    euler = np.zeros((nkeys, 2), np.int64)
    dirs = half_dirs(3)
    three_d_vertices = not per_slice or defect == 'euler_across_slices_per_slice'
    guard = np.zeros(W + 2, np.int64)
    for z0 in range(0, D, slab):
        z1 = min(D, z0 + slab)
        if z0 == 0 or (per_slice and not three_d_vertices):
            halo = np.zeros(HW, np.int64)
        elif defect == 'stale_halo':      # the slice that was there a slab ago
            halo = idx[z0 - 1 - slab].reshape(-1) if z0 - 1 - slab >= 0 else np.zeros(HW, np.int64)
        else:
            halo = idx[z0 - 1].reshape(-1)
        own = idx[z0:z1].reshape(-1)
        buf = np.concatenate([guard, halo, own, guard])      # the raveled slab with the slice below it in front
        base = len(guard) + HW
        i = np.arange(own.size)
        z, y, x = z0 + i // HW, i // W % H, i % W
        key = z * k if per_slice else 0

        def neighbour(dz, dy, dx):
            """(inside the array, the index of the label at p - (dz, dy, dx) where inside -- read from the raveled slab)"""
            inside = (y - dy >= 0) & (y - dy < H) & (z - dz >= 0) & (z - dz < D)
            if defect != 'diagonal_wraps_into_neighbouring_row':
                inside &= (x - dx >= 0) & (x - dx < W)
            return inside, buf[base + i - dz * HW - dy * W - dx]

        np.add.at(areas, (key + own)[own != 0], 1)
        for j, (dz, dy, dx) in enumerate(dirs[:4] if per_slice else dirs):
            inside, nb = neighbour(dz, dy, dx)
            differ = inside & (nb != own)
            if defect == 'seam_diagonal_pairs_dropped' and z0 > 0:
                differ &= ~((z == z0) & (dz == 1) & ((dy != 0) | (dx != 0)))
            np.add.at(icpt[:, j], (key + own)[differ & (own != 0)], 1)
            if defect != 'one_side_credited':
                np.add.at(icpt[:, j], (key + nb)[differ & (nb != 0)], 1)
            if border_faces:      # p - d outside, p + d outside: a closed form of p's coordinates
                beyond = (y + dy >= 0) & (y + dy < H) & (z + dz >= 0) & (z + dz < D) & (x + dx >= 0) & (x + dx < W)
                exact = (y - dy >= 0) & (y - dy < H) & (z - dz >= 0) & (z - dz < D) & (x - dx >= 0) & (x - dx < W)
                np.add.at(icpt[:, j], (key + own)[(own != 0) & ~exact], 1)
                np.add.at(icpt[:, j], (key + own)[(own != 0) & ~beyond], 1)
        # vertices: the 8 (per slice: 4) voxels p - t, 0 outside; vertex p + e where p is at the last index of the axes of e
        nd = 3 if three_d_vertices else 2
        o = []
        for t in range(1 << nd):
            tz, ty, tx = (t >> 2) & 1 if nd == 3 else 0, (t >> 1) & 1, t & 1
            inside, nb = neighbour(tz, ty, tx)
            inside = inside & (x - tx >= 0)
            o.append(np.where(inside, nb, 0))
        if defect == 'high_face_cells_in_every_slab':
            last_z = z == z1 - 1
        else:
            last_z = z == D - 1
        last = ((last_z * 4) if nd == 3 else 0) | ((y == H - 1) * 2) | ((x == W - 1) * 1)
        for e in range(1 << nd):
            if e and defect == 'high_face_cells_skipped':
                continue
            sel = (e & last) == e
            val = [np.where(sel, 0 if e & ~t else o[t ^ e], 0) for t in range(1 << nd)]
            for t, L in enumerate(val):
                first = L != 0
                for u in range(t):
                    first &= val[u] != L
                m = sum((val[u] == L).astype(np.int64) << u for u in range(1 << nd))
                for c, closed in enumerate((True, False)):
                    np.add.at(euler[:, c], (key + L)[first], _CHI[(nd, closed)][m[first]])
    rows = np.flatnonzero(areas)
    rows = rows[rows % k != 0]
    out = {'labels': labels[rows % k].astype(np.int64), 'areas': areas[rows], 'intercepts': icpt[rows][:, :4 if per_slice else 13], 'euler': euler[rows]}
    if per_slice:
        out['slices'] = rows // k
    return out


def same(got, want):
    return all(got[f].shape == want[f].shape and np.array_equal(got[f], want[f]) for f in want)


# ----------------------------------------------------------------------------
# the derived quantities, restated
# ----------------------------------------------------------------------------
def weights(spacing, nd):
    """per half-direction the share of the sphere (circle) nearest to +-d * spacing: scipy's spherical Voronoi areas; in 2-D half
    the angle to either neighbour on the circle"""
    d = np.array(half_dirs(nd), np.float64) * np.asarray(spacing, np.float64)
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    u = np.concatenate([u, -u])
    if nd == 3:
        from scipy.spatial import SphericalVoronoi
        a = SphericalVoronoi(u).calculate_areas() / (4 * np.pi)
    else:
        ang = np.arctan2(u[:, 0], u[:, 1])
        gap = np.sort((ang[None, :] - ang[:, None]) % (2 * np.pi), axis=1)      # [:, 1]: to the next one, [:, -1]: 2 pi - to the one before
        a = (gap[:, 1] + 2 * np.pi - gap[:, -1]) / 2 / (2 * np.pi)
    return a[:len(d)] + a[len(d):]


def weights_by_quadrature(spacing, n=2_000_000):
    """the 3-D weights from n points of a Fibonacci lattice on the sphere, each given to the nearest of the 26 unit vectors"""
    d = np.array(half_dirs(3), np.float64) * np.asarray(spacing, np.float64)
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    count = np.zeros(13)
    golden = np.pi * (3.0 - np.sqrt(5.0))
    for i0 in range(0, n, 1 << 18):
        i = np.arange(i0, min(n, i0 + (1 << 18)))
        zc = 1.0 - (2.0 * i + 1.0) / n
        r = np.sqrt(1.0 - zc * zc)
        pts = np.stack([zc, r * np.sin(golden * i), r * np.cos(golden * i)], axis=1)
        count += np.bincount(np.argmax(np.abs(pts @ u.T), axis=1), minlength=13)
    return count / n


def crofton(icpt, spacing):
    """surface (13 columns) or perimeter (4 columns) from the intercepts: 2 sum c I v / |d|, (pi / 2) sum c I a / |d|"""
    icpt = np.asarray(icpt, np.float64)
    nd = 3 if icpt.shape[1] == 13 else 2
    sp = np.asarray(spacing, np.float64)
    norm = np.linalg.norm(np.array(half_dirs(nd), np.float64) * sp, axis=1)
    c = weights(sp, nd)
    return (2.0 if nd == 3 else np.pi / 2) * np.sum(c * icpt * np.prod(sp) / norm, axis=1)


def sphericity(areas, surface, spacing):
    return np.cbrt(np.pi) * np.cbrt(6.0 * areas * np.prod(spacing)) ** 2 / surface


def circularity(areas, perimeter, spacing):
    return 4 * np.pi * areas * np.prod(spacing) / perimeter ** 2


# ----------------------------------------------------------------------------
# the known objects
# ----------------------------------------------------------------------------
def ball(r, spacing=(1, 1, 1), dtype=np.uint8):
    """sum (g * spacing)^2 <= r^2 around a voxel, one voxel of background around it"""
    n = [int(r / s) + 1 for s in spacing]
    g = np.meshgrid(*[np.arange(-k, k + 1) * float(s) for k, s in zip(n, spacing)], indexing='ij')
    return (sum(c * c for c in g) <= r * r).astype(dtype)


def hollow_ball(r=7, inner=3):
    b = ball(r)
    g = np.indices(b.shape) - (np.array(b.shape) // 2).reshape(3, 1, 1, 1)
    b[(g ** 2).sum(axis=0) <= inner * inner] = 0
    return b


def torus(R=8, r=3):
    g = np.indices((2 * r + 3, 2 * (R + r) + 3, 2 * (R + r) + 3)).astype(np.float64)
    zc, yc, xc = g[0] - (r + 1), g[1] - (R + r + 1), g[2] - (R + r + 1)
    return ((np.sqrt(yc * yc + xc * xc) - R) ** 2 + zc * zc <= r * r).astype(np.uint8)


def corner_cubes():
    v = np.zeros((6, 6, 6), np.uint8)
    v[1:3, 1:3, 1:3] = 1
    v[3:5, 3:5, 3:5] = 1
    return v


def ring(R=6, r=3):
    g = np.indices((2 * R + 3, 2 * R + 3)) - (R + 1)
    d2 = (g ** 2).sum(axis=0)
    return ((d2 <= R * R) & (d2 > r * r)).astype(np.uint8)


def diagonal_pixels():
    v = np.zeros((4, 4), np.uint8)
    v[1, 1] = v[2, 2] = 1
    return v


KNOWN_EULER = {'ball': (1, 1), 'hollow_ball': (2, 2), 'torus': (0, 0), 'corner_cubes': (1, 2), 'ring': (0, 0), 'diagonal_pixels': (1, 2)}


def known_objects():
    return {'ball': ball(6), 'hollow_ball': hollow_ball(), 'torus': torus(), 'corner_cubes': corner_cubes(), 'ring': ring(),
            'diagonal_pixels': diagonal_pixels()}


# ----------------------------------------------------------------------------
# the cases of the device test
# ----------------------------------------------------------------------------
DTYPES = [np.uint8, np.uint16, np.int32, np.uint32, np.int64]


def volume(dtype, shape=(5, 37, 61), seed=1):
    """runs of mean length 29 that cross row and slice ends, about 40 % background"""
    return LC.runs(int(np.prod(shape)), seed, dtype, run=29, top=120 if np.dtype(dtype).itemsize == 1 else 200).reshape(shape)


def small_volume(seed=3, shape=(4, 5, 6), top=4):
    """few labels, densely mixed, on every face of the array: for the per-mask definitions and the model"""
    return np.random.default_rng(seed).integers(0, top, shape).astype(np.uint8)


def seam_volume():
    """depth 11 (no multiple of 2, 3 or 5): blobs, plus staircases that cross every seam diagonally in all four diagonal
    directions, a bar along the main diagonal, a box with a cavity and objects on the faces of the array"""
    D, H, W = 11, 24, 28
    vol = LC.blobs((D, H, W), 12, 5, np.uint32, first=1000)
    for z in range(D):
        vol[z, 2 + z, 1 + z] = 7            # (+1, +1, +1) per slice: only diagonal contact
        vol[z, 20 - z, 3 + z] = 8           # (+1, -1, +1)
        vol[z, 3 + z, 26 - z] = 9           # (+1, +1, -1)
        vol[z, 22 - z, 24 - z] = 10         # (+1, -1, -1)
        vol[z, 12, z:z + 2] = 11            # a staircase along (+1, 0, +1) that touches x = 0
        vol[z, H - 1 - z:H - z, 14] = 12    # ... and one from y = H - 1 along (+1, -1, 0)
    vol[2:9, 8:13, 16:21] = 13
    vol[4:6, 10, 18] = 0                    # a cavity across the seam of slabs of 5
    vol[D - 1, H - 2:, W - 2:] = 14         # the high corner of the array
    vol[0, :2, :2] = 15                     # the low corner
    return vol


def checkerboard(shape=(6, 10, 14)):
    """labels 1 and 2 alternating in every direction"""
    z, y, x = np.indices(shape)
    return (1 + (z + y + x) % 2).astype(np.uint16)


def distinct_blocks(shape=(6, 8, 12)):
    """every 2 x 2 x 2 block of voxels holds eight labels: each neighbourhood has eight labels"""
    z, y, x = np.indices(shape)
    return (1 + (z % 2) * 4 + (y % 2) * 2 + (x % 2)).astype(np.uint8)


def full_intercepts(shape):
    """one label filling the array, border_faces: 2 (DHW - (D - |dz|)(H - |dy|)(W - |dx|)) per direction"""
    return [2 * (int(np.prod(shape)) - int(np.prod([s - abs(v) for s, v in zip(shape, d)]))) for d in half_dirs(len(shape))]


def check(m, want, shape):
    """a LabelShapes against want_shapes' dict"""
    assert m.shape == tuple(shape)
    if 'slices' in want:
        assert np.array_equal(m.slices, want['slices'])
    for f in ('labels', 'areas', 'intercepts', 'euler'):
        got = getattr(m, f)
        assert got.shape == want[f].shape and np.array_equal(got, want[f]), (f, got[got != want[f]][:8], want[f][got != want[f]][:8])
