"""Host side of Measure Labels: the numpy references of tests/measure_case.py against closed forms and scipy.ndimage, the
quantities LabelMeasures derives (pure numpy, no device), and one planted defect per rule of the kernel, each shown to be noticed
by a case the device test runs (tests/test_gpu_measure.py)."""
import numpy as np
import pytest
from scipy import ndimage

import measure_case as MC


def _box_volume():
    vol = np.zeros((9, 11, 13), np.uint16)
    vol[2:5, 3:8, 4:11] = 3      # 3 x 5 x 7, centred at (3, 5, 7)
    return vol


def _measures(want, shape, spacing=None):
    from empanada_napari_amd import labels as L
    return L.measures_from_arrays(want['labels'], want['areas'], want['boxes'], want['sum1'], want['sum2'], want['faces'], shape, spacing,
                                  slices=want.get('slices'))


# ----------------------------------------------------------------------------
# the references
# ----------------------------------------------------------------------------
def test_reference_against_closed_forms():
    w = MC.want_measures(_box_volume())
    assert w['labels'].tolist() == [3] and w['areas'].tolist() == [105] and w['boxes'].tolist() == [[2, 3, 4, 5, 8, 11]]
    assert w['faces'].tolist() == [[2 * 5 * 7, 2 * 3 * 7, 2 * 3 * 5]]
    assert w['sum1'].tolist() == [[3 * 105, 5 * 105, 7 * 105]]
    n = 105
    for j, (a, b) in enumerate(MC.PAIRS[3]):      # n * sum(ab) - sum(a) sum(b) = n^2 (k^2 - 1) / 12 on the diagonal, 0 off it
        central = n * int(w['sum2'][0, j]) - int(w['sum1'][0, a]) * int(w['sum1'][0, b])
        assert central == (n * n * ((3, 5, 7)[a] ** 2 - 1) // 12 if a == b else 0)
    # two boxes that touch along z: the shared 4 x 5 face is exposed for both (the neighbour has another value)
    two = np.zeros((8, 6, 7), np.uint8)
    two[1:3, 1:5, 1:6] = 1
    two[3:6, 1:5, 1:6] = 2
    w = MC.want_measures(two)
    assert w['faces'].tolist() == [[2 * 20, 2 * 2 * 5, 2 * 2 * 4], [2 * 20, 2 * 3 * 5, 2 * 3 * 4]]
    # a label filling the array: only border faces
    full = np.full((3, 4, 5), 2, np.uint8)
    assert MC.want_measures(full)['faces'].tolist() == [[40, 30, 24]] and MC.want_measures(full, False)['faces'].tolist() == [[0, 0, 0]]
    # an image: (y, x) columns, pixel edges
    img = np.zeros((6, 8), np.uint8)
    img[1:4, 2:7] = 4
    w = MC.want_measures(img)
    assert w['faces'].tolist() == [[2 * 5, 2 * 3]] and w['sum1'].tolist() == [[2 * 15, 4 * 15]] and w['sum2'].shape == (1, 3)


def test_reference_against_scipy():
    vol = MC.volume(np.uint32)
    w = MC.want_measures(vol)
    idx = w['labels']
    assert np.array_equal(w['areas'], ndimage.sum_labels(np.ones(vol.shape, np.int64), vol, idx))
    coords = np.indices(vol.shape)
    for a in range(3):
        assert np.array_equal(w['sum1'][:, a], ndimage.sum_labels(coords[a], vol, idx).astype(np.int64))
    for j, (a, b) in enumerate(MC.PAIRS[3]):
        assert np.array_equal(w['sum2'][:, j], ndimage.sum_labels(coords[a] * coords[b], vol, idx).astype(np.int64))
    # centroids: both sides are one division of exact integers below 2^53 -> within 2 ulp of float64
    com = np.array(ndimage.center_of_mass(np.ones(vol.shape), vol, idx))
    got = _measures(w, vol.shape).centroid
    assert np.all(np.abs(got - com) <= 2 * np.spacing(np.abs(com)))
    ps = MC.want_measures_per_slice(vol)
    z = 3
    assert np.array_equal(ps['labels'][ps['slices'] == z], np.unique(vol[z][vol[z] != 0]))
    assert np.array_equal(ps['faces'][ps['slices'] == z], MC.want_measures(vol[z])['faces'])


def test_scaled_reference_matches_the_blown_up_volume():
    small = MC.volume(np.uint32, (3, 5, 7), 3)
    f = (2, 3, 4)
    big = np.repeat(np.repeat(np.repeat(small, f[0], 0), f[1], 1), f[2], 2)
    for bf in (True, False):
        assert MC.same(MC.scaled(MC.want_measures(small, bf), f), MC.want_measures(big, bf))
    assert MC.same(MC.scaled(MC.want_measures(small[1]), f[1:]), MC.want_measures(big[2]))


# ----------------------------------------------------------------------------
# LabelMeasures: the derived quantities
# ----------------------------------------------------------------------------
def test_derived_quantities_of_a_box_with_anisotropic_spacing():
    sp = (2.0, 1.0, 0.5)
    m = _measures(MC.want_measures(_box_volume()), (9, 11, 13), sp)
    assert m.ndim == 3 and not m.per_slice
    assert m.centroid.tolist() == [[3.0, 5.0, 7.0]] and m.centroid_physical.tolist() == [[6.0, 5.0, 3.5]]
    assert m.volume.tolist() == [105.0]
    assert m.surface_area.tolist() == [70 * 1.0 * 0.5 + 42 * 2.0 * 0.5 + 30 * 2.0 * 1.0]
    var = [(k * k - 1) / 12 * s * s for k, s in zip((3, 5, 7), sp)]
    assert np.allclose(m.covariance[0], np.diag(var), rtol=1e-15, atol=0)
    assert np.allclose(m.principal_variances[0], sorted(var, reverse=True), rtol=1e-14)
    axes = m.principal_axes[0]      # unit vectors along the axes, in the order of the variances (z: 32 / 12, y: 24 / 12, x: 12 / 12)
    order = np.argsort(var)[::-1]
    assert np.allclose(np.abs(axes), np.eye(3)[order], atol=1e-12)
    assert np.isclose(m.equivalent_diameter[0], (6 * 105 / np.pi) ** (1 / 3))
    assert np.isclose(m.sphericity[0], np.pi ** (1 / 3) * (6 * 105.0) ** (2 / 3) / m.surface_area[0])
    cube = np.zeros((6, 6, 6), np.uint8)
    cube[1:5, 1:5, 1:5] = 1
    assert np.isclose(_measures(MC.want_measures(cube), cube.shape).sphericity[0], (np.pi / 6) ** (1 / 3))


def test_covariance_of_a_tilted_object_and_of_an_image():
    vol = np.zeros((12, 12, 12), np.uint8)
    for i in range(10):      # a diagonal rod in the (y, x) plane
        vol[5, 1 + i, 1 + i] = 6
    m = _measures(MC.want_measures(vol), vol.shape)
    pts = np.argwhere(vol == 6).astype(np.float64)
    assert np.allclose(m.covariance[0], np.cov(pts.T, bias=True), rtol=1e-13, atol=1e-13)
    assert np.allclose(m.principal_variances[0], [2 * 99 / 12, 0, 0], atol=1e-12)
    assert np.allclose(np.abs(m.principal_axes[0, 0]), [0, 2 ** -0.5, 2 ** -0.5], atol=1e-12)
    img = vol[5]
    m2 = _measures(MC.want_measures(img), img.shape, (3.0, 2.0))
    assert m2.ndim == 2 and m2.covariance.shape == (1, 2, 2)
    assert np.allclose(m2.covariance[0], np.cov((pts[:, 1:] * [3.0, 2.0]).T, bias=True), rtol=1e-13)
    assert m2.perimeter_faces.tolist() == [20 * 2.0 + 20 * 3.0]      # 20 edges perpendicular to y, each 2 long; 20 to x, each 3 long
    with pytest.raises(ValueError):
        m.perimeter_faces
    ps = _measures(MC.want_measures_per_slice(vol), vol.shape, (5.0, 3.0, 2.0))      # a stack's spacing: the images take (y, x)
    assert ps.per_slice and ps.slices.tolist() == [5] and ps.spacing == (3.0, 2.0) and np.allclose(ps.covariance, m2.covariance)


def test_central_moments_are_exact_where_float64_cancels():
    """A hand-built table of an image's thin object far from the origin: column x0 = 2^21 - 5 filled over 900 001 rows and column
    x0 + 1 over 33 331 of them.  sum(xx) is 2^62: float64 cannot hold it, and sum(xx) / n - (sum(x) / n)^2 is the difference of two
    numbers near 2^42 -- what is left of the variance n1 n2 / n^2 = 0.0344 is wrong in the third digit.  The integer form
    n sum(xx) - sum(x)^2 = n1 n2 has it to the last bit."""
    from empanada_napari_amd import labels as L
    x0, n1, n2 = (1 << 21) - 5, 900_001, 33_331
    n = n1 + n2
    s = lambda k: k * (k - 1) // 2                    # sum of i over [0, k)
    q = lambda k: (k - 1) * k * (2 * k - 1) // 6      # sum of i^2
    sy, syy = s(n1) + s(n2), q(n1) + q(n2)
    sx, sxx, syx = n1 * x0 + n2 * (x0 + 1), n1 * x0 * x0 + n2 * (x0 + 1) ** 2, x0 * s(n1) + (x0 + 1) * s(n2)
    assert 1 << 53 < sxx < 1 << 63 and syy < 1 << 63 and syx < 1 << 63
    m = L.measures_from_arrays([1], [n], [[0, x0, n1, x0 + 2]], [[sy, sx]], [[syy, sxx, syx]], [[4, 2 * n1]], (n1, x0 + 2))
    assert m.central_moments_exact()[0, 1, 1] == n1 * n2
    exact = n1 * n2 / (n * n)      # Python's division of integers is correctly rounded
    assert m.covariance[0, 1, 1] == exact
    naive = float(sxx) / n - (float(sx) / n) ** 2
    assert abs(naive - exact) > 5e-3 * exact
    assert m.covariance[0, 0, 1] == (n * syx - sy * sx) / (n * n) and m.covariance[0, 0, 0] == (n * syy - sy * sy) / (n * n)
    assert np.isclose(m.principal_variances[0].sum(), m.covariance[0, 0, 0] + exact, rtol=1e-15)


def test_tables_and_csv(tmp_path):
    import csv
    vol = MC.volume(np.uint16)
    m = _measures(MC.want_measures(vol), vol.shape, (1.5, 1.0, 1.0))
    t = m.to_table()
    assert list(t)[:2] == ['label', 'area'] and all(len(c) == len(m.labels) for c in t.values())
    assert {'bbox-5', 'centroid-2', 'volume', 'surface_area', 'equivalent_diameter', 'sphericity', 'principal_variance-2'} <= set(t)
    m.to_csv(tmp_path / 'm.csv')
    rows = list(csv.DictReader(open(tmp_path / 'm.csv')))
    assert [int(r['label']) for r in rows] == m.labels.tolist() and [float(r['volume']) for r in rows] == m.volume.tolist()
    ps = _measures(MC.want_measures_per_slice(vol), vol.shape)
    assert list(ps.to_table())[0] == 'slice' and 'bbox-3' in ps.to_table() and 'bbox-4' not in ps.to_table()
    empty = _measures(MC.want_measures(np.zeros((3, 4, 5), np.uint8)), (3, 4, 5))
    assert len(empty.labels) == 0 and empty.covariance.shape == (0, 3, 3) and empty.principal_axes.shape == (0, 3, 3)
    assert all(len(c) == 0 for c in empty.to_table().values())


# ----------------------------------------------------------------------------
# the kernel's rules: each one broken is noticed by a case of the device test
# ----------------------------------------------------------------------------
def test_model_of_the_kernel_agrees_with_the_reference():
    for vol in (MC.volume(np.uint32), MC.slab_volume(), MC.checkerboard(), np.full((4, 6, 8), 5, np.uint8)):
        for bf in (True, False):
            want = MC.want_measures(vol, bf)
            for slab in (None, 1, 2, 3):
                assert MC.same(MC.model_measures(vol, bf, slab), want), (vol.shape, bf, slab)


@pytest.mark.parametrize('defect, case, slab', [
    ('run_not_cut_at_row_end', 'volume', None),                    # the dtype test: runs of mean length 29 in rows of 61
    ('z_face_dropped_at_slab_border', 'slab_volume', 3),           # the slab test
    ('z_face_dropped_at_slab_border', 'slab_volume', 2),
    ('border_face_dropped_at_last_index', 'volume', None),
    ('border_face_dropped_at_last_index', 'full', None),           # one label filling the volume
    ('one_side_credited', 'volume', None),
    ('one_side_credited', 'checkerboard', None),
    ('label_0_entered', 'volume', None),
])
def test_planted_defects_are_caught(defect, case, slab):
    vol = {'volume': lambda: MC.volume(np.uint32), 'slab_volume': MC.slab_volume, 'checkerboard': MC.checkerboard,
           'full': lambda: np.full((16, 64, 64), 5, np.uint32)}[case]()
    want = MC.want_measures(vol)
    assert MC.same(MC.model_measures(vol, True, slab), want)
    assert not MC.same(MC.model_measures(vol, True, slab, defect=defect), want)
