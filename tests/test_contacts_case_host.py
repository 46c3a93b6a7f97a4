"""Host side of Contact Labels: the numpy references of tests/contacts_case.py against each other, against closed forms and against
Shape Labels' intercepts; the quantities LabelContacts derives (pure numpy, no device); and one planted defect per rule of the
kernel, each shown to be noticed by a case the device test runs (tests/test_gpu_label_contacts.py).

What is pinned and what is not: the integers are pinned against the numpy statement, which is checked here against the pair-by-pair
definition and against shape_case's intercepts.  There is no counterpart in the reference plugin, and skimage's region adjacency
graph is not available: nothing is pinned against it."""
import numpy as np
import pytest

import contacts_case as CC
import shape_case as SC


def _contacts(want, shape, spacing=None, background=False):
    from empanada_napari_amd import labels as L
    return L.contacts_from_arrays(want['a'], want['b'], want['pairs'], shape, spacing, background)


# ----------------------------------------------------------------------------
# the references
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('background', [False, True])
def test_the_two_forms_of_the_reference_agree(background):
    for seed in (3, 4, 5):
        vol = SC.small_volume(seed)
        assert CC.same(CC.want_contacts(vol, background), CC.want_contacts_per_pair(vol, background))
        img = vol[1]
        w = CC.want_contacts(img, background)
        assert w['pairs'].shape[1] == 4 and CC.same(w, CC.want_contacts_per_pair(img, background))
    w = CC.want_contacts(SC.small_volume(3), background)
    assert (w['a'] < w['b']).all() and ((w['a'] == 0).any() == background)
    assert np.array_equal(np.lexsort((w['b'], w['a'])), np.arange(len(w['a'])))


def test_reference_closed_forms():
    shape = (3, 4, 5)
    vol = CC.all_distinct(shape)      # every pair of the array is a row of its own, with one count in one column
    w = CC.want_contacts(vol)
    assert len(w['a']) == CC.distinct_rows(shape) == sum(int(np.prod([s - abs(v) for s, v in zip(shape, d)])) for d in SC.half_dirs(3))
    assert (w['pairs'].sum(axis=1) == 1).all() and (w['pairs'].max(axis=1) == 1).all()
    assert w['pairs'].sum(axis=0).tolist() == [int(np.prod([s - abs(v) for s, v in zip(shape, d)])) for d in SC.half_dirs(3)]
    assert len(CC.want_contacts(np.full(shape, 7, np.uint16), True)['a']) == 0      # one label: no pair
    board = SC.checkerboard()      # 1 and 2 alternate: they differ along the directions with an odd number of non-zero components
    w = CC.want_contacts(board)
    odd = np.abs(np.array(SC.half_dirs(3))).sum(axis=1) % 2 == 1
    assert w['a'].tolist() == [1] and w['b'].tolist() == [2] and not w['pairs'][0, ~odd].any() and w['pairs'][0, odd].all()
    D, H, W, c = 6, 5, 7, 3
    w = CC.want_contacts(CC.half_spaces((D, H, W), c))      # two half-spaces: the pairs that cross z = c, inside the array
    want = [(H - abs(dy)) * (W - abs(dx)) if dz else 0 for dz, dy, dx in SC.half_dirs(3)]
    assert w['a'].tolist() == [1] and w['b'].tolist() == [2] and w['pairs'].tolist() == [want] and want[8] == H * W


def test_row_sums_are_the_intercepts_of_shape_labels():
    """per label and direction, over its partners with the background among them: Shape Labels' intercepts without border faces"""
    for vol in (SC.small_volume(3), SC.volume(np.uint16, seed=11), SC.seam_volume(), SC.volume(np.uint8)[2]):
        w = CC.want_contacts(vol, True)
        s = SC.want_shapes(vol, border_faces=False)
        sums = np.zeros_like(s['intercepts'])
        for side in ('a', 'b'):
            keep = w[side] != 0
            np.add.at(sums, np.searchsorted(s['labels'], w[side][keep]), w['pairs'][keep])
        assert np.array_equal(sums, s['intercepts'])
        both = CC.want_contacts(vol, False)      # without the background: the same rows less those with a 0
        assert CC.same(both, {f: w[f][w['a'] != 0] for f in ('a', 'b', 'pairs')})


# ----------------------------------------------------------------------------
# the kernel's scheme and its planted defects
# ----------------------------------------------------------------------------
SLABS = (1, 2, 3, 5, None)


def test_model_equals_reference_and_every_defect_is_noticed():
    vol = SC.seam_volume()
    want = {bg: CC.want_contacts(vol, bg) for bg in (False, True)}
    for bg in (False, True):
        for slab in SLABS:
            assert CC.same(CC.model_contacts(vol, bg, slab), want[bg]), (bg, slab)
    for defect in CC.DEFECTS:
        noticed = [(bg, slab) for bg in (False, True) for slab in SLABS if not CC.same(CC.model_contacts(vol, bg, slab, defect), want[bg])]
        assert noticed, defect
    # the narrow layouts of the device test notice the row-end wrap as well: every voxel is a row end
    narrow = SC.LC.runs(15 * 2, 9, np.uint8, run=4, top=50).reshape(15, 1, 2)
    assert CC.same(CC.model_contacts(narrow, True, 4), CC.want_contacts(narrow, True))
    assert not CC.same(CC.model_contacts(narrow, True, 4, 'diagonal_wraps_into_neighbouring_row'), CC.want_contacts(narrow, True))


# ----------------------------------------------------------------------------
# what LabelContacts derives
# ----------------------------------------------------------------------------
def test_label_contacts_derived_columns():
    from empanada_napari_amd import labels as L
    vol = SC.volume(np.uint16, seed=11)
    for bg in (False, True):
        w = CC.want_contacts(vol, bg)
        for sp in ((1.0, 1.0, 1.0), (2.0, 1.0, 0.5)):
            m = _contacts(w, vol.shape, sp, bg)
            CC.check(m, w, vol.shape)
            assert m.ndim == 3 and np.array_equal(m.faces, w['pairs'][:, list(SC.AXIS_COLUMNS[3])])
            assert np.allclose(m.face_area, CC.face_size(w['pairs'], sp), rtol=1e-12, atol=0)
            assert np.allclose(m.contact_area, CC.crofton(w['pairs'], sp), rtol=1e-12, atol=0)
            with pytest.raises(ValueError):
                m.contact_length
    img = vol[2]
    w2 = CC.want_contacts(img, True)
    m2 = _contacts(w2, img.shape, (1.0, 0.5), True)
    assert m2.ndim == 2 and m2.pairs.shape[1] == 4
    assert np.allclose(m2.contact_length, CC.crofton(w2['pairs'], (1.0, 0.5)), rtol=1e-12, atol=0)
    assert np.allclose(m2.face_length, CC.face_size(w2['pairs'], (1.0, 0.5)), rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        m2.contact_area
    # the adjacency matrix: symmetric, the rows' weights at (a, b) and (b, a), nothing else
    w = CC.want_contacts(vol, True)
    m = _contacts(w, vol.shape, (2.0, 1.0, 0.5), True)
    ids = m.labels
    assert np.array_equal(ids, np.unique(np.concatenate([w['a'], w['b']])))
    for weight, col in (('contact_area', m.contact_area), ('face_area', m.face_area), ('counts', m.counts)):
        A = m.adjacency(weight)
        assert A.shape == (len(ids), len(ids)) and A.nnz == 2 * len(m.a) and abs(A - A.T).max() == 0
        dense = A.toarray()
        assert np.array_equal(dense[np.searchsorted(ids, m.a), np.searchsorted(ids, m.b)], col.astype(np.float64))
    with pytest.raises(ValueError):
        m.adjacency('volume')
    assert np.array_equal(m.degree(), np.asarray((m.adjacency('counts') > 0).sum(axis=1)).reshape(-1))
    # neighbors: every partner, or only those that share a voxel face
    lab = int(m.b[np.argmax(m.counts)])
    rows = (m.a == lab) | (m.b == lab)
    assert np.array_equal(m.neighbors(lab), np.unique(np.where(m.a == lab, m.b, m.a)[rows]))
    assert np.array_equal(m.neighbors(lab, 3), m.neighbors(lab))
    facing = rows & m.faces.any(axis=1)
    assert np.array_equal(m.neighbors(lab, connectivity=1), np.unique(np.where(m.a == lab, m.b, m.a)[facing]))
    tiny = L.contacts_from_arrays([1, 1], [2, 3], [[0] * 8 + [4] + [0] * 4, [0] * 12 + [1]], (4, 4, 4))      # 1-2 by faces, 1-3 by a corner
    assert tiny.neighbors(1).tolist() == [2, 3] and tiny.neighbors(1, connectivity=1).tolist() == [2] and tiny.neighbors(3, 1).tolist() == []
    assert tiny.degree().tolist() == [2, 1, 1] and tiny.faces.tolist() == [[4, 0, 0], [0, 0, 0]]
    with pytest.raises(ValueError):
        tiny.neighbors(1, connectivity=2)
    # fractions: a contact's share of each label's whole surface in the array; at most all of it
    f = m.fractions()
    assert f.shape == (len(m.a), 2) and (f > 0).all() and (f <= 1 + 1e-12).all()
    for side, col in ((m.a, f[:, 0]), (m.b, f[:, 1])):
        assert (np.bincount(np.searchsorted(ids, side), col, len(ids)) <= 1 + 1e-9).all()
    total = np.bincount(np.searchsorted(ids, m.a), f[:, 0], len(ids)) + np.bincount(np.searchsorted(ids, m.b), f[:, 1], len(ids))
    assert np.allclose(total, 1.0, rtol=1e-9)      # the rows of a label are its whole surface
    s = SC.want_shapes(vol, border_faces=False)      # ... which is Shape Labels' surface without border faces
    whole = SC.crofton(s['intercepts'], (2.0, 1.0, 0.5))
    keep = m.a != 0
    assert np.allclose(f[keep, 0], m.contact_area[keep] / whole[np.searchsorted(s['labels'], m.a[keep])], rtol=1e-9)
    with pytest.raises(ValueError, match='background'):
        _contacts(CC.want_contacts(vol, False), vol.shape).fractions()


def test_label_contacts_classes_groups_and_csv(tmp_path):
    import csv
    from empanada_napari_amd import labels as L
    col = lambda k, n: [n if j == k else 0 for j in range(13)]      # noqa: E731
    # a panoptic-style id set, divisor 1000: two instances of class 1, two of class 2, one of class 3, and the background
    a = [0, 0, 1001, 1001, 1002, 2001, 2001]
    b = [1001, 2002, 1002, 2001, 2001, 2002, 3001]
    pairs = [col(8, 5), col(2, 7), col(8, 9), col(0, 2), col(12, 3), col(8, 4), col(5, 6)]
    m = L.contacts_from_arrays(a[::-1], b[::-1], pairs[::-1], (8, 8, 8), background=True)      # rows in any order
    assert m.a.tolist() == a and m.b.tolist() == b and m.pairs.tolist() == pairs
    c = m.by_class(1000)
    assert list(zip(c.a.tolist(), c.b.tolist())) == [(0, 1), (0, 2), (1, 1), (1, 2), (2, 2), (2, 3)]
    assert c.pairs.tolist() == [col(8, 5), col(2, 7), col(8, 9), [2] + [0] * 11 + [3], col(8, 4), col(5, 6)]
    assert c.counts.tolist() == [5, 7, 9, 5, 4, 6] and c.background and c.shape == (8, 8, 8)
    assert np.allclose(c.contact_area.sum(), m.contact_area.sum(), rtol=1e-12)
    with pytest.raises(ValueError):
        m.by_class(0)
    # a chain 1-2-3 with a weak link 2-3, and 4-5 apart from it
    chain = L.contacts_from_arrays([1, 2, 4, 0, 0, 0], [2, 3, 5, 1, 2, 3], [col(8, 50), col(8, 2), col(8, 20), col(8, 50), col(8, 48), col(8, 98)],
                                   (16, 16, 16), background=True)
    area = dict(zip(zip(chain.a.tolist(), chain.b.tolist()), chain.contact_area.tolist()))
    weak, strong = area[(2, 3)], area[(4, 5)]
    assert weak < strong < area[(1, 2)]
    groups = lambda **kw: [g.tolist() for g in chain.merge_groups(**kw)]      # noqa: E731
    assert groups() == [[1, 2, 3], [4, 5]]      # everything that touches; the background joins nothing
    assert groups(min_area=weak) == [[1, 2, 3], [4, 5]] and groups(min_area=np.nextafter(weak, np.inf)) == [[1, 2], [4, 5]]
    assert groups(min_area=np.nextafter(strong, np.inf)) == [[1, 2]] and groups(min_area=2 * area[(1, 2)]) == []
    # shares: 1-2 is 50 / 100 of both, 2-3 is 2 / 100 of label 2 and 2 / 100 of label 3, 4-5 is all of both
    fr = dict(zip(zip(chain.a.tolist(), chain.b.tolist()), chain.fractions().tolist()))
    assert np.allclose(fr[(1, 2)], [0.5, 0.5]) and np.allclose(fr[(2, 3)], [0.02, 0.02]) and np.allclose(fr[(4, 5)], [1.0, 1.0])
    assert groups(min_fraction=0.02 - 1e-9) == [[1, 2, 3], [4, 5]] and groups(min_fraction=0.02 + 1e-9) == [[1, 2], [4, 5]]
    assert groups(min_fraction=0.75) == [[4, 5]]
    assert all(g.dtype == np.int64 for g in chain.merge_groups())
    with pytest.raises(ValueError, match='background'):
        L.contacts_from_arrays([1], [2], [col(8, 5)], (4, 4, 4)).merge_groups(min_fraction=0.1)
    # the class restriction: 1001-1002 and 2001-2002 join, 1001-2001, 1002-2001 and 2001-3001 do not
    assert [g.tolist() for g in m.merge_groups(label_divisor=1000)] == [[1001, 1002], [2001, 2002]]
    assert [g.tolist() for g in m.merge_groups()] == [[1001, 1002, 2001, 2002, 3001]]
    # the CSV round-trip
    path = tmp_path / 'c.csv'
    chain.to_csv(str(path))
    rows = list(csv.DictReader(open(path)))
    t = chain.to_table()
    assert list(rows[0]) == list(t) and list(t)[:5] == ['a', 'b', 'count', 'contact_area', 'face_area']
    assert [int(r['a']) for r in rows] == chain.a.tolist() and [int(r['b']) for r in rows] == chain.b.tolist()
    assert [int(r['count']) for r in rows] == chain.counts.tolist() and [int(r['faces-z']) for r in rows] == chain.faces[:, 0].tolist()
    assert np.allclose([float(r['contact_area']) for r in rows], chain.contact_area, rtol=1e-15)
    assert [[int(r[f'pairs-{j}']) for j in range(13)] for r in rows] == chain.pairs.tolist()
    # the constructor's refusals
    for bad in (dict(a=[1, 2], b=[2], pairs=[col(0, 1)]), dict(a=[2], b=[1], pairs=[col(0, 1)]), dict(a=[3], b=[3], pairs=[col(0, 1)]),
                dict(a=[-1], b=[1], pairs=[col(0, 1)]), dict(a=[0], b=[1], pairs=[col(0, 1)]), dict(a=[1], b=[2], pairs=[col(0, 1)], shape=(2, 3, 4, 5)),
                dict(a=[1], b=[2], pairs=[col(0, 1)], spacing=(1, 0, 1)), dict(a=[1], b=[2], pairs=[col(0, 1)], spacing=(1, 1))):
        kw = dict(shape=(4, 4, 4))
        kw.update(bad)
        with pytest.raises(ValueError):
            L.contacts_from_arrays(**kw)
    empty = L.contacts_from_arrays([], [], np.zeros((0, 13)), (4, 4, 4), background=True)
    assert len(empty.labels) == 0 and empty.contact_area.shape == (0,) and empty.merge_groups() == [] and empty.fractions().shape == (0, 2)


def test_planar_interface_against_the_hexagonal_section():
    """Two labels split by the plane through the centre of a 48^3 cube with normal (1, 1, 1): the section is a regular hexagon of
    side 48 / sqrt 2, area 3 sqrt 3 / 4 * 48^2 = 2992.98.  On an unbounded plane the estimator's error depends on the direction
    weights only: 2 sum_k c_k |n . u_k| = 0.9611 for this normal (contacts_case.plane_ratio).  In the cube the pairs with an end
    outside the array are not counted, which takes a rim off the hexagon: the numpy statement gives contact_area / hexagon =
    0.9350 and face_area / (sqrt 3 * hexagon) = 0.9861 (the voxel faces of a (1, 1, 1) staircase are sqrt 3 times the plane; the
    rim is 1.4 %).  Neither error is fixed in advance: both are computed here from the numpy statement, and what LabelContacts
    derives has to stay within 1.5 times them."""
    n = 48
    vol = CC.diagonal_halves(n)
    w = CC.want_contacts(vol)
    assert w['a'].tolist() == [1] and w['b'].tolist() == [2]
    hexagon = CC.hexagon_area(n)
    crofton_error = abs(CC.crofton(w['pairs'], (1, 1, 1))[0] / hexagon - 1)
    face_error = abs(CC.face_size(w['pairs'], (1, 1, 1))[0] / (np.sqrt(3) * hexagon) - 1)
    plane_error = abs(CC.plane_ratio((1, 1, 1)) - 1)
    print(f'contact_area / hexagon: statement {1 - crofton_error:.4f}, unbounded plane {1 - plane_error:.4f}; face_area / (sqrt 3 hexagon): {1 - face_error:.4f}')
    assert 0 < plane_error < crofton_error < 0.1 and 0 < face_error < plane_error      # the rim only takes away
    m = _contacts(w, vol.shape)
    assert abs(m.contact_area[0] / hexagon - 1) <= 1.5 * crofton_error
    assert abs(m.face_area[0] / (np.sqrt(3) * hexagon) - 1) <= 1.5 * face_error
    assert m.contact_area[0] < m.face_area[0] / np.sqrt(3) < hexagon
