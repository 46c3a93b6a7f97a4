"""The references and inputs of tests/stitch_case.py, checked on the CPU alone: the references agree with the oracle, and
every condition a test of tests/test_gpu_stitch_kernels.py relies on to reach its branch (a second scan pass, a second grid
step, a regrow of the run buffer ...) holds on the reference -- so a GPU test cannot pass by having missed its branch."""
import numpy as np
import pytest

import stitch_case as SC


def _same_seg(got, want):
    assert list(got) == list(want)
    for c in want:
        assert list(got[c]) == list(want[c])
        for k in want[c]:
            assert tuple(got[c][k]['box']) == tuple(want[c][k]['box'])
            np.testing.assert_array_equal(got[c][k]['starts'], want[c][k]['starts'])
            np.testing.assert_array_equal(got[c][k]['runs'], want[c][k]['runs'])


# ---- references against the oracle ----
def test_batched_components_equal_the_oracle():
    from oracle import sparse as osp
    imgs = SC.all_3x3()
    assert imgs.shape == (19683, 3, 3) and len(np.unique(imgs.reshape(len(imgs), -1), axis=0)) == 19683
    pick = np.random.default_rng(0).choice(len(imgs), size=500, replace=False)
    got, num = SC.components_batch(imgs[pick])
    for k, n in enumerate(pick):
        want = osp.connected_components(imgs[n])
        np.testing.assert_array_equal(got[k], want)
        assert num[k] == want.max()
    img = SC.noise((40, 50), (0, 1, 2), 3)
    got, num = SC.components_batch(img[None])
    want = osp.connected_components(img)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[0], osp.label_nd(img))
    assert num[0] == want.max() > 100


def test_exhaustive_sets_are_complete():
    b = SC.all_binary_3x5()
    assert b.shape == (32768, 3, 5) and set(np.unique(b)) == {0, 1}
    assert len(np.unique(b.reshape(len(b), -1), axis=0)) == 32768
    m = SC.mosaic_2x2x2()
    assert m.shape == (2, 242, 242) and not m[:, 2::3].any() and not m[:, :, 2::3].any()
    cubes = np.stack([m[dz, dy::3, dx::3] for dz in range(2) for dy in range(2) for dx in range(2)], axis=-1).reshape(-1, 8)
    assert len(np.unique(cubes, axis=0)) == 3 ** 8
    assert max(len(SC.all_3x3()), len(b)) <= 65535          # the image index is blockIdx.y


def test_run_reference_equals_rle_encode_per_label():
    from oracle import sparse as osp
    img = SC.blobs((23, 31), 30, 0.15, 4)
    r = SC.runs_ref(img)
    assert len(r) > 50 and np.all(np.diff(r[:, 0]) > 0)
    for lab in np.unique(img[img != 0]):
        s, n = osp.rle_encode(np.flatnonzero(img.reshape(-1) == lab))
        sel = r[r[:, 2] == lab]
        np.testing.assert_array_equal(sel[:, 0], s)
        np.testing.assert_array_equal(sel[:, 1], n)


def test_fill_morph_and_segment_references_equal_the_oracle():
    from oracle import sparse as osp
    inst = SC.overlapping_instances((6, 20, 24), n_runs=60, seed=2)
    np.testing.assert_array_equal(SC.fill_ref(np.zeros((6, 20, 24), np.int32), inst),
                                  osp.numpy_fill_instances(np.zeros((6, 20, 24), np.int32), inst))
    pan = SC.blobs((48, 70), 14, 0.15, 5)
    np.testing.assert_array_equal(SC.force_connected_ref(pan, [1, 2], SC.DIV), osp.force_connected_pan(pan.copy(), [1, 2], SC.DIV))
    _same_seg(SC.rle_seg_ref(pan, [1, 2], SC.DIV, [1]), osp.pan_seg_to_rle_seg(pan, [1, 2], SC.DIV, [1]))
    vol = SC.noise((4, 6, 5), (0, 3, 9, 70000), 6)
    assert SC.cross_morph_ref(vol, 0)[0, 0, 0] == vol[:2, :2, :2][[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]].min()


@pytest.mark.parametrize('name,gen,count', SC.ADVERSARIAL)
def test_adversarial_shapes_have_the_intended_components(name, gen, count):
    from oracle import sparse as osp
    for shape in ((257, 259), (9, 12), (12, 9)):
        img = gen(*shape)
        assert img.shape == shape and int(osp.label_nd(img).max()) == count, (name, shape)
    img = gen(257, 259)
    if name == 'staircase':             # diagonal links only: no pixel has a 4-neighbour
        assert not (img[1:] & img[:-1]).any() and not (img[:, 1:] & img[:, :-1]).any() and img.sum() == 257
    elif name != 'two_spirals':         # a path: far more pixels than the image has rows, nowhere 2 x 2 thick
        assert img.sum() > 257 * 100
        assert not (img[1:, 1:] & img[:-1, 1:] & img[1:, :-1] & img[:-1, :-1]).any()
    assert int(osp.label_nd(SC.vertical_line(4099, 1)).max()) == int(osp.label_nd(SC.vertical_line(4099, 3)).max()) == 1


# ---- group C: multi-pass scans, strided loops, the regrow ----
@pytest.fixture(scope='module')
def c513():
    return SC.multipass_513()


@pytest.fixture(scope='module')
def c1025():
    return SC.multipass_1025()


def test_multipass_513_preconditions(c513):
    from oracle import sparse as osp
    N, H, W = c513.shape
    assert -(-H * W // SC.CHUNK) == 259 and N * H * W > SC.GRID_CAP
    assert set(np.unique(c513)) == {0, *SC.TWO_CLASS}
    for n in range(N):
        for img in (c513[n], SC.in_range(c513[n], SC.DIV, 2 * SC.DIV)):
            assert int((SC.first_indices(osp.label_nd(img)) >= SC.SCAN_PASS).sum()) >= 8
    runs = [len(SC.runs_ref(c513[n])) for n in range(N)]
    assert runs[0] > 65536 > runs[1] > 0, runs                 # the regrow happens with one image overflowing


def test_multipass_1025_preconditions(c1025):
    from oracle import sparse as osp
    N, H, W = c1025.shape
    assert N == 1 and -(-H * W // SC.CHUNK) == 517
    for img in (c1025[0], SC.in_range(c1025[0], SC.DIV, 2 * SC.DIV)):
        first = SC.first_indices(osp.label_nd(img))
        assert int((first >= SC.GRID_CAP).sum()) >= 8 and int((first >= SC.SCAN_PASS).sum()) >= 8
    assert len(SC.runs_ref(c1025[0])) > 65536


# ---- group E ----
def test_strided_volume_preconditions():
    from oracle import sparse as osp
    vol = SC.strided_volume()
    assert vol.size == 1076435 > SC.GRID_CAP
    frac = [float((vol == v).mean()) for v in (3, 4, 0)]
    assert np.allclose(frac, (0.35, 0.20, 0.45), atol=0.01)
    assert int((SC.first_indices(osp.label_nd(vol)) >= SC.GRID_CAP).sum()) >= 8
    assert int((SC.first_indices(osp.label_nd(SC.in_range(vol, 3, 4))) >= SC.GRID_CAP).sum()) >= 8


# ---- group F ----
def test_run_edge_preconditions():
    mr = SC.max_runs_batch()
    counts = [len(SC.runs_ref(m)) for m in mr]
    assert counts == [2, 3, 700]
    assert [sum(c > cap for c in counts) for cap in (1, 4, 1000)] == [3, 1, 0]        # all, one, no image overflows
    b = SC.boundary_runs()
    hw = b[0].size
    assert hw == 5 * SC.CHUNK
    for n in range(2):
        r = SC.runs_ref(b[n])
        s, e = r[:, 0], r[:, 0] + r[:, 1]
        for edge in (8, SC.CHUNK):
            assert (s[s > 0] % edge == 0).any() and (e[e < hw] % edge == 0).any()
            assert ((s % edge != 0) & (s // edge != (e - 1) // edge)).any()           # a run that crosses such a boundary
        assert s[0] == 0 and e[-1] == hw
    assert b[0].reshape(-1)[-1] == b[1].reshape(-1)[0] != 0                           # equal labels across the image boundary
    junk = SC.with_junk(SC.sweep_images((70, 67))[0], SC.DIV, 2 * SC.DIV, 1)
    assert (junk < 0).any() and (junk >= 1 << 31).any()
    assert (((junk & 0xffffffff) >= SC.DIV) & ((junk & 0xffffffff) < 2 * SC.DIV) & (junk >= 1 << 31)).any()
    np.testing.assert_array_equal(SC.in_range(junk, SC.DIV, 2 * SC.DIV), SC.sweep_images((70, 67))[0])


# ---- group G ----
def test_fill_preconditions():
    starts, lens, vals, size = SC.fill_runs()
    assert len(starts) == 40000 > 32768                       # one wave per run, 32 768 waves in the capped grid
    assert set(np.unique(lens)) == {1, 63, 64, 65, 5000}
    o = np.argsort(starts)
    assert np.all(starts[o][1:] >= (starts + lens)[o][:-1]) and int((starts + lens).max()) <= size
    assert vals.min() >= 1 and vals.max() <= 255
    shape = (16, 256, 256)
    inst = SC.overlapping_instances(shape)
    assert sum(len(a['starts']) for a in inst.values()) == 40000
    cover = np.zeros(int(np.prod(shape)), np.int8)
    for a in inst.values():
        cover[SC.run_indices(a['starts'], a['runs'])] += 1
    assert float((cover >= 2).sum()) > 0.5 * float((cover >= 1).sum())                # heavily overlapping
    for a in inst.values():                                                            # runs of one instance do not overlap
        assert np.all(a['starts'][1:] >= (a['starts'] + a['runs'])[:-1])
