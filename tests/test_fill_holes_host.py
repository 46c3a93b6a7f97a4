"""Host side of Fill holes (empanada_napari_amd.labels.fill_label_holes): that the inputs of the device tests have what they are
for, that the schedule of a dilation reproduces the sequential loop, and the argument checks.  No device is needed: the levels
are emulated with the scipy statement of tests/fill_holes_case.py and compared with its sequential loop."""
import functools

import numpy as np
import pytest

import fill_holes_case as FC
import labels_case as LC


def _table(arr):
    from empanada_napari_amd import labels as L
    labels, areas, boxes = LC.want_table(arr)
    return L.table_from_arrays(labels, areas, boxes, arr.shape)


@functools.lru_cache(maxsize=None)
def _case(name):
    arr = {'image': lambda: FC.holes((96, 96), 40, 11), 'volume': lambda: FC.holes((24, 40, 40), 30, 13)}[name]()
    arr.setflags(write=False)
    return arr


def test_remove_small_holes_by_hand():
    """a 3 x 3 hole joined to a single voxel by a corner: two components of connectivity 1 (9 and 1 voxels), one of connectivity
    2; the border component (the rest of the frame) is a component like any other"""
    b = np.ones((8, 9), bool)
    b[0, :] = False      # 9 voxels that touch the border
    b[2:5, 2:5] = False
    b[5, 5] = False
    assert np.array_equal(FC.remove_small_holes(b, 0), b) and np.array_equal(FC.remove_small_holes(b, 1), b)
    one = FC.remove_small_holes(b, 2)
    assert one[5, 5] and not one[2:5, 2:5].any() and not one[0].any()
    nine = FC.remove_small_holes(b, 9)
    assert nine[5, 5] and not nine[2:5, 2:5].any() and not nine[0].any()      # strict: 9 < 9 is false
    assert FC.remove_small_holes(b, 10).all()      # the hole and the border component go together
    assert not FC.remove_small_holes(b, 10, connectivity=2)[2:5, 2:5].any()      # 10 voxels as one component
    assert FC.remove_small_holes(b, 9, strict=False)[2:5, 2:5].all()


def test_the_image_has_what_it_is_for():
    arr = _case('image')
    want, skipped = FC.fill(arr, 1, 64)
    assert (want != arr).sum() > 300
    assert ((want != arr) & (arr != 0)).sum() > 50      # voxels of other labels overwritten
    assert skipped >= 3 and len(np.unique(want)) <= len(np.unique(arr)) - 3      # labels disappear, their turns are skipped
    out, full = np.array(arr), 0
    for label in FC.turns_of(out):      # turns that fill their whole crop: the ring around the label is a small component
        nz = np.nonzero(out == label)
        if len(nz[0]) == 0:
            continue
        sl = tuple(slice(max(0, int(c.min()) - 1), min(s, int(c.max()) + 2)) for c, s in zip(nz, out.shape))
        FC.turn(out, label, 1, 64)
        full += bool((out[sl] == label).all())
    assert np.array_equal(out, want) and full >= 10
    assert (want != FC.fill_whole_array(arr, 1, 64)).sum() > 300
    assert (want != FC.fill_connectivity2(arr, 1, 64)).sum() >= 10
    assert (want != FC.fill_le(arr, 1, 64)).sum() >= 10
    assert (want != FC.fill_original_boxes(arr, 1, 64)).sum() >= 10
    for hole_size in (0, 1):
        assert np.array_equal(FC.fill(arr, 1, hole_size)[0], arr)


def test_the_volume_has_what_it_is_for():
    vol = _case('volume')
    assert (FC.fill(vol, 1, 64)[0] != FC.fill_connectivity2(vol, 1, 64)).sum() >= 10
    assert (FC.fill(vol, 1, 8)[0] != FC.fill_le(vol, 1, 8)).sum() >= 4
    assert (FC.fill(vol, 3, 10 ** 6)[0] != FC.fill_original_boxes(vol, 3, 10 ** 6)).sum() > 0
    assert not np.array_equal(FC.fill(vol, 1, 8)[0], vol)


@pytest.mark.parametrize('name', ['image', 'volume'])
@pytest.mark.parametrize('radius,hole_size', [(1, 64), (3, 8), (7, 64), (3, 10 ** 6)])
def test_the_schedule_of_a_dilation_reproduces_the_loop(name, radius, hole_size):
    """a Fill holes turn writes only inside its padded box and reads only `== label`; a repeated id can have grown by the radius
    per earlier turn: levels in order, the turns of a level in reverse order, give the sequential loop"""
    from empanada_napari_amd import labels as L
    arr = _case(name)
    t = _table(arr)
    present = t.labels[t.labels != 0]
    repeats = np.concatenate([present[::-1], present[[2, 2, 5]], present[::-1][:4]])
    for turns in (present, repeats):
        levels = L.morph_schedule(t, turns, radius, 'Dilate')
        want, _ = FC.fill(arr, radius, hole_size, ids=turns)
        assert np.array_equal(FC.fill_by_levels(arr, turns, levels, radius, hole_size), want)
        assert len(levels) > 1 and not np.array_equal(want, arr)


def test_plane_statement():
    vol = _case('volume')
    got = FC.fill_plane(vol, 1, 64, 7, 0)
    assert np.array_equal(got[7], FC.fill(vol[7], 1, 64)[0]) and not np.array_equal(got[7], vol[7])
    assert np.array_equal(np.delete(got, 7, 0), np.delete(vol, 7, 0))


def test_argument_errors(tmp_path):
    from empanada_napari_amd import labels as L, zstore
    img = np.zeros((8, 8), np.int32)
    vol = np.zeros((4, 8, 8), np.int32)
    for hole_size in (-1, 1.5, True, '64', None):
        with pytest.raises(ValueError, match='hole_size'):
            L.fill_label_holes(img, hole_size=hole_size)
    for radius in (0, 8, 1.5, True):
        with pytest.raises(ValueError, match='radius'):
            L.fill_label_holes(img, radius=radius)
    with pytest.raises(ValueError, match='apply3d=True'):
        L.fill_label_holes(vol)
    with pytest.raises(ValueError, match='plane'):
        L.fill_label_holes(vol, plane=4, axis=0)
    with pytest.raises(ValueError, match='2-D or 3-D'):
        L.fill_label_holes(np.zeros((2, 2, 4, 4), np.int32), apply3d=True)
    store = zstore.DirArray.create(str(tmp_path / 'store'), vol.shape, vol.dtype, (2, 8, 8), overwrite=True)
    with pytest.raises(ValueError, match='chunked store'):
        L.fill_label_holes(store, apply3d=True, inplace=True)
    with pytest.raises(TypeError, match='integer label type'):
        L.fill_label_holes(img.astype(np.float32))
    with pytest.raises(ValueError, match='operation.*fill_label_holes'):      # Morph Labels' own entry points at this one
        L.morph_labels(img, 'Fill holes')


def test_tile_shape_of_the_library():
    """no halo: a tile's row is 64 core voxels"""
    import ctypes as C
    from empanada_napari_amd import _abi
    lib = _abi.load(build_if_missing=True)
    for ball, want in ((0, (1, 64, 64)), (1, (8, 16, 64))):
        cz, cy, cx = C.c_int(0), C.c_int(0), C.c_int(0)
        assert lib.emp_fill_holes_tile_shape(ball, C.byref(cz), C.byref(cy), C.byref(cx)) == 0
        assert (cz.value, cy.value, cx.value) == want


def test_frames_hold_the_padded_boxes_and_tiles_cover_them():
    """the scratch layout of emp_fill_holes_labels: a turn's frame is its table box, grown by the radius per earlier turn of the
    same id, padded and clipped; its tiles start inside it and their cores cover it"""
    from empanada_napari_amd import labels as L
    arr = _case('volume')
    t = _table(arr)
    present = t.labels[t.labels != 0]
    turns = np.concatenate([present, present[:3]])
    radius, core = 3, (8, 16, 64)
    levels = L.morph_schedule(t, turns, radius, 'Dilate')
    tiles, offsets, boxes, frames = L._morph_tiles(t, turns, radius, 'Dilate', True, levels, core)
    assert offsets[0] == 0 and offsets[-1] == len(tiles) and len(offsets) == len(levels) + 1
    shape = np.asarray(arr.shape)
    for i, label in enumerate(turns.tolist()):
        row = int(np.searchsorted(t.labels, label))
        grown = radius * (2 if i >= len(present) else 1)
        lo = np.maximum(t.boxes[row, :3] - grown, 0)
        hi = np.minimum(t.boxes[row, 3:] + grown, shape)
        assert np.array_equal(frames[i, :3], lo) and np.array_equal(frames[i, 3:], hi - lo)
        mine = tiles[tiles[:, 0] == i][:, 1:]
        assert len(mine) == np.prod(-(-(hi - lo) // np.asarray(core)))
        assert (mine >= lo).all() and (mine < hi).all() and ((mine - lo) % np.asarray(core) == 0).all()
