"""The host planning of Morph Labels, Fill holes, Split Labels and the slab-by-slab components: pure numpy, no device, no library.

``labels.py`` holds the device drivers of these tools; what they decide on the host before and between the launches lives
here, as functions over plain arrays and a ``LabelTable`` (anything with its ``labels``, ``areas``, ``boxes``, ``shape``):

* Morph Labels / Fill holes: the footprints, the turns with their boxes (``_morph_turns``), the levels (``morph_schedule``), the
  tile lists (``_morph_tiles``) and where a turn's entries lie inside its level's work arrays (``fill_placement``);
* Split Labels: the turns (``split_turns``), the rule that gives the largest label a pass of its own (``split_passes``), the
  screening of the boxes (``split_screen``), the boxes of a launch (``_split_batches``, ``split_boxes``), the markers of every box
  (``split_point_markers`` / ``split_peak_markers`` with ``split_spacing``, then ``split_marker_array`` with ``split_marker_ids``)
  and the ids the reference's loop hands out turn by turn (``split_ids``);
* connected components slab by slab (``labels.label_components``): how an array is cut (``components_geometry``,
  ``components_slab`` with the cap of the default slab) and what is refused, with the texts (``components_check_labels``,
  ``components_check_count``);
* Shape Labels (``labels.shape_labels``): the half-directions of the intercept columns (``shape_directions``), the Crofton weights
  of a spacing (``crofton_weights``; scipy's spherical Voronoi cells, imported when it is called) and the surface or perimeter
  they give (``crofton_size``).

This module imports numpy only, so all of it is tested without a device (tests/test_labelplan_host.py)."""
import numpy as np

MORPH_OPS = {'Dilate': 0, 'Erode': 1, 'Close': 2, 'Open': 3}      # the widget's strings (_merge_split_widget.py:48-53) -> EMP_MORPH_*
MORPH_MAX_RADIUS = 7      # the widget's slider (:73)
_MORPH_GROWS = ('Dilate', 'Close')

FILL_MAX_HOLE_SIZE = (1 << 31) - 1      # no component can have more voxels: a level's boxes hold fewer (FILL_MAX_LEVEL_VOXELS)
FILL_MAX_LEVEL_VOXELS = (1 << 31) - 1      # emp_fill_holes_labels: int32 entries of the parent / size arrays

SPLIT_MAX_DISTANCE = 100      # the widget's slider (_merge_split_widget.py:461)
SPLIT_MAX_BOXES = 65535      # emp_split_*: boxes per launch
SPLIT_MAX_ENTRIES = (1 << 31) - 2      # ... and their voxels
SPLIT_MAX_DIAGONAL2 = 1 << 30      # nz^2 + ny^2 + nx^2 of a box stays below EMP_SPLIT_INF
SPLIT_MAX_MARKERS = 0x3fffffff      # emp_split_flood: a marker's id in a label

COMPONENTS_MAX_LABEL = (1 << 31) - 2      # emp_ccl_range: labels below 2^31 - 1
COMPONENTS_MAX_SLAB_VOXELS = 1 << 30      # emp_ccl_range: depth * H * W < 2^30, so one slice and an explicit slab must stay below
COMPONENTS_SLAB_VOXELS = 1 << 28      # the default slab holds at most this many
COMPONENTS_MAX_COUNT = (1 << 31) - 2      # int32 ids 1..count; also the provisional per-slab ids of emp_ccl_seam's parent array


# ----------------------------------------------------------------------------
# shared by the three tools
# ----------------------------------------------------------------------------
def dims3(shape):
    """(D, H, W) of a 2-D or 3-D shape: an image is a volume of one slice"""
    return (1,) * (3 - len(shape)) + tuple(shape)


def box3(lo, hi):
    """a 2-D or 3-D box (exclusive upper ends) on three axes: an image's box has the one slice [0, 1)"""
    pad = 3 - len(lo)
    return np.concatenate([np.zeros(pad, np.int64), lo]), np.concatenate([np.ones(pad, np.int64), hi])


def table_rows(table, ids):
    """per id its row of the whole-array ``table``, -1 where the id does not occur (0 is the background: never a row)"""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    if not len(table.labels) or not len(ids):
        return np.full(len(ids), -1, np.int64)
    pos = np.minimum(np.searchsorted(table.labels, ids), len(table.labels) - 1)
    return np.where((ids > 0) & (table.labels[pos] == ids), pos, -1)


# ----------------------------------------------------------------------------
# connected components, slab by slab
# ----------------------------------------------------------------------------
def components_geometry(shape, what='label_components'):
    """(rows, H, W) of a 2-D or 3-D array as the slab stream cuts it: a volume by slices, an image (R, W) by rows, as R slices of
    one row (the kernels' (z, y, x) = the image's (row, 0, column)).  One slice must be one the CCL can take."""
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (2, 3):
        raise ValueError(f'{what}: 2-D or 3-D label arrays, got shape {shape}')
    rows, H, W = (shape[0], 1, shape[1]) if len(shape) == 2 else shape
    if H * W >= COMPONENTS_MAX_SLAB_VOXELS:
        raise ValueError(f'{what}: one slice of the array, {H} x {W}, holds 2^30 voxels or more; the components of a slab need fewer')
    return rows, H, W


def components_slab(rows, slice_voxels, slab, planned, what='label_components'):
    """The slices per slab.  ``slab=None``: ``planned``, the slab stream's own choice (everything for a device tensor, about 64 MiB
    of a host source), capped so that a slab holds at most 2^28 voxels -- about 4 GiB of CCL work memory at 16 bytes per voxel --
    and never below one slice.  An explicit ``slab`` is taken as given (at most all rows) and refused, from the shape alone, when
    its slab would hold 2^30 voxels or more."""
    if slab is None:
        return max(1, min(int(planned), COMPONENTS_SLAB_VOXELS // max(1, slice_voxels)))
    if isinstance(slab, bool) or int(slab) != slab or int(slab) < 1:
        raise ValueError(f'{what}: slab must be a positive number of slices, got {slab!r}')
    slab = min(int(slab), max(rows, 1))
    if slab * slice_voxels >= COMPONENTS_MAX_SLAB_VOXELS:
        raise ValueError(f'{what}: a slab of {slab} slices of {slice_voxels} voxels holds 2^30 voxels or more; pass a smaller slab= '
                         '(or none: the default slab holds at most 2^28)')
    return slab


def components_check_labels(top, what='label_components'):
    """the largest label of the array against what emp_ccl_range reads as a label"""
    if int(top) > COMPONENTS_MAX_LABEL:
        raise ValueError(f'{what}: the connected components need labels below 2^31 - 1, the array holds {int(top)}')


def components_check_count(n, what='label_components'):
    """``n``: the components of all slabs so far, each a provisional id of the int32 union-find over them"""
    if int(n) > COMPONENTS_MAX_COUNT:
        raise ValueError(f'{what}: more than 2^31 - 2 components ({int(n)} over the slabs so far); nothing was written')


# ----------------------------------------------------------------------------
# Morph Labels and Fill holes
# ----------------------------------------------------------------------------
def _morph_args(operation, radius, what):
    if operation not in MORPH_OPS:
        raise ValueError(f"{what}: operation must be one of {list(MORPH_OPS)}, got {operation!r} ('Fill holes' is fill_label_holes)")
    if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= MORPH_MAX_RADIUS:
        raise ValueError(f'{what}: radius must be an integer in 1..{MORPH_MAX_RADIUS}, got {radius!r}')
    return int(radius)


def morph_footprint_rows(radius, ball):
    """The footprint as the kernel walks it: rows (dz, dy, h) of ``disk(radius)`` (``ball`` false: dz = 0 only) or
    ``ball(radius)``, each the x-interval [-h, h] with h = floor(sqrt(r^2 - dy^2 - dz^2)) in integers."""
    r = _morph_args('Dilate', radius, 'morph_footprint_rows')
    rows = []
    for dz in (range(-r, r + 1) if ball else (0,)):
        for dy in range(-r, r + 1):
            rem = r * r - dz * dz - dy * dy
            if rem < 0:
                continue
            h = 0
            while (h + 1) * (h + 1) <= rem:
                h += 1
            rows.append((dz, dy, h))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def morph_footprint_offsets(radius, ndim):
    """the offsets (k, ndim) of ``disk(radius)`` (ndim 2) / ``ball(radius)`` (ndim 3), sorted: ``morph_footprint_rows`` expanded"""
    if ndim not in (2, 3):
        raise ValueError('morph_footprint_offsets: ndim 2 (disk) or 3 (ball)')
    offs = [(dz, dy, dx) for dz, dy, h in morph_footprint_rows(radius, ndim == 3).tolist() for dx in range(-h, h + 1)]
    offs = np.asarray(sorted(offs), dtype=np.int64).reshape(-1, 3)
    return offs if ndim == 3 else offs[:, 1:]


def _morph_turns(table, turns, radius, operation):
    """(ids, rows, lo, hi): per turn its label, its row of the table (-1: the id does not occur) and the box that holds the
    label's voxels when the turn comes (exclusive upper ends, not clipped): the table's box, grown by the radius for every
    earlier turn of the same id where the operation can grow a label."""
    if table.per_slice:
        raise ValueError('morph_schedule: a whole-array table is needed')
    ids = np.asarray(turns, dtype=np.int64).reshape(-1)
    nd = table.boxes.shape[1] // 2
    rows = table_rows(table, ids)
    lo = np.zeros((len(ids), nd), np.int64)
    hi = np.zeros((len(ids), nd), np.int64)
    earlier = {}
    for i, (l, row) in enumerate(zip(ids.tolist(), rows.tolist())):
        if row < 0:
            continue
        k = earlier.get(l, 0)
        earlier[l] = k + 1
        grow = radius * k if operation in _MORPH_GROWS else 0
        lo[i] = table.boxes[row, :nd] - grow
        hi[i] = table.boxes[row, nd:] + grow
    return ids, rows, lo, hi


def morph_schedule(table, turns, radius, operation):
    """The loop of Morph Labels over ``turns`` (label ids in the loop's order, a repeat being a second turn) as levels: a list
    of lists of turn indices.  The turns of a level can run in any order or at once, the levels in order, with the result of
    the sequential loop (_merge_split_widget.py:123-134).  Ids that do not occur in ``table`` are in no level.

    ``Erode`` / ``Open`` never leave a label's own voxels: every label is independent of every other, and everything is one
    level -- but for a repeated id, whose turns follow each other.  ``Dilate`` / ``Close`` write into the box padded by the
    radius: two turns conflict when their padded boxes intersect, and a turn's level is 1 + the highest level of an earlier
    turn it conflicts with.  A turn's box is the ``LabelTable``'s; a repeated id's later turns take it grown by the radius per
    earlier turn, which is where that label can have got to by then."""
    radius = _morph_args(operation, radius, 'morph_schedule')
    ids, rows, lo, hi = _morph_turns(table, turns, radius, operation)
    grows = operation in _MORPH_GROWS
    level = np.zeros(len(ids), np.int64)      # 0: in no level
    plo, phi = lo - radius, hi + radius
    for i in range(len(ids)):
        if rows[i] < 0:
            continue
        if grows:
            hit = (rows[:i] >= 0) & (plo[:i] < phi[i]).all(axis=1) & (plo[i] < phi[:i]).all(axis=1)
        else:
            hit = ids[:i] == ids[i]
        level[i] = 1 + (level[:i][hit].max() if hit.any() else 0)
    return [np.flatnonzero(level == l).tolist() for l in range(1, int(level.max()) + 1 if len(level) else 1)]


def _morph_tiles(table, turns, radius, operation, ball, levels, core):
    """(tiles (n, 4) int32 {turn, z0, y0, x0}, level offsets (len(levels) + 1) int64, boxes (turns, 6) uint32, frames (turns, 6)
    int64 {z0, y0, x0, nz, ny, nx}): the tile lists of emp_morph_labels / emp_fill_holes_labels.  A turn's tiles cover its frame:
    the box its label can lie in, padded by the radius and clipped to the array."""
    ids, rows, lo, hi = _morph_turns(table, turns, radius, operation)
    shape = np.asarray(dims3(table.shape), np.int64)
    pad = np.asarray([radius if (ball or a > 0) else 0 for a in range(3)], np.int64)
    boxes = np.zeros((len(ids), 6), np.uint32)
    boxes[:, :3] = 0xffffffff
    frames = np.zeros((len(ids), 6), np.int64)
    tiles, offsets, n = [], [0], 0
    for k, lvl in enumerate(levels):
        for i in lvl:
            l3, h3 = box3(lo[i], hi[i])
            if k == 0:      # nothing has been written yet: the table's box is the label's box
                boxes[i, :3], boxes[i, 3:] = l3, h3 - 1
            a = np.maximum(l3 - pad, 0)
            b = np.minimum(h3 + pad, shape)
            frames[i, :3], frames[i, 3:] = a, b - a
            grid = np.meshgrid(*[np.arange(a[d], b[d], core[d]) for d in range(3)], indexing='ij')
            tiles.append(np.stack([np.full(grid[0].size, i, np.int64)] + [g.reshape(-1) for g in grid], axis=1))
            n += grid[0].size
        offsets.append(n)
    tiles = np.concatenate(tiles).astype(np.int32) if tiles else np.zeros((0, 4), np.int32)
    return np.ascontiguousarray(tiles), np.asarray(offsets, np.int64), boxes, frames


def fill_placement(frames, levels):
    """Where the entries of Fill holes' parent and size arrays lie: ``frames`` (turns, 6) and the ``levels`` of ``_morph_tiles``
    -> (placed (turns, 7) int64: a frame and its offset, the number of entries).  A turn's entries follow those of the turns
    before it in its level, and the arrays are as large as the largest level."""
    placed = np.zeros((len(frames), 7), np.int64)
    placed[:, :6] = frames
    entries = 0
    for k, lvl in enumerate(levels):
        voxels = frames[lvl, 3:].prod(axis=1)
        if int(voxels.sum()) >= FILL_MAX_LEVEL_VOXELS:
            raise ValueError(f'fill_label_holes: the padded boxes of the turns of level {k} hold {int(voxels.sum())} voxels; a level '
                             'must hold fewer than 2^31 - 1 (pass fewer or smaller labels as ids=)')
        placed[lvl, 6] = np.cumsum(voxels) - voxels
        entries = max(entries, int(voxels.sum()))
    return placed, entries


# ----------------------------------------------------------------------------
# Split Labels
# ----------------------------------------------------------------------------
def split_spacing(coords, values, min_distance):
    """``ensure_spacing`` of ``peak_local_max``, restated: the candidates ``coords`` (n, ndim) with their ``values`` by value
    descending, stable over the order given (raster order); one is kept unless a kept one lies at Euclidean distance
    < ``min_distance`` (strictly) -> the indices kept, in the order they were kept.  Recalled from skimage's source, not pinned."""
    if len(values) == 0:
        return np.zeros(0, np.int64)
    coords = np.asarray(coords, dtype=np.int64).reshape(len(values), -1)
    order = np.argsort(-np.asarray(values, dtype=np.int64), kind='stable')
    kept = np.zeros((len(order), coords.shape[1]), np.int64)
    idx, n, d2 = [], 0, int(min_distance) ** 2
    for i in order.tolist():
        if n and (((kept[:n] - coords[i]) ** 2).sum(axis=1) < d2).any():
            continue
        kept[n] = coords[i]
        n += 1
        idx.append(i)
    return np.asarray(idx, dtype=np.int64)


def split_marker_ids(coords):
    """``ndi.label(marker mask)[0]`` (connectivity 1, _merge_split_widget.py:446,454) at the voxels ``coords`` (n, ndim) without
    the mask: voxels that are face neighbours share an id, and ids count the components in raster order of their first voxel
    -> (ids (n,) int64 from 1, the number of components).  A voxel given twice is one voxel."""
    coords = np.asarray(coords, dtype=np.int64)
    if len(coords) == 0:
        return np.zeros(0, np.int64), 0
    where = {tuple(c): i for i, c in enumerate(coords.tolist())}
    parent = list(range(len(coords)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for i, c in enumerate(coords.tolist()):
        parent[i] = find(where[tuple(c)])      # a repeated voxel
        for a in range(len(c)):
            j = where.get(tuple(c[:a] + [c[a] - 1] + c[a + 1:]))
            if j is not None:
                ri, rj = find(i), find(j)
                if ri != rj:
                    parent[max(ri, rj)] = min(ri, rj)
    ids, seen = np.zeros(len(coords), np.int64), {}
    for i in np.lexsort(coords.T[::-1]).tolist():
        ids[i] = seen.setdefault(find(i), len(seen) + 1)
    return ids, len(seen)


def split_turns(points, under, ids):
    """The turns of the loop, in ``np.unique`` order, zeros dropped (:498-517): the labels ``under`` the ``points`` (those on the
    background are dropped, :501-505), or ``ids`` -> (turns, the points kept, the labels under them); without points the last
    two are None."""
    if points is not None:
        return np.unique(under[under != 0]), points[under != 0], under[under != 0]
    turns = np.unique(np.asarray(ids, dtype=np.int64).reshape(-1))
    return turns[turns > 0], None, None


def split_passes(table, turns, start_label):
    """The turns in the groups that can each be computed in full before anything is written: one, or two.

    Computing everything first is the sequential loop as long as no turn writes an id that a later turn picks.  One can: a part
    of a label that no marker reaches becomes max_label itself (:544), the array's largest label, and when that label has a turn
    of its own -- the last one, the turns being sorted -- the loop lets it see those voxels.  So that turn is a second group,
    which runs on the array as the first left it."""
    if len(turns) > 1 and len(table.labels) and turns[-1] == table.labels.max() and (start_label is None or int(start_label) - 1 == turns[-1]):
        return [turns[:-1], turns[-1:]]
    return [turns]


def split_screen(table, turns, points_as_markers):
    """Which turns have something to compute -> (report, todo): the report with 'label absent' and 'nothing to split' filled in
    and None for the turns still open; per open turn a row of ``todo`` (m, 7) int64 {its index among the turns, the start z0, y0,
    x0 and the sides nz, ny, nx of its label's box on three axes}.  A label that fills its box has no background: nothing to
    split by distance.  A box the kernels cannot index raises a ``ValueError``."""
    nd = len(table.shape)
    report, todo = [None] * len(turns), []
    for i, row in enumerate(table_rows(table, turns).tolist()):
        if row < 0:
            report[i] = 'label absent'
            continue
        l3, h3 = box3(table.boxes[row, :nd], table.boxes[row, nd:])
        n3 = h3 - l3
        if not points_as_markers and int(n3.prod()) == int(table.areas[row]):
            report[i] = 'nothing to split'
            continue
        if int((n3 ** 2).sum()) >= SPLIT_MAX_DIAGONAL2 or int(n3.prod()) > SPLIT_MAX_ENTRIES:
            raise ValueError(f'split_labels: the box of label {int(turns[i])}, {tuple(n3[3 - nd:].tolist())}, is too large: the squares of its '
                             'sides must add up to less than 2^30 and it must hold fewer than 2^31 - 1 voxels')
        todo.append([i, *l3, *n3])
    return report, np.asarray(todo, np.int64).reshape(-1, 7)


def _split_batches(voxels):
    """consecutive turns per launch: at most SPLIT_MAX_BOXES of them with at most SPLIT_MAX_ENTRIES voxels"""
    batches, cur, n = [], [], 0
    for i, v in enumerate(voxels):
        if cur and (len(cur) == SPLIT_MAX_BOXES or n + v > SPLIT_MAX_ENTRIES):
            batches.append(cur)
            cur, n = [], 0
        cur.append(i)
        n += v
    return batches + ([cur] if cur else [])


def split_boxes(turns, todo):
    """the boxes of a launch as emp_split_* read them, from its rows of ``split_screen``'s ``todo``: (n, 8) int64 {z0, y0, x0, nz,
    ny, nx, offset of the box's first voxel among the launch's entries, label}"""
    boxes = np.zeros((len(todo), 8), np.int64)
    boxes[:, :6], boxes[:, 7] = todo[:, 1:], turns[todo[:, 0]]
    voxels = boxes[:, 3:6].prod(axis=1)
    boxes[:, 6] = np.cumsum(voxels) - voxels
    return boxes


def split_point_markers(points, under, boxes):
    """points mode: per box the marker voxels (z, y, x) inside it, each once: the points on the box's label"""
    points3 = np.concatenate([np.zeros((len(points), 3 - points.shape[1]), np.int64), points], axis=1)
    return [np.unique(points3[under == box[7]] - box[:3], axis=0) for box in boxes]


def split_peak_markers(cand, counts, boxes, min_distance):
    """distance mode: per box the marker voxels (z, y, x) inside it: of the box's candidates {box, linear index, value} -- the
    rows of ``cand`` box after box, ``counts`` of them each -- those that ``split_spacing`` keeps"""
    per_box = []
    for box, mine in zip(boxes, np.split(cand, np.cumsum(counts)[:-1])):
        coords = np.stack(np.unravel_index(mine[:, 1], tuple(box[3:6])), axis=1).reshape(-1, 3)
        per_box.append(coords[split_spacing(coords, mine[:, 2], min_distance)])
    return per_box


def split_marker_array(per_box, boxes):
    """The markers of a launch from the marker voxels of its boxes -> (markers (m, 3) int32 {box, linear index in the box, id from
    1}, the number of markers per box).  Face neighbours are one marker (``split_marker_ids``); a box with fewer than two has
    nothing to split and nothing to flood, and none of its voxels are listed."""
    markers, n_markers = [], np.zeros(len(boxes), np.int64)
    for k, coords in enumerate(per_box):
        mids, n_markers[k] = split_marker_ids(coords)
        if n_markers[k] >= 2:
            lin = np.ravel_multi_index(tuple(coords.T), tuple(boxes[k, 3:6]))
            markers.append(np.stack([np.full(len(lin), k, np.int64), lin, mids], axis=1))
    if len(n_markers) and n_markers.max() > SPLIT_MAX_MARKERS:
        raise ValueError(f'split_labels: more than 2^30 - 1 markers in one label')
    markers = np.ascontiguousarray(np.concatenate(markers).astype(np.int32)) if markers else np.zeros((0, 3), np.int32)
    return markers, n_markers


def split_ids(turns, report, launches, cur_max, start_label, eb):
    """The ids, turn by turn as the loop would hand them out (:533-545), before anything is written.  ``report``: that of
    ``split_screen``; ``launches``: per launch (the indices of its turns, their numbers of markers); ``cur_max``: the array's
    largest label; ``eb``: the array's element size in bytes, negative for a signed type: the new ids must fit it.
    -> (the report completed: per turn the new ids, 'nothing to split' or 'ids in use'; per launch the ``bases`` of its boxes:
    max_label, or -1 where nothing is written).  ``max_label`` is the array's maximum when the turn comes -- it moves with every
    split -- or ``start_label - 1``, and the write is refused when the maximum is >= the smallest new id (:540)."""
    top = min((1 << (8 * abs(eb) - (1 if eb < 0 else 0))) - 1, (1 << 63) - 1)
    report, all_bases = list(report), []
    for which, n_markers in launches:
        bases = np.full(len(which), -1, np.int64)
        all_bases.append(bases)
        for k, i in enumerate(which):
            n = int(n_markers[k])
            if n < 2:
                report[i] = 'nothing to split'
                continue
            max_label = cur_max if start_label is None else int(start_label) - 1
            if cur_max >= max_label + 1:
                report[i] = 'ids in use'
                continue
            if max_label + n > top:
                raise ValueError(f'split_labels: the new ids of label {int(turns[i])}, up to {max_label + n}, do not fit the '
                                 f'array\'s {abs(eb)}-byte {"signed" if eb < 0 else "unsigned"} type; nothing was written')
            bases[k] = max_label
            cur_max = max_label + n
            report[i] = max_label + np.arange(1, n + 1, dtype=np.int64)
    return report, all_bases


# ----------------------------------------------------------------------------
# Shape Labels: the directions, the Crofton weights and what follows from the intercept counts
# ----------------------------------------------------------------------------
def shape_directions(ndim):
    """(13, 3) or (4, 2): the half-directions of the 26- / 8-neighbourhood, the offsets in {-1, 0, 1}^ndim whose first non-zero
    component is +1, in ascending lexicographic order -- the columns of ``LabelShapes.intercepts``"""
    import itertools
    return np.array([d for d in itertools.product((-1, 0, 1), repeat=ndim) if any(d) and next(v for v in d if v) > 0], dtype=np.int64)


SHAPE_IMAGE_COLUMNS = (0, 7, 8, 9)      # an image (R, W) goes through the kernel as the volume (R, 1, W): its directions there
SHAPE_AXIS_COLUMNS = {3: (8, 2, 0), 2: (2, 0)}      # the columns of the axis directions: measure_labels' faces


def shape_spacing(spacing, ndim, per_slice):
    """the voxel size per column: ``ndim`` positive values, default 1; a stack's (z, y, x) gives its images' (y, x)"""
    if spacing is None:
        return (1.0,) * ndim
    try:
        sp = tuple(float(v) for v in np.asarray(spacing, dtype=np.float64).reshape(-1))
    except (TypeError, ValueError):
        sp = ()
    if per_slice and len(sp) == 3:
        sp = sp[1:]
    if len(sp) != ndim or not all(np.isfinite(v) and v > 0 for v in sp):
        raise ValueError(f'shape_labels: spacing needs {ndim} positive values, got {spacing}')
    return sp


def crofton_weights(spacing=None, ndim=3):
    """(13,) or (4,): per half-direction d_k the share c_k of the unit sphere (circle) that is nearer to +-d_k * spacing than to any
    other direction; they sum to 1.  3-D: the areas of the spherical Voronoi cells of the 26 unit vectors (scipy), +- summed;
    2-D: a direction's cell reaches half way to its two neighbours on the circle."""
    sp = np.asarray(shape_spacing(spacing, ndim, False), dtype=np.float64)
    d = shape_directions(ndim) * sp
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    if ndim == 2:
        ang = np.arctan2(u[:, 0], u[:, 1])      # the four half-directions lie in [0, pi); the other four are opposite
        order = np.argsort(ang)
        a = ang[order]
        gaps = np.diff(np.concatenate([a, [a[0] + np.pi]]))      # to the next direction; the last one's next is the first's opposite
        c = np.empty(4)
        c[order] = (gaps + np.roll(gaps, 1)) / (2.0 * np.pi)
        return c
    from scipy.spatial import SphericalVoronoi
    areas = SphericalVoronoi(np.concatenate([u, -u])).calculate_areas()
    return (areas[:13] + areas[13:]) / (4.0 * np.pi)


def crofton_size(intercepts, spacing):
    """The Cauchy-Crofton surface (13 columns) or perimeter (4 columns) of every row of intercept counts: chords per direction
    (half the intercepts) times the area (length) per lattice line of that direction, v / |d_k * spacing|, averaged over the
    sphere (circle) with ``crofton_weights``, times 4 (times pi)."""
    intercepts = np.asarray(intercepts)
    ndim = 3 if intercepts.shape[1] == 13 else 2
    sp = np.asarray(spacing, dtype=np.float64)
    per_line = float(np.prod(sp)) / np.linalg.norm(shape_directions(ndim) * sp, axis=1)
    terms = intercepts * (crofton_weights(sp, ndim) * per_line)
    return (2.0 if ndim == 3 else np.pi / 2.0) * terms.sum(axis=1)


# ----------------------------------------------------------------------------
# Contact Labels: what follows from the pair counts per half-direction
# ----------------------------------------------------------------------------
def contact_spacing(spacing, ndim):
    """``shape_spacing`` with the tool's own name in the error"""
    try:
        return shape_spacing(spacing, ndim, False)
    except ValueError:
        raise ValueError(f'label_contacts: spacing needs {ndim} positive values, got {spacing}') from None


def contact_face_sizes(spacing):
    """per axis the physical size of a voxel face perpendicular to it (an image: of a pixel edge): the product of the other spacings"""
    sp = np.asarray(spacing, dtype=np.float64)
    return float(np.prod(sp)) / sp


def contact_sizes(pairs, spacing):
    """The Cauchy-Crofton area (13 columns) or length (4 columns) of the surface every row's pairs cross: a pair along d_k is one
    crossing of a lattice line of that direction, which is one intercept of either label, so this is ``crofton_size`` of the pair
    counts: 2 sum_k c_k N_k v / |d_k * spacing| (an image: pi / 2 in place of 2)"""
    pairs = np.asarray(pairs)
    if len(pairs) == 0:
        return np.zeros(0, np.float64)
    return crofton_size(pairs, spacing)


def contact_fold_classes(a, b, pairs, label_divisor):
    """the table over (a // divisor, b // divisor), lower class first: (ca, cb, pairs) sorted by (ca, cb), the columns summed.  Pairs
    of two instances of one class are kept as (c, c); the background stays class 0"""
    div = int(label_divisor)
    if div < 1:
        raise ValueError(f'by_class: label_divisor must be positive, got {label_divisor}')
    ca, cb = np.asarray(a, np.int64) // div, np.asarray(b, np.int64) // div
    lo, hi = np.minimum(ca, cb), np.maximum(ca, cb)
    both = np.stack([lo, hi], axis=1)
    keys, inv = np.unique(both, axis=0, return_inverse=True)
    out = np.zeros((len(keys), np.asarray(pairs).shape[1]), np.int64)
    np.add.at(out, inv.reshape(-1), np.asarray(pairs, np.int64))
    return keys[:, 0].copy(), keys[:, 1].copy(), out


def contact_groups(a, b, keep):
    """The groups of labels that the kept rows join, by union-find on the host: a list of ascending int64 id arrays, each of two ids
    or more, in ascending order of their smallest id"""
    a, b = np.asarray(a, np.int64)[keep], np.asarray(b, np.int64)[keep]
    ids, inv = np.unique(np.concatenate([a, b]), return_inverse=True)
    parent = list(range(len(ids)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i, j in zip(inv[:len(a)].tolist(), inv[len(a):].tolist()):
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)      # the root is the smallest id: ids is sorted
    groups = {}
    for i in range(len(ids)):
        groups.setdefault(find(i), []).append(int(ids[i]))
    return [np.array(g, np.int64) for _, g in sorted(groups.items()) if len(g) > 1]
