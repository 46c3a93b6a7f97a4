"""Clean-up of label volumes on the device: the plugin's label tools without the trip to the host.

Two device primitives (csrc/labels.hip) carry everything:

* ``label_table``: for every label that occurs its voxel count and its bounding box, in one pass -- what
  ``regionprops_table(img, properties=('label', 'area'))`` (empanada_napari/_filter_small_labels.py:16), ``regionprops(...).bbox``
  (_merge_split_widget.py:653-655) and ``np.unique`` (_label_counter_widget.py:243, _merge_split_widget.py:730) give;
* the edit: one pass that rewrites a volume through a ``from -> to`` map, instead of one ``labels[labels == l] = v`` pass per label
  (_filter_small_labels.py:10-12, _merge_split_widget.py:249-250, :385-387).

On top of them, as pure numpy on a ``LabelTable`` (no device needed): ``small_labels``, ``boundary_labels``, ``count_labels``,
``class_label_lists``, ``next_available_labels``, ``next_available_label``, ``label_bbox``; and the edits ``delete_labels``,
``merge_labels``, ``filter_out_small_label_areas``, ``remove_boundary_labels``.

``morph_labels`` (csrc/morph.hip) is Morph Labels (_merge_split_widget.py:46-209): dilation, erosion, closing and opening of single
labels with a disk or ball, every label inside its own padded box.  ``morph_schedule`` (pure numpy) orders the loop's turns into
levels whose turns touch disjoint parts of the array; a level is two or three launches over the padded boxes of its turns.
``fill_label_holes`` is the widget's fifth operation, 'Fill holes' (``remove_small_holes`` inside the same padded box): the 4- /
6-connected components of the background of every crop, by union-find over the same levels and tile lists.
``split_labels`` (csrc/split.hip) is Split Labels (_merge_split_widget.py:422-634): per label an exact distance transform, the
candidates of ``peak_local_max`` and a marker flood inside the label's tight box, batched over the labels of a call; the greedy
spacing of the peaks (``split_spacing``), ``ndi.label`` of the few survivors (``split_marker_ids``) and the id bookkeeping run on
the host.

What these three tools decide on the host lives in ``_labelplan.py``, which imports numpy only: the footprints, ``morph_schedule``
and the tile lists, the placement of Fill holes' work arrays, and of Split Labels the turns, the rule that gives the largest label
a second pass, the screening of the boxes, the boxes and markers of a launch and the loop that hands out the new ids.  This module
keeps their device drivers (``_morph_device``, ``_fill_device``, ``_split_device``: allocate, upload, call the library) and
re-exports the public names.

Inputs are those of ``metrics.label_overlap``: device tensors (read in place), numpy arrays and chunked stores
(``zstore.DirArray``, zarr arrays) streamed in leading-axis slabs by ``_labelstream.stream_slabs``, which keeps a staged slab
intact until the work queued on it has run: no tool here synchronises for it.  Results go to a ``_labelstream.Sink``, whose
destination ``_edit_target`` / ``_components_target`` choose: kernels write a device tensor directly, host rows come down through
the sink's pinned buffer.  An edit returns the kind of object it was given: a device tensor for a device tensor, a new numpy array
for a numpy array (the caller's own only with ``inplace=True``), and for a store the store given as ``out=``, written slab by slab.

skimage is not available where this package is built and tested: what ``regionprops_table`` and ``clear_border`` compute is
restated from their documented behaviour (area = voxel count; bbox = minimum and exclusive maximum per axis; clear_border =
every connected component, full connectivity and equal value, that touches a face of the array is cleared) and is not pinned
against them.  ``count_labels`` is pure numpy in the reference and is pinned (tests/golden/labels.npz).

The one deliberate difference: on an image without labels the reference's ``filter_out_small_label_areas`` dies with an
``IndexError`` (``.iloc[0]`` of an empty frame, _filter_small_labels.py:20); here that case returns the image unchanged and 0.

``measure_labels`` (csrc/measure.hip) measures the objects of a label array in one pass: per label its voxel count, box, the raw
first and second moments of its voxel coordinates and its exposed voxel faces per axis, all integers; ``LabelMeasures`` derives
centroids, volumes, face surfaces, covariances and principal axes from them as pure numpy.

``shape_labels`` (csrc/shape.hip) counts, per label, the intercepts along the 13 half-directions of the 26-neighbourhood and the
Euler number under full and under face connectivity, again all integers; ``LabelShapes`` derives the Cauchy-Crofton surface (or
perimeter), the sphericity that goes with it and the Euler numbers as pure numpy, with the weights of ``crofton_weights``.

``label_contacts`` (csrc/contacts.hip) counts, per unordered pair of different labels that occur next to each other, the voxel pairs
that join them along the same 13 half-directions; ``LabelContacts`` derives shared faces, the Cauchy-Crofton contact area, the
adjacency matrix, the share of each label's surface and the groups a threshold on them joins (``merge_groups``, whose groups
``merge_labels`` takes) as pure numpy.

``label_components`` (csrc/components.hip) splits a label array of any size into its connected components, slab by slab: per slab
``emp_ccl_range``, across the seams a union-find over the slabs' component ids, then one numbering in raster order.
``remove_boundary_labels(streamed=True)`` is the reference mode on top of it, for arrays the one-call CCL cannot take.

There is no numpy fallback: without the HIP library or a device the device entries raise like every other entry of the package.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _abi, _labelplan as P
from ._labelplan import (FILL_MAX_HOLE_SIZE, FILL_MAX_LEVEL_VOXELS, MORPH_MAX_RADIUS, MORPH_OPS, SPLIT_MAX_BOXES, SPLIT_MAX_DIAGONAL2,  # noqa: F401
                         SPLIT_MAX_DISTANCE, SPLIT_MAX_ENTRIES, _MORPH_GROWS, _morph_args, _morph_tiles, _morph_turns, _split_batches, dims3,
                         crofton_weights, morph_footprint_offsets, morph_footprint_rows, morph_schedule, shape_directions, split_marker_ids, split_spacing)
from ._labelstream import GrowableTable, RawSource, Sink, ebytes, hp, initial_capacity, need_device, pick_device, slab_plan, source, stream_slabs

__all__ = ['LabelTable', 'label_table', 'table_from_arrays', 'LabelMeasures', 'measure_labels', 'measures_from_arrays', 'LabelShapes', 'shape_labels', 'shapes_from_arrays', 'LabelContacts', 'label_contacts', 'contacts_from_arrays', 'crofton_weights', 'shape_directions', 'small_labels', 'boundary_labels', 'count_labels', 'class_label_lists',
           'next_available_labels', 'next_available_label', 'label_bbox', 'delete_labels', 'merge_labels',
           'filter_out_small_label_areas', 'remove_boundary_labels', 'label_components', 'morph_labels', 'fill_label_holes', 'morph_schedule',
           'morph_footprint_rows', 'morph_footprint_offsets', 'split_labels', 'split_spacing', 'split_marker_ids']

CCL_MAX_VOXELS = 1 << 30      # emp_ccl_range: D * H * W < 2^30
CCL_MAX_LABEL = (1 << 31) - 2      # ... and labels below 2^31 - 1


@dataclass
class LabelTable:
    """The labels of an array with their sizes and boxes.

    Whole mode: ``labels`` ascending (``np.unique``, background 0 included where it occurs), ``areas`` their voxel counts,
    ``boxes`` (k, 2 * ndim) ``(min_0, .., min_n, max_0, .., max_n)`` with exclusive upper ends, as ``regionprops.bbox``;
    ``slices`` is None.  Per-slice mode (a 3-D array as a stack of images): one row per (slice, label) that occurs, sorted by
    slice, then label; ``slices`` holds the leading-axis index and ``boxes`` (k, 4) the box within the image.  ``shape``: the
    array's shape; ``doublings``: how often the device table had to grow."""
    labels: np.ndarray
    areas: np.ndarray
    boxes: np.ndarray
    slices: object = None
    shape: tuple = ()
    doublings: int = 0

    @property
    def per_slice(self):
        return self.slices is not None


def table_from_arrays(labels, areas, boxes, shape, slices=None, doublings=0):
    """LabelTable from host arrays (rows in any order, each key once)."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    areas = np.asarray(areas, dtype=np.int64).reshape(-1)
    shape = tuple(int(s) for s in shape)
    nd = 2 if slices is not None else len(shape)
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 2 * nd)
    if not (len(labels) == len(areas) == len(boxes)):
        raise ValueError('table_from_arrays: labels, areas and boxes differ in length')
    if slices is not None:
        if len(shape) != 3:
            raise ValueError('table_from_arrays: a per-slice table belongs to a 3-D array')
        slices = np.asarray(slices, dtype=np.int64).reshape(-1)
        order = np.lexsort((labels, slices))
        slices = slices[order]
    else:
        order = np.argsort(labels, kind='stable')
    return LabelTable(labels[order], areas[order], boxes[order], slices, shape, int(doublings))


# ----------------------------------------------------------------------------
# device: the table
# ----------------------------------------------------------------------------
def _geometry(shape, per_slice, what):
    """(rows, H, W) as the kernels see a slab of `rows` leading-axis entries.  A 2-D image (R, W) is R slabs of one row each:
    the kernels' z is the image's y, so that a host image is streamed by rows like a volume by slices."""
    if len(shape) == 3:
        return shape[0], shape[1], shape[2]
    if len(shape) == 2:
        if per_slice:
            raise ValueError(f'{what}: per_slice needs a 3-D array (a stack of images)')
        return shape[0], 1, shape[1]
    raise ValueError(f'{what}: 2-D or 3-D label arrays, got shape {shape}')


def _table_of_source(src, shape, per_slice, device, slab, capacity):
    rows, H, W = _geometry(shape, per_slice, 'label_table')
    table = GrowableTable('emp_label_table', 'label_table', capacity or initial_capacity(rows * H * W), device)
    for _, z0, z1, (address,) in stream_slabs([src], slab, device):
        table.add(address, src.ebytes, z0, z1 - z0, H, W, int(per_slice))
    keys, cnt, box = (t.cpu().numpy() for t in table.finalize(extra=[(6, torch.int32)]))      # the keys lie below 2^63
    box = box.astype(np.int64)
    if len(shape) == 2:      # kernel (z, y, x) = image (y, 0, x)
        box = box[:, [0, 2, 3, 5]]
    box[:, box.shape[1] // 2:] += 1      # exclusive upper ends
    if per_slice:
        return LabelTable(keys & 0xffffffff, cnt, box[:, [1, 2, 4, 5]], keys >> 32, tuple(shape), table.doublings)
    return LabelTable(keys, cnt, box, None, tuple(shape), table.doublings)


@torch.no_grad()
def label_table(labels, per_slice=False, device=None, slab=None, capacity=None):
    """The ``LabelTable`` of a 2-D or 3-D label array (any integer dtype of 1, 2, 4 or 8 bytes; values in [0, 2^63), per slice in
    [0, 2^32); anything else raises ``EmpError``).  ``labels``: a device tensor (read in place), a numpy array or a chunked
    store; host data is streamed in slabs of ``slab`` leading-axis entries (default: about 64 MiB).  ``per_slice``: a 3-D array
    as a stack of images, one row per (slice, label).  The result is exact, does not depend on ``slab`` and is
    bit-reproducible.  ``capacity``: first size of the device table in slots (it doubles when it is too small)."""
    need_device()
    device = pick_device(device, labels)
    with torch.cuda.device(device):
        src = source(labels, device)
        return _table_of_source(src, src.shape, bool(per_slice), device, slab, capacity)


# ----------------------------------------------------------------------------
# device: the measures
# ----------------------------------------------------------------------------
_PAIRS = {3: ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)), 2: ((0, 0), (1, 1), (0, 1))}      # the columns of sum2


@dataclass
class LabelMeasures:
    """What ``measure_labels`` counts, per label that occurs (background 0 left out), and what follows from it.

    The raw columns are integers and exact.  ``labels`` ascending, ``areas`` the voxel counts, ``boxes`` as ``LabelTable``'s;
    ``sum1`` (k, ndim) the sums of the voxels' index coordinates; ``sum2`` (k, 6) the sums of zz, yy, xx, zy, zx, yx, or (k, 3) of
    yy, xx, yx; ``faces`` (k, ndim) the exposed voxel faces perpendicular to each axis.  ndim is 3 for a volume and 2 for an image
    or, per slice, for the images of a stack: there is no z column then, columns read (y, x), ``slices`` holds the leading-axis
    index and rows are sorted by slice, then label.  ``spacing``: the voxel size per column; ``doublings``: how often the device
    table had to grow.

    Everything derived is pure numpy on these columns.  Coordinates are index coordinates (a voxel is the point at its index,
    ``regionprops``' convention), ``*_physical`` and everything with a unit is scaled by ``spacing``."""
    labels: np.ndarray
    areas: np.ndarray
    boxes: np.ndarray
    sum1: np.ndarray
    sum2: np.ndarray
    faces: np.ndarray
    slices: object = None
    shape: tuple = ()
    spacing: tuple = ()
    doublings: int = 0

    @property
    def per_slice(self):
        return self.slices is not None

    @property
    def ndim(self):
        return self.sum1.shape[1]

    @property
    def centroid(self):
        """(k, ndim) mean index coordinate, ``regionprops``' ``centroid``: one division of two exact integers"""
        return self.sum1 / self.areas[:, None]

    @property
    def centroid_physical(self):
        return self.centroid * np.asarray(self.spacing, dtype=np.float64)

    @property
    def volume(self):
        """voxel count times the voxel's volume (its area for ndim 2)"""
        return self.areas * float(np.prod(self.spacing))

    @property
    def surface_area(self):
        """The voxel-face surface: every exposed face with the area the spacing gives it.  It is the surface of the voxel
        model, not of a smooth object: for a smooth surface it overestimates by the ratio of the L1 to the L2 norm of the
        normal, up to 1.5 for a sphere (sqrt(3) on a diagonal plane).  For ndim 2 it is the pixel-edge perimeter
        (``perimeter_faces``)."""
        sp = np.asarray(self.spacing, dtype=np.float64)
        face = np.array([np.prod(np.delete(sp, a)) for a in range(self.ndim)])
        return (self.faces * face).sum(axis=1)

    @property
    def perimeter_faces(self):
        if self.ndim != 2:
            raise ValueError('perimeter_faces: for images; a volume has a surface_area')
        return self.surface_area

    @property
    def equivalent_diameter(self):
        """the diameter of the ball (the disk for ndim 2) of the same volume"""
        v = self.volume
        return np.cbrt(6.0 * v / np.pi) if self.ndim == 3 else np.sqrt(4.0 * v / np.pi)

    @property
    def sphericity(self):
        """pi^(1/3) (6 V)^(2/3) / A with the voxel-face surface A (for ndim 2 the circularity 4 pi A / P^2 with the pixel-edge
        perimeter).  A is the face surface, so no voxel object reaches 1: a cube has (pi / 6)^(1/3) = 0.806, a large digital
        ball about 2 / 3"""
        v, a = self.volume, self.surface_area
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.cbrt(np.pi) * np.cbrt(6.0 * v) ** 2 / a if self.ndim == 3 else 4.0 * np.pi * v / a ** 2

    def central_moments_exact(self):
        """(k, ndim, ndim) Python integers n sum(ab) - sum(a) sum(b): n^2 times the central second moments of the index
        coordinates.  The raw sums reach 2^60, so the subtraction is done before anything is rounded."""
        n = self.areas.astype(object)
        s1, s2 = self.sum1.astype(object), self.sum2.astype(object)
        m = np.empty((len(n), self.ndim, self.ndim), dtype=object)
        for j, (a, b) in enumerate(_PAIRS[self.ndim]):
            m[:, a, b] = m[:, b, a] = n * s2[:, j] - s1[:, a] * s1[:, b]
        return m

    @property
    def covariance(self):
        """(k, ndim, ndim) covariance of the voxel positions in physical units (voxels as points; one division of exact integers)"""
        n = self.areas.astype(object)
        cov = (self.central_moments_exact() / (n * n)[:, None, None]).astype(np.float64)
        sp = np.asarray(self.spacing, dtype=np.float64)
        return cov * sp[:, None] * sp[None, :]

    @property
    def principal_variances(self):
        """(k, ndim) eigenvalues of ``covariance``, largest first"""
        return np.linalg.eigvalsh(self.covariance)[:, ::-1] if len(self.labels) else np.zeros((0, self.ndim))

    @property
    def principal_axes(self):
        """(k, ndim, ndim): ``[i, j]`` is the unit vector (in the columns' axis order) of label i's j-th principal variance"""
        if not len(self.labels):
            return np.zeros((0, self.ndim, self.ndim))
        return np.linalg.eigh(self.covariance)[1][:, :, ::-1].transpose(0, 2, 1)

    def to_table(self):
        """dict of columns, ``regionprops_table``'s naming where it has one (``bbox-0``, ``centroid-1``, ...)"""
        nd = self.ndim
        out = {'slice': self.slices} if self.per_slice else {}
        out.update({'label': self.labels, 'area': self.areas})
        out.update({f'bbox-{i}': self.boxes[:, i] for i in range(2 * nd)})
        c, pv = self.centroid_physical, self.principal_variances
        out.update({f'centroid-{i}': c[:, i] for i in range(nd)})
        out.update({'volume': self.volume, 'surface_area': self.surface_area, 'equivalent_diameter': self.equivalent_diameter,
                    'sphericity': self.sphericity})
        out.update({f'principal_variance-{i}': pv[:, i] for i in range(nd)})
        return out

    def to_csv(self, path):
        import csv
        table = self.to_table()
        with open(path, 'w', newline='') as f:
            w = csv.writer(f)
            w.writerow(table)
            w.writerows(zip(*(col.tolist() for col in table.values())))


def _spacing(spacing, nd, per_slice):
    if spacing is None:
        return (1.0,) * nd
    sp = tuple(float(v) for v in np.asarray(spacing, dtype=np.float64).reshape(-1))
    if per_slice and len(sp) == 3:      # a stack's (z, y, x): the images have (y, x)
        sp = sp[1:]
    if len(sp) != nd or not all(v > 0 for v in sp):
        raise ValueError(f'measure_labels: spacing needs {nd} positive values, got {spacing}')
    return sp


def measures_from_arrays(labels, areas, boxes, sum1, sum2, faces, shape, spacing=None, slices=None, doublings=0):
    """LabelMeasures from host arrays (rows in any order, each key once)."""
    shape = tuple(int(s) for s in shape)
    nd = 2 if slices is not None else len(shape)
    cols = [np.asarray(labels, dtype=np.int64).reshape(-1), np.asarray(areas, dtype=np.int64).reshape(-1),
            np.asarray(boxes, dtype=np.int64).reshape(-1, 2 * nd), np.asarray(sum1, dtype=np.int64).reshape(-1, nd),
            np.asarray(sum2, dtype=np.int64).reshape(-1, len(_PAIRS[nd])), np.asarray(faces, dtype=np.int64).reshape(-1, nd)]
    if len({len(c) for c in cols}) != 1:
        raise ValueError('measures_from_arrays: the columns differ in length')
    if slices is not None:
        slices = np.asarray(slices, dtype=np.int64).reshape(-1)
        order = np.lexsort((cols[0], slices))
        slices = slices[order]
    else:
        order = np.argsort(cols[0], kind='stable')
    return LabelMeasures(*(c[order] for c in cols), slices, shape, _spacing(spacing, nd, slices is not None), int(doublings))


MEASURE_MAX_CAPACITY = 1 << 20      # first size of the table at most: a slot is 136 bytes


def _measures_of_source(src, shape, spacing, per_slice, border_faces, device, slab, capacity):
    rows, H, W = _geometry(shape, per_slice, 'measure_labels')
    nd = 2 if per_slice else len(shape)
    spacing = _spacing(spacing, nd, per_slice)
    if max(rows, H, W) ** 2 * rows * H * W >= 1 << 63:      # the entry's own rule, before anything is allocated
        raise ValueError(f'measure_labels: a raw second moment could wrap: max(D, H, W)^2 * D * H * W must stay below 2^63, got shape {shape}')
    table = GrowableTable('emp_label_measure', 'measure_labels', capacity or min(initial_capacity(rows * H * W), MEASURE_MAX_CAPACITY), device)
    # The slice below a slab's first one.  A device source has it in front of the slab.  A host source's previous slab lies in
    # the staging slot that the stream refills while this slab is counted, so its last slice is kept in a buffer of its own
    host_halo = src.is_host and not per_slice
    halo = torch.empty(max(1, src.row_bytes), dtype=torch.uint8, device=device) if host_halo else None
    for _, z0, z1, (address,) in stream_slabs([src], slab, device):
        below = None if per_slice or z0 == 0 else (halo.data_ptr() if host_halo else address - src.row_bytes)
        table.add(address, src.ebytes, z0, z1 - z0, H, W, rows, below, int(per_slice), int(bool(border_faces)))
        if host_halo and z1 < rows:
            _abi.check(table.lib.emp_copy_d2d(_abi.ptr(halo), address + (z1 - z0 - 1) * src.row_bytes, src.row_bytes, _abi.stream_ptr(device)),
                       'emp_copy_d2d')
    keys, cnt, box, sums, faces = (t.cpu().numpy() for t in table.finalize(extra=[(6, torch.int32), (9, torch.int64), (3, torch.int64)]))
    box = box.astype(np.int64)
    box[:, 3:] += 1      # exclusive upper ends
    s1, s2 = sums[:, :3], sums[:, 3:]
    if per_slice:      # the images' (y, x); the kernel's z is the slice
        return LabelMeasures(keys & 0xffffffff, cnt, box[:, [1, 2, 4, 5]], s1[:, [1, 2]], s2[:, [1, 2, 5]], faces[:, [1, 2]], keys >> 32,
                             tuple(shape), spacing, table.doublings)
    if len(shape) == 2:      # kernel (z, y, x) = image (y, 0, x): zz, xx, zx are the image's yy, xx, yx
        return LabelMeasures(keys, cnt, box[:, [0, 2, 3, 5]], s1[:, [0, 2]], s2[:, [0, 2, 4]], faces[:, [0, 2]], None, tuple(shape), spacing,
                             table.doublings)
    return LabelMeasures(keys, cnt, box, s1, s2, faces, None, tuple(shape), spacing, table.doublings)


@torch.no_grad()
def measure_labels(labels, spacing=None, per_slice=False, border_faces=True, device=None, slab=None, capacity=None):
    """The ``LabelMeasures`` of a 2-D or 3-D label array: sources, dtypes, value domain, ``per_slice``, ``slab`` and ``capacity``
    as ``label_table``; label 0 is background and is not measured.  ``spacing``: the voxel size per axis (default 1).
    ``border_faces``: a voxel on a face of the array exposes a face to the outside (default); False counts only faces between
    voxels of the array.  The raw columns are exact, do not depend on ``slab`` and are bit-reproducible.  Shapes with
    max(D, H, W)^2 * D * H * W >= 2^63 raise ``ValueError``: a raw second moment could wrap."""
    need_device()
    device = pick_device(device, labels)
    with torch.cuda.device(device):
        src = source(labels, device)
        return _measures_of_source(src, src.shape, spacing, bool(per_slice), border_faces, device, slab, capacity)


# ----------------------------------------------------------------------------
# device: the shapes
# ----------------------------------------------------------------------------
@dataclass
class LabelShapes:
    """What ``shape_labels`` counts, per label that occurs (background 0 left out), and what follows from it.

    The raw columns are integers and exact.  ``labels`` ascending, ``areas`` the voxel counts; ``intercepts`` (k, 13), or (k, 4)
    for an image and, per slice, for the images of a stack: column j belongs to the half-direction ``directions[j]`` (the offsets
    in {-1, 0, 1}^ndim whose first non-zero component is +1, in lexicographic order) and holds, with M the voxels of the label,
    #{p in M : p + d not in M} + #{p in M : p - d not in M}; the axis columns are ``measure_labels``' ``faces``.  ``euler`` (k, 2):
    the Euler number under full connectivity (26 / 8: of the union of the closed voxel cubes) and under face connectivity (6 / 4:
    voxels - face pairs + quads - octets).  Per slice ``slices`` holds the leading-axis index and rows are sorted by slice, then
    label.  ``spacing``: the voxel size per axis; ``doublings``: how often the device table had to grow.

    Everything derived is pure numpy on these columns.  ``surface_area`` and ``perimeter`` are the Cauchy-Crofton estimates: the
    intercepts of a direction are twice the chords of the object along its lattice lines, every line stands for the area
    (length) v / |d * spacing| perpendicular to it, and the directions are averaged with ``crofton_weights``.  This is the estimator
    of ``skimage.measure.perimeter_crofton(directions=4)`` for an image and the same estimator with 13 directions for a volume,
    ``euler`` is ``skimage.measure.euler_number`` with connectivity ndim and 1: both restated from their documentation, not pinned
    against them (skimage is not available here).  Pinned are the integers, against a numpy statement and ``measure_labels``."""
    labels: np.ndarray
    areas: np.ndarray
    intercepts: np.ndarray
    euler: np.ndarray
    slices: object = None
    shape: tuple = ()
    spacing: tuple = ()
    doublings: int = 0

    @property
    def per_slice(self):
        return self.slices is not None

    @property
    def ndim(self):
        return 3 if self.intercepts.shape[1] == 13 else 2

    @property
    def directions(self):
        return P.shape_directions(self.ndim)

    @property
    def volume(self):
        """voxel count times the voxel's volume (its area for ndim 2)"""
        return self.areas * float(np.prod(self.spacing))

    @property
    def surface_area(self):
        """2 sum_k c_k intercepts[k] v / |d_k * spacing|: within a few per cent of a smooth surface (a digitised ball of radius 8:
        -1.3 %), where the voxel-face surface of ``LabelMeasures`` is up to 1.5 times too large"""
        if self.ndim != 3:
            raise ValueError('surface_area: for volumes; an image has a perimeter')
        return P.crofton_size(self.intercepts, self.spacing)

    @property
    def perimeter(self):
        """(pi / 2) sum_k c_k intercepts[k] a / |d_k * spacing|"""
        if self.ndim != 2:
            raise ValueError('perimeter: for images; a volume has a surface_area')
        return P.crofton_size(self.intercepts, self.spacing)

    @property
    def sphericity(self):
        """pi^(1/3) (6 V)^(2/3) / S with the Crofton surface: close to 1 for a digitised ball"""
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.cbrt(np.pi) * np.cbrt(6.0 * self.volume) ** 2 / self.surface_area

    @property
    def circularity(self):
        """4 pi A / P^2 with the Crofton perimeter"""
        with np.errstate(divide='ignore', invalid='ignore'):
            return 4.0 * np.pi * self.volume / self.perimeter ** 2

    def euler_number(self, connectivity=None):
        """objects - tunnels + cavities per label (in an image: objects - holes).  ``connectivity``: None or ndim for full
        connectivity (26 / 8), 1 for face connectivity (6 / 4)"""
        if connectivity not in (None, 1, self.ndim):
            raise ValueError(f'euler_number: connectivity 1 or {self.ndim}, got {connectivity}')
        return self.euler[:, 1 if connectivity == 1 else 0]

    def to_table(self):
        """dict of columns"""
        out = {'slice': self.slices} if self.per_slice else {}
        out.update({'label': self.labels, 'area': self.areas, 'volume': self.volume})
        if self.ndim == 3:
            out.update({'surface_area': self.surface_area, 'sphericity': self.sphericity})
        else:
            out.update({'perimeter': self.perimeter, 'circularity': self.circularity})
        out.update({'euler_number': self.euler[:, 0], 'euler_number_faces': self.euler[:, 1]})
        out.update({f'intercepts-{j}': self.intercepts[:, j] for j in range(self.intercepts.shape[1])})
        return out

    def to_csv(self, path):
        import csv
        table = self.to_table()
        with open(path, 'w', newline='') as f:
            w = csv.writer(f)
            w.writerow(table)
            w.writerows(zip(*(col.tolist() for col in table.values())))


def shapes_from_arrays(labels, areas, intercepts, euler, shape, spacing=None, slices=None, doublings=0):
    """LabelShapes from host arrays (rows in any order, each key once)."""
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (2, 3) or (slices is not None and len(shape) != 3):
        raise ValueError(f'shapes_from_arrays: 2-D or 3-D label arrays (per slice: 3-D), got shape {shape}')
    nd = 2 if slices is not None else len(shape)
    cols = [np.asarray(labels, dtype=np.int64).reshape(-1), np.asarray(areas, dtype=np.int64).reshape(-1),
            np.asarray(intercepts, dtype=np.int64).reshape(-1, 13 if nd == 3 else 4), np.asarray(euler, dtype=np.int64).reshape(-1, 2)]
    if len({len(c) for c in cols}) != 1:
        raise ValueError('shapes_from_arrays: the columns differ in length')
    if slices is not None:
        slices = np.asarray(slices, dtype=np.int64).reshape(-1)
        order = np.lexsort((cols[0], slices))
        slices = slices[order]
    else:
        order = np.argsort(cols[0], kind='stable')
    return LabelShapes(*(c[order] for c in cols), slices, shape, P.shape_spacing(spacing, nd, slices is not None), int(doublings))


def _shapes_of_source(src, shape, spacing, per_slice, border_faces, device, slab, capacity):
    rows, H, W = _geometry(shape, per_slice, 'shape_labels')
    nd = 2 if per_slice else len(shape)
    spacing = P.shape_spacing(spacing, nd, per_slice)      # refused before anything is allocated
    table = GrowableTable('emp_label_shape', 'shape_labels', capacity or min(initial_capacity(rows * H * W), MEASURE_MAX_CAPACITY), device)
    # the slice below a slab's first one, as in _measures_of_source: in front of a device slab, kept in a buffer for a host one
    host_halo = src.is_host and not per_slice
    halo = torch.empty(max(1, src.row_bytes), dtype=torch.uint8, device=device) if host_halo else None
    for _, z0, z1, (address,) in stream_slabs([src], slab, device):
        below = None if per_slice or z0 == 0 else (halo.data_ptr() if host_halo else address - src.row_bytes)
        table.add(address, src.ebytes, z0, z1 - z0, H, W, rows, below, int(per_slice), int(bool(border_faces)))
        if host_halo and z1 < rows:
            _abi.check(table.lib.emp_copy_d2d(_abi.ptr(halo), address + (z1 - z0 - 1) * src.row_bytes, src.row_bytes, _abi.stream_ptr(device)),
                       'emp_copy_d2d')
    keys, cnt, icpt, euler = (t.cpu().numpy() for t in table.finalize(extra=[(13, torch.int64), (2, torch.int64)]))
    if per_slice:      # the images' four directions are the kernel's first four
        return LabelShapes(keys & 0xffffffff, cnt, icpt[:, :4], euler, keys >> 32, tuple(shape), spacing, table.doublings)
    if len(shape) == 2:      # kernel (z, y, x) = image (y, 0, x)
        return LabelShapes(keys, cnt, icpt[:, list(P.SHAPE_IMAGE_COLUMNS)], euler, None, tuple(shape), spacing, table.doublings)
    return LabelShapes(keys, cnt, icpt, euler, None, tuple(shape), spacing, table.doublings)


@torch.no_grad()
def shape_labels(labels, spacing=None, per_slice=False, border_faces=True, device=None, slab=None, capacity=None):
    """The ``LabelShapes`` of a 2-D or 3-D label array (csrc/shape.hip): sources, dtypes, value domain, ``per_slice``, ``slab`` and
    ``capacity`` as ``measure_labels``; label 0 is background.  ``spacing``: the voxel size per axis (default 1).
    ``border_faces``: a neighbour outside the array counts as not of the label (default); False leaves out every pair with one
    end outside the array.  The Euler numbers always take the outside as background.  The raw columns are exact, do not depend
    on ``slab`` and are bit-reproducible."""
    need_device()
    device = pick_device(device, labels)
    with torch.cuda.device(device):
        src = source(labels, device)
        return _shapes_of_source(src, src.shape, spacing, bool(per_slice), border_faces, device, slab, capacity)


# ----------------------------------------------------------------------------
# device: the contacts
# ----------------------------------------------------------------------------
@dataclass
class LabelContacts:
    """What ``label_contacts`` counts, per unordered pair of different labels that occur next to each other, and what follows from
    it.  Rows are sorted by (a, b), ``a < b``; with ``background`` a pair with the background is the row (0, b), without it there
    is none.  ``pairs`` (n, 13), or (n, 4) for an image: column k belongs to the half-direction ``directions[k]`` (those of
    ``LabelShapes.intercepts``) and holds #{p : p and p + d_k both in the array, {L(p), L(p + d_k)} = {a, b}}.  A pair with an end
    outside the array is never counted.  These integers are exact and do not depend on ``slab``.  Summed over a label's rows, the
    background's included, ``pairs`` is ``shape_labels(border_faces=False).intercepts`` of that label.

    Everything derived is pure numpy.  ``contact_area`` (``contact_length`` for an image) is the Cauchy-Crofton estimate
    ``LabelShapes.surface_area`` uses, on the pairs of the row: the part of either label's surface that the other one covers.
    There is no counterpart in the reference plugin; the nearest thing is skimage's region adjacency graph (``skimage.graph.RAG``,
    ``rag_boundary``), and nothing here is pinned against it."""
    a: np.ndarray
    b: np.ndarray
    pairs: np.ndarray
    shape: tuple = ()
    spacing: tuple = ()
    background: bool = False
    doublings: int = 0

    @property
    def ndim(self):
        return 3 if self.pairs.shape[1] == 13 else 2

    @property
    def directions(self):
        return P.shape_directions(self.ndim)

    @property
    def counts(self):
        """the voxel pairs of every row, all directions"""
        return self.pairs.sum(axis=1)

    @property
    def faces(self):
        """(n, ndim): the pairs along the axes, in z, y, x order: the voxel faces the two labels share"""
        return self.pairs[:, list(P.SHAPE_AXIS_COLUMNS[self.ndim])]

    @property
    def face_area(self):
        """the shared voxel faces times their physical size: up to sqrt(3) times the smooth area on a slanted interface"""
        if self.ndim != 3:
            raise ValueError('face_area: for volumes; an image has a face_length')
        return self.faces @ P.contact_face_sizes(self.spacing)

    @property
    def face_length(self):
        if self.ndim != 2:
            raise ValueError('face_length: for images; a volume has a face_area')
        return self.faces @ P.contact_face_sizes(self.spacing)

    @property
    def contact_area(self):
        """2 sum_k c_k pairs[k] v / |d_k * spacing|"""
        if self.ndim != 3:
            raise ValueError('contact_area: for volumes; an image has a contact_length')
        return P.contact_sizes(self.pairs, self.spacing)

    @property
    def contact_length(self):
        """(pi / 2) sum_k c_k pairs[k] a / |d_k * spacing|"""
        if self.ndim != 2:
            raise ValueError('contact_length: for images; a volume has a contact_area')
        return P.contact_sizes(self.pairs, self.spacing)

    def _size(self):
        return P.contact_sizes(self.pairs, self.spacing)

    @property
    def labels(self):
        """the sorted distinct ids of all rows"""
        return np.unique(np.concatenate([self.a, self.b]))

    def neighbors(self, label, connectivity=None):
        """the ids in contact with ``label``, ascending.  ``connectivity``: None or ndim keeps every pair, 1 only pairs that share a
        voxel face"""
        if connectivity not in (None, 1, self.ndim):
            raise ValueError(f'neighbors: connectivity 1 or {self.ndim}, got {connectivity}')
        keep = np.ones(len(self.a), bool) if connectivity != 1 else self.faces.any(axis=1)
        return np.unique(np.concatenate([self.b[keep & (self.a == label)], self.a[keep & (self.b == label)]]))

    def degree(self):
        """per id of ``labels`` the number of its partners"""
        ids = self.labels
        other = self.a != self.b
        return np.bincount(np.searchsorted(ids, np.concatenate([self.a, self.b[other]])), minlength=len(ids)).astype(np.int64)

    def _weight(self, weight):
        if weight in ('contact_area', 'contact_length'):
            return self._size()
        if weight in ('face_area', 'face_length'):
            return self.faces @ P.contact_face_sizes(self.spacing)
        if weight == 'counts':
            return self.counts.astype(np.float64)
        raise ValueError(f'adjacency: weight contact_area, face_area or counts, got {weight}')

    def adjacency(self, weight='contact_area'):
        """the symmetric ``scipy.sparse.csr_matrix`` over ``labels``: entry (i, j) is the weight of the row {labels[i], labels[j]}"""
        from scipy.sparse import coo_matrix
        ids = self.labels
        i, j, w = np.searchsorted(ids, self.a), np.searchsorted(ids, self.b), self._weight(weight)
        off = i != j
        return coo_matrix((np.concatenate([w, w[off]]), (np.concatenate([i, j[off]]), np.concatenate([j, i[off]]))), shape=(len(ids),) * 2).tocsr()

    def fractions(self):
        """(n, 2): the contact's share of the whole Crofton surface that a and b have inside the array.  The whole surface of a
        label is the sum over all its rows, the background's included: it needs ``background=True``"""
        if not self.background:
            raise ValueError('fractions: the share of a surface needs the pairs with the background: label_contacts(..., background=True)')
        ids, size = self.labels, self._size()
        i, j = np.searchsorted(ids, self.a), np.searchsorted(ids, self.b)
        whole = np.bincount(i, size, len(ids)) + np.bincount(j[i != j], size[i != j], len(ids))
        return np.stack([size / whole[i], size / whole[j]], axis=1) if len(size) else np.zeros((0, 2))

    def by_class(self, label_divisor):
        """the same table over the classes (a // label_divisor, b // label_divisor).  Pairs of two instances of one class are kept
        as the row (c, c); the background stays class 0"""
        ca, cb, pairs = P.contact_fold_classes(self.a, self.b, self.pairs, label_divisor)
        return LabelContacts(ca, cb, pairs, self.shape, self.spacing, self.background, self.doublings)

    def merge_groups(self, min_area=0.0, min_fraction=None, label_divisor=None):
        """The groups of labels joined by contacts of at least ``min_area`` (``contact_area``; an image: ``contact_length``) and, if
        given, of at least ``min_fraction`` of the surface of one of the two (the larger share; needs ``background=True``).  The
        background joins nothing.  ``label_divisor``: only labels of one class are joined.  The union-find runs on the host.
        Returns a list of ascending id arrays in ascending order of their smallest id: each is a valid ``ids=`` of ``merge_labels``."""
        keep = (self.a != 0) & (self.a != self.b) & (self._size() >= float(min_area))
        if min_fraction is not None:
            keep &= self.fractions().max(axis=1) >= float(min_fraction)
        if label_divisor is not None:
            keep &= self.a // int(label_divisor) == self.b // int(label_divisor)
        return P.contact_groups(self.a, self.b, keep)

    def to_table(self):
        """dict of columns"""
        out = {'a': self.a, 'b': self.b, 'count': self.counts}
        size = 'area' if self.ndim == 3 else 'length'
        out.update({f'contact_{size}': self._size(), f'face_{size}': self.faces @ P.contact_face_sizes(self.spacing)})
        out.update({f'faces-{ax}': self.faces[:, j] for j, ax in enumerate('zyx'[3 - self.ndim:])})
        out.update({f'pairs-{j}': self.pairs[:, j] for j in range(self.pairs.shape[1])})
        return out

    def to_csv(self, path):
        import csv
        table = self.to_table()
        with open(path, 'w', newline='') as f:
            w = csv.writer(f)
            w.writerow(table)
            w.writerows(zip(*(col.tolist() for col in table.values())))


def contacts_from_arrays(a, b, pairs, shape, spacing=None, background=False, doublings=0):
    """LabelContacts from host arrays (rows in any order, each pair once, ``a < b``)."""
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (2, 3):
        raise ValueError(f'contacts_from_arrays: 2-D or 3-D label arrays, got shape {shape}')
    nd = len(shape)
    cols = [np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1),
            np.asarray(pairs, dtype=np.int64).reshape(-1, 13 if nd == 3 else 4)]
    if len({len(c) for c in cols}) != 1:
        raise ValueError('contacts_from_arrays: the columns differ in length')
    if not (cols[0] < cols[1]).all() or (cols[0] < 0).any():
        raise ValueError('contacts_from_arrays: every row needs 0 <= a < b')
    if not background and (cols[0] == 0).any():
        raise ValueError('contacts_from_arrays: a row with the background (a = 0) needs background=True')
    order = np.lexsort((cols[1], cols[0]))
    return LabelContacts(*(c[order] for c in cols), shape, P.contact_spacing(spacing, nd), bool(background), int(doublings))


def _contacts_of_source(src, shape, spacing, background, device, slab, capacity):
    rows, H, W = _geometry(shape, False, 'label_contacts')
    spacing = P.contact_spacing(spacing, len(shape))      # refused before anything is allocated
    table = GrowableTable('emp_label_contacts', 'label_contacts', capacity or min(initial_capacity(rows * H * W), MEASURE_MAX_CAPACITY), device)
    # the slice below a slab's first one, as in _measures_of_source: in front of a device slab, kept in a buffer for a host one
    halo = torch.empty(max(1, src.row_bytes), dtype=torch.uint8, device=device) if src.is_host else None
    for _, z0, z1, (address,) in stream_slabs([src], slab, device):
        below = None if z0 == 0 else (halo.data_ptr() if src.is_host else address - src.row_bytes)
        table.add(address, src.ebytes, z0, z1 - z0, H, W, rows, below, int(background))
        if src.is_host and z1 < rows:
            _abi.check(table.lib.emp_copy_d2d(_abi.ptr(halo), address + (z1 - z0 - 1) * src.row_bytes, src.row_bytes, _abi.stream_ptr(device)),
                       'emp_copy_d2d')
    keys, _, pairs = (t.cpu().numpy() for t in table.finalize(extra=[(13, torch.int64)]))
    keys = keys.view(np.uint64)      # sorted as unsigned: by (a, b)
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xffffffff)).astype(np.int64)
    if len(shape) == 2:      # kernel (z, y, x) = image (y, 0, x)
        pairs = pairs[:, list(P.SHAPE_IMAGE_COLUMNS)]
    return LabelContacts(a, b, pairs, tuple(shape), spacing, background, table.doublings)


@torch.no_grad()
def label_contacts(labels, spacing=None, background=False, device=None, slab=None, capacity=None):
    """The ``LabelContacts`` of a 2-D or 3-D label array (csrc/contacts.hip): which labels touch, over how many voxel pairs per
    half-direction.  Sources, dtypes, ``slab`` and ``capacity`` as ``shape_labels``; labels lie in [0, 2^32): a pair takes one
    64-bit key.  ``spacing``: the voxel size per axis (default 1).  ``background``: also enter the pairs of a label with the
    background 0, as rows (0, b); ``fractions`` and ``merge_groups(min_fraction=...)`` need them.  A pair with an end outside
    the array is never counted.  The raw columns are exact, do not depend on ``slab`` and are bit-reproducible.
    Not built: ``per_slice`` (slice, a and b do not fit one key: call it per image), 4-D arrays, labels at or above 2^32."""
    need_device()
    device = pick_device(device, labels)
    with torch.cuda.device(device):
        src = source(labels, device)
        return _contacts_of_source(src, src.shape, spacing, bool(background), device, slab, capacity)


# ----------------------------------------------------------------------------
# policy: pure numpy on a LabelTable
# ----------------------------------------------------------------------------
def _ids(table, keep):
    """the selected rows as ids (whole mode) or (slice, id) pairs (per-slice mode)"""
    if table.per_slice:
        return np.stack([table.slices[keep], table.labels[keep]], axis=1)
    return table.labels[keep]


def small_labels(table, minimum_area_allowed):
    """ids with ``area <= minimum_area_allowed`` (the reference's ``<=``, _filter_small_labels.py:23), background excluded; per
    slice: (slice, id) pairs"""
    return _ids(table, (table.areas <= minimum_area_allowed) & (table.labels != 0))


def boundary_labels(table):
    """ids whose box touches a face of the array -- the four edges of a 2-D image, the six faces of a volume, and in per-slice
    mode the four edges of each image -- background excluded"""
    nd = table.boxes.shape[1] // 2
    extent = np.asarray(table.shape[-nd:], dtype=np.int64)
    touch = ((table.boxes[:, :nd] == 0) | (table.boxes[:, nd:] == extent)).any(axis=1)
    return _ids(table, touch & (table.labels != 0))


def count_labels(label_values, label_divisor):
    """What _label_counter_widget.py:105-118 returns: ({class id: [label ids]}, [class ids]) of the label values given (the
    widget passes the non-zero ones), classes ascending, class = value // divisor; a divisor of 0 puts all of them into class 1.
    ``label_divisor`` is not negative."""
    values = np.asarray(label_values).reshape(-1)
    if label_divisor == 0:
        return {1: values.tolist()}, [1]
    # group the values by class in one stable sort: every class keeps its values in the order given
    classes = np.floor_divide(values, label_divisor)
    order = np.argsort(classes, kind='stable')
    present, first = np.unique(classes[order], return_index=True)
    groups = np.split(values[order], first[1:])
    present = present.tolist()
    return {c: g.tolist() for c, g in zip(present, groups)}, present


def _per_slice_values(table):
    """label values as the widgets collect them, np.unique(...)[1:]: the values that occur without the smallest one"""
    if not table.per_slice:
        return table.labels[1:]
    return {z: table.labels[table.slices == z][1:] for z in range(table.shape[0])}


def class_label_lists(table, label_divisor):
    """the ids per class as Count Labels prints them (_label_counter_widget.py:243-246, :281-283): ``count_labels`` of
    ``np.unique(labels)[1:]``; per slice a dict {slice: that}"""
    v = _per_slice_values(table)
    if table.per_slice:
        return {z: count_labels(x, label_divisor)[0] for z, x in v.items()}
    return count_labels(v, label_divisor)[0]


def _queue(label_values, label_divisor):
    """per class that occurs the free ids of its register: a mask over the register's offsets, of which offset 0 (the class's
    own base id, which no instance gets) is never free"""
    used = np.unique(np.asarray(label_values, dtype=np.int64))
    d = int(label_divisor)
    free = {}
    for c in np.unique(used // d).tolist():
        taken = np.zeros(d, dtype=bool)
        taken[0] = True
        lo, hi = np.searchsorted(used, [c * d, (c + 1) * d])
        taken[used[lo:hi] - c * d] = True
        free[c] = (c * d + np.flatnonzero(~taken)).tolist()
    return free


def next_available_labels(table, label_divisor):
    """the widget's ``label_queue`` (_merge_split_widget.py:730-744): per class that occurs the unused ids of
    (class * divisor, (class + 1) * divisor), ascending; per slice a dict {slice: that}"""
    if not label_divisor > 0:
        raise ValueError('Label divisor must be a positive integer!')
    v = _per_slice_values(table)
    if table.per_slice:
        return {z: _queue(x, label_divisor) for z, x in v.items()}
    return _queue(v, label_divisor)


def next_available_label(queue, class_id, label_divisor):
    """_merge_split_widget.py:751-759: pops the first free id of the class from ``queue`` (in place); a class that does not
    occur gets its whole register, of which the first id is returned"""
    free = queue.get(class_id)
    if free is None:
        base = class_id * label_divisor
        free = queue[class_id] = list(range(base + 1, base + label_divisor))
    return free.pop(0)


def label_bbox(table, label_id, slice_index=None):
    """``regionprops.bbox`` of one label for Jump to Label (_merge_split_widget.py:652-659); raises on an absent id as the widget
    does.  Per-slice tables take the slice as well."""
    hit = table.labels == int(label_id)
    if table.per_slice:
        if slice_index is None:
            raise ValueError('label_bbox: a per-slice table needs slice_index')
        hit &= table.slices == int(slice_index)
    if int(label_id) == 0 or not hit.any():
        raise Exception(f'No label {label_id} in the table')
    return tuple(int(v) for v in table.boxes[np.flatnonzero(hit)[0]])


# ----------------------------------------------------------------------------
# device: the edit
# ----------------------------------------------------------------------------
class _Map:
    """from -> to on the device (emp_label_map_build)"""

    def __init__(self, keys, vals, device):
        lib = _abi.load()
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        vals = np.ascontiguousarray(vals, dtype=np.uint64)
        cap = 64
        while cap < 2 * len(keys):
            cap *= 2
        self.capacity = cap
        self.keys = torch.empty(cap, dtype=torch.int64, device=device)
        self.vals = torch.empty(cap, dtype=torch.int64, device=device)
        _abi.check(lib.emp_label_map_build(hp(keys), hp(vals), len(keys), _abi.ptr(self.keys), _abi.ptr(self.vals), cap,
                                           _abi.stream_ptr(device)), 'emp_label_map_build')

    def apply(self, key_addr, key_bytes, src_addr, src_bytes, out_addr, z0, depth, H, W, per_slice, device):
        _abi.check(_abi.load().emp_label_apply_map(C.c_void_p(key_addr), key_bytes, C.c_void_p(src_addr), src_bytes, C.c_void_p(out_addr),
                                                   z0, depth, H, W, int(per_slice), _abi.ptr(self.keys), _abi.ptr(self.vals),
                                                   self.capacity, _abi.stream_ptr(device)), 'emp_label_apply_map')


def _is_numpy(x):
    return isinstance(x, np.ndarray)


def _check_values(vals, dtype, what):
    dt = np.dtype(str(dtype).replace('torch.', ''))
    top = 1 if dt.kind == 'b' else np.iinfo(dt).max
    vals = np.asarray(vals, dtype=np.int64)
    if len(vals) and (vals.min() < 0 or vals.max() > top):
        raise ValueError(f'{what}: a new label does not fit the array\'s dtype {dtype}')


def _edit_target(labels, out, inplace, shape, dtype, what):
    """The output rules of an edit: every check of (labels, out, inplace), and the ``Sink`` the result goes to.  A device tensor
    gives a device tensor and a numpy array a numpy array, the caller's own with ``inplace=True`` and a new one without; a chunked
    store of ``shape`` and ``dtype`` is written into ``out=``, or into itself with ``inplace=True``."""
    if isinstance(labels, torch.Tensor):
        if not labels.is_cuda:
            raise TypeError(f'{what}: a torch tensor must be on the device (pass host data as a numpy array)')
        if out is not None:
            raise TypeError(f'{what}: out= is for chunked stores; a device tensor is returned as a device tensor')
        if inplace and not labels.is_contiguous():
            raise ValueError(f'{what}: inplace=True needs a contiguous tensor')
        return Sink(labels if inplace else None, shape, dtype, labels.device)
    if _is_numpy(labels):
        if out is not None:
            raise TypeError(f'{what}: out= is for chunked stores; a numpy array is returned as a new array (or edited with inplace=True)')
        return Sink(labels if inplace else None, shape, dtype)
    if out is None:
        if not inplace:
            raise TypeError(f'{what}: a chunked store is written into out= (or into itself with inplace=True)')
        return Sink(labels, shape, dtype)
    if tuple(out.shape) != tuple(shape) or np.dtype(out.dtype) != np.dtype(dtype):
        raise ValueError(f'{what}: out= must have the shape and dtype of the labels')
    return Sink(out, shape, dtype)


def _apply(labels, keys, vals, per_slice, device, out, inplace, slab, what, *, key_labels=None):
    """out[i] = map[key(i)] if present else labels[i]; the key of i is labels[i] -- or ``key_labels[i]``, an array of the labels'
    shape from any kind of source --, or slice << 32 | that with per_slice.  A host slab is edited where it was staged"""
    src = source(labels, device)
    sink = _edit_target(labels, out, inplace, src.shape, src.dtype, what)
    rows, H, W = _geometry(src.shape, per_slice, what)
    _check_values(vals, src.dtype, what)
    m = _Map(keys, vals, device)
    sources = [src] if key_labels is None else [source(key_labels, device), src]
    for k, z0, z1, addrs in stream_slabs(sources, slab, device):
        m.apply(addrs[0], sources[0].ebytes, addrs[-1], src.ebytes, addrs[-1] if sink.is_host else sink.address(z0), z0, z1 - z0, H, W,
                per_slice, device)
        if sink.is_host:
            sink.write(z0, z1, src.slab_bytes(k, z0, z1))
    return sink.made()


def _map_keys(ids, per_slice):
    ids = np.asarray(ids, dtype=np.int64)
    if per_slice:
        ids = ids.reshape(-1, 2)
        return (ids[:, 0].astype(np.uint64) << np.uint64(32)) | ids[:, 1].astype(np.uint64)
    return ids.reshape(-1).astype(np.uint64)


@torch.no_grad()
def delete_labels(labels, ids, device=None, out=None, inplace=False, slab=None):
    """Delete Labels (_merge_split_widget.py:246-250): every voxel of the given ids becomes 0, all ids in one pass.  Zeros in
    ``ids`` are dropped, as the widget does."""
    need_device()
    device = pick_device(device, labels)
    ids = np.unique(np.asarray(ids, dtype=np.int64).reshape(-1))
    ids = ids[ids > 0]
    with torch.cuda.device(device):
        return _apply(labels, _map_keys(ids, False), np.zeros(len(ids), np.int64), False, device, out, inplace, slab, 'delete_labels')


@torch.no_grad()
def merge_labels(labels, ids, new_label_id=None, device=None, out=None, inplace=False, slab=None):
    """Merge Labels (_merge_split_widget.py:373-387): every voxel of the given ids becomes ``new_label_id`` (default: the
    smallest of them, :378-381).  Zeros in ``ids`` are dropped."""
    need_device()
    device = pick_device(device, labels)
    ids = np.unique(np.asarray(ids, dtype=np.int64).reshape(-1))
    ids = ids[ids > 0]
    if len(ids) == 0:
        raise ValueError('merge_labels: no label to merge')
    new = int(ids.min()) if new_label_id is None else int(new_label_id)
    ids = ids[ids != new]
    with torch.cuda.device(device):
        return _apply(labels, _map_keys(ids, False), np.full(len(ids), new, np.int64), False, device, out, inplace, slab, 'merge_labels')


@torch.no_grad()
def filter_out_small_label_areas(img, minimum_area_allowed, per_slice=False, device=None, out=None, inplace=False, slab=None):
    """_filter_small_labels.py:15-40: labels with ``area <= minimum_area_allowed`` are removed -> (image, number removed).
    ``per_slice``: every image of a 3-D stack on its own (the widget's '2D patches'); the number is then the total over the
    images.  An image without labels comes back unchanged with 0 (the reference raises an IndexError there)."""
    need_device()
    device = pick_device(device, img)
    with torch.cuda.device(device):
        table = label_table(img, per_slice=per_slice, device=device, slab=slab)
        ids = small_labels(table, minimum_area_allowed)
        res = _apply(img, _map_keys(ids, per_slice), np.zeros(len(ids), np.int64), per_slice, device, out, inplace, slab,
                     'filter_out_small_label_areas')
    return res, len(ids)


def _vanished(before, after):
    """how many keys of `before` (background excluded) do not occur in `after`"""
    def keys(t):
        k = t.labels[t.labels != 0]
        return k if not t.per_slice else (t.slices[t.labels != 0] << 32) | k
    return int(len(np.setdiff1d(keys(before), keys(after))))


@torch.no_grad()
def remove_boundary_labels(labels, whole_labels=False, per_slice=False, device=None, out=None, inplace=False, slab=None, streamed=False,
                           components=None):
    """_filter_small_labels.py:43-60 -> (labels, number of labels removed).

    ``whole_labels=False`` reproduces the reference's ``clear_border``: the array is split into connected components (full
    connectivity: 8 neighbours in an image, 26 in a volume; equal value) and the components that touch a face are cleared; a
    label that has another, interior component keeps it and is not counted as removed (:47-49).  The components come from
    ``emp_ccl_range``, whose limits this mode inherits: the whole array on the device, fewer than 2^30 voxels, labels below
    2^31 - 1 (int32 / int64 input; narrower types are converted on the device).  Outside those limits a ``ValueError`` names
    the alternative: ``whole_labels=True`` removes every voxel of a label whose box touches a face, needs the table only and
    works slab by slab on arrays of any size.  ``per_slice``: every image of a 3-D stack on its own; the number is then the
    total over the images.

    ``streamed=True`` runs the reference mode slab by slab, on device tensors, numpy arrays and chunked stores of any size (one
    image or one volume: not ``per_slice``): the components come from ``label_components`` into ``components=`` -- an int32 array
    or store of the caller's, of the labels' shape; by default a new numpy array --, their boxes from ``label_table`` on them, and
    the edit is one pass over labels and components together.  Its limits are ``label_components``'s: labels below 2^31 - 1 and
    one slice (or an explicit ``slab``) of fewer than 2^30 voxels."""
    need_device()
    device = pick_device(device, labels)
    what = 'remove_boundary_labels'
    with torch.cuda.device(device):
        if whole_labels:
            table = label_table(labels, per_slice=per_slice, device=device, slab=slab)
            ids = boundary_labels(table)
            res = _apply(labels, _map_keys(ids, per_slice), np.zeros(len(ids), np.int64), per_slice, device, out, inplace, slab, what)
            return res, len(ids)
        if streamed:
            return _clear_border_streamed(labels, per_slice, device, out, inplace, slab, components, what)
        shape = tuple(int(s) for s in labels.shape)
        _geometry(shape, per_slice, what)
        if int(np.prod(shape, dtype=np.int64)) >= CCL_MAX_VOXELS:
            raise ValueError(f'{what}: the connected components of the reference mode need fewer than 2^30 voxels, the array has '
                             f'{shape}; use whole_labels=True (removes whole labels by their boxes, slab by slab) or streamed=True '
                             '(the same components, slab by slab)')
        # what the call cannot do is said before any work: nothing is written, on the device or to the caller's array, by then
        sink = _edit_target(labels, out, inplace, shape, labels.dtype, what)
        edit_own = bool(inplace) and isinstance(labels, torch.Tensor)      # the result replaces the caller's tensor
        return _whole_array(labels, sink, device, False, lambda t, eb: _clear_border(t, eb, shape, per_slice, edit_own, device))


def _whole_array(labels, sink, device, clone, run):
    """The way of a whole array to the device and back, for the tools that need all of it there at once.  ``labels``: a device
    tensor or host data that passed ``_edit_target``, which chose ``sink``.  ``run(t, eb)`` gets it as one contiguous device
    buffer -- the tensor itself, a clone of it with ``clone``, or host data uploaded as bytes (torch has no arithmetic on uint16 /
    uint32) -- and returns (the device buffer that holds the result, anything else) -> (the result as the kind that was given: that
    buffer for a device tensor, else downloaded in one piece into the sink, anything else)."""
    if isinstance(labels, torch.Tensor):      # a tensor that passed the check is on the device
        t = labels if labels.is_contiguous() else labels.contiguous()
        return run(t.clone() if clone else t, ebytes(t.dtype))
    host = np.ascontiguousarray(labels if _is_numpy(labels) else labels[...])
    res, rest = run(torch.from_numpy(host.view(np.uint8).reshape(-1)).to(device), ebytes(host.dtype))
    return sink.put(0, host.shape[0], res.cpu()), rest


def _clear_border(t, eb, shape, per_slice, edit_own, device):
    """``clear_border`` on the contiguous device buffer ``t`` -> (the device buffer with the result -- ``t`` itself with
    ``edit_own`` --, the number of labels that vanished)"""
    before = _table_of_source(RawSource(t, eb, shape), shape, per_slice, device, None, None)
    # the largest label of any row: a per-slice table is sorted by slice first, its last row is only the last slice's
    top = int(before.labels.max()) if len(before.labels) else 0
    if top > CCL_MAX_LABEL:
        raise ValueError('remove_boundary_labels: the connected components of the reference mode need labels below 2^31 - 1, the array '
                         f'holds {top}; use whole_labels=True')
    lib = _abi.load()
    # component ids: per image (8-connected) or of the one volume (26-connected)
    images = len(shape) == 2 or per_slice
    N, depth, cH, cW = (shape[0] if len(shape) == 3 else 1, 0, shape[-2], shape[-1]) if images else (1, shape[0], shape[1], shape[2])
    wide = _as_ccl_input(t, eb, shape)
    comps = torch.empty((N if images else depth, cH, cW), dtype=torch.int32, device=device)
    work = torch.empty(int(lib.emp_ccl8_work_bytes(N, cH, cW) if images else lib.emp_ccl8_work_bytes(1, depth * cH, cW)),
                       dtype=torch.uint8, device=device)
    _abi.check(lib.emp_ccl_range(_abi.ptr(wide), 8 if wide.dtype == torch.int64 else 4, N, depth, cH, cW, 1, CCL_MAX_LABEL + 1,
                                 _abi.ptr(comps), None, _abi.ptr(work), _abi.stream_ptr(device)), 'emp_ccl_range')
    del wide, work
    # components are numbered per image: their key is slice << 32 | id there
    ctable = _table_of_source(RawSource(comps, -4, tuple(comps.shape)), tuple(comps.shape), images, device, None, None)
    cids = boundary_labels(ctable)
    # the edit runs in the components' geometry, the images of a stack or the one volume, on the buffer's elements
    res = _apply(_elements(t, eb).reshape(comps.shape), _map_keys(cids, images), np.zeros(len(cids), np.int64), images, device, None,
                 edit_own, None, 'remove_boundary_labels', key_labels=comps)
    res = t if edit_own else res.reshape(-1).view(torch.uint8).view(t.dtype).reshape(t.shape)
    after = _table_of_source(RawSource(res, eb, shape), shape, per_slice, device, None, None)
    return res, _vanished(before, after)


def _as_ccl_input(t, eb, shape):
    """the labels as the int32 / int64 tensor emp_ccl_range reads: itself, or a widened copy made on the device"""
    raw = t.reshape(-1).view(torch.uint8)
    if abs(eb) == 8:
        return raw.view(torch.int64)      # values are below 2^31 - 1 (checked on the table): signedness does not matter
    if eb == -4:
        return raw.view(torch.int32)
    if eb == 4:
        return raw.view(torch.int32).to(torch.int64) & 0xffffffff
    if abs(eb) == 2:
        return raw.view(torch.int16).to(torch.int32) & 0xffff if eb > 0 else raw.view(torch.int16).to(torch.int32)
    return (raw if eb > 0 else raw.view(torch.int8)).to(torch.int32)


# ----------------------------------------------------------------------------
# connected components, slab by slab
# ----------------------------------------------------------------------------
COMPONENTS_CAPACITY = 1 << 16      # first size of the union-find over the slabs' components (entries; it doubles)


def _components_target(src, out, device, what):
    """Where the components go, every check of ``out`` included: the ``Sink`` of a device tensor, or of an array / store on the
    host.  None: a new device tensor for a device source, a new numpy array otherwise."""
    if out is None:
        return Sink(None, src.shape, np.int32) if src.is_host else Sink(None, src.shape, torch.int32, device)
    if isinstance(out, torch.Tensor):
        if not out.is_cuda:
            raise TypeError(f'{what}: a torch tensor given as out= must be on the device (pass host memory as a numpy array)')
        if out.device != device:
            raise ValueError(f'{what}: out= on {out.device}, the work on {device}')
        if tuple(out.shape) != src.shape or out.dtype != torch.int32:
            raise ValueError(f'{what}: out= must be int32 and have the shape of the labels')
        if not out.is_contiguous():
            raise ValueError(f'{what}: out= needs a contiguous tensor')
        return Sink(out, src.shape, torch.int32)
    if not (hasattr(out, 'shape') and hasattr(out, 'dtype') and hasattr(out, '__setitem__')):
        raise TypeError(f'{what}: out= is an int32 device tensor, numpy array or chunked store')
    if tuple(out.shape) != src.shape or np.dtype(out.dtype) != np.dtype(np.int32):
        raise ValueError(f'{what}: out= must be int32 and have the shape of the labels')
    return Sink(out, src.shape, np.int32)


def _components_of_source(src, out, slab, device, capacity, table, stats, what):
    rows, H, W = P.components_geometry(src.shape, what)
    HW = H * W
    slab = P.components_slab(rows, HW, slab, slab_plan(rows, src.row_bytes if src.is_host else None, None)[0], what)
    sink = _components_target(src, out, device, what)
    if rows * HW == 0:
        return sink.made(), 0
    # the largest label, off the table as _clear_border reads it; the table's pass also refuses what is no label at all
    if table is None:
        table = _table_of_source(src, src.shape, False, device, slab, None)
    P.components_check_labels(table.labels.max() if len(table.labels) else 0, what)

    lib = _abi.load()
    ids = torch.empty(slab * HW, dtype=torch.int32, device=device)
    num = torch.empty(1, dtype=torch.int32, device=device)
    work = torch.empty(int(lib.emp_ccl8_work_bytes(1, slab * H, W)), dtype=torch.uint8, device=device)
    st = {'slabs': 0, 'ccl_runs': 0, 'doublings': 0, 'provisional': 0}

    def ccl(k, z0, z1):
        """the slab's local ids in ``ids`` -> the labels as the kernel read them"""
        wide = _as_ccl_input(src.slab_bytes(k, z0, z1), src.ebytes, None)
        _abi.check(lib.emp_ccl_range(_abi.ptr(wide), 8 if wide.dtype == torch.int64 else 4, 1, z1 - z0, H, W, 1, CCL_MAX_LABEL + 1,
                                     _abi.ptr(ids), _abi.ptr(num), _abi.ptr(work), _abi.stream_ptr(device)), 'emp_ccl_range')
        st['ccl_runs'] += 1
        return wide

    # pass 1: per slab its components, as provisional ids base + local id, and the unions across the seam to the slab before
    parent = torch.zeros(max(2, int(capacity)), dtype=torch.int32, device=device)
    bases, G = [], 0
    prev_vals = prev_ids = None
    for k, z0, z1, _ in stream_slabs([src], slab, device):
        wide = ccl(k, z0, z1)
        K = int(num.item())      # synchronises
        P.components_check_count(G + K, what)
        if G + K + 1 > len(parent):
            cap = len(parent)
            while cap < G + K + 1:
                cap *= 2
                st['doublings'] += 1
            grown = torch.zeros(min(cap, P.COMPONENTS_MAX_COUNT + 1), dtype=torch.int32, device=device)
            grown[:G + 1] = parent[:G + 1]
            parent = grown
        if K:
            parent[G + 1:G + K + 1] = torch.arange(G + 1, G + K + 1, dtype=torch.int32, device=device)
        if k > 0:
            _abi.check(lib.emp_ccl_seam(_abi.ptr(prev_vals), _abi.ptr(prev_ids), _abi.ptr(wide), _abi.ptr(ids), wide.element_size(), H, W,
                                        bases[-1], G, _abi.ptr(parent), len(parent), _abi.stream_ptr(device)), 'emp_ccl_seam')
        bases.append(G)
        G += K
        if z1 < rows:
            # the last slice, values and ids, for the next seam: `ids` is written again by then, and so is a host source's slot
            n = (z1 - z0) * HW
            prev_vals, prev_ids = wide[n - HW:n].clone(), ids[n - HW:n].clone()
        del wide
    st['slabs'], st['provisional'] = len(bases), G

    # the final numbers: the roots ranked in id order, which is raster order of the components' first voxels
    single = len(bases) == 1
    if single:
        count = G      # no seam: the slab's own numbering is the result
    else:
        lut = torch.empty(G + 1, dtype=torch.int32, device=device)
        rwork = torch.empty(int(lib.emp_ccl_rank_roots_work_bytes(G)), dtype=torch.uint8, device=device)
        _abi.check(lib.emp_ccl_rank_roots(_abi.ptr(parent), G, _abi.ptr(lut), _abi.ptr(num), _abi.ptr(rwork), _abi.stream_ptr(device)),
                   'emp_ccl_rank_roots')
        count = int(num.item())
        del rwork
    del parent
    if stats is not None:
        stats.update(st, count=count)

    # pass 2: nothing has been written so far
    if single:      # `ids` holds the result
        if sink.is_host:
            sink.write(0, rows, ids.view(torch.uint8))
        elif sink.dest is None:
            sink.dest = ids.reshape(src.shape)
        else:
            sink.dest.copy_(ids.reshape(src.shape))
        return sink.dest, count
    for k, z0, z1, _ in stream_slabs([src], slab, device):
        ccl(k, z0, z1)      # deterministic, numbered in raster order: the local ids of pass 1
        dst = ids.data_ptr() if sink.is_host else sink.address(z0)      # a host slab is finished in `ids` and downloaded from there
        _abi.check(lib.emp_ccl_lut(_abi.ptr(ids), _abi.ptr(lut), bases[k], G + 1, C.c_void_p(dst), (z1 - z0) * HW, _abi.stream_ptr(device)),
                   'emp_ccl_lut')
        if sink.is_host:
            sink.write(z0, z1, ids.view(torch.uint8))
    if stats is not None:
        stats.update(ccl_runs=st['ccl_runs'])
    return sink.dest, count


@torch.no_grad()
def label_components(labels, out=None, slab=None, device=None, return_count=True, _capacity=None, _table=None, _stats=None):
    """The connected components of equal non-zero value of a 2-D or 3-D label array under full connectivity (8 neighbours in an
    image, 26 in a volume) -> (components, count): int32, numbered 1..count in raster order of each component's first element,
    background 0.  This is ``skimage.measure.label(labels)`` restated from its documented behaviour (skimage is not available here;
    not pinned against it), and what ``sparse.ccl26`` gives for a volume that fits one call.  ``return_count=False``: the
    components only.

    ``labels``: a device tensor, a numpy array or a chunked store, of any integer dtype, of any size.  The array is cut into slabs
    of ``slab`` leading-axis entries (slices of a volume, rows of an image); every slab is labelled on its own with
    ``emp_ccl_range``, the pieces are joined across the seams by a union-find over the slabs' component ids
    (csrc/components.hip) and numbered, and a second pass over the slabs writes the result.  The result does not depend on
    ``slab``.  Default slab: the slab stream's choice (everything for a device tensor, about 64 MiB of a host source), capped at
    2^28 voxels (about 4 GiB of work memory); with one slab there is no second pass.

    ``out``: None -- a new device tensor for a device source, a new numpy array otherwise -- or an int32 device tensor, numpy array
    or chunked store of the labels' shape, which is written and returned.

    ``ValueError``, before anything is written: a label above 2^31 - 2, one slice (or an explicit slab) of 2^30 voxels or more, an
    array that is not 2-D or 3-D, more than 2^31 - 2 components over the slabs."""
    need_device()
    device = pick_device(device, labels, out)
    with torch.cuda.device(device):
        src = source(labels, device)
        res, count = _components_of_source(src, out, slab, device, _capacity or COMPONENTS_CAPACITY, _table, _stats, 'label_components')
    return (res, count) if return_count else res


def _clear_border_streamed(labels, per_slice, device, out, inplace, slab, components, what):
    """``clear_border`` slab by slab -> (the result as ``_edit_target`` says, the number of labels that vanished)"""
    if per_slice:
        raise ValueError(f'{what}: streamed=True takes the array as one image or one volume; per_slice is not streamed')
    src = source(labels, device)
    P.components_geometry(src.shape, what)
    _edit_target(labels, out, inplace, src.shape, src.dtype, what)      # what the edit would refuse, before any work
    if components is None:
        components = np.empty(src.shape, np.int32)
    before = _table_of_source(src, src.shape, False, device, slab, None)
    comps, _ = label_components(labels, out=components, slab=slab, device=device, _table=before)
    csrc = source(comps, device)
    cids = boundary_labels(_table_of_source(csrc, csrc.shape, False, device, slab, None))
    res = _apply(labels, _map_keys(cids, False), np.zeros(len(cids), np.int64), False, device, out, inplace, slab, what, key_labels=comps)
    after = _table_of_source(source(res, device), src.shape, False, device, slab, None)
    return res, _vanished(before, after)


# ----------------------------------------------------------------------------
# Morph Labels
# ----------------------------------------------------------------------------
def _morph_plan(t, eb, shape, ids, radius, operation, ball, core, device):
    """What a device loop over the labels of the contiguous buffer ``t`` starts from: the turns (``ids``, or every label
    ascending), their levels under ``operation``'s scheduling rule, the tile lists for tiles of ``core`` and the statistics"""
    table = _table_of_source(RawSource(t, eb, shape), shape, False, device, None, None)
    if ids is None:
        turns = table.labels[table.labels != 0]
    else:
        turns = np.asarray(ids, dtype=np.int64).reshape(-1)
        turns = turns[turns > 0]
    levels = morph_schedule(table, turns, radius, operation)
    tiles, offsets, boxes, frames = _morph_tiles(table, turns, radius, operation, ball, levels, core)
    stats = {'turns': int(len(turns)), 'turns_scheduled': int(sum(len(l) for l in levels)), 'levels': len(levels), 'tiles': int(len(tiles)),
             'launches': 0}
    return turns, levels, tiles, offsets, boxes, frames, stats


def _stage(events, name, entry, *args):
    """the library's ``entry(*args)``; with a list ``events``, between a pair of HIP events that is appended to it under ``name``"""
    pair = None if events is None else (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    if pair:
        pair[0].record()
    _abi.check(getattr(_abi.load(), entry)(*args), entry)
    if pair:
        pair[1].record()
        events.append((name, *pair))


def _timed_launches(stats, events, entry, *args):
    """The launches of the levels: the library's ``entry(*args, launch counter)`` -> ``stats`` with the number of launches and,
    with ``events``, a pair of HIP events around them"""
    launches, pair = C.c_int(0), ([] if events else None)
    _stage(pair, entry, entry, *args, C.byref(launches))
    stats['launches'] = launches.value
    if events:
        stats['events'] = pair[0][1:]
    return stats


def _upload_turns(turns, boxes, tiles, device):
    """what both device loops upload: the labels of the turns, their boxes and the tile list"""
    return [torch.from_numpy(a).to(device) for a in (turns.astype(np.int64), boxes.view(np.int32), tiles)]


def _morph_device(t, eb, shape, operation, radius, ball, ids, device, events=False):
    """Morph Labels in place on the contiguous device buffer ``t`` (element size ``eb``, a 2-D or 3-D ``shape``) -> statistics:
    turns, levels, tiles, launches and, with ``events``, a pair of HIP events around the launches (for tools/morph_labels_bench.py)"""
    op = MORPH_OPS[operation]
    cz, cy, cx = C.c_int(0), C.c_int(0), C.c_int(0)
    _abi.check(_abi.load().emp_morph_tile_shape(radius, int(ball), op, C.byref(cz), C.byref(cy), C.byref(cx)), 'emp_morph_tile_shape')
    turns, levels, tiles, offsets, boxes, _, stats = _morph_plan(t, eb, shape, ids, radius, operation, ball, (cz.value, cy.value, cx.value),
                                                                 device)
    if len(tiles) == 0:
        return stats
    d_labels, d_boxes, d_tiles = _upload_turns(turns, boxes, tiles, device)
    words = int(np.diff(offsets).max()) * cz.value * cy.value
    scratch = torch.empty(words, dtype=torch.int64, device=device)
    return _timed_launches(stats, events, 'emp_morph_labels', C.c_void_p(t.data_ptr()), eb, *dims3(shape), radius, int(ball), op,
                           _abi.ptr(d_labels), _abi.ptr(d_boxes), len(turns), _abi.ptr(d_tiles), hp(offsets), len(levels), _abi.ptr(scratch),
                           words, _abi.stream_ptr(device))


def _fill_device(t, eb, shape, radius, hole_size, ball, ids, device, events=False):
    """Fill holes in place on the contiguous device buffer ``t`` -> the statistics of ``_morph_device`` and ``scratch_entries``.
    A turn writes only inside its padded box and reads only ``== label``: the levels are those of a dilation.  The parent and
    size arrays hold one entry per voxel of the frames (padded, clipped boxes) of the largest level, not of the array."""
    cz, cy, cx = C.c_int(0), C.c_int(0), C.c_int(0)
    _abi.check(_abi.load().emp_fill_holes_tile_shape(int(ball), C.byref(cz), C.byref(cy), C.byref(cx)), 'emp_fill_holes_tile_shape')
    turns, levels, tiles, offsets, boxes, frames, stats = _morph_plan(t, eb, shape, ids, radius, 'Dilate', ball,
                                                                      (cz.value, cy.value, cx.value), device)
    stats['scratch_entries'] = 0
    if len(tiles) == 0:
        return stats
    placed, stats['scratch_entries'] = P.fill_placement(frames, levels)
    d_labels, d_boxes, d_tiles = _upload_turns(turns, boxes, tiles, device)
    d_frames = torch.from_numpy(placed).to(device)
    parent, size = (torch.empty(stats['scratch_entries'], dtype=torch.int32, device=device) for _ in range(2))
    return _timed_launches(stats, events, 'emp_fill_holes_labels', C.c_void_p(t.data_ptr()), eb, *dims3(shape), radius, int(ball), hole_size,
                           _abi.ptr(d_labels), _abi.ptr(d_boxes), _abi.ptr(d_frames), len(turns), _abi.ptr(d_tiles), hp(offsets), len(levels),
                           _abi.ptr(parent), _abi.ptr(size), stats['scratch_entries'], _abi.stream_ptr(device))


_RAW_DTYPE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}      # an element of that size, whatever it means


def _elements(t, eb):
    """the bytes of the buffer ``t`` as elements of their size ``abs(eb)``"""
    return t.reshape(-1).view(torch.uint8).view(_RAW_DTYPE[abs(eb)])


@torch.no_grad()
def morph_labels(labels, operation, radius=1, apply3d=False, ids=None, plane=None, axis=0, device=None, out=None, inplace=False):
    """Morph Labels (_merge_split_widget.py:46-209): ``operation`` -- 'Dilate', 'Erode', 'Close' (erode(dilate)) or 'Open'
    (dilate(erode)), the widget's strings -- on single labels with ``disk(radius)`` / ``ball(radius)``, radius 1..7.

    The loop (:123-134) runs over ``ids``: every non-zero label ascending with ``ids=None`` (no points layer, :101), otherwise
    the ids given, in their order, a repeat being a second turn (the labels under the points, :113); zeros are dropped
    (:117).  A turn takes the box of its label as the array is then, pads it by the radius and clips it to the array (:56-67);
    inside that crop the label's voxels become 0, the mask ``crop == label`` goes through the operation, and the voxels of the
    result become the label, whatever they were.  Dilation sees false outside the crop and erosion true
    (``ndi.binary_dilation(structure=footprint)``, ``ndi.binary_erosion(structure=footprint, border_value=True)``: skimage's
    documented behaviour restated, not pinned against skimage, which is not available here).

    A 2-D array takes the disk (``apply3d`` is ignored, as the widget does, :97-98).  A 3-D array takes the ball with
    ``apply3d=True``, or with ``plane=k`` the disk on the image ``take(labels, k, axis)``, all other planes untouched (:153-169,
    without the reference's clipping of the image's box by the volume's shape).  A 3-D array with neither raises a
    ``ValueError`` (the reference's branch for it compares an int with a list, :143, and cannot run).

    Inputs and outputs are those of ``delete_labels``: a device tensor gives a device tensor (its own with ``inplace=True``), a
    numpy array a new numpy array (its own with ``inplace=True``); ``out=`` is for chunked stores, and a chunked store raises a
    ``ValueError``: the whole array must be on the device, a ball needs a halo across slabs.  Any integer dtype of 1-8 bytes,
    labels in [0, 2^63).  The result is exact and bit-reproducible; there is no numpy fallback.

    The one deliberate difference: a label that has no voxel left when its turn comes -- eaten by earlier dilations, or an id
    that never occurred -- is skipped; the reference dies there with an ``IndexError`` (``[...][0]`` of an empty list, :125)."""
    what = 'morph_labels'
    radius = _morph_args(operation, radius, what)
    return _morph_call(labels, what, lambda t, eb, shape, ball, device: _morph_device(t, eb, shape, operation, radius, ball, ids, device),
                       apply3d, plane, axis, device, out, inplace)


def _morph_call(labels, what, run, apply3d, plane, axis, device, out, inplace):
    """The inputs and outputs of ``morph_labels`` and ``fill_label_holes``: every check of the array, ``apply3d`` / ``plane`` /
    ``axis`` and ``out`` / ``inplace``, the way to the device and back, and in between ``run(t, eb, shape, ball, device)`` on the
    contiguous device buffer ``t`` -- the whole array, or the image ``take(labels, plane, axis)``"""
    if not isinstance(labels, torch.Tensor) and not _is_numpy(labels):
        if hasattr(labels, 'shape') and hasattr(labels, 'dtype') and hasattr(labels, '__getitem__'):
            raise ValueError(f'{what}: a chunked store is not supported: the whole array must be on the device (a ball needs a halo '
                             'across slabs); load it as a numpy array')
        raise TypeError(f'{what}: a device tensor or a numpy array, got {type(labels).__name__}')
    shape = tuple(int(s) for s in labels.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f'{what}: 2-D or 3-D label arrays, got shape {shape}')
    ball = len(shape) == 3 and bool(apply3d)
    if len(shape) == 3 and not ball:
        if plane is None:
            raise ValueError(f'{what}: a 3-D array needs apply3d=True (the ball) or plane=k (the disk on one image)')
        if axis not in (0, 1, 2) or not 0 <= int(plane) < shape[axis]:
            raise ValueError(f'{what}: plane {plane} of axis {axis} is not in an array of shape {shape}')
    ebytes(labels.dtype)      # a dtype that is not supported is refused here, before any work
    need_device()
    device = pick_device(device, labels)
    with torch.cuda.device(device):
        sink = _edit_target(labels, out, inplace, shape, labels.dtype, what)

        def whole(t, eb):
            if len(shape) == 3 and not ball:
                vol = _elements(t, eb).reshape(shape)
                img = vol.select(axis, int(plane)).contiguous()
                run(img, eb, tuple(img.shape), False, device)
                vol.select(axis, int(plane)).copy_(img)
            else:
                run(t, eb, shape, ball, device)
            return t, None
        return _whole_array(labels, sink, device, not inplace, whole)[0]


@torch.no_grad()
def fill_label_holes(labels, hole_size=64, radius=1, apply3d=False, ids=None, plane=None, axis=0, device=None, out=None, inplace=False):
    """Morph Labels' fifth operation, 'Fill holes' (_merge_split_widget.py:53, :90-91), on single labels:
    ``skimage.morphology.remove_small_holes(crop == label, hole_size)`` inside the label's padded box.

    The loop, ``ids``, the crop -- the label's box as the array is when its turn comes, padded by ``radius`` (1..7; the widget's
    slider applies to every operation, :56-67) and clipped -- ``apply3d`` / ``plane`` / ``axis``, the inputs and outputs and the
    dtypes are those of ``morph_labels``; chunked stores and 4-D arrays are refused in the same way.  A turn (:123-134): the
    complement of ``crop == label`` INSIDE THE CROP is split into its components of connectivity 1 (4 neighbours in an image, 6
    in a volume: no diagonals), and every voxel of a component with fewer than ``hole_size`` voxels (``<``) becomes the label.
    So voxels of other labels inside a small component are overwritten (a label that disappears that way has its own turn
    skipped, as in ``morph_labels``); a component that touches the crop's border is a component like any other -- this is not
    ``binary_fill_holes`` -- and when the background left around a label in its crop is smaller than ``hole_size`` the whole
    crop becomes the label; and the result depends on the crop: voxels outside it are in no component.

    ``hole_size``: an integer >= 0 (the widget's default is 64); 0 and 1 change nothing, and nothing is launched.
    ``remove_small_holes`` / ``remove_small_objects`` are restated from their source and, like the rest of Morph Labels, are not
    pinned against skimage, which is not available here; the tests state the loop with ``scipy.ndimage.label``.

    The work arrays are as large as the padded boxes of the turns that run together, not as the array; such a level whose boxes
    hold 2^31 - 1 voxels or more raises a ``ValueError``.  The result is exact and bit-reproducible; there is no numpy fallback."""
    what = 'fill_label_holes'
    radius = _morph_args('Dilate', radius, what)
    if isinstance(hole_size, bool) or not isinstance(hole_size, (int, float, np.integer, np.floating)) or int(hole_size) != hole_size \
            or hole_size < 0:
        raise ValueError(f'{what}: hole_size must be an integer >= 0, got {hole_size!r}')
    hole_size = min(int(hole_size), FILL_MAX_HOLE_SIZE)

    def run(t, eb, shape, ball, device):
        if hole_size > 1:      # no component has fewer than 1 voxel
            _fill_device(t, eb, shape, radius, hole_size, ball, ids, device)
    return _morph_call(labels, what, run, apply3d, plane, axis, device, out, inplace)


# ----------------------------------------------------------------------------
# Split Labels
# ----------------------------------------------------------------------------
def _labels_under(t, eb, shape, points, device):
    """the labels at ``points`` (n, ndim) of the device buffer ``t``, as int64 (labels lie below 2^63)"""
    under = _elements(t, eb)[torch.from_numpy(np.ravel_multi_index(tuple(points.T), shape)).to(device)].cpu().numpy()
    return (under.view(under.dtype.str.replace('i', 'u')) if eb > 0 else under).astype(np.int64)


def _split_edt(t, eb, shape, boxes, N, device, events):
    """emp_split_edt: the squared distance to the crop's background at the ``N`` voxels of ``boxes`` -> (the boxes on the device, d2)"""
    d_boxes = torch.empty(8 * len(boxes), dtype=torch.int64, device=device)
    d2 = torch.empty(N, dtype=torch.int32, device=device)
    work = torch.empty(int(_abi.load().emp_split_edt_work_bytes(N)), dtype=torch.uint8, device=device)
    _stage(events, 'edt', 'emp_split_edt', _abi.ptr(t), eb, *dims3(shape), hp(boxes), len(boxes), _abi.ptr(d_boxes), _abi.ptr(d2), N, _abi.ptr(work),
           _abi.stream_ptr(device))
    return d_boxes, d2


def _split_peaks(shape, boxes, d_boxes, d2, N, min_distance, device, events):
    """emp_split_peaks: the candidates of ``peak_local_max`` -> (cand (total, 3) int64 {box, linear index, value}, box after box;
    their number per box)"""
    work = torch.empty(int(_abi.load().emp_split_peaks_work_bytes(N, len(boxes))), dtype=torch.uint8, device=device)
    counts = torch.empty(len(boxes), dtype=torch.int32, device=device)
    cap = max(4096, N // 64)
    while True:
        cand = torch.empty(3 * cap, dtype=torch.int32, device=device)
        _stage(events, 'peaks', 'emp_split_peaks', hp(boxes), len(boxes), _abi.ptr(d_boxes), *dims3(shape), _abi.ptr(d2), N, min_distance,
               _abi.ptr(cand), cap, _abi.ptr(counts), _abi.ptr(work), _abi.stream_ptr(device))
        h_counts = counts.cpu().numpy().astype(np.int64)
        total = int(h_counts.sum())
        if total <= cap:
            break
        cap = total      # a ridge of equal distances: once more with room for all of them
    return cand[:3 * total].cpu().numpy().reshape(-1, 3).astype(np.int64), h_counts


def _split_flood(shape, boxes, d_boxes, d2, N, plateau, markers, device, events):
    """emp_split_flood: per voxel of the boxes the marker whose basin it lies in -> (that, the number of sweeps); without markers
    there is nothing to flood: (None, 0)"""
    if len(markers) == 0:
        return None, 0
    new = torch.empty(N, dtype=torch.int32, device=device)
    work = torch.empty(int(_abi.load().emp_split_flood_work_bytes(N, len(markers))), dtype=torch.uint8, device=device)
    sweeps = C.c_int64(0)
    _stage(events, 'flood', 'emp_split_flood', hp(boxes), len(boxes), _abi.ptr(d_boxes), *dims3(shape), _abi.ptr(d2), N, int(plateau), hp(markers),
           len(markers), _abi.ptr(new), _abi.ptr(work), _abi.stream_ptr(device), C.byref(sweeps))
    return new, int(sweeps.value)


def _split_write(t, eb, shape, boxes, d_boxes, new, bases, device, events):
    """emp_split_write: the label's voxels in every box with a base become base + marker"""
    d_bases = torch.from_numpy(bases).to(device)
    _stage(events, 'write', 'emp_split_write', _abi.ptr(t), eb, *dims3(shape), hp(boxes), len(boxes), _abi.ptr(d_boxes), _abi.ptr(new),
           int(boxes[:, 3:6].prod(axis=1).sum()), _abi.ptr(d_bases), _abi.stream_ptr(device))


def _split_pass(t, eb, shape, table, turns, points, under, min_distance, points_as_markers, start_label, device, stats, events):
    """One group of turns on the buffer ``t`` whose table is ``table``: everything is computed, launch by launch, before
    anything is written -> the report of these turns; ``stats`` is added to"""
    report, todo = P.split_screen(table, turns, points_as_markers)
    done = []      # per launch: (the turns, the boxes, their device copy, the markers of every voxel, the number of markers per box)
    for batch in _split_batches(todo[:, 4:].prod(axis=1).tolist()):
        boxes = P.split_boxes(turns, todo[batch])
        N = int(boxes[:, 3:6].prod(axis=1).sum())
        d_boxes, d2 = _split_edt(t, eb, shape, boxes, N, device, events)
        if points_as_markers:
            per_box = P.split_point_markers(points, under, boxes)
        else:
            cand, counts = _split_peaks(shape, boxes, d_boxes, d2, N, min_distance, device, events)
            stats['candidates'] += len(cand)
            per_box = P.split_peak_markers(cand, counts, boxes, min_distance)
        markers, n_markers = P.split_marker_array(per_box, boxes)
        new, sweeps = _split_flood(shape, boxes, d_boxes, d2, N, points_as_markers, markers, device, events)
        del d2
        for key, more in (('boxes', len(boxes)), ('entries', N), ('markers', int(n_markers.sum())), ('sweeps', sweeps)):
            stats[key] += more
        done.append((todo[batch, 0], boxes, d_boxes, new, n_markers))
    cur_max = int(table.labels.max()) if len(table.labels) else 0
    report, all_bases = P.split_ids(turns, report, [(mine, n_markers) for mine, _, _, _, n_markers in done], cur_max, start_label, eb)
    for (_, boxes, d_boxes, new, _), bases in zip(done, all_bases):
        if new is not None and (bases >= 0).any():
            _split_write(t, eb, shape, boxes, d_boxes, new, bases, device, events)
    return [(int(l), r) for l, r in zip(turns.tolist(), report)]


def _split_device(t, eb, shape, points, ids, min_distance, points_as_markers, start_label, device, stages=None):
    """Split Labels in place on the contiguous device buffer ``t`` (an image, or a volume as a whole) -> (the report, statistics).
    ``stages``: a dict that receives the device time of every stage in ms (tools/split_labels_bench.py)."""
    first = _table_of_source(RawSource(t, eb, shape), shape, False, device, None, None)
    turns, points, under = P.split_turns(points, None if points is None else _labels_under(t, eb, shape, points, device), ids)
    passes = P.split_passes(first, turns, start_label)
    stats = {'turns': int(len(turns)), 'boxes': 0, 'entries': 0, 'candidates': 0, 'markers': 0, 'sweeps': 0}
    events = None if stages is None else []
    # two passes: each has the table of the array as it is then, and new ids that do not fit raise before their pass writes: then
    # the first pass is undone
    report, before = [], (t.clone() if len(passes) > 1 else None)
    try:
        for mine in passes:
            table = first if before is None else _table_of_source(RawSource(t, eb, shape), shape, False, device, None, None)
            report += _split_pass(t, eb, shape, table, mine, points, under, min_distance, points_as_markers, start_label, device, stats, events)
    except ValueError:
        if before is not None:
            t.copy_(before)
        raise
    if stages is not None:
        if events:
            events[-1][2].synchronize()      # the last event of the stream: every pair before it has been reached
        for name, a, b in events:
            stages[name] = stages.get(name, 0.0) + a.elapsed_time(b)
    return report, stats


@torch.no_grad()
def split_labels(labels, points=None, ids=None, min_distance=10, points_as_markers=False, apply3d=False, start_label=None, plane=None,
                 axis=0, device=None, out=None, inplace=False, report=False):
    """Split Labels (_merge_split_widget.py:422-634): every label picked is cut into the basins of a watershed inside its own tight
    box, and the pieces get fresh ids.

    ``points``: an (n, ndim) integer array, the widget's points layer.  The labels under the points have a turn each, in
    ``np.unique`` order (:498-517); points on the background are dropped (:501-505).  ``ids=`` instead of points names the labels
    directly (distance mode only; ``np.unique`` order as well, zeros dropped).  A turn (:517-547): ``binary = crop == label`` in
    the label's box without padding, then

    * distance mode (the default, :428-447): the markers are ``peak_local_max(distance_transform_edt(binary), min_distance)``,
      ``min_distance`` 1..100, joined by ``ndi.label``; the energy is minus the distance.  A label that fills its box has no
      background (scipy's transform returns an artefact without an interior peak there): nothing to split.
    * ``points_as_markers`` (:449-456): the markers are the label's points, joined by ``ndi.label``; the energy is one plateau.

    With fewer than two markers there is nothing to split.  Otherwise ``new = watershed(energy, markers, mask=binary)`` and the
    label's voxels become ``new + max_label`` (:544), where ``max_label`` is the array's maximum when the turn comes -- it moves
    with every split -- or ``start_label - 1`` (the widget's 'Specify new label IDs').  The write is refused when the array's
    maximum is >= the smallest new id (:540): so a ``start_label`` in use is refused, and a second turn with the same
    ``start_label`` always is.  As in the reference, a part of the label that no marker reaches (its voxels are joined by
    corners only) becomes ``max_label`` itself, and when that id is a label with a turn of its own, that turn sees those voxels
    (it runs as a second pass).  New ids that do not fit the dtype raise a ``ValueError`` before anything is written.

    What is pinned and what is not.  The distance transform and the maximum filter are exact against ``scipy.ndimage``.
    ``peak_local_max`` (threshold ``image.min()``, the full (2d + 1)^n window with ``mode='nearest'``, ``exclude_border``, the
    squeeze of size-1 axes), ``ensure_spacing`` (greedy by distance, a kept peak rejects those at Euclidean distance < d, strictly)
    and the order of ``watershed``'s queue are restated from memory of skimage's source, which is not available here, and are NOT
    pinned.  The flood deviates on purpose: skimage's is a sequential priority queue over (value, age) that no parallel machine
    reproduces; here every voxel takes the label of the face neighbour with the smallest (level, steps at that level, label), the
    level-synchronous form of the same flood (``emp_split_flood``, tests/split_case.py ``flood_levels``).  Against a heap
    restatement of skimage's flood: identical on every voxel in points mode; in distance mode up to a few per cent of a label's
    voxels differ (0-4.3 % on the test cases), next to the border between two regions; every region is connected and holds its
    marker.

    A 2-D array, a 3-D array with ``apply3d=True``, or with ``plane=k`` the image ``take(labels, k, axis)`` (:549-588: the points
    must lie in that plane, and ``max_label`` is the image's); inputs, outputs, ``out`` / ``inplace`` and dtypes as in
    ``morph_labels``; chunked stores and 4-D arrays are refused.  The work arrays are as large as the boxes of the labels picked;
    a box needs ``nz^2 + ny^2 + nx^2 < 2^30``.  ``report=True``: also a list of ``(label, outcome)`` per turn, the outcome being the
    new ids or ``'nothing to split'``, ``'ids in use'``, ``'label absent'``.  Bit-reproducible; there is no numpy fallback."""
    what = 'split_labels'
    if isinstance(min_distance, bool) or int(min_distance) != min_distance or not 1 <= int(min_distance) <= SPLIT_MAX_DISTANCE:
        raise ValueError(f'{what}: min_distance must be an integer in 1..{SPLIT_MAX_DISTANCE}, got {min_distance!r}')
    if (points is None) == (ids is None):
        raise ValueError(f'{what}: give points= or ids=, one of them')
    if points_as_markers and points is None:
        raise ValueError(f'{what}: points_as_markers needs points=; ids= is for distance mode')
    if start_label is not None and (isinstance(start_label, bool) or int(start_label) != start_label or int(start_label) < 1):
        raise ValueError(f'{what}: start_label must be an integer >= 1, got {start_label!r}')
    shape = tuple(int(s) for s in getattr(labels, 'shape', ()))
    if points is not None:
        points = np.asarray(points)
        if points.size and not np.issubdtype(points.dtype, np.integer):
            raise ValueError(f'{what}: points must be integers (indices into the array)')
        points = points.astype(np.int64).reshape(-1, len(shape)) if len(shape) in (2, 3) else points
    found = []

    def run(t, eb, shp, ball, device):
        pts = points
        if pts is not None:
            if ((pts < 0) | (pts >= np.asarray(shape))).any():
                raise ValueError(f'{what}: a point lies outside the array of shape {shape}')
            if len(shp) < len(shape):      # the image of a plane: the points lose that axis
                if (pts[:, axis] != int(plane)).any():
                    raise ValueError(f'{what}: every point must lie in plane {plane} of axis {axis}')
                pts = np.delete(pts, axis, axis=1)
        found.extend(_split_device(t, eb, shp, pts, ids, int(min_distance), bool(points_as_markers), start_label, device)[0])
    res = _morph_call(labels, what, run, apply3d, plane, axis, device, out, inplace)
    return (res, found) if report else res
