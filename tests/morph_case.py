"""The statement the Morph Labels tests compare against, in numpy / scipy (tests/test_morph_host.py, tests/test_gpu_morph.py):
the loop of empanada_napari/_merge_split_widget.py:123-134 restated.  Everything is integer: every comparison is exact.

* footprints: ``x^2 + y^2 (+ z^2) <= r^2`` on a (2r + 1)-cube (skimage.morphology.disk / ball)
* dilation:   ``scipy.ndimage.binary_dilation(binary, structure=footprint)`` (outside the crop is false)
* erosion:    ``scipy.ndimage.binary_erosion(binary, structure=footprint, border_value=True)`` (outside the crop is true)
* Close = erosion(dilation), Open = dilation(erosion)
* a turn: the box of the label as the array is now, padded by the radius and clipped; ``binary = crop == label``;
  ``crop[binary] = 0``; ``crop[op(binary)] = label``.  A label that has no voxel left is skipped (the reference raises there).

skimage is not available here: that its ``binary_dilation`` / ``binary_erosion`` are the two scipy calls above is restated from
its documented behaviour and is not pinned against it (as for regionprops / clear_border in tests/labels_case.py)."""
import numpy as np
from scipy import ndimage as ndi

OPS = ('Dilate', 'Erode', 'Close', 'Open')


def footprint(radius, ndim):
    g = np.indices((2 * radius + 1,) * ndim) - radius
    return (g ** 2).sum(axis=0) <= radius * radius


def dilate(binary, fp):
    return ndi.binary_dilation(binary, structure=fp)


def erode(binary, fp):
    return ndi.binary_erosion(binary, structure=fp, border_value=True)


def binary_op(binary, operation, fp):
    if operation == 'Dilate':
        return dilate(binary, fp)
    if operation == 'Erode':
        return erode(binary, fp)
    if operation == 'Close':
        return erode(dilate(binary, fp), fp)
    if operation == 'Open':
        return dilate(erode(binary, fp), fp)
    raise ValueError(operation)


def turn(arr, label, operation, radius, fp):
    """one turn of the loop, in place; False: the label has no voxel (skipped)"""
    nz = np.nonzero(arr == label)
    if len(nz[0]) == 0:
        return False
    sl = tuple(slice(max(0, int(c.min()) - radius), min(s, int(c.max()) + 1 + radius)) for c, s in zip(nz, arr.shape))
    crop = arr[sl]
    binary = crop == label
    crop[binary] = 0
    crop[binary_op(binary, operation, fp)] = label
    return True


def turns_of(arr, ids=None):
    if ids is None:
        return [int(v) for v in np.unique(arr) if v != 0]
    return [int(v) for v in np.asarray(ids).reshape(-1) if v > 0]


def morph(arr, operation, radius, ids=None):
    """the sequential loop on a 2-D image (disk) or a 3-D volume (ball) -> (new array, number of skipped turns)"""
    out = np.array(arr, copy=True)
    fp = footprint(radius, out.ndim)
    skipped = 0
    for label in turns_of(out, ids):
        skipped += not turn(out, label, operation, radius, fp)
    return out, skipped


def morph_plane(vol, operation, radius, plane, axis, ids=None):
    """the disk on the image take(vol, plane, axis); the rest of the volume is untouched"""
    out = np.array(vol, copy=True)
    img, _ = morph(np.take(out, plane, axis), operation, radius, ids)
    idx = [slice(None)] * 3
    idx[axis] = plane
    out[tuple(idx)] = img
    return out


def morph_by_levels(arr, turns, levels, operation, radius):
    """the schedule emulated: levels in order, the turns of a level in REVERSE order"""
    out = np.array(arr, copy=True)
    fp = footprint(radius, out.ndim)
    for level in levels:
        for i in reversed(level):
            turn(out, int(turns[i]), operation, radius, fp)
    return out


def morph_whole_image(arr, operation, radius):
    """the same loop without the crop: every label's mask goes through the operation on the whole array (dilation with false,
    erosion with true outside the ARRAY) -- what the device path must NOT compute"""
    out = np.array(arr, copy=True)
    fp = footprint(radius, out.ndim)
    for label in turns_of(out):
        binary = out == label
        if not binary.any():
            continue
        out[binary] = 0
        out[binary_op(binary, operation, fp)] = label
    return out


def blobs(shape, n, seed, dtype=np.int32, first=1):
    """n ellipsoids, semi-axes 2..8, centres anywhere in the array (some touch the border), labels first .. first + n - 1 painted
    in a shuffled order (ids are not spatially sorted; later ones overwrite earlier ones)"""
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, dtype)
    grid = np.indices(shape)
    centres = [[rng.uniform(0, s) for s in shape] for _ in range(n)]
    axes = [[rng.uniform(2, 8) for _ in shape] for _ in range(n)]
    for i in rng.permutation(n):
        v[sum(((g - c) / a) ** 2 for g, c, a in zip(grid, centres[i], axes[i])) <= 1] = first + i
    return v
