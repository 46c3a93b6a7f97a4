"""The statement the Fill holes tests compare against, in numpy / scipy (tests/test_fill_holes_host.py,
tests/test_gpu_fill_holes.py): the loop of empanada_napari/_merge_split_widget.py:123-134 with ``operation == 'Fill holes'``
(:53, :90-91) restated.  Everything is integer: every comparison is exact.

* ``remove_small_holes(binary, hole_size)``: the complement of ``binary`` is labelled with connectivity 1 (4 neighbours in an
  image, 6 in a volume: ``ndi.label(~binary, generate_binary_structure(ndim, 1))``) and every component with FEWER than
  ``hole_size`` voxels (``sizes < hole_size``) becomes foreground; a component that touches the border of the array it is given
  is a component like any other (this is not ``binary_fill_holes``); ``hole_size == 0`` returns the mask unchanged
* a turn: the box of the label as the array is now, padded by the radius and clipped (the radius slider applies to every
  operation, :56-67); ``binary = crop == label``; ``crop[remove_small_holes(binary, hole_size)] = label``.  The mask only grows,
  so the reference's ``crop[binary] = 0`` before it changes nothing.  A label that has no voxel left is skipped (the reference
  raises there).

skimage is not available here: ``remove_small_holes`` / ``remove_small_objects`` are restated from their source and are not
pinned against skimage, like the rest of Morph Labels (tests/morph_case.py)."""
import numpy as np
from scipy import ndimage as ndi

from morph_case import blobs, turns_of


def remove_small_holes(binary, hole_size, connectivity=1, strict=True):
    """skimage.morphology.remove_small_holes(binary, hole_size); ``connectivity=2`` and ``strict=False`` (``<=``) are the wrong
    variants below"""
    binary = np.asarray(binary, dtype=bool)
    if hole_size == 0:
        return binary.copy()
    comps, _ = ndi.label(~binary, ndi.generate_binary_structure(binary.ndim, connectivity))
    sizes = np.bincount(comps.ravel())
    small = sizes < hole_size if strict else sizes <= hole_size
    small[0] = False      # component 0 is the mask itself
    return binary | small[comps]


def _crop_of(arr, label, radius, box_of=None):
    nz = np.nonzero((arr if box_of is None else box_of) == label)
    if len(nz[0]) == 0:
        return None
    return tuple(slice(max(0, int(c.min()) - radius), min(s, int(c.max()) + 1 + radius)) for c, s in zip(nz, arr.shape))


def turn(arr, label, radius, hole_size, connectivity=1, strict=True, box_of=None):
    """one turn of the loop, in place; False: the label has no voxel (skipped).  ``box_of``: the array the label's box is taken
    from (a wrong variant: the original array instead of the current one)"""
    if not (arr == label).any():
        return False
    sl = _crop_of(arr, label, radius, box_of)
    if sl is None:
        return False
    crop = arr[sl]
    binary = crop == label
    crop[remove_small_holes(binary, hole_size, connectivity, strict)] = label
    return True


def fill(arr, radius, hole_size, ids=None):
    """the sequential loop on a 2-D image or a 3-D volume -> (new array, number of skipped turns)"""
    out = np.array(arr, copy=True)
    skipped = 0
    for label in turns_of(out, ids):
        skipped += not turn(out, label, radius, hole_size)
    return out, skipped


def fill_plane(vol, radius, hole_size, plane, axis, ids=None):
    """the loop on the image take(vol, plane, axis); the rest of the volume is untouched"""
    out = np.array(vol, copy=True)
    img, _ = fill(np.take(out, plane, axis), radius, hole_size, ids)
    idx = [slice(None)] * 3
    idx[axis] = plane
    out[tuple(idx)] = img
    return out


def fill_by_levels(arr, turns, levels, radius, hole_size):
    """the schedule emulated: levels in order, the turns of a level in REVERSE order"""
    out = np.array(arr, copy=True)
    for level in levels:
        for i in reversed(level):
            turn(out, int(turns[i]), radius, hole_size)
    return out


# ----------------------------------------------------------------------------
# what the device path must NOT compute
# ----------------------------------------------------------------------------
def fill_connectivity2(arr, radius, hole_size, ids=None):
    """components of the background with diagonal neighbours (8 in an image, 18 in a volume)"""
    out = np.array(arr, copy=True)
    for label in turns_of(out, ids):
        turn(out, label, radius, hole_size, connectivity=2)
    return out


def fill_le(arr, radius, hole_size, ids=None):
    """``sizes <= hole_size`` instead of ``<``"""
    out = np.array(arr, copy=True)
    for label in turns_of(out, ids):
        turn(out, label, radius, hole_size, strict=False)
    return out


def fill_whole_array(arr, radius, hole_size, ids=None):
    """the same loop without the crop: the holes of every label's mask over the whole array"""
    out = np.array(arr, copy=True)
    for label in turns_of(out, ids):
        binary = out == label
        if binary.any():
            out[remove_small_holes(binary, hole_size)] = label
    return out


def fill_original_boxes(arr, radius, hole_size, ids=None):
    """every crop from the label's box in the ORIGINAL array instead of the array as it is when the turn comes (a label that
    is gone by then is still skipped)"""
    out = np.array(arr, copy=True)
    for label in turns_of(out, ids):
        turn(out, label, radius, hole_size, box_of=arr)
    return out


def holes(shape, n, seed, dtype=np.int32):
    """``blobs(shape, n, seed)`` with holes and inclusions: 3 * n draws, each a voxel and, where it lies in a label, a box with
    sides 1..4 around it that becomes 0 (probability 0.7) or a fresh label counted from 1000"""
    v = blobs(shape, n, seed, dtype)
    rng = np.random.default_rng(seed)
    fresh = 1000
    for _ in range(3 * n):
        at = [int(rng.integers(0, s)) for s in shape]
        if v[tuple(at)] == 0:
            continue
        sides = [int(rng.integers(1, 5)) for _ in shape]
        sl = tuple(slice(max(0, a - s // 2), a - s // 2 + s) for a, s in zip(at, sides))
        if rng.random() < 0.7:
            v[sl] = 0
        else:
            v[sl] = fresh
            fresh += 1
    return v
