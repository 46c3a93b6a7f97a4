"""Clean up a label volume on the device and print one JSON object: the plugin's Filter Small Labels, Delete Labels, Merge Labels,
Count Labels, Morph Labels and Split Labels on a file.
Usage: python tools/clean_labels.py IN [OUT] [--min-area N | --boundary [--whole-labels | --streamed] | --delete IDS | --merge IDS [--into ID] |
                                             --count --label-divisor D | --morph OP [--radius R] [--3d] |
                                             --fill-holes [HOLE_SIZE] [--radius R] [--3d] |
                                             --split IDS [--min-distance D] [--3d]] [--per-slice]
IN / OUT: .npy files (IN is memory-mapped and streamed in slabs, OUT is created) or zarr array directories (OUT is created with
IN's shape, dtype and chunks).  IDS: comma-separated label ids.  --count needs no OUT.  --boundary --streamed: the reference mode
(only the components that touch a face go) slab by slab, for volumes the one-call components cannot take.  --morph OP: Dilate, Erode, Close or Open
of every label with a disk of radius R (a 2-D IN) or, with --3d, a ball (a 3-D IN); IN must be a .npy file (the whole array goes
to the device); labels_affected is the number of labels that had a turn.  --fill-holes [HOLE_SIZE]: Morph Labels' 'Fill holes' on
every label: the holes of fewer than HOLE_SIZE voxels (default 64) inside the label's box padded by R; same rules and the same JSON
line as --morph.  --split IDS: Split Labels in distance mode on the labels named: each is cut into the basins of a watershed from
the peaks of its distance transform that are at least D apart (default 10) and the pieces get fresh ids above the array's maximum;
IN must be a .npy file; labels_affected is the number of labels that were split, and `new_ids` lists their pieces."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.load_package()
from empanada_napari_amd import labels as L, zstore  # noqa: E402


def _open(path):
    return np.load(path, mmap_mode='r') if path.endswith('.npy') else zstore.DirArray(path)


def _create(path, like):
    if path.endswith('.npy'):
        return np.lib.format.open_memmap(path, mode='w+', dtype=np.dtype(like.dtype), shape=tuple(like.shape))
    chunks = getattr(like, 'chunks', None) or tuple(min(s, 64) for s in like.shape)
    return zstore.DirArray.create(path, tuple(like.shape), np.dtype(like.dtype), chunks, overwrite=True)


def _ids(text):
    return [int(v) for v in text.split(',') if v.strip()]


def _occurring(table, ids):
    """how many of the ids given occur in the volume (background never counts)"""
    ids = np.unique(np.asarray(ids, dtype=np.int64))
    return int(np.isin(ids[ids > 0], table.labels).sum())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('src')
    ap.add_argument('dst', nargs='?')
    op = ap.add_mutually_exclusive_group(required=True)
    op.add_argument('--min-area', type=int)
    op.add_argument('--boundary', action='store_true')
    op.add_argument('--delete', type=_ids)
    op.add_argument('--merge', type=_ids)
    op.add_argument('--count', action='store_true')
    op.add_argument('--morph', choices=list(L.MORPH_OPS), metavar='OP')
    op.add_argument('--fill-holes', type=int, nargs='?', const=64, default=None, metavar='HOLE_SIZE')
    op.add_argument('--split', type=_ids, metavar='IDS')
    ap.add_argument('--min-distance', type=int, default=10, help='--split: the least distance between two peaks, 1..100')
    ap.add_argument('--radius', type=int, default=1, help='--morph: radius of the disk / ball, 1..7; --fill-holes: the padding of the box')
    ap.add_argument('--3d', dest='apply3d', action='store_true', help='--morph / --fill-holes / --split: the ball / the volume\'s components / the volume\'s watershed on a 3-D array')
    ap.add_argument('--whole-labels', action='store_true')
    ap.add_argument('--streamed', action='store_true', help='--boundary: the components slab by slab, for a volume of any size')
    ap.add_argument('--into', type=int, default=None, help='--merge: the id the others become (default: the smallest)')
    ap.add_argument('--label-divisor', type=int, default=0)
    ap.add_argument('--per-slice', action='store_true')
    args = ap.parse_args(argv)
    if not args.count and not args.dst:
        ap.error('OUT is needed for every operation but --count')
    src = _open(args.src)
    if args.count:
        table = L.label_table(src, per_slice=args.per_slice)
        lists = L.class_label_lists(table, args.label_divisor)
        count = (lambda q: {str(k): len(v) for k, v in q.items()})
        out = {'shape': list(table.shape), 'labels': {str(z): count(q) for z, q in lists.items()} if args.per_slice else count(lists)}
        print(json.dumps(out))
        return out
    dst = _create(args.dst, src)

    def run(fn, *a, **k):
        """stores are written slab by slab; a .npy input is an array to the library: its result is copied into the output map"""
        if isinstance(src, np.ndarray):
            res = fn(np.asarray(src), *a, **k)
            dst[...] = res[0] if isinstance(res, tuple) else res
        else:
            res = fn(src, *a, out=dst, **k)
        return res[1] if isinstance(res, tuple) else None

    extra = {}
    if args.split is not None:
        if not isinstance(src, np.ndarray):
            ap.error('--split needs a .npy input: the whole array goes to the device')
        res, report = L.split_labels(np.asarray(src), ids=args.split, min_distance=args.min_distance, apply3d=args.apply3d, report=True)
        dst[...] = res
        extra['new_ids'] = {str(label): [int(v) for v in new] for label, new in report if not isinstance(new, str)}
        n = len(extra['new_ids'])
    elif args.morph is not None or args.fill_holes is not None:
        n = len(np.unique(src)) - int((np.asarray(src) == 0).any())
        if args.morph is not None:
            run(L.morph_labels, args.morph, radius=args.radius, apply3d=args.apply3d)
        else:
            run(L.fill_label_holes, hole_size=args.fill_holes, radius=args.radius, apply3d=args.apply3d)
    elif args.min_area is not None:
        n = run(L.filter_out_small_label_areas, args.min_area, per_slice=args.per_slice)
    elif args.boundary and args.streamed:
        if args.whole_labels or args.per_slice:
            ap.error('--streamed is the reference mode of --boundary on one image or volume: not with --whole-labels or --per-slice')
        if isinstance(src, np.ndarray):      # slab by slab also for a .npy file: the output map is edited in place
            dst[...] = src
            n = L.remove_boundary_labels(dst, streamed=True, inplace=True)[1]
        else:
            n = L.remove_boundary_labels(src, streamed=True, out=dst)[1]
    elif args.boundary:
        n = run(L.remove_boundary_labels, whole_labels=args.whole_labels, per_slice=args.per_slice)
    else:      # the edits by id do not look at the volume's labels: the number of ids that occur comes from its table
        ids = args.delete if args.delete is not None else args.merge
        n = _occurring(L.label_table(src), ids)
        if args.delete is not None:
            run(L.delete_labels, ids)
        else:
            run(L.merge_labels, ids, new_label_id=args.into)
    if hasattr(dst, 'flush'):
        dst.flush()
    out = {'shape': list(src.shape), 'labels_affected': int(n), 'out': args.dst, **extra}
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
