"""Which objects of a label volume touch, and over how much surface, on the device: per pair of labels in contact the voxel pairs per
half-direction, the shared voxel faces and the Cauchy-Crofton contact area (contact length for an image)
(empanada_napari_amd.labels.label_contacts).  Prints one JSON summary line and, with --csv, writes one row per pair.
Usage: python tools/label_contacts.py IN [--spacing Z Y X] [--background] [--label-divisor N] [--csv OUT]
IN: a .npy file (memory-mapped and streamed in slabs) or a zarr array directory.  --spacing: the voxel size per axis (two values for
an image).  --background: also the contacts of every label with the background 0, as pairs (0, b).  --label-divisor: panoptic ids
(class * N + instance): the summary also holds the contact area class by class, pairs of two instances of one class included."""
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('src')
    ap.add_argument('--spacing', type=float, nargs='+', default=None, metavar='S')
    ap.add_argument('--background', action='store_true', help='also the pairs of a label with the background 0')
    ap.add_argument('--label-divisor', type=int, default=None, metavar='N')
    ap.add_argument('--csv', default=None, metavar='OUT')
    args = ap.parse_args(argv)
    src = np.load(args.src, mmap_mode='r') if args.src.endswith('.npy') else zstore.DirArray(args.src)
    c = L.label_contacts(src, spacing=args.spacing, background=args.background)
    if args.csv:
        c.to_csv(args.csv)
    size_name = 'contact_area' if c.ndim == 3 else 'contact_length'
    size = getattr(c, size_name)
    n = len(c.a)
    big = int(np.argmax(size)) if n else None
    out = {'shape': list(c.shape), 'spacing': list(c.spacing), 'background': bool(args.background), 'labels': len(c.labels), 'pairs': n,
           'voxel_pairs': int(c.counts.sum()), size_name + '_total': float(size.sum()),
           'largest': None if big is None else {'a': int(c.a[big]), 'b': int(c.b[big]), 'count': int(c.counts[big]), size_name: float(size[big]),
                                                'faces': c.faces[big].tolist()},
           'csv': args.csv}
    if args.label_divisor is not None:
        k = c.by_class(args.label_divisor)
        out['label_divisor'] = args.label_divisor
        out['classes'] = [{'a': int(a), 'b': int(b), 'count': int(cnt), size_name: float(s)}
                          for a, b, cnt, s in zip(k.a, k.b, k.counts, getattr(k, size_name))]
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
