"""Shape of the objects of a label volume on the device: per label its voxel count, volume, Cauchy-Crofton surface (perimeter for an
image or per slice), the sphericity (circularity) that goes with it, the Euler number under full and under face connectivity and
the raw intercept counts (empanada_napari_amd.labels.shape_labels).  Prints one JSON summary line and, with --csv, writes one row per
label (per slice and label with --per-slice).
Usage: python tools/shape_labels.py IN [--spacing Z Y X] [--per-slice] [--no-border-faces] [--csv OUT]
IN: a .npy file (memory-mapped and streamed in slabs) or a zarr array directory.  --spacing: the voxel size per axis (two values for
an image).  An Euler number other than 1 is the usual sign of a cavity, a handle or an object in several pieces."""
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
    ap.add_argument('--per-slice', action='store_true')
    ap.add_argument('--no-border-faces', action='store_true', help='do not count intercepts with the outside of the array')
    ap.add_argument('--csv', default=None, metavar='OUT')
    args = ap.parse_args(argv)
    src = np.load(args.src, mmap_mode='r') if args.src.endswith('.npy') else zstore.DirArray(args.src)
    s = L.shape_labels(src, spacing=args.spacing, per_slice=args.per_slice, border_faces=not args.no_border_faces)
    if args.csv:
        s.to_csv(args.csv)
    k = len(s.labels)
    size = s.surface_area if s.ndim == 3 else s.perimeter
    round_ = s.sphericity if s.ndim == 3 else s.circularity
    big = int(np.argmax(s.areas)) if k else None
    out = {'shape': list(s.shape), 'spacing': list(s.spacing), 'per_slice': bool(args.per_slice), 'labels': k,
           'voxels_labelled': int(s.areas.sum()), 'volume_total': float(s.volume.sum()),
           'surface_total' if s.ndim == 3 else 'perimeter_total': float(size.sum()),
           'labels_with_euler_number_not_1': int(np.count_nonzero(s.euler[:, 0] != 1)),
           'largest': None if big is None else {'label': int(s.labels[big]), 'area': int(s.areas[big]), 'size': float(size[big]),
                                                'roundness': float(round_[big]), 'euler_number': int(s.euler[big, 0])},
           'csv': args.csv}
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
