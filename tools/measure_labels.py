"""Measure the objects of a label volume on the device: per label its voxel count, box, centroid, volume, voxel-face surface,
equivalent diameter, sphericity and principal variances (empanada_napari_amd.labels.measure_labels).  Prints one JSON summary
line and, with --csv, writes one row per label (per slice and label with --per-slice).
Usage: python tools/measure_labels.py IN [--spacing Z Y X] [--per-slice] [--no-border-faces] [--csv OUT]
IN: a .npy file (memory-mapped and streamed in slabs) or a zarr array directory.  --spacing: the voxel size per axis (two values for
an image).  The surface is the sum of the exposed voxel faces, which overestimates a smooth surface by up to 1.5 x."""
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
    ap.add_argument('--no-border-faces', action='store_true', help='do not count the faces on the faces of the array')
    ap.add_argument('--csv', default=None, metavar='OUT')
    args = ap.parse_args(argv)
    src = np.load(args.src, mmap_mode='r') if args.src.endswith('.npy') else zstore.DirArray(args.src)
    m = L.measure_labels(src, spacing=args.spacing, per_slice=args.per_slice, border_faces=not args.no_border_faces)
    if args.csv:
        m.to_csv(args.csv)
    k = len(m.labels)
    big = int(np.argmax(m.areas)) if k else None
    out = {'shape': list(m.shape), 'spacing': list(m.spacing), 'per_slice': bool(args.per_slice), 'labels': k,
           'voxels_labelled': int(m.areas.sum()), 'volume_total': float(m.volume.sum()), 'surface_total': float(m.surface_area.sum()),
           'largest': None if big is None else {'label': int(m.labels[big]), 'area': int(m.areas[big]),
                                                'centroid': [float(v) for v in m.centroid_physical[big]]},
           'csv': args.csv}
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
