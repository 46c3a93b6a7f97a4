"""Split a label volume into its connected components on the device, slab by slab, and print one JSON line with their number:
equal non-zero value, full connectivity (8 neighbours in an image, 26 in a volume), numbered 1..count in raster order of each
component's first element (empanada_napari_amd.labels.label_components).
Usage: python tools/label_components.py IN OUT [--slab N]
IN / OUT: .npy files (IN is memory-mapped and streamed in slabs, OUT is created as an int32 map and written slab by slab) or zarr
array directories (OUT is created as int32 with IN's shape and chunks).  --slab: leading-axis entries per slab (default: about 64 MiB
of IN, at most 2^28 voxels); the result does not depend on it."""
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
    ap.add_argument('dst')
    ap.add_argument('--slab', type=int, default=None)
    args = ap.parse_args(argv)
    src = np.load(args.src, mmap_mode='r') if args.src.endswith('.npy') else zstore.DirArray(args.src)
    shape = tuple(src.shape)
    if args.dst.endswith('.npy'):
        dst = np.lib.format.open_memmap(args.dst, mode='w+', dtype=np.int32, shape=shape)
    else:
        chunks = getattr(src, 'chunks', None) or tuple(min(s, 64) for s in shape)
        dst = zstore.DirArray.create(args.dst, shape, np.int32, chunks, overwrite=True)
    stats = {}
    _, count = L.label_components(src, out=dst, slab=args.slab, _stats=stats)
    if hasattr(dst, 'flush'):
        dst.flush()
    out = {'shape': list(shape), 'components': int(count), 'slabs': int(stats.get('slabs', 0)), 'out': args.dst}
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
