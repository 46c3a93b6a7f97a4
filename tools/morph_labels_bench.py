"""Time Morph Labels on the device (csrc/morph.hip through labels.morph_labels) against the scipy restatement of the reference's
loop (empanada_napari/_merge_split_widget.py:123-134) on the same machine, and write one JSON line.
Cases: a procedural 2-D image and a 3-D volume of ellipsoid labels, each sparse and dense; every op at radius 1, 3 and 7.
Per case and (op, radius):
  call_ms      host clock around morph_labels(device tensor, inplace=True) ending in a device synchronise: the label table, the
               schedule and tile lists on the host, the uploads and the launches -- median, min and max of --reps calls after a
               warm-up call, each on a fresh copy of the input
  kernels_ms   HIP events around the launches of the levels alone (same calls)
  levels, launches, tiles, turns
  scipy_s      the sequential loop with scipy.ndimage (tests/morph_case.py's statement, restated here so that the tool stands
               alone), timed once over the first --host-turns turns and extrapolated to all turns where there are more
               (scipy_turns_timed says how many were run); where every turn was run the two results are compared (equal_to_scipy)
Usage: python tools/morph_labels_bench.py [--reps 5] [--host-turns 40] [--quick] [--out profiles/morph_labels_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.load_package()
from empanada_napari_amd import labels as L  # noqa: E402
from empanada_napari_amd._labelstream import ebytes  # noqa: E402

OPS = ('Dilate', 'Erode', 'Close', 'Open')


def ellipsoids(shape, n, seed, dtype=np.int32):
    """n ellipsoids with semi-axes 2..8 and centres anywhere, labels 1..n painted in a shuffled order, each inside its own box"""
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, dtype)
    centres = rng.uniform(0, 1, (n, len(shape))) * np.asarray(shape)
    axes = rng.uniform(2, 8, (n, len(shape)))
    for i in rng.permutation(n):
        lo = np.maximum(np.floor(centres[i] - axes[i]).astype(int), 0)
        hi = np.minimum(np.ceil(centres[i] + axes[i]).astype(int) + 1, shape)
        sl = tuple(slice(a, b) for a, b in zip(lo, hi))
        g = np.indices(tuple(hi - lo)) + lo.reshape((-1,) + (1,) * len(shape))
        inside = sum(((g[d] - centres[i][d]) / axes[i][d]) ** 2 for d in range(len(shape))) <= 1
        v[sl][inside] = i + 1
    return v


def _footprint(radius, ndim):
    g = np.indices((2 * radius + 1,) * ndim) - radius
    return (g ** 2).sum(axis=0) <= radius * radius


def _binary_op(binary, operation, fp):
    dil = lambda b: ndi.binary_dilation(b, structure=fp)      # noqa: E731
    ero = lambda b: ndi.binary_erosion(b, structure=fp, border_value=True)      # noqa: E731
    return {'Dilate': dil, 'Erode': ero, 'Close': lambda b: ero(dil(b)), 'Open': lambda b: dil(ero(b))}[operation](binary)


def scipy_loop(arr, operation, radius, max_turns):
    """the reference's loop without its regionprops pass per label: boxes from one find_objects-like scan per turn's crop"""
    out = arr.copy()
    fp = _footprint(radius, out.ndim)
    turns = [int(v) for v in np.unique(out) if v != 0]
    done = 0
    t0 = time.perf_counter()
    for label in turns[:max_turns]:
        nz = np.nonzero(out == label)
        if len(nz[0]) == 0:
            continue
        sl = tuple(slice(max(0, int(c.min()) - radius), min(s, int(c.max()) + 1 + radius)) for c, s in zip(nz, out.shape))
        crop = out[sl]
        binary = crop == label
        crop[binary] = 0
        crop[_binary_op(binary, operation, fp)] = label
        done += 1
    dt = time.perf_counter() - t0
    timed = min(len(turns), max_turns)
    return out, dt, timed, len(turns)


def device_case(arr, operation, radius, reps):
    t0 = torch.from_numpy(arr).cuda()
    eb = ebytes(t0.dtype)
    call, kern, stats, res = [], [], None, None
    for i in range(reps + 1):      # the first call is the warm-up
        t = t0.clone()
        torch.cuda.synchronize()
        c0 = time.perf_counter()
        stats = L._morph_device(t, eb, tuple(arr.shape), operation, radius, arr.ndim == 3, None, t.device, events=True)
        torch.cuda.synchronize()
        c1 = time.perf_counter()
        if i > 0:
            call.append((c1 - c0) * 1e3)
            kern.append(stats['events'][0].elapsed_time(stats['events'][1]) if 'events' in stats else 0.0)
        res = t
    spread = lambda ms: {'median': round(float(np.median(ms)), 3), 'min': round(min(ms), 3), 'max': round(max(ms), 3)}      # noqa: E731
    stats.pop('events', None)
    return {'call_ms': spread(call), 'kernels_ms': spread(kern), **stats}, res.cpu().numpy()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-turns', type=int, default=40)
    ap.add_argument('--quick', action='store_true', help='small cases (a rehearsal of the tool, not a measurement)')
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'morph_labels_bench needs the MI355X'
    q = args.quick
    cases = {
        'image_1024^2_sparse_100': ((256, 256) if q else (1024, 1024), 20 if q else 100),
        'image_1024^2_dense_3000': ((256, 256) if q else (1024, 1024), 200 if q else 3000),
        'volume_64x128x128_sparse_60': ((16, 64, 64) if q else (64, 128, 128), 10 if q else 60),
        'volume_64x128x128_dense_600': ((16, 64, 64) if q else (64, 128, 128), 60 if q else 600),
    }
    out = {'reps': args.reps, 'host_turns': args.host_turns, 'quick': bool(q), 'cases': {}}
    for seed, (name, (shape, n)) in enumerate(cases.items()):
        arr = ellipsoids(shape, n, seed)
        rec = {'shape': list(shape), 'labels': int(len(np.unique(arr)) - 1), 'foreground_fraction': round(float((arr != 0).mean()), 4)}
        for operation in OPS:
            for radius in (1, 3, 7):
                dev, got = device_case(arr, operation, radius, args.reps)
                want, dt, timed, total = scipy_loop(arr, operation, radius, args.host_turns)
                dev.update({'scipy_s': round(dt / max(timed, 1) * total, 4), 'scipy_turns_timed': timed})
                if timed == total:
                    dev['equal_to_scipy'] = bool(np.array_equal(got, want))
                dev['scipy_over_call'] = round(dev['scipy_s'] * 1e3 / max(dev['call_ms']['median'], 1e-6), 1)
                rec[f'{operation}_r{radius}'] = dev
        out['cases'][name] = rec
    line = json.dumps(out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)
