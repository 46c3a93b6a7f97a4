"""Time Fill holes on the device (csrc/morph.hip through labels.fill_label_holes) against the scipy restatement of the reference's
loop (empanada_napari/_merge_split_widget.py:53,90-91,123-134) on the same machine, and write one JSON line.
Cases: a procedural 2-D image and a 3-D volume of ellipsoid labels with holes and inclusions, each sparse and dense; radius 1 and
7, hole_size 64 and 10^6.  Per case and (radius, hole_size):
  call_ms      host clock around the device loop on a device tensor, in place, ending in a device synchronise: the label table,
               the schedule, tile lists and frames on the host, the uploads and the launches -- median, min and max of --reps
               calls after a warm-up call, each on a fresh copy of the input
  kernels_ms   HIP events around the launches of the levels alone (same calls)
  levels, launches, tiles, turns, scratch_entries
  scipy_s      the sequential loop with scipy.ndimage.label (tests/fill_holes_case.py's statement, restated here so that the tool
               stands alone), timed once over the first --host-turns turns (0: all of them) and extrapolated where there are
               more; where every turn was run the two results are compared (equal_to_scipy)
and per case and radius, for the overhead of a level: close_r<radius>, the same figures of morph_labels(..., 'Close') on the same
input (the levels are the same ones: both operations are scheduled as a dilation).
Usage: python tools/fill_holes_bench.py [--reps 5] [--host-turns 0] [--quick] [--out profiles/fill_holes_bench.json]"""
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


def ellipsoids_with_holes(shape, n, seed, dtype=np.int32):
    """n ellipsoids with semi-axes 2..8 and centres anywhere, labels 1..n painted in a shuffled order, each inside its own box;
    then 3 * n draws of a voxel: where it lies in a label, a box with sides 1..4 around it becomes 0 (probability 0.7) or a
    fresh label counted from n + 1000"""
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
    fresh = n + 1000
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


def scipy_loop(arr, radius, hole_size, max_turns):
    """the reference's loop without its regionprops pass per label: the box from one scan of the array per turn"""
    out = arr.copy()
    structure = ndi.generate_binary_structure(out.ndim, 1)
    turns = [int(v) for v in np.unique(out) if v != 0]
    timed = len(turns) if max_turns <= 0 else min(len(turns), max_turns)
    t0 = time.perf_counter()
    for label in turns[:timed]:
        nz = np.nonzero(out == label)
        if len(nz[0]) == 0:
            continue
        sl = tuple(slice(max(0, int(c.min()) - radius), min(s, int(c.max()) + 1 + radius)) for c, s in zip(nz, out.shape))
        crop = out[sl]
        binary = crop == label
        comps, _ = ndi.label(~binary, structure)
        small = np.bincount(comps.ravel()) < hole_size
        small[0] = False
        crop[small[comps]] = label
    dt = time.perf_counter() - t0
    return out, dt, timed, len(turns)


def device_case(arr, reps, run):
    """``run(t, eb)`` is the device loop in place on the tensor ``t`` and returns its statistics"""
    t0 = torch.from_numpy(arr).cuda()
    eb = ebytes(t0.dtype)
    call, kern, stats, res = [], [], None, None
    for i in range(reps + 1):      # the first call is the warm-up
        t = t0.clone()
        torch.cuda.synchronize()
        c0 = time.perf_counter()
        stats = run(t, eb)
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
    ap.add_argument('--host-turns', type=int, default=0, help='turns of the scipy loop that are timed (0: all of them)')
    ap.add_argument('--quick', action='store_true', help='small cases (a rehearsal of the tool, not a measurement)')
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'fill_holes_bench needs the MI355X'
    q = args.quick
    cases = {
        'image_1024^2_sparse_100': ((256, 256) if q else (1024, 1024), 20 if q else 100),
        'image_1024^2_dense_3000': ((256, 256) if q else (1024, 1024), 200 if q else 3000),
        'volume_64x128x128_sparse_60': ((16, 64, 64) if q else (64, 128, 128), 10 if q else 60),
        'volume_64x128x128_dense_600': ((16, 64, 64) if q else (64, 128, 128), 60 if q else 600),
    }
    out = {'reps': args.reps, 'host_turns': args.host_turns, 'quick': bool(q), 'cases': {}}
    for seed, (name, (shape, n)) in enumerate(cases.items()):
        arr = ellipsoids_with_holes(shape, n, seed)
        ball = arr.ndim == 3
        rec = {'shape': list(shape), 'labels': int(len(np.unique(arr)) - 1), 'foreground_fraction': round(float((arr != 0).mean()), 4)}
        for radius in (1, 7):
            rec[f'close_r{radius}'], _ = device_case(
                arr, args.reps, lambda t, eb: L._morph_device(t, eb, tuple(arr.shape), 'Close', radius, ball, None, t.device, events=True))
            for hole_size in (64, 10 ** 6):
                dev, got = device_case(
                    arr, args.reps, lambda t, eb: L._fill_device(t, eb, tuple(arr.shape), radius, hole_size, ball, None, t.device, events=True))
                want, dt, timed, total = scipy_loop(arr, radius, hole_size, args.host_turns)
                dev.update({'scipy_s': round(dt / max(timed, 1) * total, 4), 'scipy_turns_timed': timed})
                if timed == total:
                    dev['equal_to_scipy'] = bool(np.array_equal(got, want))
                dev['voxels_changed'] = int((got != arr).sum())
                dev['scipy_over_call'] = round(dev['scipy_s'] * 1e3 / max(dev['call_ms']['median'], 1e-6), 1)
                rec[f'r{radius}_h{hole_size}'] = dev
        out['cases'][name] = rec
    line = json.dumps(out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)
