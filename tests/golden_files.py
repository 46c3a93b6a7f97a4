"""Golden vectors stored in parts, each file under 1 MiB: ``tests/golden/<name>.<part>.npz``, read back as one mapping."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load(name, golden_dir=GOLDEN):
    """-> {array name: array} over every part of ``name``"""
    parts = sorted(glob.glob(os.path.join(golden_dir, f'{name}.*.npz')))
    if not parts:
        raise FileNotFoundError(f'no part of the golden {name!r} under {golden_dir}')
    out = {}
    for p in parts:
        with np.load(p) as z:
            out.update({k: z[k] for k in z.files})
    return out
