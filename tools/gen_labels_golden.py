"""Record the reference's count_labels on a handful of label lists: tests/golden/labels.npz (tests/test_labels_host.py).

    python tools/gen_labels_golden.py /path/to/empanada-napari [out.npz]      # CPU only, seconds

The reference checkout is imported, not copied: ``count_labels`` of empanada_napari/_label_counter_widget.py (:105-118), loaded by
file so that the plugin's package import stays out of the way.  napari, magicgui, napari_plugin_engine, openpyxl and dask (and
pandas where it is missing) are replaced by empty shims: count_labels itself is pure numpy.  Per case the file holds the input
(``values``, ``divisor``) and the output: ``class_ids`` and the lists of the returned dict in key order, back to back
(``lists``) with their boundaries (``offsets``) and keys (``keys``).  Fixed zip timestamps: the same reference gives the same bytes.
"""
import importlib
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shims():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules.setdefault(name, m)
        return sys.modules[name]
    module('napari_plugin_engine', napari_hook_implementation=lambda *a, **k: (lambda f: f))
    module('magicgui', magicgui=lambda *a, **k: (lambda f: f))
    nap = module('napari', Viewer=object)
    nap.layers = module('napari.layers', Labels=object)
    nap.viewer = module('napari.viewer', Viewer=object)
    module('openpyxl', Workbook=object)
    dask = module('dask')
    dask.array = module('dask.array', Array=type('Array', (), {}))
    try:
        importlib.import_module('pandas')
    except ImportError:
        module('pandas')


def cases():
    """name -> (label values as the widget passes them: np.unique(labels)[1:], label divisor)"""
    rng = np.random.default_rng(0)
    three = np.unique(np.concatenate([rng.integers(1, 1000, 40), 1000 + rng.integers(0, 1000, 25), 5000 + rng.integers(1, 999, 7)]))
    return {
        'divisor_0': (three, 0),
        'divisor_1000': (three, 1000),
        'divisor_10000': (np.unique(np.concatenate([three, 10000 + three, [29999, 30000, 30001]])), 10000),
        'one_class': (np.arange(1001, 1020, dtype=np.int64), 1000),
        'class_0_only': (np.array([3, 4, 9], dtype=np.int64), 1000),
        'empty': (np.zeros(0, dtype=np.int64), 1000),
        'empty_divisor_0': (np.zeros(0, dtype=np.int64), 0),
        'uint16_values': (np.array([1, 999, 1000, 1999, 2000], dtype=np.uint16), 1000),
    }


def main(ref_root, out_path):
    _shims()
    spec = importlib.util.spec_from_file_location('_ref_label_counter', os.path.join(ref_root, 'empanada_napari', '_label_counter_widget.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    arrays, names = {}, []
    for name, (values, divisor) in cases().items():
        names.append(name)
        queue, class_ids = tool.count_labels(values, divisor)
        keys = list(queue)
        arrays[f'{name}/values'] = values
        arrays[f'{name}/divisor'] = np.int64(divisor)
        arrays[f'{name}/class_ids'] = np.asarray(class_ids, dtype=np.int64)
        arrays[f'{name}/keys'] = np.asarray(keys, dtype=np.int64)
        arrays[f'{name}/lists'] = np.asarray([v for k in keys for v in queue[k]], dtype=np.int64)
        arrays[f'{name}/offsets'] = np.cumsum([0] + [len(queue[k]) for k in keys]).astype(np.int64)
        print(name, {k: len(queue[k]) for k in keys}, class_ids, flush=True)
    arrays['names'] = np.array(names)
    with zipfile.ZipFile(out_path, 'w', zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(out_path, os.path.getsize(out_path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]), sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden', 'labels.npz'))
