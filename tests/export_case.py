"""TorchScript exports laid out like the reference's fused models, rebuilt without the reference's code (tests/test_load_export.py).

``tests/golden/export_<case>.npz`` (oracle/gen_golden.py ``exports``) records, per export of the reference: the parameter
and buffer names, shapes and dtypes of its fused ``state_dict()`` and which names share one tensor (the BiFPN reuses one
node block across its nodes); the scalar attributes of its scripted submodules that a loader can read (conv ``stride`` /
``dilation``, PointRend's ``subdivision_num_points``); an input and the scripted model's outputs on it.  The values of the
parameters are never stored: ``fused_values`` draws them from a seed, the generator loads them into the reference's model
before it runs it, and ``build_export`` writes a TorchScript file with the same module tree, names and attributes holding
the same values."""
import ast
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ATTRS = ('stride', 'dilation', 'subdivision_num_points')
OUTPUTS = ('sem_logits', 'ctr_hmp', 'offsets')


def ties(state_dict):
    """per name, the index of the first name holding the same tensor (its own index when the tensor is its own)"""
    first = {}
    return [first.setdefault(v.data_ptr(), i) for i, v in enumerate(state_dict.values())]


def fused_values(keys, shapes, dtypes, seed, tie=None):
    """name -> tensor: weights of variance 1 / fan-in (fan-in over every axis but the first: activations stay O(1) through
    the residual trunks), BatchNorm scales, variances and BiFPN fusion weights near 1, small biases and means, zero
    counters; one numpy RandomState over the names in the order given.  A name tied to an earlier one (``tie``, as the
    export's state dict has them) holds that one's value."""
    rng = np.random.RandomState(seed)
    out = {}
    for k, shp, dt in zip(keys, shapes, dtypes):
        shp = tuple(int(d) for d in shp)
        if np.dtype(dt).kind in 'iub':
            v = np.zeros(shp)
        elif k.endswith('running_var'):
            v = rng.uniform(0.5, 1.5, shp)
        elif len(shp) >= 2:
            v = rng.standard_normal(shp) * np.sqrt(1.0 / max(1, int(np.prod(shp[1:]))))
        elif k.endswith(('weight', 'weights')):
            v = rng.uniform(0.5, 1.5, shp)
        else:
            v = rng.standard_normal(shp) * 0.1
        out[k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.dtype(dt)))
    for i, j in enumerate(tie if tie is not None else []):
        if j != i:
            out[keys[i]] = out[keys[j]]
    return out


class _Node(torch.nn.Module):
    pass


class _Export(torch.nn.Module):
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x


def build_export(values, attrs, path):
    """values: name -> tensor; attrs: (module path, attribute, value).  Writes the TorchScript file and returns its path."""
    top = _Export()

    def node(p):
        mod = top
        for part in (p.split('.') if p else []):
            child = dict(mod.named_children()).get(part)
            if child is None:
                child = _Node()
                mod.add_module(part, child)
            mod = child
        return mod

    for k, v in values.items():
        p, _, name = k.rpartition('.')
        node(p).register_buffer(name, v)
    for p, name, v in attrs:
        setattr(node(p), name, v)
    torch.jit.save(torch.jit.script(top), path)
    return path


def record(scripted, x, seed):
    """The fixture of a scripted reference model whose parameters are ``fused_values(..., seed)``: what ``load`` returns."""
    sd = scripted.state_dict()
    keys = list(sd.keys())
    attrs = []
    for p, mod in scripted.named_modules():
        for name in ATTRS:
            try:
                v = getattr(mod, name)
            except AttributeError:
                continue
            if isinstance(v, int) or (isinstance(v, tuple) and all(isinstance(e, int) for e in v)):
                attrs.append((p, name, repr(v)))
    with torch.no_grad():
        want = scripted(x, 2, False)
    out = {'keys': np.array(keys), 'shapes': np.array([','.join(str(d) for d in sd[k].shape) for k in keys]),
           'dtypes': np.array([str(sd[k].numpy().dtype) for k in keys]), 'tie': np.array(ties(sd), np.int64),
           'seed': np.int64(seed), 'attr_paths': np.array([a[0] for a in attrs]),
           'attr_names': np.array([a[1] for a in attrs]), 'attr_values': np.array([a[2] for a in attrs]), 'x': x.numpy()}
    out.update({k: want[k].numpy() for k in OUTPUTS})
    return out


def load(case):
    """-> (values, attrs, x, want) of ``tests/golden/export_<case>.npz``."""
    z = np.load(os.path.join(GOLDEN, f'export_{case}.npz'))
    shapes = [tuple(int(d) for d in s.split(',') if d) for s in z['shapes']]
    values = fused_values([str(k) for k in z['keys']], shapes, [str(d) for d in z['dtypes']], int(z['seed']),
                          [int(i) for i in z['tie']])
    attrs = [(str(p), str(n), ast.literal_eval(str(v))) for p, n, v in zip(z['attr_paths'], z['attr_names'], z['attr_values'])]
    return values, attrs, torch.from_numpy(z['x']), {k: torch.from_numpy(z[k]) for k in OUTPUTS}
