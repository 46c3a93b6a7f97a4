"""The forward fence: every schedule branch of csrc/pdl_net.hip / pdl_net32.hip pinned to the bits it produced when
tests/forward_fence.json was recorded -- the three heads, ``last_flops()``, the EMP_LAYER_LOG text of the forward (fp16
engine) and, at the small sizes, every tap the engine serves.  No tolerance anywhere: hashes and exact values.  Besides the single
forwards at render_steps 2: render_steps 1 and 3, and four forwards on ONE model (a smaller batch, the full batch again, another size),
which pin the heads and ``last_flops()`` of every step.

A refactor of the scheduler (named arguments, shared dispatch helpers, moved files) must leave every case equal in every
field.  ``python tests/test_gpu_forward_fence.py --record`` rewrites tests/forward_fence.json; the file is re-recorded ONLY
by a change that means to alter numerics or launches (a new kernel, another fusion rule, another summation order), from
two recordings in two fresh processes that agree, and its header names the commit and the compiler it was recorded with.
``--record --add`` records only the cases the file does not hold yet and lists them, with their commit, under "added": what a
refactor does FIRST, at its parent commit, for the paths it is about to move."""
import hashlib
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

FENCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'forward_fence.json')

# every switch emp_pdl reads when a network is created: a case sets its own and clears the rest
FP16_SWITCHES = ('EMP_FUSE_SEPCONV', 'EMP_FUSE_STEM', 'EMP_FUSE_DS', 'EMP_FUSE_B2B', 'EMP_FUSE_PROJ', 'EMP_FUSE_ASPP', 'EMP_FUSE_PR',
                 'EMP_CONV256_PACK', 'EMP_PRECISE_WSPLIT', 'EMP_PRECISE_FSPLIT', 'EMP_REGNET_GROUPED')
X3_SWITCHES = ('EMP_X3_FUSE_DS', 'EMP_X3_FUSE_HEAD', 'EMP_X3_FUSE_SEP', 'EMP_X3_FUSE_STEM', 'EMP_X3_MERGE_PROJ', 'EMP_X3_MERGE_ASPP',
               'EMP_X3_KSPLIT', 'EMP_X3_SMALL_ASPP', 'EMP_X3_PLANES')
OTHER = ('EMP_PRECISE_SEPCONV', 'EMP_SEPCONV_MIN_TILES', 'EMP_X3_PLANES_MIN_TILES', 'EMP_X3_SEP_MIN_TILES', 'EMP_REGNET_GROUP_TILES',
         'EMP_PAR_DECODERS', 'EMP_PRECISION', 'EMP_LAYER_LOG')
FP16_OFF = dict({k: '0' for k in FP16_SWITCHES}, EMP_PRECISE_SEPCONV='0')
X3_OFF = {k: '0' for k in X3_SWITCHES}
PLANES1 = {'EMP_X3_PLANES_MIN_TILES': '1'}


def _case(net, precision, batch, size, env=None, interp=False, ncls=None, steps=2, cfg=None):
    """cfg: changes to the network's configuration (the seeded parameters follow it)"""
    return dict(net=net, precision=precision, batch=batch, size=size, env=env or {}, interp=interp, ncls=ncls, steps=steps, cfg=cfg or {})


SINGLE = {'ins_decoder': False}
STAGES321 = {'low_level_stages': [3, 2, 1], 'low_level_channels_project': [128, 64, 32], 'stage4_stride': 32}

# one model, four forwards: a smaller batch in the planned layout, the full batch again, then another size (a re-plan)
SEQ = ((2, 256), (1, 256), (2, 256), (1, 384))


def _seq(net, precision):
    return dict(net=net, precision=precision, seq=SEQ, env={}, ncls=None)


CASES = {
    # ---- fp16 engine ----
    'fp16-pdl-b2-256': _case('pdl', 'fp16', 2, 256),                       # two streams, precise fuse blocks and centre head
    'fp16-pdl-b2-256-interp': _case('pdl', 'fp16', 2, 256, interp=True),
    'fp16-pdl-b1-1024': _case('pdl', 'fp16', 1, 1024),                     # back-to-back conv1 fusion active
    'fp16-pdl-b8-1024': _case('pdl', 'fp16', 8, 1024),                     # merged ASPP branches (192 tiles), one stream
    'fp16-mini-b2-256': _case('mini', 'fp16', 2, 256),                     # unfused semantic nodes, precise hi + lo instance nodes
    'fp16-mini4-b4-1024': _case('mini', 'fp16', 4, 1024, ncls=4),          # nodes at 512 tiles: the sepconv5 node path
    'fp16-regnetx-b2-256': _case('regnetx', 'fp16', 2, 256),               # the grouped launch
    'fp16-regnety-b2-256': _case('regnety', 'fp16', 2, 256),
    'fp16-regnetx-b4-1024': _case('regnetx', 'fp16', 4, 1024),             # stage 1 at 2048 tiles: per-group launches
    'fp16-pdl-b2-256-alloff': _case('pdl', 'fp16', 2, 256, FP16_OFF),
    'fp16-mini-b2-256-alloff': _case('mini', 'fp16', 2, 256, FP16_OFF),
    'fp16-pdl-b2-256-precise2': _case('pdl', 'fp16', 2, 256, {'EMP_PRECISE_SEPCONV': '2'}),
    'fp16-mini-b2-256-precise2': _case('mini', 'fp16', 2, 256, {'EMP_PRECISE_SEPCONV': '2'}),
    # ---- fp16x3 (the default) and fp32 ----
    'x3-pdl-b1-384': _case('pdl', 'fp16x3', 1, 384),                       # K-split small ASPP, merged projections, fused blocks
    'x3-pdl-b2-384-planes': _case('pdl', 'fp16x3', 2, 384, PLANES1),       # the plane region and the merged ASPP
    'x3-mini4-b1-384-planes': _case('mini', 'fp16x3', 1, 384, PLANES1, ncls=4),   # fp32 copies of P4 / P5
    'x3-pdl-b1-384-alloff': _case('pdl', 'fp16x3', 1, 384, X3_OFF),
    'x3-pdl-b1-384-nofusesep': _case('pdl', 'fp16x3', 1, 384, {'EMP_X3_FUSE_SEP': '0'}),   # the head in the pointwise conv's epilogue
    'fp32-pdl-b2-256': _case('pdl', 'fp32', 2, 256),
    'fp32-mini-b2-256': _case('mini', 'fp32', 2, 256),
    'fp32-regnety-b2-256': _case('regnety', 'fp32', 2, 256),               # squeeze-excite
    'x3-regnety-b2-256': _case('regnety', 'fp16x3', 2, 256),
    # ---- other render steps: the pr.sem<k> buffers and the sizes that depend on render_steps ----
    'fp16-pdl-b2-256-rs1': _case('pdl', 'fp16', 2, 256, steps=1),
    'fp16-pdl-b2-256-rs3': _case('pdl', 'fp16', 2, 256, steps=3),
    'x3-pdl-b1-384-rs3': _case('pdl', 'fp16x3', 1, 384, steps=3),
    # ---- re-batch and re-plan on one model (heads and last_flops() per step) ----
    'fp16-pdl-seq': _seq('pdl', 'fp16'),                                   # rebatch() and the re-plan path
    'x3-regnety-seq': _seq('regnety', 'fp16x3'),                           # buffer reuse, row tails cleared for a new geometry
    'fp32-regnety-seq': _seq('regnety', 'fp32'),
    # ---- one decoder, and more than one fuse stage (change detectors; the evidence is tests/test_gpu_net_configs.py) ----
    'fp16-pdl-single-b2-256': _case('pdl', 'fp16', 2, 256, ncls=2, cfg=SINGLE),          # semantic_decoder. is the precise site, one stream
    'fp16-mini-single-b2-256': _case('mini', 'fp16', 2, 256, ncls=3, cfg=SINGLE),        # precise hi + lo semantic nodes, the .pw head
    'x3-pdl-single-b1-384': _case('pdl', 'fp16x3', 1, 384, ncls=2, cfg=SINGLE),          # no merged projection, no merged ASPP
    'fp32-pdl-single-b2-256': _case('pdl', 'fp32', 2, 256, ncls=2, cfg=SINGLE),
    'fp16-pdl-stages321-b2-256': _case('pdl', 'fp16', 2, 256, cfg=STAGES321),            # three stages, layer4 at stride 2
}

HEADS = ('sem_logits', 'ctr_hmp', 'offsets')
_WEIGHTS = {}


def _weights(net, ncls, change=None):
    """(cfg, folded parameters) of a case's network, built once per process"""
    change = change or {}
    key = (net, ncls, repr(sorted(change.items())))
    if key not in _WEIGHTS:
        from empanada_napari_amd import weights
        if net in ('regnetx', 'regnety'):
            from test_regnet import regnet_model
            _WEIGHTS[key] = regnet_model(net[-1])
        else:
            cfg = dict(weights.MITONET_PDL_CFG if net == 'pdl' else weights.MITONET_MINI_CFG)
            if ncls is not None:
                cfg['num_classes'] = ncls
            cfg.update(change)
            _WEIGHTS[key] = cfg, weights.fold_state_dict(weights.seeded_state_dict(cfg, seed=0 if net == 'pdl' else 3), cfg)
    return _WEIGHTS[key]


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _input(batch, size):
    import torch
    from empanada_napari_amd import synth
    from empanada_napari_amd.preprocess import normalize
    return torch.from_numpy(normalize(synth.em_tiles(batch, size, seed=5), 0.57571, 0.12765))[:, None].cuda()


def run_seq(c):
    """The forwards of a sequence case on ONE model -> the heads and last_flops() of every step."""
    import torch
    from empanada_napari_amd.engines import HipPanopticDeepLab
    cfg, P = _weights(c['net'], c['ncls'])
    model = HipPanopticDeepLab(P, cfg, folded=True, precision=c['precision'])
    assert model.precision == c['precision']
    steps = []
    for batch, size in c['seq']:
        out = model(_input(batch, size), 2, False)
        torch.cuda.synchronize()
        steps.append(dict({k: _sha(out[k]) for k in HEADS}, flops=repr(model.last_flops())))
    del model
    return {'steps': steps}


def run_case(name, setenv, delenv, tmpdir):
    """The forward(s) of case ``name`` -> the record the fence file holds for it."""
    import torch
    from empanada_napari_amd.engines import HipPanopticDeepLab
    c = CASES[name]
    for k in FP16_SWITCHES + X3_SWITCHES + OTHER:
        delenv(k, raising=False)
    for k, v in c['env'].items():
        setenv(k, v)
    if 'seq' in c:
        return run_seq(c)
    cfg, P = _weights(c['net'], c['ncls'], c.get('cfg'))
    log = os.path.join(str(tmpdir), name + '.layers.log')
    fp16 = c['precision'] == 'fp16'
    if fp16:
        setenv('EMP_LAYER_LOG', log)
    model = HipPanopticDeepLab(P, cfg, folded=True, precision=c['precision'])      # the switches are read here
    delenv('EMP_LAYER_LOG', raising=False)
    assert model.precision == c['precision']
    out = model(_input(c['batch'], c['size']), c['steps'], c['interp'])
    torch.cuda.synchronize()
    rec = {k: _sha(out[k]) for k in HEADS}
    rec['flops'] = repr(model.last_flops())
    if fp16:
        with open(log, 'rb') as f:
            rec['layer_log'] = hashlib.sha256(f.read()).hexdigest()
    if c['size'] <= 384:
        names = model.tap_names()
        rec['tap_names'] = names
        rec['taps'] = {t: _sha(model.tap(t)) for t in names}
    del model
    return rec


def _fence():
    with open(FENCE) as f:
        return json.load(f)


@pytest.mark.parametrize('name', list(CASES))
def test_forward_equals_the_recorded_fence(name, monkeypatch, tmp_path):
    want = _fence()['cases']
    assert name in want, f'{name}: not in the fence file (a case is left out only if its two recordings differed)'
    got = run_case(name, monkeypatch.setenv, monkeypatch.delenv, tmp_path)
    for field in sorted(set(got) | set(want[name])):
        if field == 'taps':
            diff = [t for t in got['tap_names'] if got['taps'].get(t) != want[name]['taps'].get(t)]
            assert not diff, f'{name}: taps differ from the fence, first {diff[:5]} of {len(diff)}'
        else:
            assert got.get(field) == want[name].get(field), f'{name}: {field} differs from the fence'
    if name == 'fp16-pdl-seq':      # the full batch in a fresh plan and again after a smaller one: the single-forward case's bits
        single = {k: want['fp16-pdl-b2-256'][k] for k in HEADS + ('flops',)}
        assert got['steps'][0] == single and got['steps'][2] == single, f'{name}: a batch-2 step differs from fp16-pdl-b2-256'


def _record(out_path, parent, add=False):
    import subprocess
    import tempfile
    import conftest  # noqa: F401  (imports the package the way the suite does)

    def setenv(k, v):
        os.environ[k] = v

    def delenv(k, raising=False):
        os.environ.pop(k, None)

    hipcc = [line for line in subprocess.run(['hipcc', '--version'], capture_output=True, text=True).stdout.splitlines()
             if 'HIP version' in line or 'clang version' in line]
    doc = {'parent_commit': parent, 'hipcc_version': ' | '.join(hipcc), 'cases': {}}
    if add:      # cases added later: the entries the file holds stay as they are, the new ones are listed with their commit
        doc = _fence()
        new = [name for name in CASES if name not in doc['cases']]
        doc.setdefault('added', []).append({'parent_commit': parent, 'hipcc_version': ' | '.join(hipcc), 'cases': new})
    with tempfile.TemporaryDirectory() as tmp:
        for name in CASES:
            if name in doc['cases']:
                continue
            doc['cases'][name] = run_case(name, setenv, delenv, tmp)
            print('recorded', name, [r['flops'] for r in doc['cases'][name].get('steps', [doc['cases'][name]])], flush=True)
            with open(out_path, 'w') as f:      # (kept current: a recording that stops half-way leaves what it has)
                json.dump(doc, f, indent=1, sort_keys=True)
                f.write('\n')


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--record', action='store_true')
    ap.add_argument('--add', action='store_true', help='record only the cases the fence file does not hold yet')
    ap.add_argument('--out', default=FENCE)
    ap.add_argument('--parent', default='unknown', help='hash of the commit whose sources the library was built from')
    a = ap.parse_args()
    if not a.record:
        sys.exit('run under pytest, or with --record')
    _record(a.out, a.parent, a.add)
