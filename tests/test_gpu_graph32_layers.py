"""The fp32 and fp16x3 forwards map by map, teacher-forced (csrc/pdl_net32.hip run32).

Every kernel run32 launches has its own element-by-element test; what run32 MAKES of them -- which map feeds which launch, at
which channel offset, in which format, with which per-image bias -- was seen at the three heads only, through a gate that leaves a
factor of 40 of room.  Here one fresh model per (network, precision, schedule) runs one forward; ``HipPanopticDeepLab.maps32()``
lists every buffer that forward made; oracle.pdl_model.Graph32Walk recomputes each of them in float64 from the engine's own input
buffers with the operands finalize32 packs, and tests/graph32_case.py bounds the difference per element with the bounds of the
kernel that made it (none taken from a kernel's output; accepted: min(worst, 6 rss), x3_range_case.RSS_GPU).  No buffer of the
forward may go unchecked but the selection's work buffers (graph32_case.ALLOW: checked as a selection), no element of a checked
buffer is exempt, every zero pad must be zero.

Sizes: the smallest at which the sites can go wrong -- non-square (H / W swaps), p5 of 8 x 10 against the largest atrous rate 6
at stride 16 (128 x 160, batch 2: a per-image bias of the wrong image shows); the plane region needs N (H/16) (W/16) / 256 >= 1
with EMP_X3_PLANES_MIN_TILES=1: batch 2 of 128 x 256.  The largest ratios per (network, schedule, map family) go to
graph32_layers.json beside the suite's other reports (REPORT; committed as profiles/graph32_layers.json).

What the end of a forward no longer holds cannot be forced on the engine's own inputs and is forced through its producer
instead: RegNetY's gate overwrites the map it gates (graph32_case 'conv_prop' / 'conv_gated'); PointRend's row buffers are
overwritten layer by layer and step by step, so of the point head the last fc layer, the predictor, the coarse columns and the
selection of the LAST step are forced (render_steps 1 makes step 0 that step), and every cell of an inner step's ``pr.sem<k>``
is the plain up-sampling or, at no more than k cells, the point head's logits of that cell within the bound composed over
all its layers."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph32_case as G  # noqa: E402
import x3_range_case as X3  # noqa: E402
from test_gpu_forward_fence import FP16_SWITCHES, OTHER, X3_OFF, X3_SWITCHES, _weights  # noqa: E402
from test_gpu_net_configs import MEAN, NETS, STD, Nets  # noqa: E402
from test_gpu_parity_fullsize import REPORT as _PARITY_REPORT  # noqa: E402

pytestmark = pytest.mark.gpu

REPORT = os.path.join(os.path.dirname(_PARITY_REPORT), 'graph32_layers.json')      # where the suite's other reports go
PLANES1 = {'EMP_X3_PLANES_MIN_TILES': '1'}
NO_REGION_NO_SMALL = {'EMP_X3_PLANES_MIN_TILES': '100000', 'EMP_X3_SMALL_ASPP': '0'}
SMALL, WIDE, ONE = (2, 128, 160), (2, 128, 256), (1, 128, 256)      # (BiFPN networks need multiples of 128)


def _case(tag, precision, sched='default', env=None, shape=SMALL, steps=2, interp=False, raw=False):
    return dict(tag=tag, precision=precision, sched=sched, env=env or {}, shape=shape, steps=steps, interp=interp, raw=raw)


DEEPLABS = ['pdl', 'pdl_single', 'pdl_stages321', 'pdl_odd', 'pdl_single_s16x3']
OTHERS = ['mini', 'mini4', 'bifpn_single', 'bifpn_l2', 'regnetx', 'regnety']
CASES = [_case(t, p) for t in DEEPLABS for p in ('fp32', 'fp16x3')] + [_case(t, p, shape=ONE) for t in OTHERS for p in ('fp32', 'fp16x3')] + [
    _case('mini4', 'fp16x3', 'planes', PLANES1, (4, 128, 256)),      # stride 32: twice the tiles; the fp32 copies of P4 / P5
    _case('bifpn_single', 'fp16x3', 'planes', PLANES1, (4, 128, 256)),
    _case('mini4', 'fp16x3', 'alloff', X3_OFF, ONE),
    _case('bifpn_single', 'fp16x3', 'alloff', X3_OFF, ONE),
    _case('mini', 'fp16x3', 'interp', shape=ONE, interp=True),
    _case('pdl', 'fp16x3', 'planes', PLANES1, WIDE),
    _case('pdl_stages321', 'fp16x3', 'planes', PLANES1, WIDE),      # a low-level skip from layer3: the region never opens (x3_planes_complete)
    _case('pdl', 'fp16x3', 'alloff', X3_OFF, WIDE),
    _case('pdl_stages321', 'fp16x3', 'alloff', X3_OFF, WIDE),
    _case('pdl', 'fp16x3', 'noregion_nosmall', NO_REGION_NO_SMALL),
    _case('pdl', 'fp16x3', 'nofusesep', {'EMP_X3_FUSE_SEP': '0'}),      # the heads through .part + head_finish
    _case('pdl', 'fp16x3', 'steps3', steps=3),
    # render_steps 1: step 0 is the LAST step, so its selection, rows, fc chain and predictor are forced on the engine's own
    # buffers at every cell (5120 cells against 8192 points: all of them are refined) -- what an inner step cannot show
    _case('pdl', 'fp16x3', 'steps1', steps=1),
    _case('pdl', 'fp32', 'steps1', steps=1),
    _case('pdl_odd', 'fp16x3', 'steps1', steps=1),      # two fc layers, three classes
    _case('mini4', 'fp16x3', 'steps1', shape=ONE, steps=1),
    _case('regnetx', 'fp16x3', 'steps1', shape=ONE, steps=1),
    _case('regnetx', 'fp16x3', 'interp', shape=ONE, interp=True),
    _case('pdl', 'fp32', 'interp', interp=True),
    _case('pdl', 'fp16x3', 'interp', interp=True),
    _case('pdl', 'fp16x3', 'raw_u8', raw=True),
    _case('pdl', 'fp32', 'raw_u8', raw=True),
]
IDS = [f"{c['tag']}-{c['precision']}-{c['sched']}" for c in CASES]


@pytest.fixture(scope='module')
def nets(tmp_path_factory):
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    return Nets(tmp_path_factory.mktemp('graph32'))


def _network(nets, tag):
    """(cfg, folded parameters): 'pdl' as tests/test_gpu_forward_fence.py builds it, the others as tests/test_gpu_net_configs.py does"""
    if tag in ('pdl', 'mini', 'regnetx', 'regnety'):
        return _weights(tag, None)
    if tag == 'mini4':
        return _weights('mini', 4)
    assert tag in NETS
    c = nets.case(tag)
    return c['cfg'], c['P']


_INPUTS = {}


def _input(shape, raw):
    """-> (the tensor the model is called with, pad_to, sub, mul, the walk's image: normalised float64 (N, vh, vw) + padded size)"""
    key = (shape, raw)
    if key not in _INPUTS:
        from empanada_napari_amd import synth
        from empanada_napari_amd.preprocess import normalize
        N, H, W = shape
        img = synth.em_tiles(N, max(H, W), seed=17)[:, :H, :W]
        if raw:      # a ragged valid area inside the padded one: the stem pads AFTER normalising
            img = np.ascontiguousarray(img[:, :H - 9, :W - 13])
            sub, mul = np.float32(MEAN * 255), np.float32(1.0 / (STD * 255))
            x = (torch.from_numpy(img).double() - float(sub)) * float(mul)
            _INPUTS[key] = (torch.from_numpy(img)[:, None], (H, W), float(sub), float(mul), G.image_of(x, H, W))
        else:
            x = torch.from_numpy(normalize(img, MEAN, STD))
            _INPUTS[key] = (x[:, None], None, 0.0, 1.0, G.image_of(x, H, W))
    return _INPUTS[key]


def _report(key, val):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    d = {}
    if os.path.exists(REPORT):
        try:
            d = json.load(open(REPORT))
        except Exception:
            d = {}
    d[key] = val
    json.dump(d, open(REPORT, 'w'), indent=1, sort_keys=True)


def _region_expected(cfg, c):
    """run32's rule for the plane region, restated: fp16x3, every low-level skip below layer3, and enough pixel tiles"""
    N, H, W = c['shape']
    bifpn = 'BiFPN' in cfg.get('arch', '')
    if c['precision'] != 'fp16x3' or c['env'].get('EMP_X3_PLANES') == '0' or str(cfg.get('encoder', 'resnet50')) != 'resnet50':
        return False
    if not bifpn and max(cfg['low_level_stages']) > 2:
        return False
    tiles = N * (H // 16) * (W // 16) // 256
    return tiles >= int(c['env'].get('EMP_X3_PLANES_MIN_TILES', 128)) * (2 if bifpn or cfg['stage4_stride'] == 32 else 1)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_every_map_of_the_forward_teacher_forced(nets, monkeypatch, c):
    from empanada_napari_amd.engines import HipPanopticDeepLab
    for k in FP16_SWITCHES + X3_SWITCHES + OTHER:
        monkeypatch.delenv(k, raising=False)
    for k, v in c['env'].items():
        monkeypatch.setenv(k, v)      # read when the model is created
    cfg, P = _network(nets, c['tag'])
    model = HipPanopticDeepLab(P, cfg, folded=True, precision=c['precision'])      # fresh: buffers persist by name
    assert model.precision == c['precision']
    xin, pad_to, sub, mul, image = _input(c['shape'], c['raw'])
    out = model(xin.cuda(), c['steps'], c['interp'], sub=sub, mul=mul, pad_to=pad_to)
    torch.cuda.synchronize()
    maps = model.maps32()
    cache = {k: v.double().cpu() for k, v in out.items()}

    def get(name):
        if name not in cache:
            cache[name] = model.map32(maps[name])
        return cache[name]

    rows, seen, faults = G.run_walk(P, cfg, image, lambda n: n in maps, lambda n: maps[n]['fmt'], get, c['precision'], c['steps'],
                                    c['interp'], X3.RSS_GPU)
    # the largest ratios per map family, reported before anything is asserted
    fam = {}
    for r in rows:
        f = fam.setdefault(r['family'], dict(worst=0.0, rss=0.0, checks=0, elements=0))
        f['worst'], f['rss'] = max(f['worst'], r['worst']), max(f['rss'], r['rss'] or 0.0)
        f['checks'], f['elements'] = f['checks'] + 1, f['elements'] + r['n']
    print(f"{c['tag']} [{c['precision']}, {c['sched']}]: {len(maps)} buffers, {len(rows)} checks;",
          {k: (round(v['worst'], 3), round(v['rss'], 3)) for k, v in fam.items()}, '(accepted: 1 of worst and', X3.RSS_GPU, 'of rss)')
    _report('-'.join((c['tag'], c['precision'], c['sched'])), dict(buffers=len(maps), checks=len(rows), shape=list(c['shape']), families=fam))
    assert not faults, faults
    bad = [r for r in rows if r['viol']]
    assert not bad, bad[:5]
    # no map escapes
    unchecked = set(maps) - seen - set(G.ALLOW)
    assert not unchecked, sorted(unchecked)
    assert set(G.OUTPUTS) <= seen | ({'ctr_hmp', 'offsets'} if not c['interp'] else set())
    # every row tail is zero
    for name, rec in maps.items():
        if rec['kind'] == 'map' and rec['ld'] > rec['C']:
            _, tail, _ = model.map32(rec, parts=True)
            assert not bool(tail.any()), f'{name}: the row tail [{rec["C"]}, {rec["ld"]}) is not zero'
    # the formats: hl32 inside the plane region, fp32 everywhere else
    region = _region_expected(cfg, c)
    hl = sorted(n for n, r in maps.items() if r['fmt'])
    if region:
        inside = ['encoder.layer3.0', 'encoder.layer3.5', 'encoder.layer4.0', 'encoder.layer4.2']
        for n in inside + (['semantic_decoder.aspp.cat'] if 'semantic_decoder.aspp.cat' in maps else ['encoder.layer3.5.f32', 'encoder.layer4.2.f32']):
            assert n in maps and maps[n]['fmt'] == (0 if n.endswith('.f32') else 1), f'{n}: wrong format inside the plane region'
        hi, lo = model.map32(maps['encoder.layer4.2'], parts=True)[2]
        assert float(lo.abs().max()) > 0 and bool((lo.abs().double() <= 2.0 ** -10 * hi.abs().double() + 2.0 ** -24).all()), 'layer4.2: not hi / lo pairs'
    else:
        assert hl in ([], ['p5.hl32']), hl
