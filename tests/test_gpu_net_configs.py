"""Single-decoder and non-default networks on the device.

``emp_pdl_create`` accepts a family of networks; until this file the GPU suite built four of them (MITONET_PDL_CFG,
MITONET_MINI_CFG with 1 and 4 classes, the two 6.4GF RegNets), all with two decoders and default widths.  Here the
scheduler (csrc/pdl_net.hip, csrc/pdl_net32.hip) runs the others, at the smallest sizes its planners accept:

  pdl_single        MITONET_PDL_CFG without an instance decoder, 2 classes (what the training widget exports for a model
                    without thing classes): the single-decoder walks, ``semantic_decoder.`` as the precise site, no merged
                    launch, one stream; 64^2, batch 2                                  -- tests/golden/export_pdl_single.npz
  bifpn_single      MITONET_MINI_CFG without an instance FPN, 3 classes (the ``.pw`` route of the semantic head; the
                    ``semantic_fpn.`` nodes are the precise hi + lo nodes); 128^2        -- export_bifpn_single.npz
  pdl_stages321     the reference class's constructor defaults: stages [3, 2, 1], layer4 at stride 2; 64^2
                                                                                       -- export_pdl_stages321.npz
  pdl_odd           3 classes, 128 decoder / 192 ASPP channels, stages [2, 1], rates [3, 6, 9], num_fc 2; 64^2
                                                                                       -- export_pdl_odd.npz
  bifpn_l2          two BiFPN layers, 4 classes, 2048 points; 128^2                     -- export_bifpn.npz
  pdl_single_s16x3  pdl_single with stages [3, 1] at stride 16 (layer3 and layer4 at one resolution: the first
                    up-sampling is a copy); 64^2                                        -- oracle only
  regnetx_single    regnetx_6p4gf Panoptic-DeepLab without an instance decoder; 128^2, default precision only
                                                                                       -- oracle only

The export-backed networks take parameters, configuration, input and expected output from the fixture exactly as
tests/test_load_export.py does (``export_case.load`` + ``inference.load_model_spec`` + ``weights.fold_state_dict``): the
host tests pin the oracle to the reference's scripted model on those, so the oracle stands in for the reference here.

Gates (none of them new): fp32 mode 1e-4 of the map's scale in the max norm (tests/test_gpu_regnet.py); fp16x3 the
contract's 1e-3 in the max norm; the fp16 engine layer by layer, teacher-forced, one fp16 ulp + 1e-4 of the scale
(gpu_common.teacher_forced_rows).  The worst figures go to net_configs.json, next to the report of
tests/test_gpu_parity_fullsize.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import export_case  # noqa: E402
from gpu_common import teacher_forced_rows  # noqa: E402
from test_gpu_forward_fence import FP16_OFF, FP16_SWITCHES, OTHER, X3_SWITCHES  # noqa: E402
from test_gpu_parity_fullsize import REPORT as _PARITY_REPORT  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-3                                   # BASELINE.json north_star, the default precision's contract (max norm)
GATE = {'fp32': 1e-4, 'fp16x3': TOL}         # per precision, relative to max(1, rms of the reference map)
HEADS = ('sem_logits', 'ctr_hmp', 'offsets')
REPORT = os.path.join(os.path.dirname(_PARITY_REPORT), 'net_configs.json')      # where the suite's other reports go
MEAN, STD = 0.57571, 0.12765

# tag -> the export fixture it is loaded from, or the configuration changes and the seed of its parameters
NETS = {
    'pdl_single': dict(export='pdl_single', size=64, batch=2),
    'bifpn_single': dict(export='bifpn_single', size=128),
    'pdl_stages321': dict(export='pdl_stages321', size=64),
    'pdl_odd': dict(export='pdl_odd', size=64),
    'bifpn_l2': dict(export='bifpn', size=128),
    'pdl_single_s16x3': dict(change=dict(ins_decoder=False, num_classes=2, low_level_stages=[3, 1], low_level_channels_project=[64, 32],
                                         stage4_stride=16), seed=41, size=64),
    'regnetx_single': dict(change=dict(encoder='regnetx_6p4gf', ins_decoder=False), seed=42, size=128),
}
RESNETS = [t for t in NETS if t != 'regnetx_single']
FORWARD = [(t, p) for t in RESNETS for p in ('fp32', 'fp16x3')] + [('regnetx_single', 'fp16x3')]
TEACHER_FORCED = ['pdl_single', 'pdl_single_s16x3', 'pdl_stages321', 'pdl_odd', 'bifpn_single', 'bifpn_l2']
SINGLE = ['pdl_single', 'bifpn_single']


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


def _prob(logits):
    """engines.py:22-30: sigmoid for one class, softmax over the classes otherwise"""
    return torch.sigmoid(logits) if logits.shape[1] == 1 else torch.softmax(logits, 1)


def _rel(got, ref):
    """max |got - ref| over max(1, rms(ref)): the measure of tests/test_gpu_regnet.py and the fp32 heads"""
    return float((got - ref).abs().max()) / max(1.0, float(ref.pow(2).mean().sqrt()))


def _is_bifpn(cfg):
    return 'BiFPN' in cfg.get('arch', '')


def _semx_name(cfg):
    return 'semantic_decoder.out' if _is_bifpn(cfg) else 'semantic_decoder.stage%d.out' % (len(cfg['low_level_stages']) - 1)


def _clear_switches(monkeypatch):
    for k in FP16_SWITCHES + X3_SWITCHES + OTHER:
        monkeypatch.delenv(k, raising=False)


def _param_names(model):
    return [model.lib.emp_pdl_param_name(model._h, i).decode() for i in range(model.lib.emp_pdl_num_params(model._h))]


def _synth_input(batch, size, seed):
    from empanada_napari_amd import synth
    from empanada_napari_amd.preprocess import normalize
    img = synth.em_tiles(batch, size, seed=seed)
    return img, torch.from_numpy(normalize(img, MEAN, STD))[:, None]


class Nets:
    """every network once: configuration, folded parameters, input, the fixture's expected output, the oracle's fp32
    forward with its taps (computed once, never changed), and one model per precision"""

    def __init__(self, tmpdir):
        self.tmpdir, self.cases, self.models = str(tmpdir), {}, {}

    def export(self, name):
        """-> (path of the rebuilt TorchScript export, state dict, cfg, input, the scripted reference model's outputs)"""
        from empanada_napari_amd import inference
        values, attrs, x, want = export_case.load(name)
        path = export_case.build_export(values, attrs, os.path.join(self.tmpdir, name + '.pth'))
        sd, cfg = inference.load_model_spec({'model': path})
        return path, sd, cfg, x, want

    def case(self, tag):
        if tag in self.cases:
            return self.cases[tag]
        from empanada_napari_amd import weights
        from oracle import pdl_model
        spec = NETS[tag]
        size = spec['size']
        if 'export' in spec:
            _, sd, cfg, x, want = self.export(spec['export'])
            assert tuple(x.shape) == (1, 1, size, size)
            if spec.get('batch', 1) > 1:      # the fixture's image first: image 0 of every output is still the fixture's
                x = torch.cat([x, torch.randn(spec['batch'] - 1, 1, size, size, generator=torch.Generator().manual_seed(7))])
        else:
            cfg = dict(weights.MITONET_PDL_CFG, **spec['change'])
            if weights.is_regnet(cfg):
                cfg['regnet'] = weights.regnet_cfg(cfg)
            sd, want = weights.seeded_state_dict(cfg, seed=spec['seed']), None
            x = torch.randn(1, 1, size, size, generator=torch.Generator().manual_seed(spec['seed']))
        P = weights.fold_state_dict(sd, cfg)
        taps = {}
        ref = pdl_model.model_forward(P, x, cfg, 2, False, taps)
        c = dict(tag=tag, cfg=cfg, P=P, x=x, want=want, ref=ref, sem_coarse=taps['sem_coarse'], size=size)
        self.cases[tag] = c
        return c

    def model(self, tag, precision):
        if (tag, precision) not in self.models:
            from empanada_napari_amd.engines import HipPanopticDeepLab
            c = self.case(tag)
            m = HipPanopticDeepLab(c['P'], c['cfg'], folded=True, precision=precision)
            assert m.precision == precision
            self.models[(tag, precision)] = m
        return self.models[(tag, precision)]

    def forward(self, tag, precision):
        """one forward of the case's input -> (model, heads on the host, coarse logits on the host)"""
        c, m = self.case(tag), self.model(tag, precision)
        out = {k: v.cpu() for k, v in m(c['x'].cuda(), 2, False).items()}
        torch.cuda.synchronize()
        q = c['size'] // 4
        coarse = m.tap_raw('semantic_head.out', (c['x'].shape[0], c['cfg']['num_classes'], q, q)).cpu()
        return m, out, coarse


@pytest.fixture(scope='module')
def nets(tmp_path_factory):
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    n = Nets(tmp_path_factory.mktemp('net_configs'))
    yield n
    n.models.clear()


# ---------------------------------------------------------------------------------------------------------------------
# 1 - 3: the heads, the coarse logits and the final semantic logits, fp32 mode and fp16x3
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,precision', FORWARD)
def test_heads_and_coarse_logits_against_the_oracle(nets, tag, precision):
    """centre heat-map and offsets: max |d| within the precision's gate of max(1, rms); the coarse semantic logits the same
    in fp32 mode, as probabilities within 1e-3 in fp16x3 -- against the oracle's fp32 forward and, where the network comes
    from an export fixture, against the reference's own recorded output"""
    c = nets.case(tag)
    _, out, coarse = nets.forward(tag, precision)
    gate = GATE[precision]
    rep = {}
    for k in ('ctr_hmp', 'offsets'):
        rep[k] = _rel(out[k], c['ref'][k])
        if c['want'] is not None:
            rep[k + '_vs_reference'] = _rel(out[k][:1], c['want'][k])
    if precision == 'fp32':
        rep['sem_coarse'] = _rel(coarse, c['sem_coarse'])
    else:
        rep['sem_coarse'] = float((_prob(coarse) - _prob(c['sem_coarse'])).abs().max())
    print(f'{tag} [{precision}] heads over the gate {gate:g}:', {k: round(v / gate, 4) for k, v in rep.items()})
    _report(f'heads.{tag}.{precision}', dict(gate=gate, worst_over_gate=max(rep.values()) / gate, **rep))
    for k, v in rep.items():
        assert v < gate, (tag, precision, k, v)


@pytest.mark.parametrize('tag,precision', FORWARD)
def test_final_semantic_logits_after_pointrend(nets, tag, precision):
    """64^2 with >= 4096 points: both subdivision steps refine EVERY cell (32^2 and 64^2 <= subdivision_num_points, k = plane in
    Fwd::pointrend), no selection and no tie exists -- every probability within the precision's gate.  128^2: the last step
    selects; the suite's rule for two fp32-accurate forwards applies (the share of cells beyond 1e-3 in probability stays
    below 2e-3), on a seed for which the oracle and the reference's recorded output have NO such cell."""
    c = nets.case(tag)
    _, out, _ = nets.forward(tag, precision)
    P = c['cfg']['subdivision_num_points']
    size = c['size']
    d = (_prob(out['sem_logits']) - _prob(c['ref']['sem_logits'])).abs()
    if size == 64:
        assert size * size <= P, f'{tag}: {size}^2 cells > {P} points: the last step would select'
        gate = GATE[precision]
        rep = dict(prob_max=float(d.max()), gate=gate)
        if c['want'] is not None:
            rep['prob_max_vs_reference'] = float((_prob(out['sem_logits'][:1]) - _prob(c['want']['sem_logits'])).abs().max())
            assert rep['prob_max_vs_reference'] < gate, (tag, precision, rep)
        print(f'{tag} [{precision}] final semantic probability:', rep)
        _report(f'final_sem.{tag}.{precision}', rep)
        assert rep['prob_max'] < gate, (tag, precision, rep)
    else:
        assert P < size * size, f'{tag}: the last step must select'
        if c['want'] is not None:      # the condition under which the rule is a statement about the engine: no near-tie on this seed
            dw = (_prob(c['ref']['sem_logits'][:1]) - _prob(c['want']['sem_logits'])).abs()
            assert int((dw > TOL).sum()) == 0, f'{tag}: oracle and reference disagree on {int((dw > TOL).sum())} cells: pick another seed'
        rep = dict(prob_max=float(d.max()), share_over_1e3=float((d > TOL).float().mean()), cells=int(d.numel()))
        print(f'{tag} [{precision}] final semantic probability:', rep)
        _report(f'final_sem.{tag}.{precision}', rep)
        assert rep['share_over_1e3'] < 2e-3, (tag, precision, rep)


# ---------------------------------------------------------------------------------------------------------------------
# 4, 5: the fp16 engine layer by layer
# ---------------------------------------------------------------------------------------------------------------------
def _expected_rows(cfg, P):
    """rows a teacher-forced walk of ``cfg`` yields: encoder (p1 + three maps per bottleneck [+ ``.ds``]) + per decoder (the ASPP concat
    and projection + concat and output per stage | the BiFPN's maps) + one per head (two where the head stores ``.pw``)"""
    enc = 1 + 3 * 16 + (4 if os.environ.get('EMP_FUSE_DS', '1')[:1] == '0' else 0)      # the shortcuts as maps of their own
    decs = ['semantic'] + (['instance'] if cfg['ins_decoder'] else [])
    unfused = os.environ.get('EMP_FUSE_SEPCONV', '1')[:1] == '0'      # every head through ``.pw``
    heads = 3 + (3 if unfused else 1 if cfg['num_classes'] > 2 else 0)
    if not _is_bifpn(cfg):
        return enc + len(decs) * (2 + 2 * len(cfg['low_level_stages'])) + heads
    rows = enc + 1                                                                       # p2f
    for d in decs:
        resampled = sum(1 for k in P if k.startswith(f'{d}_fpn.') and '.resamplings.' in k)
        rows += 3 + 16 * cfg['fpn_layers'] + resampled + 5 + 1      # p6pre, P6, P7; 8 nodes x (fused map, output); cat0..4, out
    return rows + heads


def _teacher_forced(c, model, out, coarse):
    from oracle import pdl_model
    cfg, P = c['cfg'], c['P']
    fp32_heads = {'semantic_head.out': coarse, 'ins_center.out': out['ctr_hmp'], 'ins_xy.out': out['offsets']}

    def tap(name):
        return model.tap(name).float().cpu().permute(0, 3, 1, 2).contiguous()

    gen = (pdl_model.teacher_forced_layers_bifpn if _is_bifpn(cfg) else pdl_model.teacher_forced_layers)(P, cfg, c['x'], tap)
    rows = teacher_forced_rows(gen, tap, fp32_heads)
    names = [r[0] for r in rows]
    assert len(names) == len(set(names)) == _expected_rows(cfg, P), (len(names), _expected_rows(cfg, P))
    if not _is_bifpn(cfg):
        for d in ['semantic_decoder'] + (['instance_decoder'] if cfg['ins_decoder'] else []):
            for i in range(len(cfg['low_level_stages'])):
                assert f'{d}.stage{i}.cat' in names and f'{d}.stage{i}.out' in names, (d, i)
    if not cfg['ins_decoder']:
        assert not [n for n in names if n.startswith('instance_')]
    return rows


def _tf_report(key, rows):
    heads = {r[0]: r[2] / (1e-4 * max(1.0, r[1])) for r in rows if r[0] in ('semantic_head.out', 'ins_center.out', 'ins_xy.out')}
    rep = dict(layers=len(rows), worst_differing_fraction=max(r[3] for r in rows), worst_error_over_tolerance=max(r[4] for r in rows),
               worst_at=max(rows, key=lambda r: r[4])[0], fp32_heads_over_tolerance=heads)
    print(key, rep)
    _report(key, rep)


@pytest.mark.parametrize('tag', TEACHER_FORCED)
def test_fp16_engine_every_layer_teacher_forced(nets, tag):
    """every map of the fp16 forward recomputed by the oracle from the engine's own input maps: one fp16 ulp + 1e-4 of the
    scale, < 5 % of the elements off the correctly rounded value, 1e-4 of the scale on the fp32 heads"""
    model, out, coarse = nets.forward(tag, 'fp16')
    rows = _teacher_forced(nets.case(tag), model, out, coarse)
    _tf_report(f'teacher_forced.{tag}.fp16', rows)


@pytest.mark.parametrize('tag', TEACHER_FORCED)
def test_fp16_engine_pointrend_on_identical_inputs(nets, tag):
    """the oracle's PointRend, with the engine's fp16 roundings, on the ENGINE's coarse logits and feature map: at 64^2 every
    cell is refined and every probability agrees to 1e-3; at 128^2 a cell whose uncertainty ties with the last selected
    one may be picked by one side only (at most 16, as tests/test_gpu_parity_fullsize.py allows)"""
    from oracle import pdl_model
    c = nets.case(tag)
    cfg, P = c['cfg'], c['P']
    model, out, coarse = nets.forward(tag, 'fp16')
    semx = model.tap(_semx_name(cfg)).float().cpu().permute(0, 3, 1, 2).contiguous()
    pdl_model._EMU = pdl_model.Fp16Emu().bind(P)
    try:
        want = pdl_model.point_rend_forward(P, coarse, semx, 2, cfg['subdivision_num_points'], cfg['num_fc'])
    finally:
        pdl_model._EMU = None
    d = (_prob(out['sem_logits']) - _prob(want)).abs()
    over = int((d > TOL).sum())
    rep = dict(prob_max=float(d.max()), cells_over_1e3=over, cells=int(d.numel()))
    print(f'{tag} PointRend on identical inputs:', rep)
    _report(f'pointrend_identical_inputs.{tag}', rep)
    if c['size'] == 64:
        assert c['size'] ** 2 <= cfg['subdivision_num_points']
        assert over == 0, rep
    else:
        assert over <= 16, rep
        assert float(np.sort(d.numpy().ravel())[-17 if over else -1]) < TOL


@pytest.mark.parametrize('tag', ['pdl_single', 'pdl_stages321'])
def test_fp16_engine_fallback_launches_teacher_forced(nets, tag, monkeypatch, tmp_path):
    """every fusion switch off (the FP16_OFF set of the forward fence, read when the network is made): the depthwise launch
    + conv pair of ``sepblock``, the head through ``.pw`` and ``launch_head1x1``, separate projections, no precise site --
    the same arithmetic as the fused kernels (oracle ``_tf_sepconv``), so the same check; ``precise_block`` follows
    EMP_PRECISE_SEPCONV=0"""
    from empanada_napari_amd.engines import HipPanopticDeepLab
    c = nets.case(tag)
    _clear_switches(monkeypatch)
    for k, v in FP16_OFF.items():
        monkeypatch.setenv(k, v)
    log = str(tmp_path / 'layers.log')
    monkeypatch.setenv('EMP_LAYER_LOG', log)
    model = HipPanopticDeepLab(c['P'], c['cfg'], folded=True, precision='fp16')
    monkeypatch.delenv('EMP_LAYER_LOG')
    out = {k: v.cpu() for k, v in model(c['x'].cuda(), 2, False).items()}
    torch.cuda.synchronize()
    q = c['size'] // 4
    coarse = model.tap_raw('semantic_head.out', (c['x'].shape[0], c['cfg']['num_classes'], q, q)).cpu()
    kinds = {line.split(',')[0] for line in open(log).read().split()}
    assert kinds == {'conv', 'end'}, f'a fused launch ran with every switch off: {sorted(kinds)}'
    rows = _teacher_forced(c, model, out, coarse)
    _tf_report(f'teacher_forced.{tag}.fp16_alloff', rows)
    del model


# ---------------------------------------------------------------------------------------------------------------------
# 6: what "single decoder" means structurally
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp16', 'fp16x3', 'fp32'])
@pytest.mark.parametrize('tag', SINGLE)
def test_single_decoder_network_has_no_instance_side(nets, tag, precision):
    model, _, _ = nets.forward(tag, precision)
    params = _param_names(model)
    assert params and not [n for n in params if n.startswith(('instance_', 'decoders.'))]
    taps = model.tap_names()
    assert (precision != 'fp16' or taps) and not [n for n in taps if n.startswith(('instance_', 'decoders.'))]


def _true_cin(P, name):
    """input channels of the launch logged as ``name`` as ``conv()`` / ``sepblock()`` count them (unpadded)"""
    for key in (name, name + '1', name + '.sepconv.1'):
        if key in P:
            w = P[key][0]
            if '.upsamplings.' in key:                       # ConvTranspose2d weight: (Cin, Cout, 2, 2)
                return int(w.shape[0])
            if key.endswith('.aspp.project.0'):              # the pooled branch's fifth enters as a per-image bias
                return int(w.shape[1]) * 4 // 5
            return int(w.shape[1])
    raise KeyError(name)


def _instance_share(log_text, P, cfg, N, size):
    """the algorithmic flops of one fp16 forward of the TWO-decoder network that belong to its instance side: the
    launches its layer log names ``instance_*``, the instance couts of the merged launches, and -- the log lists the
    matrix-pipe launches only -- the depthwise halves of the instance side's separable blocks, counted as the scheduler
    books them (2 * taps * pixels * channels)"""
    from empanada_napari_amd import weights
    share = 0.0
    lines = [ln.split(',') for ln in log_text.split() if ln != 'end']
    for f in lines:
        kind, name, M, cout, ks = f[0], f[1], int(f[2]), int(f[4]), int(f[5])
        if name.startswith('instance_'):
            kk = ks * ks if kind == 'conv' else 1
            share += 2.0 * M * cout * _true_cin(P, name) * kk
        elif name.startswith('decoders.project.') or '+project.' in name:
            i = int(name.rsplit('.', 1)[1])
            w = P[f'instance_decoder.project.{i}.0'][0]
            share += 2.0 * M * w.shape[0] * w.shape[1]
        else:
            assert not name.startswith('decoders.'), f'{name}: a merged ASPP launch at this size?'
    if _is_bifpn(cfg):
        Fd = cfg['fpn_dim']
        lv = [size // 8 >> i for i in range(5)]                                     # P3 .. P7
        nodes = sum(lv[i] ** 2 for i in (3, 2, 1, 0)) + sum(lv[i] ** 2 for i in (1, 2, 3, 4))
        share += cfg['fpn_layers'] * 2.0 * 9.0 * N * nodes * Fd + 2.0 * 25.0 * N * (size // 4) ** 2 * 2 * Fd
    else:
        stride = {1: 4, 2: 8, 3: 16}
        xch = cfg['aspp_channels'] or cfg['decoder_channels']
        for st, lp in zip(cfg['low_level_stages'], weights.ins_projection_widths(cfg)):
            share += 2.0 * 25.0 * N * (size // stride[st]) ** 2 * (xch + lp)
            xch = cfg['decoder_channels']
    return share


@pytest.mark.parametrize('tag', SINGLE)
def test_single_decoder_arena_layer_log_and_flops(nets, tag, monkeypatch, tmp_path):
    """against the same network WITH an instance side (seeded parameters): a smaller arena after the same ``reserve``; a
    layer log that names no ``instance_*`` and no merged ``decoders.*`` / ``+project`` launch; ``last_flops()`` smaller by
    exactly the instance side's share of the two-decoder forward (sums of integers below 2^53: exact in a double)"""
    from empanada_napari_amd import weights
    from empanada_napari_amd.engines import HipPanopticDeepLab
    c = nets.case(tag)
    _clear_switches(monkeypatch)
    cfg2 = dict(c['cfg'], ins_decoder=True, ins_ratio=0.5)
    cfg2.pop('low_level_channels_project_ins', None)
    P2 = weights.fold_state_dict(weights.seeded_state_dict(cfg2, seed=11), cfg2)
    N, size = c['x'].shape[0], c['size']
    got = {}
    for key, P, cfg in (('single', c['P'], c['cfg']), ('two', P2, cfg2)):
        log = str(tmp_path / (key + '.log'))
        monkeypatch.setenv('EMP_LAYER_LOG', log)
        m = HipPanopticDeepLab(P, cfg, folded=True, precision='fp16')
        monkeypatch.delenv('EMP_LAYER_LOG')
        m.reserve(N, size, size)
        arena = m.arena_bytes()
        m(c['x'].cuda(), 2, False)
        torch.cuda.synchronize()
        assert m.arena_bytes() == arena      # the forward ran in the reserved plan
        got[key] = dict(arena=arena, flops=m.last_flops(), log=open(log).read())
        del m
    assert 0 < got['single']['arena'] < got['two']['arena']
    names = [ln.split(',')[1] for ln in got['single']['log'].split() if ln != 'end']
    assert names and not [n for n in names if n.startswith(('instance_', 'decoders.')) or '+project' in n], names
    assert [n for n in (ln.split(',')[1] for ln in got['two']['log'].split() if ln != 'end') if n.startswith('instance_')]
    share = _instance_share(got['two']['log'], P2, cfg2, N, size)
    rep = dict(flops_single=got['single']['flops'], flops_two=got['two']['flops'], instance_share=share,
               arena_single=got['single']['arena'], arena_two=got['two']['arena'])
    print(tag, rep)
    _report(f'structure.{tag}', rep)
    assert share > 0 and got['single']['flops'] == got['two']['flops'] - share, rep


# ---------------------------------------------------------------------------------------------------------------------
# 7: calling conventions on the new branches
# ---------------------------------------------------------------------------------------------------------------------
CALLS = [(t, p) for t in SINGLE for p in ('fp16', 'fp16x3')]


@pytest.mark.parametrize('tag,precision', CALLS)
def test_single_decoder_batch_equals_single_images(nets, tag, precision):
    model = nets.model(tag, precision)
    _, x = _synth_input(2, nets.case(tag)['size'], seed=31)
    full = {k: v.clone() for k, v in model(x.cuda(), 2, False).items()}
    for i in range(2):
        one = model(x[i:i + 1].cuda(), 2, False)
        for k in HEADS:
            assert torch.equal(one[k][0], full[k][i]), (k, i)


@pytest.mark.parametrize('tag,precision', CALLS)
def test_single_decoder_interpolate_ins(nets, tag, precision):
    """``interpolate_ins=True`` (the x4 bilinear up-sampling of the two instance heads, here behind the SEMANTIC decoder and on
    one stream).  fp16x3: against the oracle at the contract's gate.  fp16: against the engine's own quarter-resolution
    heads up-sampled by torch, at 1e-5 of the scale (one fp32 kernel against another)."""
    c, model = nets.case(tag), nets.model(tag, precision)
    xd = c['x'].cuda()
    up = {k: v.cpu() for k, v in model(xd, 2, True).items()}
    quarter = {k: v.cpu() for k, v in model(xd, 2, False).items()}
    assert torch.equal(up['sem_logits'], quarter['sem_logits'])
    for k in ('ctr_hmp', 'offsets'):
        assert up[k].shape[-2:] == (c['size'], c['size'])
        if precision == 'fp16':
            want = F.interpolate(quarter[k], scale_factor=4.0, mode='bilinear', align_corners=True)
            assert _rel(up[k], want) < 1e-5, (k, _rel(up[k], want))
        else:      # what the oracle does with interpolate_ins=True (oracle.pdl_model.pdl_forward), on its quarter-resolution heads
            want = F.interpolate(c['ref'][k], scale_factor=4.0, mode='bilinear', align_corners=True)
            assert _rel(up[k], want) < GATE[precision], (k, _rel(up[k], want))


@pytest.mark.parametrize('tag,precision', CALLS)
def test_single_decoder_rebatch_and_replan_equal_fresh_models(nets, tag, precision):
    """one model through batch 2 -> batch 1 (the planned layout's prefix) -> batch 2 -> another size (a re-plan) gives, step
    by step, the bits of a model made for that step alone"""
    from empanada_napari_amd.engines import HipPanopticDeepLab
    c = nets.case(tag)
    s = c['size']
    seq = ((2, s), (1, s), (2, s), (1, 2 * s))
    one = HipPanopticDeepLab(c['P'], c['cfg'], folded=True, precision=precision)
    fresh = {}
    for step, (batch, size) in enumerate(seq):
        x = _synth_input(batch, size, seed=5)[1].cuda()
        got = one(x, 2, False)
        torch.cuda.synchronize()
        if (batch, size) not in fresh:
            m = HipPanopticDeepLab(c['P'], c['cfg'], folded=True, precision=precision)
            fresh[(batch, size)] = {k: v.clone() for k, v in m(x, 2, False).items()}
            torch.cuda.synchronize()
            del m
        for k in HEADS:
            assert torch.equal(got[k], fresh[(batch, size)][k]), (step, batch, size, k)
    del one


@pytest.mark.parametrize('tag,precision', CALLS)
def test_single_decoder_raw_uint8_input(nets, tag, precision):
    """raw uint8 with the normalisation inside the stem == the normalised float input: bit for bit on the fp16 engine (as
    tests/test_gpu_model.py requires), within 1e-3 * max(1, |out|max) on fp16x3 (as tests/test_gpu_regnet.py does)"""
    from empanada_napari_amd.preprocess import normalize_params
    model = nets.model(tag, precision)
    img, x = _synth_input(2, nets.case(tag)['size'], seed=31)
    sub, mul = normalize_params(MEAN, STD, 255)
    a = {k: v.clone() for k, v in model(torch.from_numpy(img)[:, None].cuda(), 2, False, sub=float(sub), mul=float(mul)).items()}
    b = model(x.cuda(), 2, False)
    for k in HEADS:
        if precision == 'fp16':
            assert torch.equal(a[k], b[k]), k
        elif k != 'sem_logits':
            assert float((a[k] - b[k]).abs().max()) < 1e-3 * max(1.0, float(b[k].abs().max())), k
        else:
            assert float((_prob(a[k]) - _prob(b[k])).abs().max()) < 1e-3, k


# ---------------------------------------------------------------------------------------------------------------------
# 8: refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp16', 'fp16x3', 'fp32'])
def test_projection_widths_off_the_channel_granule_are_refused(nets, precision):
    """widths 22 / 15 (tests/golden/export_pdl_ratio.npz), and a single-decoder network with a semantic width of 20"""
    from empanada_napari_amd import _abi
    from empanada_napari_amd.engines import HipPanopticDeepLab
    if 'pdl_ratio' not in nets.cases:
        _, sd, cfg, _, _ = nets.export('pdl_ratio')
        nets.cases['pdl_ratio'] = (sd, cfg)
    sd, cfg = nets.cases['pdl_ratio']
    assert cfg['low_level_channels_project'] == [22]
    with pytest.raises(_abi.EmpError, match='multiples of 8'):
        HipPanopticDeepLab(sd, cfg, precision=precision)
    single = dict(nets.case('pdl_single')['cfg'], low_level_channels_project=[20])
    with pytest.raises(_abi.EmpError, match='multiples of 8'):
        HipPanopticDeepLab({}, single, folded=True, precision=precision)


def test_instance_widths_are_not_consulted_without_an_instance_decoder():
    """the twin of the refused 22 / 15 network: semantic width 32, an ``ins_ratio`` that would give the instance projection 22
    channels, and NO instance decoder -- builds and runs (``!cfg->ins_decoder ||`` in ``create``); one forward against the oracle"""
    from empanada_napari_amd import weights
    from empanada_napari_amd.engines import HipPanopticDeepLab
    from oracle import pdl_model
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    cfg = dict(weights.MITONET_PDL_CFG, ins_decoder=False, low_level_channels_project=[32], ins_ratio=0.7)
    assert weights.ins_projection_widths(cfg) == [22]
    P = weights.fold_state_dict(weights.seeded_state_dict(cfg, seed=43), cfg)
    model = HipPanopticDeepLab(P, cfg, folded=True, precision='fp16x3')
    x = torch.randn(1, 1, 64, 64, generator=torch.Generator().manual_seed(43))
    out = {k: v.cpu() for k, v in model(x.cuda(), 2, False).items()}
    ref = pdl_model.model_forward(P, x, cfg, 2, False)
    for k in ('ctr_hmp', 'offsets'):
        assert _rel(out[k], ref[k]) < TOL, (k, _rel(out[k], ref[k]))
    assert float((_prob(out['sem_logits']) - _prob(ref['sem_logits'])).abs().max()) < TOL      # 64^2 <= 8192 points: no selection


# ---------------------------------------------------------------------------------------------------------------------
# 9: the all-semantic pipeline end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_all_semantic_pipeline_end_to_end(nets):
    """``Engine2d`` on the pdl_single export with no thing class, default precision, a 200 x 232 crop (padded to 208 x 240): the
    label map of the device post-processing of the model's heads EQUALS the oracle's post-processing of the same arrays, and
    ``infer`` returns it cropped.  A semantic-only map holds ``class * label_divisor`` (engines.py:277-292 through
    merge_semantic_and_instance): classes {0, 1, 2} and no instance part."""
    from empanada_napari_amd import synth
    from empanada_napari_amd.inference import Engine2d
    from empanada_napari_amd.preprocess import normalize_params
    from oracle import postprocess as opp
    path = nets.export('pdl_single')[0]
    divisor = 1000
    mc = {'model': path, 'thing_list': [], 'labels': [1, 2], 'class_names': {1: 'a', 2: 'b'}, 'padding_factor': 16,
          'norms': {'mean': MEAN, 'std': STD}}
    eng = Engine2d(mc, label_divisor=divisor, nms_kernel=3, nms_threshold=0.1, confidence_thr=0.5)
    model = eng.engine.model
    assert model.precision == os.environ.get('EMP_PRECISION', 'fp16x3') and not model.cfg['ins_decoder'] and model.cfg['num_classes'] == 2
    img = synth.em_tiles(1, 256, seed=21)[0][:200, :232]
    # the model once, the way ``infer`` calls it for a raw image: normalisation and the padding to 208 x 240 inside the stem
    sub, mul = normalize_params(MEAN, STD, 255)
    raw = torch.from_numpy(np.ascontiguousarray(img))[None, None].cuda()
    out = model(raw, 2, interpolate_ins=False, sub=float(sub), mul=float(mul), pad_to=(208, 240))
    from empanada_napari_amd.engines import logits_to_prob
    sem = logits_to_prob(out['sem_logits'])
    assert tuple(sem.shape) == (1, 2, 208, 240) and tuple(out['ctr_hmp'].shape) == (1, 1, 52, 60)
    cells, _, _, kmax = eng.engine.instance_cells_int(out['ctr_hmp'], out['offsets'], 1)
    pan = eng.engine.panoptic_merge_int(sem, cells, kmax).cpu().numpy()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    o['sem'] = sem.cpu().numpy()
    oeng = opp.RenderEngine(lambda *_: o, [], label_divisor=divisor, nms_threshold=0.1, nms_kernel=3, confidence_thr=0.5,
                            coarse_boundaries=True)
    want = oeng.postprocess(o['sem'], oeng.cells(o['ctr_hmp'], o['offsets'], 1))
    assert pan.shape == want.shape == (1, 208, 240)
    assert np.array_equal(pan, want), f'{int((pan != want).sum())} label mismatches on identical heads'
    got = eng.infer(img)
    assert got.shape == img.shape and got.dtype == np.int32
    assert np.array_equal(got, want[0, :200, :232])
    assert set(np.unique(got).tolist()) <= {0, divisor, 2 * divisor}, np.unique(got)
    assert len(np.unique(got)) > 1, 'the crop shows one class only: nothing was compared'
