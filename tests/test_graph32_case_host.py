"""Host tests (no GPU) of the map-by-map check of the fp32 / fp16x3 forward (tests/graph32_case.py,
oracle.pdl_model.Graph32Walk): the walk and its bounds hold a CPU stand-in of the engine -- the same graph in float32 on torch's CPU
kernels, in the engine's buffers and formats -- inside every bound, and put each planted defect outside the bound at the map
where it is planted.  For every defect the head-level figures the existing GPU tests assert are computed too (a defective
stand-in against the clean one) and printed with whether the 1e-3 gate would have seen it: a measurement, not an assertion.

The bound of conv32_kernel (layers_case.conv32_ref_bound) is checked against a float32 evaluation of the same sums, in
ascending and in a shuffled K order, on the walk's own layers."""
import numpy as np
import pytest
import torch

import graph32_case as G
import layers_case as LC
import x3_range_case as X3

H, W, BATCH = 128, 160, 2      # p5 of a stride-16 network is 8 x 10: larger than the largest atrous rate (6) in both directions
GATE = 1e-3

# the network configurations of tests/test_gpu_net_configs.py, seeded (the host has no export to rebuild)
NETS = {
    'pdl': {},
    'pdl_single': dict(ins_decoder=False, num_classes=2),
    'pdl_stages321': dict(low_level_stages=[3, 2, 1], low_level_channels_project=[128, 64, 32], stage4_stride=32),
    'pdl_odd': dict(num_classes=3, decoder_channels=128, aspp_channels=192, low_level_stages=[2, 1], low_level_channels_project=[64, 32],
                    atrous_rates=[3, 6, 9], num_fc=2),
    'pdl_single_s16x3': dict(ins_decoder=False, num_classes=2, low_level_stages=[3, 1], low_level_channels_project=[64, 32], stage4_stride=16),
    # BiFPN networks need multiples of 128; RegNets run their ASPP at stride 32
    'mini': dict(base='mini', shape=(1, 128, 256)),
    'mini4': dict(base='mini', num_classes=4, shape=(1, 128, 256)),
    'bifpn_single': dict(base='mini', num_classes=3, ins_decoder=False, shape=(1, 128, 256)),
    'bifpn_l2': dict(base='mini', num_classes=4, fpn_layers=2, subdivision_num_points=2048, shape=(1, 128, 256)),
    'regnetx': dict(encoder='regnetx_6p4gf', shape=(2, 128, 128)),      # (batch 2: the per-image bias)
    'regnety': dict(encoder='regnety_6p4gf', shape=(2, 128, 128)),
}
SCHEDULES = {'fp32': ('fp32', G.F32), 'x3': ('fp16x3', G.X3_DEFAULT), 'x3_planes': ('fp16x3', G.X3_PLANES), 'x3_off': ('fp16x3', G.X3_OFF),
             'x3_part': ('fp16x3', G.X3_PART)}
CLEAN = [(n, 'x3') for n in NETS] + [(n, 'fp32') for n in ('pdl', 'pdl_odd', 'mini4', 'regnety')] + [
    ('pdl', s) for s in ('x3_planes', 'x3_off', 'x3_part')] + [('pdl_single', 'x3_planes'), ('mini4', 'x3_planes'), ('bifpn_single', 'x3_off')]
# defect -> the networks that have the site; every defect is planted on EVERY network (on the schedule that can hold it), and
# where a network has no such site the stand-in must say so
DEEPLAB = ('pdl', 'pdl_single', 'pdl_stages321', 'pdl_odd', 'pdl_single_s16x3', 'regnetx', 'regnety')
TWO_DECODERS = ('pdl', 'pdl_stages321', 'pdl_odd', 'regnetx', 'regnety')
HAS_SITE = {
    'aspp_dilation': DEEPLAB,
    # the plane region: a ResNet whose low-level skips all leave below layer3
    'hl32_hi_only': ('pdl', 'pdl_single', 'pdl_odd', 'mini', 'mini4', 'bifpn_single', 'bifpn_l2'),
    'bias_n_image0': DEEPLAB,                  # (all of them run at batch 2)
    'residual_from_input': tuple(NETS),
    'align_corners_false': DEEPLAB,            # the BiFPN decoder up-samples with transposed convolutions
    'cat_pad_nonzero': TWO_DECODERS,           # the instance decoder's 16-channel projection leaves a pad in a 32-channel walk
    'projection_offset': TWO_DECODERS,
    'pr_neighbour': tuple(NETS),
    'se_gate_skipped': ('regnety',),
}
SITES = [(d, t, 'x3_planes' if d == 'hl32_hi_only' else 'x3') for d in HAS_SITE for t in NETS] + [
    ('aspp_dilation', 'pdl', 'x3_planes'), ('aspp_dilation', 'pdl_single', 'fp32'), ('bias_n_image0', 'pdl_odd', 'fp32'),
    ('residual_from_input', 'pdl', 'fp32'), ('residual_from_input', 'regnety', 'fp32'), ('align_corners_false', 'pdl_single_s16x3', 'fp32'),
    ('projection_offset', 'pdl', 'fp32'), ('pr_neighbour', 'mini4', 'fp32'), ('se_gate_skipped', 'regnety', 'fp32')]
_CACHE = {}


def network(tag):
    if ('net', tag) not in _CACHE:
        from empanada_napari_amd import weights
        change = dict(NETS[tag])
        base, shape = change.pop('base', 'pdl'), change.pop('shape', (BATCH, H, W))
        cfg = dict(weights.MITONET_MINI_CFG if base == 'mini' else weights.MITONET_PDL_CFG, **change)
        if weights.is_regnet(cfg):
            cfg['regnet'] = weights.regnet_cfg(cfg)
        P = weights.fold_state_dict(weights.seeded_state_dict(cfg, seed=11), cfg)
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(5))
        _CACHE[('net', tag)] = cfg, P, G.image_of(x)
    return _CACHE[('net', tag)]


def standin(tag, sched, defect=None):
    key = ('standin', tag, sched, defect)
    if key not in _CACHE:
        cfg, P, im = network(tag)
        prec, flags = SCHEDULES[sched]
        _CACHE[key] = G.StandIn(P, cfg, im, prec, flags, 2, False, defect)
    return _CACHE[key]


def walk(tag, sched, s):
    cfg, P, im = network(tag)
    return G.run_walk(P, cfg, im, s.has, s.fmt, s.get, SCHEDULES[sched][0], 2, False, X3.RSS_HOST)


@pytest.fixture(autouse=True)
def _threads():
    torch.set_num_threads(min(__import__('os').cpu_count() or 1, 16))


@pytest.mark.parametrize('tag,sched', CLEAN)
def test_the_stand_in_is_inside_every_bound(tag, sched):
    """every buffer of the stand-in's forward within min(worst, 3 rss) of the walk's expectation, exact where the operator is exact,
    and no buffer but the selection's work buffers goes unchecked"""
    s = standin(tag, sched)
    rows, seen, faults = walk(tag, sched, s)
    assert not faults, faults
    bad = [r for r in rows if r['viol']]
    print(f'{tag} [{sched}]: {len(rows)} checks, largest |err| / worst {max(r["worst"] for r in rows):.3f}, '
          f'/ rss {max(r["rss"] or 0 for r in rows):.3f} (accepted: 1 and {X3.RSS_HOST:g})')
    assert not bad, bad[:4]
    assert set(s.maps) - seen - set(G.ALLOW) - set(G.OUTPUTS) == set()
    # the stand-in is the walk itself in float32: its topology is held against the oracle's own fp32 forward, which is pinned to
    # the reference -- the heads and the coarse logits within the fp32 mode's gate (1e-4 of max(1, rms)) and, where the
    # stand-in stores hl32 pairs or is compared after PointRend's selection, the contract's 1e-3 on the probabilities
    from oracle import pdl_model
    cfg, P, im = network(tag)
    taps = {}
    ref = pdl_model.model_forward(P, im['x'][:, None], cfg, 2, False, taps)
    for k, want in (('ctr_hmp', ref['ctr_hmp']), ('offsets', ref['offsets']), ('semantic_head.out', taps['sem_coarse'])):
        d = float((s.maps[k] - want.double()).abs().max()) / max(1.0, float(want.pow(2).mean().sqrt()))
        assert d < 1e-4, (tag, sched, k, d)
    if sched == 'x3_planes' and tag.startswith('pdl'):
        assert s.fmt('encoder.layer3.0') and s.fmt('encoder.layer4.2') and s.fmt('semantic_decoder.aspp.cat')


@pytest.mark.parametrize('defect,tag,sched', SITES)
def test_a_planted_defect_leaves_the_bound_at_its_own_map(defect, tag, sched):
    clean, s = standin(tag, sched), standin(tag, sched, defect)
    if tag not in HAS_SITE[defect]:
        assert s.planted is None, (defect, tag, s.planted)
        return
    assert s.planted is not None, 'the network has no such site'
    rows, _, faults = walk(tag, sched, s)
    assert not faults, faults
    name, ch = s.planted
    hit = [r for r in rows if r['viol'] and r['name'] == name and (ch is None or r.get('channels') == ch)]
    assert hit, (defect, name, ch, [r for r in rows if r['viol']][:3])
    # teacher-forced: a map computed from the defective one is right GIVEN its input, so no other map leaves its worst-case bound.
    # (The rss form is not asked of the other maps here: a defect moves them away from the inputs the clean test holds, and the
    #  float32 stand-in rounds K times per output where the split-product arithmetic behind the fp16x3 rss form rounds
    #  3 K / 32 + 32 times -- one fc layer came out at 3.1 of rss after a planted align_corners defect.  Not asked of the garbage
    #  residual at all: it drives every later map far from unit scale.)
    other = [r for r in rows if r['viol'] and r['worst'] > 1.0 and r['name'] != name
             and not (defect == 'pr_neighbour' and r['name'].startswith('pr.x'))]
    assert not other or defect == 'residual_from_input', other[:3]
    fig = G.head_figures(s.heads(), clean.heads())
    seen_by_gate = max(fig['ctr_hmp'], fig['offsets'], fig['sem_prob']) >= GATE
    print(f'PLANTED {defect} {tag} [{sched}] at {name}{list(ch) if ch else ""}: |err| / worst {hit[0]["worst"]:.3g}, / rss '
          f'{hit[0]["rss"] if hit[0]["rss"] is not None else float("nan"):.3g}; heads ctr {fig["ctr_hmp"]:.2e} offsets {fig["offsets"]:.2e} '
          f'sem prob {fig["sem_prob"]:.2e} (share > 1e-3: {fig["sem_share_over_1e3"]:.1e}) -> the {GATE:g} gate '
          f'{"sees" if seen_by_gate else "MISSES"} it')


def test_conv32_bound_against_a_float32_evaluation_of_the_walks_layers():
    """layers_case.conv32_ref_bound on every c32 launch of a fp32-mode walk: a float32 fmaf chain of the same sums, in the kernel's
    ascending K order and in a shuffled one, never leaves `worst` and stays within 3 of `rss` (48 output rows x 24 couts per
    launch, drawn at random)"""
    from oracle import pdl_model
    cfg, P, im = network('pdl')
    s = standin('pdl', 'fp32')
    rng = np.random.default_rng(0)
    w = pdl_model.Graph32Walk(P, cfg, im, s.has, s.fmt, s.get, 'fp32', 2, False)
    worst_w = worst_r = 0.0
    n = 0
    for name, value, d in w.walk():
        if d['kind'] != 'conv':
            continue
        c, p = d['case'], d['p']
        b = LC.conv32_ref_bound(c, p)
        M, Cout = b['ref'].shape
        rows, cols = rng.choice(M, min(M, 48), replace=False), rng.choice(Cout, min(Cout, 24), replace=False)
        K = X3.k_of(c)
        sub = {k: v[np.ix_(rows, cols)] for k, v in b.items()}
        for order in (None, rng.permutation(K)):
            got = LC.conv32_emulate(c, p, order, rows, cols)
            rw, rr, _ = X3.ratios(got, sub)
            worst_w, worst_r = max(worst_w, rw), max(worst_r, rr)
            assert rw <= 1.0 and rr <= X3.RSS_HOST, (name, 'ascending' if order is None else 'shuffled', rw, rr)
        n += 1
    print(f'conv32 bound on {n} launches: largest |err| / worst {worst_w:.3f}, / rss {worst_r:.3f} (accepted: 1 and {X3.RSS_HOST:g})')
    assert n > 60


def test_conv32_bound_on_the_op_tests_cases():
    """the cases of tests/test_gpu_fp32_mode.py::test_conv32_equals_torch_fp32 (strides, dilation, SiLU, residual): the float32
    evaluation inside the bound.  The bound's largest element against the tensor-wide 2e-6 sqrt(K / 64 + 1) max|ref| that test also
    asserts is printed: per element the derived bound is the tighter one almost everywhere, not everywhere."""
    from test_gpu_fp32_mode import CONV_CASES
    for case in CONV_CASES:
        N, H_, W_, Cin, Cout, k, stride, pad, dil, act, res = case
        g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
        x = torch.randn((N, H_, W_, Cin), generator=g)
        w = torch.randn((Cout, Cin, k, k), generator=g) / np.sqrt(Cin * k * k)
        b = torch.randn((Cout,), generator=g)
        c = X3._c('conv32', 'nhwc', H_, W_, Cin, Cout, k, stride, pad, dil, act, res='f32' if res else '', N=N)
        p = dict(x=x.numpy(), w=w.permute(0, 2, 3, 1).reshape(Cout, k * k, Cin).contiguous().numpy(), b=b.numpy())
        if res:
            Ho, Wo = X3.out_hw(c)
            p['r'] = torch.randn((N, Ho, Wo, Cout), generator=g).numpy()
        bd = LC.conv32_ref_bound(c, p)
        accept = np.minimum(bd['worst'], X3.RSS_GPU * bd['rss'])
        old = 2e-6 * float(np.abs(bd['ref']).max()) * np.sqrt(Cin * k * k / 64.0 + 1.0)
        print(f'{case}: derived acceptance median {float(np.median(accept)):.2e}, max {float(accept.max()):.2e}; tensor-wide tolerance {old:.2e}; '
              f'share of elements where the derived one is tighter {float((accept < old).mean()):.4f}')
        got = LC.conv32_emulate(c, p, None, np.arange(min(64, bd['ref'].shape[0])), np.arange(min(16, Cout)))
        sub = {kk: v[:got.shape[0], :got.shape[1]] for kk, v in bd.items()}
        rw, rr, _ = X3.ratios(got, sub)
        assert rw <= 1.0 and rr <= X3.RSS_HOST, (case, rw, rr)
