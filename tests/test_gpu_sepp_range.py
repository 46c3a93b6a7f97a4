"""The precise separable block (csrc/sepconv_precise.hip: depthwise KxK with fp32 taps -> hi + lo fp16 pair -> pointwise on the
matrix pipe -> bias / act [-> fp32 1x1 head]; SeparableConv2d of blocks.py:15-33 / bifpn.py:24-45 and the heads' last 1x1,
heads.py:12-15) across operand magnitudes, element by element.  tests/sepp_range_case.py holds the inputs, the float64 reference
and the derivation of the bounds; tests/test_sepp_range_case_host.py checks that module on the CPU.  Every case goes through the
real pack entries and emp_sepconvp_nhwc_f16 / emp_sepconvp_ws_nhwc_f16 into sentinel-filled buffers with guard elements.

1. every output element inside |got - y64| <= E + h(|y64| + E), E = min(worst, 6 rss); `exact` bit for bit; +-inf exactly where the
   value the kernel rounds is beyond 65520; `dover`: depthwise values beyond 65520 carried by the pair;  2. bit identities, three
   repetitions each: repeated launches, a batch and its images one by one, the weight-split form with fp16-representable weights
   and the plain form, head mode with a one-hot head and the stored map;  3. refusals leave the output alone;  4. the measured
   ratios per (entry, family), and the kernel next to the fp16 pair it exists to beat along the dn ladder, go to sepp_range.json
   next to the suite's other reports (committed as profiles/sepp_operand_range.json)."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f16_range_case as fc  # noqa: E402
import sepp_range_case as sc  # noqa: E402
from test_gpu_fp16x3 import REPORT as _X3_REPORT  # noqa: E402

pytestmark = pytest.mark.gpu

REPORT = os.path.join(os.path.dirname(_X3_REPORT), 'sepp_range.json')      # where the suite's other reports go
SENTINEL = 7.0
GUARD = 64          # guard rows (floats in head mode) in front of and behind every destination
REPS = 3            # LDS-DMA in flight across barriers: a race would not show in every run
PAIRS = [(c['id'], f) for c in sc.CASES for f in sc.families_of(c)]
SCALES = ('ladder_dn0', 'ladder_dn8', 'tiny', 'top')      # where the bit identities are asked: unit scale and three others


def _save(key, vals, keep_max=True):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    d = {}
    if os.path.exists(REPORT):
        try:
            d = json.load(open(REPORT))
        except Exception:
            d = {}
    old = d.get(key, {})
    d[key] = {k: max(float(v), float(old.get(k, 0.0))) if keep_max else float(v) for k, v in vals.items()}
    json.dump(d, open(REPORT, 'w'), indent=1, sort_keys=True)


def _lib():
    from empanada_napari_amd import _abi
    return _abi, _abi.load()


def _dev():
    from gpu_common import dev
    return dev()


def _packed(c, p, ws):
    """the taps and the pointwise weights through the pack entries, into buffers with a guard tail"""
    _abi, lib = _lib()
    P, st = _abi.ptr, _abi.stream_ptr(_dev())
    C, Co, kk = c['C'], c['Cout'], c['ks'] * c['ks']
    dw = torch.from_numpy(p['dw']).to(_dev())
    dwp = torch.full((kk * C + GUARD,), SENTINEL, dtype=torch.float32, device=_dev())
    _abi.check(lib.emp_sepconvp_pack_dw(P(dw), c['ks'], C, P(dwp), st), 'emp_sepconvp_pack_dw')
    pw = torch.from_numpy(p['pw']).to(_dev())
    n = (2 if ws else 1) * Co * C
    pwp = torch.full((n + GUARD,), SENTINEL, dtype=torch.float16, device=_dev())
    _abi.check((lib.emp_sepconvp_ws_pack_pw if ws else lib.emp_sepconvp_pack_pw)(P(pw), C, C, Co, P(pwp), st), 'pack_pw')
    torch.cuda.synchronize()
    assert torch.all(dwp[kk * C:] == SENTINEL) and torch.all(pwp[n:] == SENTINEL), 'a packer wrote past its output'
    assert torch.equal(dwp[:kk * C].sort().values, dw.flatten().sort().values), 'pack_dw is not a permutation of the taps'
    return dwp, pwp


def _launch(c, p, ws=None, head=None):
    """one launch -> (M, Cout) fp16 or, in head mode, (M, head_c) fp32, on the device.  ws: the form (default: the case's);
    head: (hw, hb) numpy, or False for the stored map of a head case (default: the case's head)"""
    _abi, lib = _lib()
    P, st = _abi.ptr, _abi.stream_ptr(_dev())
    ws = c['ws'] if ws is None else ws
    if head is None and c['head_c']:
        head = (p['hw'], p['hb'])
    N, H, W, C, Co = c['N'], c['H'], c['W'], c['C'], c['Cout']
    M = N * H * W
    dwp, pwp = _packed(c, p, ws)
    x, b = torch.from_numpy(p['x']).to(_dev()), torch.from_numpy(p['b']).to(_dev())
    fn = lib.emp_sepconvp_ws_nhwc_f16 if ws else lib.emp_sepconvp_nhwc_f16
    if not head:
        buf = torch.full((M + 2 * GUARD, Co + 8), SENTINEL, dtype=torch.float16, device=_dev())
        _abi.check(fn(P(x), N, H, W, C, c['in_ld'], c['ks'], P(dwp), P(pwp), P(b), Co, c['act'], P(buf[GUARD:]), Co + 8, None, None, 0,
                      None, st), 'emp_sepconvp_nhwc_f16')
        torch.cuda.synchronize()
        assert torch.all(buf[:GUARD] == SENTINEL) and torch.all(buf[GUARD + M:] == SENTINEL) and torch.all(buf[:, Co:] == SENTINEL), \
            'a store landed outside H x W x Cout'
        return buf[GUARD:GUARD + M, :Co]
    hw, hb = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(_dev()) for v in head)
    hc = hw.shape[0]
    buf = torch.full((N * hc * H * W + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=_dev())
    _abi.check(fn(P(x), N, H, W, C, c['in_ld'], c['ks'], P(dwp), P(pwp), P(b), Co, c['act'], None, 0, P(hw), P(hb), hc, P(buf[GUARD:]), st),
               'emp_sepconvp_nhwc_f16 (head)')
    torch.cuda.synchronize()
    assert torch.all(buf[:GUARD] == SENTINEL) and torch.all(buf[GUARD + N * hc * H * W:] == SENTINEL), 'a store landed outside the head planes'
    return buf[GUARD:GUARD + N * hc * H * W].reshape(N, hc, H * W).permute(0, 2, 1).reshape(M, hc)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f'{what}: {int((_bits(a) != _bits(b)).sum())} of {a.numel()} values differ'


# ----------------------------------------------------------------------------
# 1. per-element bounds
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('cid,family', PAIRS)
def test_every_output_element_within_the_derived_bounds(cid, family):
    c, p, r = sc.case_reference(cid, family)
    if cid == 'multi':      # the premise of its shape: the persistent grid of an MI355X
        assert torch.cuda.get_device_properties(_dev()).multi_processor_count // 8 * 8 == sc.GRID
    got = _launch(c, p).cpu().numpy()
    a, b, rel = sc.ratios(got, r)
    print(f'{cid} {family}: factor on worst {a:.3f}, on rss {b:.3f}, max|err| / max|ref| {rel:.2e}')
    g64 = got.astype(np.float64)
    if family == 'dover':
        print(f'{cid} dover: {int(np.isnan(g64).sum())} NaN, {int(np.isinf(g64).sum())} inf, {int((g64 == 0).sum())} zeros of {g64.size}')
    assert not np.isnan(g64).any(), (cid, family, 'NaN', int(np.isnan(g64).sum()))
    ok, amb = sc.accept(got, r, sc.RSS_GPU)
    assert ok.all(), (cid, family, f'{int((~ok).sum())} of {ok.size} elements outside the bound', a, b)
    assert amb.sum() <= (0.01 * amb.size if family in sc.OVERFLOW_FAMILIES else 0), (cid, family, int(amb.sum()))
    if family == 'exact':
        want, tol, _ = sc.exact_expected(c, p)
        assert sc.exact_mismatches(c, got, want, tol) == 0, (cid, 'not the exact result')
    _save(f'{c["entry"]}/{family}', {'worst_ratio': a, 'rss_ratio': b, 'rel_max': rel})


# ----------------------------------------------------------------------------
# 2. bit identities
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('cid,family', [(c['id'], f) for c in sc.CASES for f in SCALES if f in sc.families_of(c)])
def test_repeatable_and_batch_invariant(cid, family):
    """the summation order is fixed: repeated launches are identical, and N = 2 equals two N = 1 calls"""
    c = dict(sc.CASE[cid], N=2)
    p = sc.build(c, family)
    both = _launch(c, p)
    for rep in range(REPS):
        _same(_launch(c, p), both, f'{cid} {family} rep {rep}')
    M = c['H'] * c['W']
    for i in range(2):
        one = _launch(dict(c, N=1), dict(p, x=np.ascontiguousarray(p['x'][i:i + 1])))
        _same(one, both[i * M:(i + 1) * M], f'{cid} {family} image {i} alone')


@pytest.mark.parametrize('family', SCALES)
@pytest.mark.parametrize('cid', [c['id'] for c in sc.CASES if c['ws']])
def test_weight_split_form_with_fp16_weights_equals_the_plain_form(cid, family):
    """every w_lo = +0: the third MFMA adds products (+0) x hi = +-0, whose sum leaves an accumulator that is not zero unchanged --
    the two kernels agree bit for bit on every output that is not +-0.  An accumulator of exactly -0 (a bias of -0 and nothing
    but -0 products) plus a +0 is +0 in round-to-nearest: a zero may lose its sign, so zeros are compared as values"""
    c, p, _ = sc.case_reference(cid, family)
    q = dict(p, pw=p['pw'].astype(np.float16).astype(np.float32))
    plain = _launch(c, q, ws=False)
    nz = plain != 0
    assert int(nz.sum()) > 0.2 * plain.numel()
    for rep in range(REPS):
        split = _launch(c, q, ws=True)
        assert torch.equal(split == 0, ~nz), f'{cid} {family} rep {rep}: not the same zeros'
        _same(split[nz], plain[nz], f'{cid} {family} rep {rep}')


@pytest.mark.parametrize('family', SCALES)
@pytest.mark.parametrize('cid', [c['id'] for c in sc.CASES if c['head_c']])
def test_one_hot_head_is_the_activated_accumulator(cid, family):
    """head_w a one-hot and head_b = 0: the plane is float(act(acc)) of that cout (the other couts add +-0, the other waves' shares
    are +-0), so the stored fp16 map of the same operands is r16 of it -- the one rounding the non-head store adds"""
    c, p, _ = sc.case_reference(cid, family)
    Co, hc = c['Cout'], c['head_c']
    # in the first and in the last mma wave: there the cout that the float64 reference leaves non-zero behind the ReLU most often
    live = np.count_nonzero(sc.reference(dict(c, head_c=0), p)['ref'], axis=0)
    q = Co // sc.NMW
    couts = [int(np.argmax(live[:q])), Co - q + int(np.argmax(live[Co - q:]))][:hc]
    hw = np.zeros((hc, Co), np.float32)
    hw[np.arange(hc), couts] = 1.0
    stored = _launch(c, p, head=False)[:, couts].cpu().numpy().astype(np.float32)
    assert np.count_nonzero(stored) > 0.2 * stored.size
    for rep in range(REPS):
        planes = sc.r16(_launch(c, p, head=(hw, np.zeros(hc, np.float32))).cpu().numpy())
        assert np.array_equal(planes, stored), f'{cid} {family} rep {rep}: {int((planes != stored).sum())} of {stored.size} differ'


# ----------------------------------------------------------------------------
# 3. refusals
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('what,C,Cout,ks,hc,ws', [('C = 64', 64, 128, 5, 0, False), ('C = 576', 576, 128, 5, 0, False),
                                                  ('Cout = 192', 128, 192, 5, 0, False), ('3x3 with a head', 128, 128, 3, 1, False),
                                                  ('hi + lo weights with 256 couts', 128, 256, 5, 0, True)])
def test_refused_shapes_leave_the_output_alone(what, C, Cout, ks, hc, ws):
    _abi, lib = _lib()
    P, st = _abi.ptr, _abi.stream_ptr(_dev())
    x = torch.zeros((1, 8, 16, C), dtype=torch.float16, device=_dev())
    dw = torch.zeros((25 * 576,), dtype=torch.float32, device=_dev())
    pw = torch.zeros((2 * 576 * 256,), dtype=torch.float16, device=_dev())
    b = torch.zeros((256,), dtype=torch.float32, device=_dev())
    out = torch.full((8 * 16, 256), SENTINEL, dtype=torch.float16, device=_dev())
    ho = torch.full((2 * 8 * 16,), SENTINEL, dtype=torch.float32, device=_dev())
    fn = lib.emp_sepconvp_ws_nhwc_f16 if ws else lib.emp_sepconvp_nhwc_f16
    rc = fn(P(x), 1, 8, 16, C, C, ks, P(dw), P(pw), P(b), Cout, 1, None if hc else P(out), 0 if hc else 256, P(b) if hc else None,
            P(b) if hc else None, hc, P(ho) if hc else None, st)
    torch.cuda.synchronize()
    assert rc != 0 and lib.emp_last_error(), what
    assert torch.all(out == SENTINEL) and torch.all(ho == SENTINEL), what
    if ws:
        assert lib.emp_sepconvp_ws_pack_pw(P(dw), C, C, Cout, P(out), st) != 0
        torch.cuda.synchronize()
        assert torch.all(out == SENTINEL)


# ----------------------------------------------------------------------------
# 4. next to the fp16 pair the kernel exists to beat
# ----------------------------------------------------------------------------
def _pair(c, p):
    """emp_dwconv_nhwc_f16 + emp_conv2d_nhwc_f16 on the same activations, taps and pointwise weights rounded to fp16"""
    _abi, lib = _lib()
    P, st = _abi.ptr, _abi.stream_ptr(_dev())
    N, H, W, C, Co = c['N'], c['H'], c['W'], c['C'], c['Cout']
    x = torch.from_numpy(np.ascontiguousarray(p['x'][..., :C])).to(_dev())
    dw, pw = (torch.from_numpy(p[n].astype(np.float16)).to(_dev()) for n in ('dw', 'pw'))
    b = torch.from_numpy(p['b']).to(_dev())
    mid = torch.empty((N * H * W, C), dtype=torch.float16, device=_dev())
    _abi.check(lib.emp_dwconv_nhwc_f16(P(x), N, H, W, C, C, P(dw), c['ks'], P(mid), C, st), 'emp_dwconv_nhwc_f16')
    out = torch.empty((N * H * W, Co), dtype=torch.float16, device=_dev())
    _abi.check(lib.emp_conv2d_nhwc_f16(P(mid), N, H, W, C, C, P(pw), P(b), None, None, 0, P(out), Co, Co, 1, 1, 1, 0, 1, c['act'], 0, st),
               'emp_conv2d_nhwc_f16')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('E', sc.LADDER_E)
@pytest.mark.parametrize('cid', ['p5_128', 'p3_256'])
def test_against_the_fp16_pair_along_the_dn_ladder(cid, E):
    """the header's claim, measured where nobody had: max|err| / max|ref| and the rms error against y64 (fp32 taps) of this kernel
    and of dwconv + conv, one exponent per channel in [-E, 0].  `closer than the pair` is asserted only where the derived bounds
    of the two already imply it (sepp_range_case.pair_advantage); everywhere the figures are recorded"""
    family = f'ladder_dn{E}'
    c, p, r = sc.case_reference(cid, family)
    y = r['ref']
    scale = float(np.abs(y).max())
    ep = _launch(c, p).cpu().numpy().astype(np.float64) - y
    eu = _pair(c, p).cpu().numpy().astype(np.float64) - y
    fig = {'precise_rel_max': np.abs(ep).max() / scale, 'pair_rel_max': np.abs(eu).max() / scale,
           'precise_rms': np.sqrt((ep ** 2).mean()) / scale, 'pair_rms': np.sqrt((eu ** 2).mean()) / scale}
    low, B = sc.pair_advantage(cid, family)
    print(f'{cid} dn{E}: max|err| / max|ref| precise {fig["precise_rel_max"]:.2e} pair {fig["pair_rel_max"]:.2e}; rms / max|ref| precise '
          f'{fig["precise_rms"]:.2e} pair {fig["pair_rms"]:.2e}; implied by the bounds: {low > B}')
    _save(f'pair/{cid}/dn{E}', fig, keep_max=False)
    assert np.isfinite(eu).all()
    if low > B:
        assert fig['precise_rms'] < fig['pair_rms']


def test_zz_print_the_table():
    """the report as the table of FINDINGS: factor on worst / factor on rss / max|err| over max|ref| per entry and family"""
    if not os.path.exists(REPORT):
        return
    d = json.load(open(REPORT))
    fams = [f for f in sc.FAMILIES if f != 'exact']
    print('| entry | ' + ' | '.join(f.replace('ladder_', '') for f in fams) + ' |')
    for e in sc.ENTRIES:
        cells = [('{worst_ratio:.2f} / {rss_ratio:.2f} / {rel_max:.1e}'.format(**d[f'{e}/{f}']) if f'{e}/{f}' in d else '--') for f in fams]
        print(f'| {e} | ' + ' | '.join(cells) + ' |')
        for f in fams:
            if f'{e}/{f}' in d:
                assert d[f'{e}/{f}']['rss_ratio'] <= sc.RSS_GPU
    for k in sorted(k for k in d if k.startswith('pair/')):
        print(k, ' '.join(f'{n} {v:.2e}' for n, v in sorted(d[k].items())))
