"""The fp16 engine's convolutions across operand magnitudes, element by element (tests/f16_range_case.py holds the inputs, the
float64 references and the derivation of the bounds; tests/test_f16_range_case_host.py checks that module on the CPU).  Every
kernel of the family -- csrc/conv_igemm.hip (also as the grouped kernel), conv_igemm256.hip, conv_igemm_s64.hip, conv3x3c64.hip,
sepconv.hip, the dwconv of layers.hip; nn.Conv2d + folded BatchNorm + activation (+ skip add) of resnet.py:109-129, the
transposed convolutions of blocks.py:154-171, SeparableConv2d of blocks.py:15-33 / bifpn.py:24-45 -- through its C ABI entry, on
every tile the `variant` word can force, with every ConvParams feature the network uses (second source, pixel-shuffle store,
two and three destinations, the fused next conv, groups): integer operands whose result must be the float64 result bit for bit,
an exponent ladder per input channel, the top and the bottom of fp16's range, outputs pushed over it.

1. every output element inside |got - y64| <= E + h(|y64| + E), E = min(worst, 6 rss), +-inf exactly where the value the kernel
   rounds is beyond 65520;  2. bit identity where the code claims it: all variants of a case, a split store and the
   single-destination run, a pixel-shuffle store and the plain run, next_out and a separate 1x1 launch, a grouped launch and one
   launch per group, the fused separable block and dwconv + conv;  3. the measured ratios per (entry, family) go to
   f16_range.json next to the suite's other reports (committed as profiles/f16_operand_range.json)."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f16_range_case as fc  # noqa: E402
from test_gpu_fp16x3 import REPORT as _X3_REPORT  # noqa: E402

pytestmark = pytest.mark.gpu

REPORT = os.path.join(os.path.dirname(_X3_REPORT), 'f16_range.json')      # where the suite's other reports go
SENTINEL = 7.0
REPS = 3            # LDS-DMA in flight across barriers: a race would not show in every run
IDS = [c['id'] for c in fc.CASES]


def _save_max(key, vals):
    """keep the largest of each figure per (entry, family)"""
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    d = {}
    if os.path.exists(REPORT):
        try:
            d = json.load(open(REPORT))
        except Exception:
            d = {}
    old = d.get(key, {})
    d[key] = {k: max(float(v), float(old.get(k, 0.0))) for k, v in vals.items()}
    json.dump(d, open(REPORT, 'w'), indent=1, sort_keys=True)


def _lib():
    from empanada_napari_amd import _abi
    return _abi, _abi.load()


def _dev():
    from gpu_common import dev
    return dev()


def _buf(rows, width, slack=8, dtype=torch.float16):
    """a sentinel-filled buffer whose first `width` channels are the destination"""
    return torch.full((rows, width + slack), SENTINEL, dtype=dtype, device=_dev())


def _take(buf, width):
    assert torch.all(buf[:, width:] == SENTINEL), 'wrote outside its channel slice'
    return buf[:, :width]


@functools.lru_cache(maxsize=2)
def _inputs(cid, family):
    """(numpy inputs, device tensors) of a case"""
    c = fc.CASE[cid]
    p = fc.build(c, family)
    T = {k: torch.from_numpy(v).to(_dev()) for k, v in p.items()}
    if fc.is_gemm(c):
        w = p['w'].reshape(p['w'].shape[0], -1)
        T['wcat'] = torch.from_numpy(np.ascontiguousarray(np.concatenate([w, p['w2']], 1) if c['Cin2'] else w)).to(_dev())
    return p, T


@functools.lru_cache(maxsize=2)
def _reference(cid, family):
    """computed once per (case, family) and not to be modified"""
    return fc.reference(fc.CASE[cid], _inputs(cid, family)[0])


# ----------------------------------------------------------------------------
# one launch per entry -> (M, Cout_total | head_c) on the device
# ----------------------------------------------------------------------------
def _conv(c, T, variant, plain=False):
    """the implicit-GEMM entries.  plain: the same convolution through emp_conv2d_nhwc_f16_ex without the pixel shuffle, the
    further destinations and the fused next conv.  -> (out (M, Cout), next_out or None)"""
    _abi, lib = _lib()
    P, st = _abi.ptr, _abi.stream_ptr(_dev())
    N, H, W, k, Co = c['N'], c['H'], c['W'], c['k'], c['Cout']
    Ho, Wo = fc.out_hw(c)
    M = N * Ho * Wo
    x, b = T['x'], T['b']
    w = T['wcat']
    if variant & fc.PACKED:
        wp = torch.empty_like(w)
        _abi.check(lib.emp_conv256_pack_weights(P(w), P(wp), Co, k * k, c['Cin'], c['Cin2'], st), 'pack')
        w = wp
    bn, r = T.get('bn'), T.get('r')
    geo = (k, k, c['stride'], c['pad'], c['dil'], c['act'], variant)
    if c['entry'] == 'nhwc':
        out = _buf(M, Co)
        _abi.check(lib.emp_conv2d_nhwc_f16(P(x), N, H, W, c['Cin'], c['Cin'], P(w), P(b), P(bn), P(r), Co if r is not None else 0, P(out),
                                           Co + 8, Co, *geo, st), 'emp_conv2d_nhwc_f16')
        torch.cuda.synchronize()
        return _take(out, Co), None
    if c['entry'] == 'dual':
        out = _buf(M, Co)
        _abi.check(lib.emp_conv1x1_dual_nhwc_f16(P(x), N, H, W, c['Cin'], c['Cin'], P(T['x2']), c['H2'], c['W2'], c['Cin2'], c['Cin2'],
                                                 c['stride2'], P(w), P(b), P(out), Co + 8, Co, c['act'], variant, st), 'emp_conv1x1_dual_nhwc_f16')
        torch.cuda.synchronize()
        return _take(out, Co), None
    ps = 0 if plain else c['ps']
    split, split3 = (0, 0) if plain else (c['split'], c['split3'])
    nxt = 0 if plain else c['next']
    w1 = ps or split or Co
    out = _buf(4 * M if ps else M, w1)
    o2 = _buf(M, (split3 or Co) - split) if split else None
    o3 = _buf(M, Co - split3) if split3 else None
    no = _buf(M, nxt) if nxt else None
    x2 = T.get('x2')
    _abi.check(lib.emp_conv2d_nhwc_f16_ex(P(x), N, H, W, c['Cin'], c['Cin'], P(w), P(b), P(bn), P(r), Co if r is not None else 0, P(out), w1 + 8, Co,
                                          *geo, P(x2), c['H2'], c['W2'], c['Cin2'], c['Cin2'], c['stride2'], ps,
                                          P(o2), o2.shape[1] if split else 0, split, P(o3), o3.shape[1] if split3 else 0, split3,
                                          P(T['nw']) if nxt else None, P(T['nb']) if nxt else None, P(no), nxt, nxt + 8 if nxt else 0, st),
               'emp_conv2d_nhwc_f16_ex')
    torch.cuda.synchronize()
    o = _take(out, w1)
    if ps:      # (n, 2y + dy, 2x + dx, c) -> (n, y, x, (dy * 2 + dx) * ps + c)
        o = o.reshape(N, Ho, 2, Wo, 2, ps).permute(0, 1, 3, 2, 4, 5).reshape(M, Co)
    if split:
        o = torch.cat([o, _take(o2, o2.shape[1] - 8)] + ([_take(o3, Co - split3)] if split3 else []), 1)
    return o, (_take(no, nxt) if nxt else None)


def _grouped(c, T, tile):
    _abi, lib = _lib()
    P = _abi.ptr
    N, H, W, k, G, gw = c['N'], c['H'], c['W'], c['k'], c['groups'], c['gw']
    Ho, Wo = fc.out_hw(c)
    x = T['x']
    out = _buf(N * Ho * Wo, G * gw)
    _abi.check(lib.emp_conv2d_grouped_nhwc_f16(P(x), N, H, W, c['Cin'], x.shape[-1], P(T['w']), P(T['b']), P(out), G * gw + 8, c['Cout'], k, k,
                                               c['stride'], c['pad'], c['dil'], c['act'], G, gw, c['Cout'] * k * k * c['Cin'], gw, tile,
                                               _abi.stream_ptr(_dev())), 'emp_conv2d_grouped_nhwc_f16')
    torch.cuda.synchronize()
    return _take(out, G * gw)


def _per_group(c, T, variant):
    """the grouped case as one emp_conv2d_nhwc_f16 launch per group on channel slices of the same buffers"""
    _abi, lib = _lib()
    P = _abi.ptr
    N, H, W, k, G, gw, Co = c['N'], c['H'], c['W'], c['k'], c['groups'], c['gw'], c['Cout']
    Ho, Wo = fc.out_hw(c)
    x = T['x']
    outs = []
    for g in range(G):
        out = _buf(N * Ho * Wo, Co)
        _abi.check(lib.emp_conv2d_nhwc_f16(P(x[..., g * gw:]), N, H, W, c['Cin'], x.shape[-1], P(T['w'][g * Co:]), P(T['b'][g * Co:]), None, None, 0,
                                           P(out), Co + 8, Co, k, k, c['stride'], c['pad'], c['dil'], c['act'], variant, _abi.stream_ptr(_dev())),
                   'emp_conv2d_nhwc_f16')
        torch.cuda.synchronize()
        outs.append(_take(out, Co))
    return torch.cat(outs, 1)


def _dwconv(c, T):
    _abi, lib = _lib()
    N, H, W, C = c['N'], c['H'], c['W'], c['Cin']
    out = _buf(N * H * W, C)
    _abi.check(lib.emp_dwconv_nhwc_f16(_abi.ptr(T['x']), N, H, W, C, C, _abi.ptr(T['dw']), c['k'], _abi.ptr(out), C + 8, _abi.stream_ptr(_dev())),
               'emp_dwconv_nhwc_f16')
    torch.cuda.synchronize()
    return _take(out, C)


def _sep(c, T):
    _abi, lib = _lib()
    P, st = _abi.ptr, _abi.stream_ptr(_dev())
    N, H, W, C, Co, hc = c['N'], c['H'], c['W'], c['Cin'], c['Cout'], c['head_c']
    pwp = torch.empty_like(T['pw'])
    _abi.check(lib.emp_sepconv5x5_pack_pw(P(T['pw']), C, C, Co, P(pwp), st), 'pack')
    if c['k'] == 3:
        out = _buf(N * H * W, Co)
        _abi.check(lib.emp_sepconv3x3_nhwc_f16(P(T['x']), N, H, W, C, C, P(T['dw']), P(pwp), P(T['b']), Co, c['act'], P(out), Co + 8, st),
                   'emp_sepconv3x3_nhwc_f16')
        torch.cuda.synchronize()
        return _take(out, Co)
    out = None if hc else _buf(N * H * W, Co)
    ho = torch.full((N, hc, H * W), SENTINEL, dtype=torch.float32, device=_dev()) if hc else None
    _abi.check(lib.emp_sepconv5x5_nhwc_f16(P(T['x']), N, H, W, C, C, P(T['dw']), P(pwp), P(T['b']), Co, c['act'], P(out), Co + 8 if not hc else 0,
                                           P(T.get('hw')), P(T.get('hb')), hc, P(ho), st), 'emp_sepconv5x5_nhwc_f16')
    torch.cuda.synchronize()
    return ho[0].t().contiguous() if hc else _take(out, Co)


def _run(c, T, variant):
    """-> (out, next_out or None) as numpy"""
    if fc.is_gemm(c) and c['entry'] != 'grouped':
        o, n = _conv(c, T, variant)
    else:
        o, n = (_grouped(c, T, variant) if c['entry'] == 'grouped' else _dwconv(c, T) if c['entry'] == 'dw' else _sep(c, T)), None
    return o.cpu().numpy(), (n.cpu().numpy() if n is not None else None)


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


# ----------------------------------------------------------------------------
# 1. per-element bounds (and all variants of a case agree bit for bit)
# ----------------------------------------------------------------------------
@pytest.mark.parametrize('family', fc.FAMILIES)
@pytest.mark.parametrize('cid', IDS)
def test_every_output_element_within_the_derived_bounds(cid, family):
    c = fc.CASE[cid]
    p, T = _inputs(cid, family)
    r = _reference(cid, family)
    want = fc.exact_expected(c, p) if family == 'exact' else None
    first, fig = None, {}
    for v in c['variants']:
        got, nxt = _run(c, T, v)
        pairs = [('out', got, r)] + ([('next_out', nxt, fc.next_reference(c, p, got))] if c['next'] else [])
        for tag, g, rr in pairs:
            a, b, rel = fc.ratios(g, rr)
            print(f'{cid} {family} variant {v} {tag}: factor on worst {a:.3f}, on rss {b:.3f}, max|err| / max|ref| {rel:.2e}')
            fig = {'worst_ratio': max(a, fig.get('worst_ratio', 0.0)), 'rss_ratio': max(b, fig.get('rss_ratio', 0.0)),
                   'rel_max': max(rel, fig.get('rel_max', 0.0))}
            ok, amb = fc.accept(g, rr, fc.RSS_GPU)
            assert not np.isnan(g.astype(np.float64)).any(), (cid, family, v, tag, 'NaN')
            assert ok.all(), (cid, family, v, tag, f'{int((~ok).sum())} of {ok.size} elements outside the bound', a, b)
            assert amb.sum() <= (0.01 * amb.size if family == 'over' else 0), (cid, family, tag, int(amb.sum()))
        if want is not None:
            assert fc.exact_mismatches(c, got, want[0], r) == 0, (cid, v, 'not the exact result')
            if c['next']:
                assert np.array_equal(nxt.astype(np.float64), want[1]), (cid, v, 'next_out is not the exact result')
        if first is None:
            first = (got, nxt)
        elif (v >> 8) & 255 == 0:      # the same K order and the same epilogue code on every tile: the same bits, SiLU included
            # (a variant that sets its own K-walk group walks K in another order: held to the bounds, not to the bits)
            assert np.array_equal(_bits(got), _bits(first[0])), (cid, family, v, f'{int((_bits(got) != _bits(first[0])).sum())} values differ from variant {c["variants"][0]}')
    _save_max(f'{c["entry"]}/{family}', fig)


# ----------------------------------------------------------------------------
# 2. bit identity where the code claims it
# ----------------------------------------------------------------------------
def _same(a, b, what):
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f'{what}: {int((a.view(torch.int16) != b.view(torch.int16)).sum())} of {a.numel()} values differ'


@pytest.mark.parametrize('family', fc.FAMILIES)
@pytest.mark.parametrize('cid', [c['id'] for c in fc.CASES if c['split'] or c['ps']])
def test_split_and_shuffle_stores_equal_the_plain_store(cid, family):
    """couts [split, split3) and [split3, Cout) in their own tensors, and the pixel-shuffle store, hold the values the
    single-destination launch of the same convolution on the same tile puts at those couts"""
    c = fc.CASE[cid]
    _, T = _inputs(cid, family)
    for v in c['variants']:
        plain, _ = _conv(c, T, v, plain=True)
        for rep in range(REPS):
            _same(_conv(c, T, v)[0], plain, f'{cid} {family} variant {v} rep {rep}')


@pytest.mark.parametrize('family', fc.FAMILIES)
@pytest.mark.parametrize('cid', [c['id'] for c in fc.CASES if c['next']])
def test_fused_next_conv_equals_the_separate_launch(cid, family):
    """conv_igemm256.hip: "K ascends in 32-channel steps from a zero accumulator, i.e. the result is bit-identical to the separate
    launch" -- next_out against emp_conv2d_nhwc_f16 (1x1, ReLU, variant 19) on the returned out; out against the unfused tile"""
    c = fc.CASE[cid]
    _abi, lib = _lib()
    _, T = _inputs(cid, family)
    M, Co, nc = c['N'] * c['H'] * c['W'], c['Cout'], c['next']
    plain, _ = _conv(c, T, 64, plain=True)
    for rep in range(REPS):
        out, nxt = _conv(c, T, 0)
        _same(out, plain, f'{cid} {family} out rep {rep}')
        xin = out.contiguous()
        sep = _buf(M, nc)
        _abi.check(lib.emp_conv2d_nhwc_f16(_abi.ptr(xin), 1, 1, M, Co, Co, _abi.ptr(T['nw']), _abi.ptr(T['nb']), None, None, 0, _abi.ptr(sep), nc + 8, nc,
                                           1, 1, 1, 0, 1, 1, 19, _abi.stream_ptr(_dev())), 'emp_conv2d_nhwc_f16')
        torch.cuda.synchronize()
        _same(nxt, _take(sep, nc), f'{cid} {family} next_out rep {rep}')


@pytest.mark.parametrize('family', fc.FAMILIES)
@pytest.mark.parametrize('cid', [c['id'] for c in fc.CASES if c['groups'] > 1])
def test_grouped_launch_equals_one_launch_per_group(cid, family):
    c = fc.CASE[cid]
    _, T = _inputs(cid, family)
    want = _per_group(c, T, 19)
    for tile in c['variants']:
        for rep in range(REPS):
            _same(_grouped(c, T, tile), want, f'{cid} {family} tile {tile} rep {rep}')


@pytest.mark.parametrize('cid', [c['id'] for c in fc.CASES if c['groups'] > 1])
def test_grouped_automatic_tile_is_the_128x64_one(cid):
    """launch_conv_igemm_grouped's second condition holds for every Cout, so widths 56 and 72 both take 128 x 64 today (FINDINGS
    101): the choice pinned -- bit for bit it cannot tell the tiles apart, so the 128 x 128 one is compared as well"""
    c = fc.CASE[cid]
    _, T = _inputs(cid, 'ladder_up0')
    auto = _grouped(c, T, 0)
    _same(auto, _grouped(c, T, 2), f'{cid} tile 0 against tile 2')
    _same(auto, _grouped(c, T, 1), f'{cid} tile 0 against tile 1')


@pytest.mark.parametrize('family', fc.FAMILIES)
@pytest.mark.parametrize('cid', [c['id'] for c in fc.CASES if c['entry'] == 'sep' and not c['head_c']])
def test_fused_separable_block_equals_dwconv_and_conv(cid, family):
    """sepconv.hip: the summation order of the taps and of the GEMM "equals the unfused dwconv_kernel + conv_igemm_kernel pair" --
    at every scale, subnormal depthwise values and SiLU included"""
    c = fc.CASE[cid]
    _abi, lib = _lib()
    _, T = _inputs(cid, family)
    N, H, W, C, Co = c['N'], c['H'], c['W'], c['Cin'], c['Cout']
    mid = _dwconv(c, T).contiguous()
    out = _buf(N * H * W, Co)
    _abi.check(lib.emp_conv2d_nhwc_f16(_abi.ptr(mid), N, H, W, C, C, _abi.ptr(T['pw']), _abi.ptr(T['b']), None, None, 0, _abi.ptr(out), Co + 8, Co,
                                       1, 1, 1, 0, 1, c['act'], 0, _abi.stream_ptr(_dev())), 'emp_conv2d_nhwc_f16')
    torch.cuda.synchronize()
    for rep in range(REPS):
        _same(_sep(c, T), _take(out, Co), f'{cid} {family} rep {rep}')


def test_refused_combinations_return_the_launchers_errors():
    """the two test entries fill ConvParams and nothing else: what a launcher refuses comes back in ITS words"""
    _abi, lib = _lib()
    P, st = _abi.ptr, _abi.stream_ptr(_dev())
    x = torch.zeros((1, 8, 8, 64), dtype=torch.float16, device=_dev())
    w = torch.zeros((128, 64), dtype=torch.float16, device=_dev())
    o = torch.zeros((1, 16, 16, 128), dtype=torch.float16, device=_dev())
    b = torch.zeros((128,), device=_dev())

    def ex(res=None, ps=0, nw=None, variant=19):
        return lib.emp_conv2d_nhwc_f16_ex(P(x), 1, 8, 8, 64, 64, P(w), P(b), None, P(res), 128 if res is not None else 0, P(o), 128, 128, 1, 1, 1, 0, 1, 1,
                                          variant, None, 0, 0, 0, 0, 1, ps, None, 0, 0, None, 0, 0, P(nw), P(b) if nw is not None else None,
                                          P(o) if nw is not None else None, 64, 64, st)
    assert ex(res=o, ps=32) != 0 and b'pixel-shuffle store needs' in lib.emp_last_error()
    assert ex(nw=w) != 0 and b'fused next convolution needs' in lib.emp_last_error()
    assert ex(ps=32, variant=64) != 0 and b'conv256: unsupported shape' in lib.emp_last_error()
    rc = lib.emp_conv2d_grouped_nhwc_f16(P(x), 1, 8, 8, 64, 64, P(w), P(b), P(o), 128, 64, 1, 1, 1, 0, 1, 1, 1, 64, 64 * 64, 64, 3, st)
    assert rc != 0 and b'tile must be' in lib.emp_last_error()
    rc = lib.emp_conv2d_grouped_nhwc_f16(P(x), 1, 8, 8, 64, 64, P(w), P(b), P(o), 128, 64, 1, 1, 1, 0, 1, 1, 2, 64, 64 * 64, 64, 0, st)
    assert rc != 0 and b'grouped conv: Cin' in lib.emp_last_error()      # two groups of 64 do not fit a row of 64
    torch.cuda.synchronize()
