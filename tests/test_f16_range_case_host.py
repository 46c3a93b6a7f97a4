"""The case module of the fp16 engine's operand-range tests (tests/f16_range_case.py), checked on the CPU: the emulation of the
kernels' arithmetic stays inside the derived bounds on every (case, family), the `exact` family is exact, every planted defect
leaves the GPU test's acceptance, and the band where inf and finite are both accepted stays small.  What holds here of the
emulation is what tests/test_gpu_f16_range.py asks of the kernels.

The two fused-next cases run here at 16 x 16 pixels: their 224 x 224 only buys the launcher's 192 pixel tiles, the emulation has
no tiles, and 12.8 M float64 elements per family would take minutes."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f16_range_case as fc  # noqa: E402

IDS = [c['id'] for c in fc.CASES]


def _case(cid):
    c = fc.CASE[cid]
    if c['next']:
        c = dict(c, H=16, W=16, H2=16 if c['Cin2'] else 0, W2=16 if c['Cin2'] else 0)
    return c


@functools.lru_cache(maxsize=None)
def _ref(cid, family):
    c = _case(cid)
    p = fc.build(c, family)
    return c, p, fc.reference(c, p)


def _pairs(c, p, r, got):
    """-> [(tag, got, reference)]: a fused-next case also holds next_out against the reference made from ITS out"""
    if not c['next']:
        return [('out', got, r)]
    return [('out', got[0], r), ('next_out', got[1], fc.next_reference(c, p, got[0]))]


def test_the_case_list_is_the_issues():
    assert len(IDS) == len(set(IDS)) == 24
    assert set(c['entry'] for c in fc.CASES) == set(fc.ENTRIES)
    assert fc.CASE['next']['N'] * 224 * 224 // 256 == 196 and fc.CASE['next']['H'] == 224      # >= 192 tiles of 256 pixels
    for c in fc.CASES:
        if c['groups'] > 1:
            p = fc.build(c, 'ladder_up0')
            assert p['x'].shape[-1] == (c['groups'] - 1) * c['gw'] + c['Cin'] + 8 and np.all(p['x'] != 0) and np.isfinite(p['x']).all()
            assert np.all(p['w'][:, :, c['gw']:] == 0) and np.all(p['w'][:, :, :c['gw']] != 0)


@pytest.mark.parametrize('family', fc.FAMILIES)
@pytest.mark.parametrize('cid', IDS)
def test_emulation_within_the_bounds(cid, family):
    c, p, r = _ref(cid, family)
    for tag, got, rr in _pairs(c, p, r, fc.emulate(c, p)):
        ok, amb = fc.accept(got, rr, fc.RSS_HOST)
        a, b, rel = fc.ratios(got, rr)
        print(f'{cid} {family} {tag}: factor on worst {a:.3f}, on rss {b:.3f}, max|err| / max|ref| {rel:.2e}')
        assert ok.all(), (cid, family, tag, int((~ok).sum()), a, b)
        assert a <= 1.0 and b <= fc.RSS_HOST
        # the band where inf and finite are both right: none outside `over`, at most 1 % inside it
        assert amb.sum() <= (0.01 * amb.size if family == 'over' else 0), (cid, family, tag, int(amb.sum()))
        assert not np.isnan(np.asarray(got, np.float64)).any()


@pytest.mark.parametrize('cid', IDS)
def test_exact_family_is_the_float64_result_bit_for_bit(cid):
    c, p, r = _ref(cid, 'exact')
    want, want_next, mag = fc.exact_expected(c, p)
    assert mag <= fc.EXACT_MAG
    got = fc.emulate(c, p)
    out = got[0] if c['next'] else got
    assert fc.exact_mismatches(c, out, want, r) == 0
    if c['act'] != 2:
        assert np.array_equal(np.asarray(out, np.float64), r['ref'])      # reference() and exact_expected() agree
    if c['next']:
        assert np.array_equal(got[1].astype(np.float64), want_next)


@pytest.mark.parametrize('cid', [c['id'] for c in fc.CASES if c['entry'] != 'dw' and not c['head_c']])      # an epilogue and an fp16 store
def test_over_family_pushes_outputs_over_and_keeps_65504(cid):
    """about 2 % of the couts beyond +-2 x 65520 before the activation, by the float64 reference alone; a residual of 65504 next
    to an O(1) sum stays finite"""
    c, p, r = _ref(cid, 'over')
    t, E = r['ref'], r['worst']
    up, dn = fc.over_channels(c)
    assert (t[:, up] - E[:, up] >= 2 * fc.INF16).all()
    if c['act'] == 0:
        assert (t[:, dn] + E[:, dn] <= -2 * fc.INF16).all()
    else:
        assert (np.abs(t[:, dn]) <= 1e-300).all()      # 0 behind ReLU, -0 behind SiLU
    frac = (len(up) + len(dn)) / t.shape[1]
    assert 0.01 <= frac <= 0.055, frac
    if c['res']:
        rest = np.setdiff1d(np.arange(t.shape[1]), np.concatenate([up, dn]))
        big = np.abs(np.asarray(p['r'], np.float64).reshape(t.shape))[:, rest] == 65504.0
        assert big.any() and (np.abs(t[:, rest][big]) + E[:, rest][big] < fc.INF16).all()


@pytest.mark.parametrize('cid,variant', [(c['id'], v) for c in fc.CASES for v in fc.VARIANTS if fc.has_feature(c, v)])
def test_planted_defect_leaves_the_gpu_acceptance(cid, variant):
    """on every case that runs the code the defect touches (has_feature), on every family named for it, at least one element of
    the defective emulation is outside the acceptance the GPU test uses (factor 6): that test would fail on such a kernel"""
    for family in fc.DEFECT_FAMILIES[variant]:
        c, p, r = _ref(cid, family)
        bad = sum(int((~fc.accept(got, rr, fc.RSS_GPU)[0]).sum()) for _, got, rr in _pairs(c, p, r, fc.emulate(c, p, variant))[:1])
        assert bad > 0, (cid, variant, family)


def test_has_feature_covers_every_defect():
    for v in fc.VARIANTS:
        assert sum(fc.has_feature(c, v) for c in fc.CASES) >= 4, v
    assert all(fc.has_feature(c, 'flush_in') for c in fc.CASES)
