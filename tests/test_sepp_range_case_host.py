"""The case module of the precise separable block's operand-range tests (tests/sepp_range_case.py), checked on the CPU: the
emulation of the kernel's arithmetic stays inside the derived bounds on every (case, family), the `exact` family is exact, every
planted defect leaves the GPU test's acceptance on every family listed for it, the band where inf and finite are both accepted
stays small, the families hold what their descriptions promise, and the emulated round-toward-zero split equals a direct
truncation.  What holds here of the emulation is what tests/test_gpu_sepp_range.py asks of the kernel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sepp_range_case as sc  # noqa: E402

IDS = [c['id'] for c in sc.CASES]
PAIRS = [(c['id'], f) for c in sc.CASES for f in sc.families_of(c)]


def test_the_case_list_is_the_issues():
    assert IDS == ['p5_128', 'p5_ld', 'p5_512', 'p5_silu', 'p5_head1', 'p5_head2', 'p3_silu', 'p3_256', 'ws5_128', 'ws3_silu',
                   'ws5_head1', 'multi']
    assert set(c['entry'] for c in sc.CASES) == set(sc.ENTRIES)
    assert sc.CASE['p5_ld']['in_ld'] == 200 and sc.CASE['p5_ld']['in_ld'] % 8 == 0 and sc.CASE['p5_ld']['C'] + 8 == 200
    assert sorted({c['C'] // 64 for c in sc.CASES}) == [2, 3, 4, 8]
    assert all('over' not in sc.families_of(c) for c in sc.CASES if c['head_c'])
    # multi: tiles dealt as tile_of(it) = (it * 8 + xcd) * (grid / 8) + jx -- workgroup 0's second tile is tile `grid`
    m = sc.CASE['multi']
    tx, ty = -(-m['W'] // sc.TILE_W), -(-m['H'] // sc.TILE_H)
    assert (m['H'], m['W'], m['N']) == (1025, 1, 2) and m['N'] * tx * ty > sc.GRID >= tx * ty      # ... and it lies in image 1
    assert m['N'] * max(1, tx - 1) * ty <= sc.GRID or m['N'] * tx * (ty - 1) <= sc.GRID            # one tile less: none has two
    assert sc.families_of(m) == ('exact', 'ladder_dn0')


@pytest.mark.parametrize('cid,family', PAIRS)
def test_emulation_within_the_bounds(cid, family):
    c, p, r = sc.case_reference(cid, family)
    got = sc.emulate(c, p)
    ok, amb = sc.accept(got, r, sc.RSS_HOST)
    a, b, rel = sc.ratios(got, r)
    print(f'{cid} {family}: factor on worst {a:.3f}, on rss {b:.3f}, max|err| / max|ref| {rel:.2e}')
    assert not np.isnan(np.asarray(got, np.float64)).any()
    assert ok.all(), (cid, family, int((~ok).sum()), a, b)
    assert a <= 1.0 and b <= sc.RSS_HOST
    # the band where inf and finite are both right: none outside `over`, at most 1 % inside it
    assert amb.sum() <= (0.01 * amb.size if family in sc.OVERFLOW_FAMILIES else 0), (cid, family, int(amb.sum()))


@pytest.mark.parametrize('cid', IDS)
def test_exact_family_is_the_float64_result_bit_for_bit(cid):
    c, p, r = sc.case_reference(cid, 'exact')
    want, tol, mag = sc.exact_expected(c, p)
    assert mag <= sc.EXACT_MAG
    got = sc.emulate(c, p)
    assert sc.exact_mismatches(c, got, want, tol) == 0
    if c['act'] != 2:
        assert np.array_equal(np.asarray(got, np.float64), r['ref'])      # reference() and exact_expected() agree
    assert np.count_nonzero(want) > 0.2 * want.size


@pytest.mark.parametrize('cid', [c['id'] for c in sc.CASES if 'over' in sc.families_of(c)])
def test_over_family_pushes_outputs_over(cid):
    c, p, r = sc.case_reference(cid, 'over')
    t, E = r['ref'], r['worst']
    up, dn = sc.over_channels(c)
    assert (t[:, up] - E[:, up] >= 2 * sc.INF16).all()
    if c['act'] == 0:
        assert (t[:, dn] + E[:, dn] <= -2 * sc.INF16).all()
    else:
        assert (np.abs(t[:, dn]) <= 1e-300).all()      # 0 behind ReLU, -0 behind SiLU
    assert 0.01 <= (len(up) + len(dn)) / t.shape[1] <= 0.055


@pytest.mark.parametrize('cid', [c['id'] for c in sc.CASES if 'top' in sc.families_of(c)])
def test_top_tiny_and_dover_hold_what_they_promise(cid):
    c = sc.CASE[cid]
    # top: activations at +-65504, every depthwise value inside fp16's range
    _, p, r = sc.case_reference(cid, 'top')
    d, e_dw, _ = sc.depthwise64(c, p)
    assert (np.abs(p['x'].astype(np.float64)) == sc.MAX16).mean() > 0.005
    assert (np.abs(d) + e_dw).max() <= sc.MAX16 and np.abs(d).max() > 2048.0
    # tiny: most hi halves subnormal, every lo half subnormal or zero, some of both present
    _, p, r = sc.case_reference(cid, 'tiny')
    d32, _, _ = sc.depthwise(np.asarray(p['x'][..., :c['C']], np.float32), p['dw'], c['ks'], np.float32)
    hi, lo = (np.abs(v.astype(np.float64)) for v in sc.split_rtz(d32))
    assert (hi < sc.MIN16).mean() > 0.5 and (lo < sc.MIN16).all() and (lo > 0).any() and ((hi > 0) & (hi < sc.MIN16)).any()
    # dover: about 1 % of |d| beyond 65520 and below 131008 - margin, nothing beyond, every output finite
    _, p, r = sc.case_reference(cid, 'dover')
    d, e_dw, _ = sc.depthwise64(c, p)
    share = float((np.abs(d) - e_dw > sc.INF16).mean())
    assert 0.004 <= share <= 0.0125, share
    assert (np.abs(d) + e_dw).max() < sc.PAIR_MAX - sc.DOVER_MARGIN
    dep = (np.abs(d) > sc.MAX16).any(1).mean()
    print(f'{cid} dover: {share:.4f} of the depthwise values beyond 65520, {dep:.3f} of the pixels hold one')
    assert np.isfinite(r['ref']).all()
    if not c['head_c']:
        assert (np.abs(r['ref']) + r['worst'] < sc.INF16).all()


@pytest.mark.parametrize('cid,variant', [(c['id'], v) for c in sc.CASES for v in sc.VARIANTS
                                         if sc.has_feature(c, v) and sc.defect_families(c, v)])
def test_planted_defect_leaves_the_gpu_acceptance(cid, variant):
    """on every case that runs the code the defect touches, on every family listed for it, at least one element of the defective
    emulation is outside the acceptance the GPU test uses (factor 6): that test would fail on such a kernel"""
    for family in sc.defect_families(sc.CASE[cid], variant):
        c, p, r = sc.case_reference(cid, family)
        bad = int((~sc.accept(sc.emulate(c, p, variant), r, sc.RSS_GPU)[0]).sum())
        assert bad > 0, (cid, variant, family)


def test_every_defect_is_planted_somewhere():
    for v in sc.VARIANTS:
        n = sum(1 for c in sc.CASES if sc.has_feature(c, v) and sc.defect_families(c, v))
        assert n >= (3 if v == 'ws_no_third' else 8), (v, n)


def _trunc16(v):
    """truncation of |v| to fp16's grid (11 bits, steps of 2^-24 below 2^-14), clamped at 65504 -- in float64, no conversions"""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 1e-300)))
    q = 2.0 ** np.maximum(e - 10.0, -24.0)
    return np.copysign(np.minimum(np.floor(a / q) * q, 65504.0), v)


def test_emulated_split_is_a_truncation_split():
    edge = [0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -30, 2.0 ** -15 + 2.0 ** -26, 2.0 ** -20,
            1.0, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -11, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, 0.125, 0.125 - 2.0 ** -27, 3.14159274,
            2047.999, 65504.0, 65519.0, 65519.996, 65520.0, 65535.996, 65536.0, 100000.25, 131007.0, 131007.992]
    rng = np.random.default_rng(5)
    v = np.concatenate([edge, [-x for x in edge], rng.standard_normal(4096) * 2.0 ** rng.integers(-30, 17, 4096)]).astype(np.float32)
    v = v[np.abs(v) < sc.PAIR_MAX]
    hi, lo = sc.split_rtz(v)
    v64 = v.astype(np.float64)
    whi = _trunc16(v64)
    wlo = _trunc16(v64 - whi)
    assert np.array_equal(hi.astype(np.float64), whi) and np.array_equal(lo.astype(np.float64), wlo)
    assert np.array_equal(np.signbit(hi), np.signbit(v)) and np.isfinite(hi.astype(np.float32)).all()
    # the pair is short of the value by less than u_pair, on the value's side of zero
    short = v64 - (whi + wlo)
    assert (short * np.sign(v64) >= 0).all() and (np.abs(short) <= sc.u_pair(np.abs(v64))).all()
    assert (np.abs(short) < sc.u_pair(np.abs(v64)))[np.abs(v64) >= 2.0 ** -24].all()      # (below: the pair is zero, short by |v|)
    assert (np.abs(wlo) <= sc.lo_mag(np.abs(v64))).all()
    for x, (a, b) in {65504.0: (65504.0, 0.0), 65519.0: (65504.0, 15.0), 131007.0: (65504.0, 65472.0), 2.0 ** -24: (2.0 ** -24, 0.0),
                      2.0 ** -25: (0.0, 0.0), -2.0 ** -25: (-0.0, -0.0)}.items():
        h1, l1 = sc.split_rtz(np.float32(x))
        assert (float(h1), float(l1)) == (a, b), (x, float(h1), float(l1))


def test_pair_advantage_by_the_bounds_alone():
    """where the derived bounds of the two already imply `closer than the fp16 pair` along the dn ladder (printed; the GPU test asserts
    the comparison at those E only)"""
    for cid in ('p5_128', 'p3_256'):
        for E in sc.LADDER_E:
            low, B = sc.pair_advantage(cid, f'ladder_dn{E}')
            print(f'{cid} dn{E}: the pair is at least {low:.3e} rms from y64, the precise kernel at most {B:.3e}: implied {low > B}')
            assert np.isfinite(low) and np.isfinite(B)
