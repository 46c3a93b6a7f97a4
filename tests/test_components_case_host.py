"""The slab-by-slab connected components on the host (tests/components_case.py): the numpy emulation of the algorithm equals
``oracle.sparse.label_nd`` of the whole array for every slab size, and an emulation with one planted defect does not -- so the
cases that the device tests run can tell a wrong implementation from a right one.  The pure planning (the slab cap and the
refusals of ``_labelplan``) is checked here as well: it needs no device."""
import numpy as np
import pytest

import components_case as CC

CASES = CC.cases()


def _slabs(arr):
    D = arr.shape[0]
    return sorted({s for s in CC.SLABS if s < D} | {D})


@pytest.mark.parametrize('name', sorted(CASES))
def test_emulation_equals_the_reference_for_every_slab(name):
    arr = CASES[name]
    want = CC.cached_reference(name, arr)
    for slab in _slabs(arr):
        got, count = CC.slab_components(arr, slab)
        assert np.array_equal(got, want), (name, slab)
        assert count == int(want.max())


def test_the_cases_are_what_they_say():
    ref = {k: CC.cached_reference(k, v) for k, v in CASES.items()}
    assert ref['empty'].max() == 0 and ref['full'].max() == 1 and (ref['full'] == 1).all()
    assert ref['touching'].max() == 8
    assert ref['u'].max() == 2 and ref['serpent'].max() == 2
    assert all(ref[k].max() == 1 for k in CASES if k.startswith('pair'))
    assert len([k for k in CASES if k.startswith('pair')]) == 49      # 9 spots x 9 offsets less the partners outside
    assert all(v.shape[0] <= 12 and v.shape[1] <= 16 and v.shape[2] <= 24 for k, v in CASES.items() if v.ndim == 3)
    assert 30 <= ref['random0'].max() and ref['random_12x16x24'].max() >= 100
    late = ref['late']      # B's first voxel precedes A's in raster order; C and B's second piece start in slice 1
    assert late[0, 1, 1] == 1 and late[0, 4, 6] == 2 and late[1, 0, 3] == 3 and late[1, 1, 5] == 1 and late[3, 5, 0] == 4
    assert CC.reference(CC.capacity_volume()).max() > 2048


@pytest.mark.parametrize('defect', CC.DEFECTS)
def test_a_planted_defect_is_caught(defect):
    """on every random draw at every slab below the depth, and by the case written for it"""
    for name in ('random0', 'random1', 'random2', 'random3', 'random_12x16x24'):
        arr, want = CASES[name], CC.cached_reference(name, CASES[name])
        for slab in _slabs(arr)[:-1]:
            if defect == 'stale_halo' and slab * 2 >= arr.shape[0]:
                continue      # one seam only: the first slab's halo is the right one
            assert not np.array_equal(CC.slab_components(arr, slab, defect)[0], want), (defect, name, slab)
    written_for = {'no_diagonals': 'pair+1+1_at0_0', 'no_value_test': 'touching', 'local_order': 'late', 'no_base': 'late', 'stale_halo': 'serpent'}
    name = written_for[defect]
    assert not np.array_equal(CC.slab_components(CASES[name], 1, defect)[0], CC.cached_reference(name, CASES[name]))
    # with one slab there is no seam, no base and no halo: every emulation is the reference
    assert np.array_equal(CC.slab_components(CASES[name], CASES[name].shape[0], defect)[0], CC.cached_reference(name, CASES[name]))


def test_seam_shortcut_is_implied():
    """emp_ccl_seam unites with the voxel straight below only, where that one matches: the other eight matches are its in-plane
    neighbours, which the previous slab's own components have joined already.  Here: the sets are the same either way."""
    rng = np.random.default_rng(3)
    for _ in range(20):
        vol = (rng.integers(1, 3, (2, 6, 7)) * (rng.random((2, 6, 7)) < 0.6)).astype(np.int32)
        pid, cid = CC.reference(vol[:1])[0], CC.reference(vol[1:])[0]
        base = int(pid.max())

        def sets(pairs):
            f = CC.Forest()
            f.extend(base + int(cid.max()))
            for a, b in pairs:
                f.union(a, b)
            return f.lut()[0].tolist()
        full = CC.seam_unions(vol[0], pid, vol[1], cid, 0, base)
        short = CC.seam_unions(vol[0], pid, vol[1], cid, 0, base, shortcut=True)
        assert len(short) < len(full) and sets(short) == sets(full)


def test_planning_refusals_and_the_slab_cap():
    from empanada_napari_amd import _labelplan as P
    assert P.components_geometry((5, 6, 7)) == (5, 6, 7) and P.components_geometry((40, 56)) == (40, 1, 56)
    for shape in ((3,), (2, 3, 4, 5)):
        with pytest.raises(ValueError, match='2-D or 3-D'):
            P.components_geometry(shape)
    with pytest.raises(ValueError, match='one slice'):
        P.components_geometry((4, 1 << 15, 1 << 15))
    assert P.components_geometry((4096, (1 << 15) - 1, 1 << 15))[0] == 4096      # any number of slices below 2^30 voxels each
    # the default: the stream's choice, capped at 2^28 voxels, never below one slice
    assert P.components_slab(4096, 4096 * 4096, None, 4096) == 16
    assert P.components_slab(100, 50, None, 100) == 100 and P.components_slab(100, 50, None, 7) == 7
    assert P.components_slab(8, (1 << 30) - 1, None, 8) == 1
    # an explicit slab is taken as given, at most all rows, and refused from the shape alone
    assert P.components_slab(100, 1 << 20, 1000, 100) == 100 and P.components_slab(100, 1 << 20, 5, 100) == 5
    assert P.components_slab(4096, 1 << 24, 63, 4096) == 63
    with pytest.raises(ValueError, match='smaller slab='):
        P.components_slab(4096, 1 << 24, 64, 4096)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='positive'):
            P.components_slab(10, 10, bad, 10)
    P.components_check_labels((1 << 31) - 2)
    with pytest.raises(ValueError, match=r'labels below 2\^31 - 1'):
        P.components_check_labels((1 << 31) - 1)
    P.components_check_count((1 << 31) - 2)
    with pytest.raises(ValueError, match=r'more than 2\^31 - 2 components'):
        P.components_check_count((1 << 31) - 1)
