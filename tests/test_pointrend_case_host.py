"""The references and inputs of tests/pointrend_case.py, checked on the CPU alone: every input reaches the branch of
csrc/pointrend.hip it is named for (so a GPU test cannot pass by having missed it), the references agree with
oracle/pdl_model.py on tie-free inputs, and a CPU model of the four-pass radix select with its ordered compaction returns the
set of the stable argsort on every selection input -- which documents what the kernel is meant to do and shows that every input
has one right answer."""
import numpy as np
import pytest
import torch

import pointrend_case as PC


def _oracle():
    from oracle import pdl_model
    return pdl_model


# ---- branch proofs: selection ----
def test_planes_reach_the_structural_edges():
    nb = {p: PC.scan_rounds(p) for p in PC.TOPK_PLANES}
    assert [nb[p][0] for p in (1, 7, 100, 2048)] == [1, 1, 1, 1]                  # below / exactly one chunk
    assert nb[2049] == (2, 1) and 2049 % PC.CHUNK == 1                            # one past a multiple
    assert any(p % 8 for p in PC.TOPK_PLANES if p > 8)                            # the 8-keys-per-thread guard
    assert nb[4099] == (3, 1) and nb[16384] == (8, 1)
    assert nb[530437] == (260, 2)                                                 # compact_scan_kernel: a second round with carries
    for p in PC.TOPK_PLANES:
        for d in PC.topk_dists(p):
            keys = PC.topk_keys(d, p)
            assert keys.dtype == np.uint32 and keys.shape == (p,) and keys.max() <= PC.KEY_MAX
            ks = PC.topk_ks(d, keys)
            assert {1, p, min(8192, p)} <= set(ks) and (p == 1 or p - 1 in ks)


def test_second_scan_round_carries_selected_cells():
    """with k = 8192 random keys are selected in the chunks of the second round, below a non-zero carry"""
    keys = PC.topk_keys('random', 530437)
    sel = PC.topk_ref(keys, 8192)[0]
    assert (sel // PC.CHUNK >= PC.SCAN_ROUND).sum() > 10 and (sel // PC.CHUNK < PC.SCAN_ROUND).sum() > 1000


@pytest.mark.parametrize('plane', [p for p in PC.TOPK_PLANES if 'straddle' in PC.topk_dists(p)])
def test_straddle_cut_is_inside_a_block(plane):
    keys = PC.topk_keys('straddle', plane)
    k = PC.tie_cut('straddle', keys)
    T, krem, _ = PC.select_threshold(keys, k)
    assert T == PC.STRADDLE_T and krem == PC.STRADDLE_TAKEN
    tied = np.nonzero(keys == T)[0]
    assert len(tied) > krem                                                       # more equal keys than are taken
    chunks = np.unique(tied // PC.CHUNK)
    assert len(chunks) >= 3                                                       # they lie in three chunks
    last, first_left = tied[krem - 1], tied[krem]
    assert last // PC.CHUNK == first_left // PC.CHUNK == 1                        # the cut is inside chunk 1, an odd block,
    assert (tied[:krem] // PC.CHUNK == 1).sum() > 0 and (tied[:krem] // PC.CHUNK == 0).sum() > 0      # after a boundary,
    assert last // 8 == first_left // 8                                           # and inside one thread's eight keys
    np.testing.assert_array_equal(PC.topk_ref(keys, k)[0], np.sort(np.concatenate([np.nonzero(keys < T)[0], tied[:krem]])))


@pytest.mark.parametrize('dist', ['all_equal', 'all_zero', 'two_valued', 'with_inf'])
def test_tie_cases_cut_their_group(dist):
    for plane in PC.TOPK_PLANES[1:]:
        keys = PC.topk_keys(dist, plane)
        k = PC.tie_cut(dist, keys)
        T, krem, _ = PC.select_threshold(keys, k)
        assert 0 < krem < (keys == T).sum(), (dist, plane)
        if dist == 'with_inf':
            assert T == PC.KEY_MAX
        if plane >= 2 * PC.CHUNK:
            assert len(np.unique(np.nonzero(keys == T)[0] // PC.CHUNK)) >= 2


@pytest.mark.parametrize('b', [0, 1, 2, 3])
def test_byte_cases_are_decided_by_one_radix_pass(b):
    """the keys agree outside byte b, so the pass of byte b alone narrows the candidates: every pass before it keeps them all,
    and the k-th key differs from its neighbours in the sorted order first (from the top) in byte b"""
    for plane in (100, 2049, 16384):
        keys = PC.topk_keys('byte%d' % b, plane)
        mask = np.uint32(0xff << (8 * b))
        assert len(np.unique(keys & ~mask)) == 1 and len(np.unique(keys & mask)) > 1
        k = plane // 3
        T, _, entered = PC.select_threshold(keys, k)
        p = 3 - b                                                                   # pass index of byte b
        assert entered[:p + 1] == [plane] * (p + 1) and (p == 3 or entered[p + 1] < plane)
        assert entered[p + 1:] == [int((keys == T).sum())] * (3 - p)
        vals = np.unique(keys)
        at = int(np.searchsorted(vals, T))
        for nbr in vals[max(0, at - 1):at + 2]:
            if nbr != T:
                diff = int(nbr) ^ int(T)
                assert diff.bit_length() - 1 >> 3 == b


def test_batch_images_have_different_thresholds():
    for plane in PC.TOPK_PLANES[1:]:
        dists, keys = PC.topk_batch_keys(plane)
        k = min(8192, plane) if plane > 8192 else max(1, plane // 2)
        assert len({PC.select_threshold(row, k)[0] for row in keys}) == 3, (plane, dists)


# ---- the CPU model of the select ----
@pytest.mark.parametrize('dist,plane', PC.topk_cases(), ids=lambda v: str(v))
def test_select_model_equals_stable_argsort(dist, plane):
    keys = PC.topk_keys(dist, plane)
    for k in PC.topk_ks(dist, keys):
        got = PC.select_model(keys, k)
        np.testing.assert_array_equal(got, PC.topk_ref(keys, k)[0], err_msg=f'{dist} plane {plane} k {k}')
        assert len(np.unique(got)) == k


def test_select_model_on_the_batches():
    for plane in PC.TOPK_PLANES[1:]:
        _, keys = PC.topk_batch_keys(plane)
        k = max(1, min(8192, plane - 1))
        want = PC.topk_ref(keys, k)
        for n in range(3):
            np.testing.assert_array_equal(PC.select_model(keys[n], k), want[n])


# ---- branch proofs: up-sampling, sampling, point head ----
def test_upsample_shapes_reach_the_grid_stride_loop_and_the_odd_maps():
    outs = [4 * n * h * w for n, c, h, w in PC.UPSAMPLE_SHAPES]
    assert max(outs) == 1081600 > PC.GRID_CAP and sorted(outs)[-2] < PC.GRID_CAP
    assert any(h == 1 and w == 1 for _, _, h, w in PC.UPSAMPLE_SHAPES) and any(h == 1 and w > 1 for _, _, h, w in PC.UPSAMPLE_SHAPES)
    assert any(h % 2 and w % 2 and c > 1 for _, c, h, w in PC.UPSAMPLE_SHAPES)
    for shape in PC.UPSAMPLE_SHAPES:
        if shape[1] > 1:
            v = PC.upsample_ref(PC.upsample_input('tied', shape)).astype(np.float32)
            s = np.sort(v, axis=1)
            top_tie = s[:, -1] == s[:, -2]
            assert top_tie.any() and not top_tie.all()                              # ties among the two largest classes, and none
            assert (np.argmax(v, axis=1)[top_tie] == 0).any()                       # among them the lifted pair of classes 0, 1
            assert (PC.keys_ref(v)[top_tie.reshape(len(v), -1)] == 0).all()
    x = PC.upsample_input('const', (2, 4, 6, 10))
    assert (x == x[:, :, :1, :1]).all()


@pytest.mark.parametrize('hw', [(12, 20), (8, 8), (48, 80)])
def test_index_lists_contain_corners_and_borders(hw):
    H2, W2 = hw
    corners = {0, W2 - 1, (H2 - 1) * W2, H2 * W2 - 1}
    for idx in (PC.all_cells(2, H2, W2), PC.subset_cells(2, H2, W2, 40, seed=3)):
        for row in idx:
            assert len(np.unique(row)) == len(row) and row.min() >= 0 and row.max() < H2 * W2
            assert corners <= set(row.tolist())
            y, x = row // W2, row % W2
            inner = (y > 0) & (y < H2 - 1) & (x > 0) & (x < W2 - 1)
            assert ((y == 0) & (x > 0) & (x < W2 - 1)).any() and ((y == H2 - 1) & (x > 0) & (x < W2 - 1)).any()
            assert ((x == 0) & (y > 0) & (y < H2 - 1)).any() and ((x == W2 - 1) & (y > 0) & (y < H2 - 1)).any() and inner.any()
    assert not np.array_equal(PC.all_cells(1, H2, W2)[0], np.arange(H2 * W2))       # shuffled


def test_border_samples_need_the_zero_padding():
    """at the x2 grid the corner cell's sample lies at -0.25: its left and upper taps are outside the map"""
    H2, W2, fh, fw = 12, 20, 6, 10
    c = PC.point_coords(np.array([[0, H2 * W2 - 1]]), H2, W2).numpy()[0]
    sx, sy = c[:, 0] * fw - 0.5, c[:, 1] * fh - 0.5
    assert np.floor(sx[0]) == -1 and np.floor(sy[0]) == -1 and np.floor(sx[1]) + 1 == fw and np.floor(sy[1]) + 1 == fh
    ones = np.ones((1, 1, fh, fw))
    got = PC.point_sample_ref(ones, PC.point_coords(np.array([[0, 1, W2 + 1]]), H2, W2))[0, 0]
    np.testing.assert_allclose(got, [0.75 * 0.75, 0.75, 1.0], rtol=1e-6)


def test_head_cases_reach_their_branches():
    tiles = {PC.head_case_id(c): PC.head_tiles(c[4], c[5]) for c in PC.HEAD_CASES}
    pts = sorted({c[4] * c[5] for c in PC.HEAD_CASES})
    assert pts == [100, 256, 257, 3 * 8192, 9 * 8192]
    assert 100 % PC.TILE != 0 and 257 % PC.TILE == 1                                # dead rows in the last tile
    assert PC.head_tiles(9, 8192) == 288 > PC.HEAD_GRID and PC.head_tiles(3, 8192) <= PC.HEAD_GRID      # the tile loop runs twice
    for cl in ((256, 320), (128, 192)):
        mine = [c for c in PC.HEAD_CASES if (c[0], c[1]) == cl]
        assert {c[2] for c in mine} == {1, 3, 4} and {c[3] for c in mine} == {1, 3, 8}
        assert {c[4] * c[5] for c in mine} >= {100, 257, 3 * 8192, 9 * 8192}
        assert all(c[1] == PC.ld_of(c[0], c[3]) for c in mine)
    assert len(tiles) == len(PC.HEAD_CASES)
    for c in PC.HEAD_CASES:
        assert c[5] <= c[6] * c[7] * c[8] * c[8]                                    # P distinct cells fit the grid


# ---- agreement with the oracle on tie-free inputs ----
def test_keys_and_upsampling_equal_the_oracle():
    import torch.nn.functional as F
    om = _oracle()
    for shape in [(2, 1, 5, 7), (2, 4, 6, 10)]:
        x = PC.upsample_input('gauss', shape)
        up32 = F.interpolate(torch.from_numpy(x), scale_factor=2.0, mode='bilinear', align_corners=False)
        ref = PC.upsample_ref(x)
        assert np.abs(up32.numpy() - ref).max() <= PC.upsample_bound(x)
        unc = om.calculate_uncertainty(torch.from_numpy(ref)).numpy()
        np.testing.assert_array_equal(-unc.reshape(shape[0], -1), PC.keys_ref(ref))


def test_selection_equals_torch_topk_on_tie_free_keys():
    om = _oracle()
    rng = np.random.default_rng(5)
    H, W = 40, 60
    keys = rng.permutation(3 * H * W).astype(np.float32).reshape(3, H * W) / 7.0     # distinct per image
    for k in (1, 100, H * W - 1, H * W):
        idx, coords = om.uncertain_points_on_grid(torch.from_numpy(-keys).view(3, 1, H, W), k)
        np.testing.assert_array_equal(np.sort(idx.numpy(), axis=1), PC.topk_ref(keys.view(np.uint32), k))
        np.testing.assert_array_equal(coords.numpy(), PC.point_coords(idx.numpy(), H, W).numpy())


def test_point_rows_equal_the_oracle_point_sample():
    om = _oracle()
    N, fh, fw, C, ncls, H2, W2 = 2, 6, 10, 8, 3, 24, 40
    feat, coarse = PC.sample_input(N, fh, fw, C, C + 8, ncls, seed=2, half=False)
    idx = PC.all_cells(N, H2, W2, seed=1)
    ld = PC.ld_of(C, ncls)
    rows = PC.point_rows_ref(feat, C, coarse, idx, H2, W2, ld)
    coords = PC.point_coords(idx, H2, W2)
    fine = om.point_sample(torch.from_numpy(feat[..., :C]).permute(0, 3, 1, 2).contiguous(), coords)
    crs = om.point_sample(torch.from_numpy(coarse), coords)
    got = torch.cat([fine, crs], dim=1).permute(0, 2, 1).reshape(N * idx.shape[1], C + ncls).numpy()
    bound = PC.sample_bound(rows, feat, C, coarse, half=False)
    assert (np.abs(got - rows[:, :C + ncls]) <= bound[:, :C + ncls]).all()
    assert (rows[:, C + ncls:] == 0).all() and (bound[:, C + ncls:] == 0).all()
    assert np.abs(got - rows[:, :C + ncls]).max() > 0                                # fp32 against float64: not the same numbers


def test_point_head_reference_equals_the_oracle():
    om = _oracle()
    C, ncls, num_fc, R = 16, 3, 3, 50
    rng = np.random.default_rng(9)
    fc_w = [(rng.standard_normal((C, C + ncls)) / 4).astype(np.float32) for _ in range(num_fc)]
    fc_b = [(0.1 * rng.standard_normal(C)).astype(np.float32) for _ in range(num_fc)]
    pw, pb = (rng.standard_normal((ncls, C + ncls)) / 4).astype(np.float32), rng.standard_normal(ncls).astype(np.float32)
    fine, coarse = rng.standard_normal((R, C)).astype(np.float32), rng.standard_normal((R, ncls)).astype(np.float32)
    P = {f'semantic_pr.point_head.fc_layers.{k}.0': (fc_w[k][:, :, None], fc_b[k]) for k in range(num_fc)}
    P['semantic_pr.point_head.predictor'] = (pw[:, :, None], pb)
    got = om.point_head_forward(P, torch.from_numpy(fine.T[None].copy()), torch.from_numpy(coarse.T[None].copy()), num_fc)[0].numpy().T
    ref, bound = PC.point_head_ref(fine, coarse, fc_w, fc_b, pw, pb)
    assert got.shape == ref.shape == (R, ncls)
    assert (np.abs(got - ref) <= bound).all() and bound.max() < 1e-3
    one, b1 = PC.predictor_ref(np.concatenate([fine, coarse], axis=1), pw, pb)
    ref0, _ = PC.point_head_ref(fine, coarse, [], [], pw, pb)
    np.testing.assert_array_equal(one, ref0)


def test_scatter_reference_touches_only_the_indexed_cells():
    tgt = np.arange(2 * 3 * 10, dtype=np.float64).reshape(2, 3, 10)
    idx = np.array([[9, 0], [4, 5]])
    out = PC.scatter_ref(tgt, -np.arange(1, 13, dtype=np.float64).reshape(4, 3), idx)
    changed = out != tgt
    assert changed.sum() == 12 and changed[0][:, [0, 9]].all() and changed[1][:, [4, 5]].all()
    np.testing.assert_array_equal(out[0][:, 9], [-1, -2, -3])
    np.testing.assert_array_equal(out[1][:, 5], [-10, -11, -12])
