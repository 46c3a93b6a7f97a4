"""On the CPU: every shape of tests/glue_ab_case.py reaches the boundary it is named for, by plain models of the launchers'
decisions in their own fp32 arithmetic, and the ownership claims of the two rewritten kernels hold on every shape they take."""
import numpy as np

import glue_ab_case as GC


def test_stem_shapes_reach_the_tile_loop_and_every_border():
    partial_x = partial_y = False
    most_tiles, sides = 0, set()
    for shape in GC.STEM_SHAPES:
        H, W, vh, vw = shape
        assert H % 4 == 0 and W % 4 == 0 and 1 <= vh <= H and 1 <= vw <= W
        ty, tx = GC.stem_tiles(shape)
        partial_y |= (H // 4) % GC.STEM_PT != 0
        partial_x |= (W // 4) % GC.STEM_PT != 0
        most_tiles = max(most_tiles, GC.N * ty * tx)
        sides |= GC.stem_patch_sides(shape)
    assert partial_x and partial_y
    assert most_tiles // 2 >= 3          # with two workgroups each still takes three tiles or more
    assert sides == {'top', 'left', 'bottom', 'right'}
    assert any(s[2] == 1 for s in GC.STEM_SHAPES)
    assert GC.STEM_GRIDS == ('1', '2', None)
    # a single-tile shape: with the grid unset (and with it 1 or 2 at N = 2) no workgroup has a successor to fetch
    assert GC.stem_tiles(GC.STEM_SHAPES[0]) == (1, 1)


def test_up4_cases_reach_the_form_they_are_named_for():
    for name, (shape, in_pad, out_pad, takes) in GC.UP4_CASES.items():
        assert GC.takes_4x4(*shape) == takes, name
        assert in_pad % 8 == 0 and out_pad % 8 == 0 and shape[0] % 8 == 0, name


def test_up4_each_condition_has_a_shape_on_either_side():
    only = {}
    for name, (shape, _, _, _) in GC.UP4_CASES.items():
        cond = GC.up4_conditions(*shape)
        if sum(cond) == 4:
            only[cond.index(False)] = name
    assert sorted(only) == [0, 1, 2, 3, 4], f'conditions failing alone: {only}'
    C = GC.UP4_CASES
    assert C['W_equals_4ppb'][0][4] == 4 * (256 // (C['W_equals_4ppb'][0][0] // 8))
    assert C['W_below_4ppb'][0][4] == C['W_equals_4ppb'][0][4] - 4
    for inside, outside, axis in (('three_sy_inside', 'three_sy_outside', 0), ('three_sx_inside', 'three_sx_outside', 1)):
        si = GC.scales(*C[inside][0][1:])[axis]
        so = GC.scales(*C[outside][0][1:])[axis]
        # (n - 1) / (3 (n - 1) + 1) and 1 / 3: the nearest ratios of small integers on either side of 1 / 3
        assert np.float32(3) * si < 1 <= np.float32(3) * so and si > 0.28, (inside, outside)
    # the legacy form takes what fails only in H (the two forms differ in the kernel that runs, not in the result)
    assert GC.takes_1x4(*C['H_mod_4_outside'][0]) and GC.takes_1x4(*C['three_sy_outside'][0])


def test_up4_layouts():
    shape, in_pad, out_pad, _ = GC.UP4_CASES['concat_slice']
    assert shape[0] + in_pad == 264 and shape[0] + out_pad == 320
    assert any(out_pad for _, _, out_pad, _ in GC.UP4_CASES.values()) and any(not out_pad for _, _, out_pad, _ in GC.UP4_CASES.values())
    # more than one workgroup in x and in y, a ragged last segment, idle threads
    C_, h, w, H, W = GC.UP4_CASES['ragged_segment'][0]
    ppb = 256 // (C_ // 8)
    assert (W // 4) % ppb != 0 and W // 4 > ppb and H // 4 > 1
    C_, h, w, H, W = GC.UP4_CASES['decoder_ratio'][0]
    assert (W // 4) // (256 // (C_ // 8)) >= 2 and (h, H) == (16, 64)
    assert 256 % (GC.UP4_CASES['idle_threads'][0][0] // 8) != 0


def test_up4_blocks_span_three_sources():
    """a 4 x 4 block's sources are rows ya .. ya + 2 and columns xa .. xa + 2: every output's x0 and y0 is at most one past the
    block's first, in the kernel's fp32 coordinates, on every shape the 4 x 4 form takes"""
    for name, (shape, _, _, takes) in GC.UP4_CASES.items():
        if not takes:
            continue
        _, h, w, H, W = shape
        sy, sx = GC.scales(h, w, H, W)
        assert GC.block_spread(sy, H) <= 1 and GC.block_spread(sx, W) <= 1, name
        assert GC.source_index(sy, H).max() <= h - 1 and GC.source_index(sx, W).max() <= w - 1, name
    # and the claim fails just outside: 1 / 3 reaches two past the first
    assert GC.block_spread(np.float32(1) / np.float32(3), 16) == 1 and GC.block_spread(np.float32(0.4), 64) == 2


def test_up2x_shapes_reach_every_store_width_and_tail():
    widths, tails = set(), set()
    for shape in GC.UP2X_SHAPES:
        for off in GC.UP2X_OFFSETS:
            widths.add(GC.up2x_store_width(shape[3], off))
        groups, tail = GC.up2x_groups(shape)
        tails.add(tail)
        assert groups * 4 >= shape[0] * 4 * shape[2] * shape[3]
    assert widths == {1, 2, 4} and tails == {2, 4}
    assert {s[3] for s in GC.UP2X_SHAPES} >= {1, 2, 3, 5, 8} and {s[2] for s in GC.UP2X_SHAPES} >= {1, 3}
    assert {s[1] for s in GC.UP2X_SHAPES} >= {1, 2, 8}
    groups, _ = GC.up2x_groups((GC.N, 2, 260, 260))
    assert groups % 256 != 0 and groups > 256           # several workgroups and a ragged last one


def test_up2x_four_outputs_read_four_columns():
    """outputs 4q .. 4q + 3 of a row take x0, x1 from columns 2q - 1 .. 2q + 2 clamped into the row, as the kernel selects them"""
    for w in (1, 2, 3, 5, 8, 260):
        W = 2 * w
        for q in range((W + 3) // 4):
            cols = [min(max(2 * q - 1 + k, 0), w - 1) for k in range(4)]
            pick = [(1, 2) if q == 0 else (0, 1), (1, 2), (1, 2), (2, 3)]
            for j in range(min(4, W - 4 * q)):
                fx = max(np.float32(0.5) * (np.float32(4 * q + j) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
                x0 = int(fx)
                x1 = x0 + (1 if x0 < w - 1 else 0)
                assert (cols[pick[j][0]], cols[pick[j][1]]) == (x0, x1), (w, q, j)


def test_inputs_are_what_the_docstrings_say():
    x = GC.up2x_input((2, 2, 3, 8), 1)
    assert x.dtype == np.float32 and (x == 0.5).sum() > 4 and np.abs(x).max() > 100
    assert GC.up4_input((16, 3, 5, 12, 20), 2).shape == (GC.N, 3, 5, 16)
