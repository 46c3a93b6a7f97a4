"""Shapes of the A/B tests of the rewritten glue kernels (tests/test_gpu_glue_ab.py): the second form of the fused stem against
the first (EMP_STEM_POOL_LEGACY=1), the 4 x 4 form of the four-pixel bilinear kernel against its 1 x 4 form
(EMP_BILINEAR_UP4_LEGACY=1) and the four-output PointRend up-sampler against the one-output kernel (EMP_PR_UP2X_LEGACY=1).  All comparisons are exact, so this file holds no tolerance: it holds the shapes, the reason for each,
and plain models of the launchers' decisions that tests/test_glue_ab_case_host.py runs on the CPU to show that every shape
reaches the boundary it is named for.

Stem (H, W, vh, vw): padded and valid size, N = 2, uint8 / uint16 / float images.  A workgroup pools 8 x 8 outputs per tile from a
40 x 40 input patch that starts five pixels before the tile, and walks the tiles blockIdx.x, blockIdx.x + grid, ...; the second
form fetches the next tile's patch while it works on this one.  EMP_STEM_POOL_GRID = 1 makes one workgroup take every tile in
turn (each with a successor but the last), 2 makes two alternate, unset gives every tile its own workgroup (no successor at
all).  16 x 16 is one partial tile; 48 x 80 is 2 x 3 tiles per image, partial in x and in y; 36 x 68 with 33 x 65 valid has one
pooled pixel in the second tile both ways and a valid region that ends inside the last patch; 48 x 64 with 37 x 50 valid ends
well inside; vh = 1 is a single image row.

Bilinear (C, h, w, H, W), N = 2.  The 4 x 4 form takes a shape when, with ppb = 256 // (C / 8) blocks per workgroup,
W % 4 == 0, 3 sx < 1, W >= 4 ppb (the 1 x 4 form's conditions) and H % 4 == 0, 3 sy < 1 (its own), sx = (w - 1) / (W - 1) in
fp32.  UP4_CASES names, for each condition, a shape just inside and one just outside; what is outside goes to the one-pixel
kernel (new) or to whichever kernel took it before (legacy), and both must agree bit for bit.  The kernel does not loop: a
workgroup writes one band of four rows x 4 ppb columns, so "more than one block per workgroup" does not exist; 32 x 36 at
C = 256 has two segments per band (the second ragged: one block of eight) and eight bands per image.

PointRend (N, C, h, w): w in {1, 2, 3, 5, 8} x h in {1, 3} x C in {1, 2, 8} with N = 2, and 260 x 260 (1 040 groups of 256
threads plus a ragged one: the grid-size edge of the 520 x 520 case of tests/pointrend_case.py).  Odd w makes W % 4 == 2: 8-byte
stores and a last group of two outputs; w = 1 is one such group per row.  Every shape runs a second time through views that start
one float past a 16-byte boundary: the guarded 4-byte stores."""
import numpy as np

N = 2
GUARD = 64

# ----------------------------------------------------------------------------
# fused stem
# ----------------------------------------------------------------------------
STEM_SHAPES = [(16, 16, 16, 16), (48, 80, 48, 80), (36, 68, 33, 65), (48, 64, 37, 50), (16, 16, 1, 16)]
STEM_GRIDS = ('1', '2', None)      # EMP_STEM_POOL_GRID
STEM_PT, STEM_IP = 8, 40           # pooled tile side, input patch side (csrc/stem.hip)


def stem_tiles(shape):
    """-> (tiles per image in y, in x)"""
    H, W, _, _ = shape
    return -(-(H // 4) // STEM_PT), -(-(W // 4) // STEM_PT)


def stem_patch_sides(shape):
    """which sides of the valid image some tile's patch leaves: {'top', 'left', 'bottom', 'right'}"""
    _, _, vh, vw = shape
    ty, tx = stem_tiles(shape)
    sides = set()
    for t in range(ty):
        y0 = 4 * t * STEM_PT - 5
        sides |= {'top'} if y0 < 0 else set()
        sides |= {'bottom'} if y0 + STEM_IP - 1 >= vh else set()
    for t in range(tx):
        x0 = 4 * t * STEM_PT - 5
        sides |= {'left'} if x0 < 0 else set()
        sides |= {'right'} if x0 + STEM_IP - 1 >= vw else set()
    return sides


# ----------------------------------------------------------------------------
# bilinear, four-pixel kernel
# ----------------------------------------------------------------------------
# name -> ((C, h, w, H, W), in_ld - C, out_ld - C, takes the 4 x 4 form)
UP4_CASES = {
    'concat_slice': ((256, 8, 8, 32, 32), 8, 64, True),          # the network's layout: 256 channels into a 320-wide buffer
    'one_block_per_workgroup': ((2048, 2, 2, 8, 8), 0, 0, True),  # ppb = 1
    'W_equals_4ppb': ((64, 4, 32, 16, 128), 0, 0, True),
    'ragged_segment': ((256, 8, 8, 32, 36), 0, 8, True),
    'idle_threads': ((48, 5, 30, 7, 100), 0, 8, False),           # 42 blocks of 6 channel groups; W < 4 ppb and H % 4 != 0
    'H_mod_4_outside': ((256, 8, 8, 30, 32), 0, 8, False),        # only H % 4 fails: the 1 x 4 form takes it
    'three_sy_inside': ((256, 3, 8, 8, 32), 0, 8, True),          # sy = 2 / 7
    'three_sy_outside': ((256, 2, 8, 4, 32), 0, 8, False),        # sy = 1 / 3: only 3 sy < 1 fails
    'three_sx_inside': ((2048, 3, 3, 8, 8), 0, 0, True),          # sx = sy = 2 / 7
    'three_sx_outside': ((512, 4, 6, 16, 16), 0, 0, False),       # sx = 1 / 3
    'W_below_4ppb': ((64, 4, 31, 16, 124), 0, 0, False),
    'W_mod_4_outside': ((256, 8, 8, 32, 34), 0, 8, False),
    'decoder_ratio': ((64, 16, 72, 64, 288), 8, 16, True),        # the decoder's 64 -> 256 rows; three segments of 32 blocks, the last ragged
}


def scales(h, w, H, W):
    """area_pixel_compute_scale(align_corners=True) in fp32, as the launcher computes it"""
    sy = np.float32(h - 1) / np.float32(H - 1) if H > 1 else np.float32(0)
    sx = np.float32(w - 1) / np.float32(W - 1) if W > 1 else np.float32(0)
    return np.float32(sy), np.float32(sx)


def up4_conditions(C, h, w, H, W):
    """the launcher's five conditions, in its arithmetic: (W % 4, 3 sx < 1, W >= 4 ppb, H % 4, 3 sy < 1)"""
    sy, sx = scales(h, w, H, W)
    ppb = 256 // (C // 8)
    return (W % 4 == 0, bool(np.float32(3) * sx < np.float32(1)), W >= 4 * ppb, H % 4 == 0, bool(np.float32(3) * sy < np.float32(1)))


def takes_4x4(C, h, w, H, W):
    return all(up4_conditions(C, h, w, H, W))


def takes_1x4(C, h, w, H, W):
    return all(up4_conditions(C, h, w, H, W)[:3])


def source_index(scale, o):
    """(int)(scale * (float)o) in fp32"""
    return (np.float32(scale) * np.arange(o, dtype=np.int64).astype(np.float32)).astype(np.int64)


def block_spread(scale, n_out):
    """largest source index of an aligned block of four outputs less the index of its first output"""
    s = source_index(scale, n_out)[:n_out // 4 * 4].reshape(-1, 4)
    return int((s - s[:, :1]).max()) if s.size else 0


def up4_input(shape, seed):
    C, h, w, _, _ = shape
    return np.random.default_rng(seed).standard_normal((N, h, w, C)).astype(np.float16)


# ----------------------------------------------------------------------------
# PointRend x2 up-sampler
# ----------------------------------------------------------------------------
UP2X_SHAPES = [(N, C, h, w) for w in (1, 2, 3, 5, 8) for h in (1, 3) for C in (1, 2, 8)] + [(N, 2, 260, 260)]
UP2X_OFFSETS = (0, 1)          # floats between a 16-byte boundary and the first element of the output and of the keys


def up2x_store_width(w, offset):
    """elements per store of the four-output kernel: the launcher's choice"""
    if offset % 4 == 0 and (2 * w) % 4 == 0:
        return 4
    return 2 if offset % 2 == 0 else 1


def up2x_groups(shape):
    """threads of the four-output kernel and the outputs of the last one of each row"""
    n, _, h, w = shape
    wq = (2 * w + 3) // 4
    return n * 2 * h * wq, 2 * w - 4 * (wq - 1)


def up2x_input(shape, seed):
    """signed logits with ties between classes and between neighbours (keys of exactly 0) and a few large values"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    x[rng.random(shape) < 0.2] = np.float32(0.5)
    x[rng.random(shape) < 0.05] *= np.float32(1e4)
    return x
