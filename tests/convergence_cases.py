"""Inputs for the fold of the convergence estimate's per-block records (k_converge_summary, csrc/pt_converge.hip), shared by
tests/test_convergence_reference.py (what the inputs are, without a device) and tests/test_gpu_convergence.py (the device against the
reference on them).  No test lives in this file.

k_converge_tiles writes one record per 16 tiles (tile index = tile row * tiles per row + tile column); one block of 256 threads folds
them: thread j takes the records j, j + 256, ..., then seven LDS stages fold thread j + s into thread j, s = 128 .. 1.  520 x 512 is
65 x 64 tiles = 4160 tiles = 260 records: every thread holds one, threads 0 .. 3 two."""
import numpy as np

F = np.float32
W, H = 520, 512
TILES_X, TILES_Y = (W + 7) // 8, (H + 7) // 8
RECORD_TILES = 16
RECORDS = (TILES_X * TILES_Y + RECORD_TILES - 1) // RECORD_TILES
FOLD_WIDTH = 256
# one record of the upper half of each LDS stage (1, 2, .. 128: folded at stage s = p), the last thread, and the second round of the
# strided loop (256: thread 0 again; 259: the last record)
PLACED = (1, 2, 4, 8, 16, 32, 64, 128, 255, 256, 259)
# (threshold, min_frames): the placed tile's per-texel mean is above 3 * 0.06^2 = 0.0108 and the base's 0.0074 below; its texel's n = 15
# is young at min_frames 16 and not at 0, where the tile is above by its mean alone
PLACED_PARAMS = ((0.06, 16), (0.06, 0))


def base():
    """(accumulation, moments): means 0.5, M2 = 3, n = 16 everywhere -- r = (9 / 240) / 1.5^4 in every texel"""
    acc = np.ones((H, W, 4), F)
    acc[..., :3] = F(0.5)
    mo = np.empty((H, W, 4), F)
    mo[...] = (3, 3, 3, 16)
    return acc, mo


def placed_texel(p):
    """(y, x) of the one texel that differs from base(): in tile 16 p + (p + p / 16) % 16 (the places in a record are the waves and
    rounds of k_converge_tiles), at another lane of the tile for every p"""
    t = RECORD_TILES * p + (p + p // RECORD_TILES) % RECORD_TILES
    lane = (5 * p + p // RECORD_TILES + 3) % 64
    return (t // TILES_X) * 8 + lane // 8, (t % TILES_X) * 8 + lane % 8


def placed(p):
    """base() with one texel of record p holding M2 = 300 at n = 15: the largest per-texel error of the image, the smallest n, and the
    only tile whose per-texel mean is above 0.0108"""
    acc, mo = base()
    y, x = placed_texel(p)
    mo[y, x] = (300, 300, 300, 15)
    return acc, mo
