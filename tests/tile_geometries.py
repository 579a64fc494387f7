"""Tile lists that cut the kernels' pixel blocks, as plain data (importable without a GPU).  mp_render_tiles_device accepts any
non-empty block up to tile_size anywhere in the frame; per-rank shards and adaptive sampling hand it such lists.  Every list here
is an exact partition of its frame, so every pixel is rendered once and the untiled frame is the oracle's, whatever the tiling:
the oracle frames of the dispatch matrix serve every geometry.

  grid    the matrix's own: the row-major grid at the matrix's tile size (the clipped column and row are 8 pixels: whole units)
  grid13  the row-major grid at tile_size 13: on 72 x 40 the last column is 7 wide and the last row 1 high, on 24 x 16 11 and 3
  grid1   tile_size 1, one tile per pixel: every unit of every block shape but 1 x 1 holds exactly one live pixel
  ragged  the matrix's tile size, the products of unaligned column and row cuts (blocks of widths 1, 3, 5, 31 and heights 1, 3,
          7, 29 on the main frame), handed out in the order i -> 7 i mod n
  ragged26  staged pipeline only, tile_size 64: the main frame's ragged blocks with each of the two 31 x 29 blocks split at
          y = 25: 26 blocks in 64 x 64 slots, more than one tile batch of the staged pipeline at 64 samples or more

The kernels lay their work units out per SLOT, not per block: anchored at the tile's min corner, ceil(ts / BW) x ceil(ts / BH)
units of BW x BH pixels, whatever the block's extent (units())."""
from minipath_amd.screen_block import ScreenBlock

# BW x BH of render_tiles_packet_kernel for 1, 2, 4, 8, 16 and 32 samples in flight (64 in flight: 1 x 1, never partial); 4 x 2 is
# also render_tiles_packet2_kernel's and the pooled path kernel's, 2 x 2 wf_camera_kernel's
BLOCK_SHAPES = ((8, 8), (8, 4), (4, 4), (4, 2), (2, 2), (2, 1))
RAGGED_CUTS = {
    (72, 40): ((0, 1, 4, 9, 40, 41, 72), (0, 3, 4, 11, 40)),
    (24, 16): ((0, 1, 4, 9, 24), (0, 3, 4, 16)),
}
GEOMETRIES = ("grid13", "grid1", "ragged")  # what every render / paths / wf / aov row of the matrix runs on besides "grid"
STAGED_TS = 64


def grid(res, ts):
    """the row-major grid (mp_tile_ordering without a shuffle), in plain Python"""
    return [ScreenBlock(x, y, min(x + ts, res[0]), min(y + ts, res[1])) for y in range(0, res[1], ts) for x in range(0, res[0], ts)]


def ragged(res):
    xs, ys = RAGGED_CUTS[tuple(res)]
    cells = [ScreenBlock(x0, y0, x1, y1) for y0, y1 in zip(ys, ys[1:]) for x0, x1 in zip(xs, xs[1:])]
    n = len(cells)
    return [cells[7 * i % n] for i in range(n)]


def ragged26(res):
    out = []
    for b in ragged(res):
        if (b.width(), b.height()) == (31, 29):
            out += [ScreenBlock(b.min_x, b.min_y, b.max_x, 25), ScreenBlock(b.min_x, 25, b.max_x, b.max_y)]
        else:
            out.append(b)
    return out


def geometry(name, res, ts):
    """(tile_size, [ScreenBlock...]) of geometry `name` for a frame of `res` whose matrix case runs at tile size `ts`"""
    if name == "grid":
        return ts, grid(res, ts)
    if name == "grid13":
        return 13, grid(res, 13)
    if name == "grid1":
        return 1, grid(res, 1)
    if name == "ragged":
        return ts, ragged(res)
    if name == "ragged26":
        return STAGED_TS, ragged26(res)
    raise KeyError(name)


def units(block, ts, bw, bh):
    """live pixels of every work unit of the block's slot, as the kernels lay the units out"""
    out = []
    for uy in range(0, ts, bh):
        for ux in range(0, ts, bw):
            out.append(max(0, min(ux + bw, block.width()) - ux) * max(0, min(uy + bh, block.height()) - uy))
    return out


def partial_units(blocks, ts, bw, bh):
    """how many units hold some but not all of their pixels inside their tile"""
    return sum(1 for b in blocks for live in units(b, ts, bw, bh) if 0 < live < bw * bh)


def owned(blocks, ts):
    """[n, ts, ts] bool: the pixels of every slot its block covers"""
    import numpy as np

    own = np.zeros((len(blocks), ts, ts), bool)
    for i, b in enumerate(blocks):
        own[i, :b.height(), :b.width()] = True
    return own
