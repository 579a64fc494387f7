"""The tile lists of tests/tile_geometries.py on the CPU: each is an exact partition of its frame made of blocks the API accepts,
each cuts work units of every pixel-block shape (so that the GPU cases on them are not vacuous), every row of the dispatch
matrix keeps its kernel names on each of them (so that the GPU cases can assert the row's own name), and the staged frames of
dispatch_cases.STAGED_BATCHES do take more than one tile batch and more than one sample chunk."""
import numpy as np
import pytest

from tests import dispatch_cases as dc
from tests import plan_probe as pp
from tests import tile_geometries as tg

FRAMES = [(dc.RES, dc.TS), (dc.AOV_RES, dc.AOV_TS)]
LISTS = [(name, res, ts) for name in tg.GEOMETRIES for res, ts in FRAMES] + [("ragged26", dc.RES, dc.TS)]


@pytest.mark.parametrize("name, res, ts", LISTS)
def test_exact_partition_of_blocks_the_api_accepts(name, res, ts):
    tile_size, blocks = tg.geometry(name, res, ts)
    cover = np.zeros((res[1], res[0]), np.int32)
    for b in blocks:
        assert b.min_x < b.max_x and b.min_y < b.max_y, "non-empty"
        assert b.width() <= tile_size and b.height() <= tile_size
        assert b.max_x <= res[0] and b.max_y <= res[1]
        cover[b.min_y:b.max_y, b.min_x:b.max_x] += 1
    assert np.all(cover == 1), "every pixel exactly once"
    assert sum(b.area() for b in blocks) == res[0] * res[1]
    own = tg.owned(blocks, tile_size)
    assert own.sum() == res[0] * res[1]


def test_the_lists_are_what_the_module_says():
    ts, b = tg.geometry("grid13", dc.RES, dc.TS)
    assert (ts, len(b)) == (13, 6 * 4) and (b[5].width(), b[-1].height()) == (7, 1)
    ts, b = tg.geometry("grid13", dc.AOV_RES, dc.AOV_TS)
    assert (ts, len(b)) == (13, 2 * 2) and (b[1].width(), b[-1].height()) == (11, 3)
    assert [len(tg.geometry("grid1", res, ts)[1]) for res, ts in FRAMES] == [2880, 384]
    ts, b = tg.geometry("ragged", dc.RES, dc.TS)
    assert (ts, len(b)) == (32, 24)
    assert {x.width() for x in b} == {1, 3, 5, 31} and {x.height() for x in b} == {1, 3, 7, 29}
    assert sorted((x.width(), x.height()) for x in b).count((31, 29)) == 2
    ts, b = tg.geometry("ragged", dc.AOV_RES, dc.AOV_TS)
    assert (ts, len(b)) == (16, 12)
    # the hand-out order is the fixed permutation of the row-major products, not the products themselves
    xs, ys = tg.RAGGED_CUTS[dc.RES]
    cells = [(x0, y0, x1, y1) for y0, y1 in zip(ys, ys[1:]) for x0, x1 in zip(xs, xs[1:])]
    got = [(x.min_x, x.min_y, x.max_x, x.max_y) for x in tg.ragged(dc.RES)]
    assert got == [cells[7 * i % 24] for i in range(24)] and got != cells and sorted(got) == sorted(cells)
    ts, b = tg.geometry("ragged26", dc.RES, dc.TS)
    assert (ts, len(b)) == (64, dc.STAGED_TILES)
    assert sorted((x.width(), x.height()) for x in b).count((31, 14)) == 2 and max(x.area() for x in b) == 31 * 15
    # the default geometry is the grid mp_tile_ordering gives the matrix today
    ts, b = tg.geometry("grid", dc.RES, dc.TS)
    assert (ts, len(b)) == (32, 6) and [(x.width(), x.height()) for x in b] == [(32, 32), (32, 32), (8, 32), (32, 8), (32, 8), (8, 8)]


def test_units_walk():
    """units(): anchored at the tile's min, ceil(ts / BW) x ceil(ts / BH) of them, whatever the block's extent"""
    from minipath_amd.screen_block import ScreenBlock

    b = ScreenBlock(9, 11, 14, 12)  # 5 x 1 in a slot of 13
    u = tg.units(b, 13, 4, 2)
    assert len(u) == 4 * 7 and u[:4] == [4, 1, 0, 0] and sum(u) == 5 and not any(u[4:])
    assert tg.partial_units([b], 13, 4, 2) == 2
    assert tg.units(ScreenBlock(0, 0, 13, 13), 13, 8, 8) == [64, 40, 40, 25]


@pytest.mark.parametrize("bw, bh", tg.BLOCK_SHAPES)
def test_units_are_cut_by_their_tiles(bw, bh):
    """what makes the GPU cases non-vacuous: units with some but not all pixels inside their tile, for every block shape; the
    matrix's own grid has none"""
    for res, ts in FRAMES:
        tile_size, blocks = tg.geometry("grid", res, ts)
        assert tg.partial_units(blocks, tile_size, bw, bh) == 0
        for name in ("grid13", "ragged"):
            tile_size, blocks = tg.geometry(name, res, ts)
            assert tg.partial_units(blocks, tile_size, bw, bh) > 0, (name, res)
        # one tile per pixel: every live unit holds exactly one pixel
        tile_size, blocks = tg.geometry("grid1", res, ts)
        assert all(tg.units(b, tile_size, bw, bh) == [1] for b in blocks[:: max(1, len(blocks) // 17)])
    tile_size, blocks = tg.geometry("ragged26", dc.RES, dc.TS)
    assert tg.partial_units(blocks, tile_size, 2, 2) > 0  # wf_camera_kernel's block


def _tiling(name, row):
    res, ts = (dc.AOV_RES, dc.AOV_TS) if row["api"] == "aov" else (dc.RES, dc.TS)
    tile_size, blocks = tg.geometry(name, res, ts)
    return tile_size, len(blocks)


@pytest.mark.parametrize("geometry", tg.GEOMETRIES)
def test_every_row_keeps_its_names(geometry):
    """the selection rules read the tile size and count (small launches); none of the geometries moves a row to another kernel,
    and every launch stays small: units * 16 < CUs * 32 * 24 = 12 288 units at 256 CUs"""
    rows = [k for k, row in dc.CASES.items() if row["api"] in ("render", "paths", "wf", "aov")]
    assert len(rows) > 70 and set(dc.tiled_rows()) <= set(rows)
    for name in rows:
        row = dc.CASES[name]
        tiling = _tiling(geometry, row)
        assert tiling[1] * ((tiling[0] + 7) // 8) ** 2 < 12288
        assert pp.row_names(row, tiling=tiling) == pp.row_names(row) == {name, *row["also"]}, name
    for guard, (expected, row) in dc.GATES.items():
        assert pp.row_names(row, tiling=_tiling(geometry, row)) == {expected}, guard


@pytest.mark.parametrize("geometry", ("grid13", "ragged"))
@pytest.mark.parametrize("which", list(dc.RAGGED))
def test_ragged_passes_keep_their_names(which, geometry):
    row, passes = dc.RAGGED[which]
    begin = 0
    for n, expected in passes:
        assert pp.row_names(row, passes=(begin, n), tiling=_tiling(geometry, row)) == {expected}, (begin, n)
        begin += n


def test_the_staged_rows_cover_every_configuration():
    cfg = dc.wf_configurations()
    assert len(cfg) == 8 and sum(len(v) for v in cfg.values()) == 13
    for first, keys in cfg.items():
        for k in keys:  # one run per configuration reports every name of the rows that share it
            assert {k, *dc.CASES[k]["also"]} == {first, *dc.CASES[first]["also"]}


def _staged_plan(scene, spp, begin, count, chunked):
    out = pp.plan(pp.STAGED, pp.launch(dc.scene_facts(scene), dc.STAGED_TILES, tg.STAGED_TS, spp, (begin, count), max_depth=dc.DEPTH,
                                      chunked=1 if chunked else 0))
    assert out.rc == 0, out.error
    return out


@pytest.mark.parametrize("case", list(dc.STAGED_BATCHES))
def test_staged_frames_take_several_batches_and_chunks(case):
    """must fail if a change to the batch rule makes these frames single-batch again"""
    scene, spp, passes, chunked = dc.STAGED_BATCHES[case]
    assert sum(passes) == spp and len(tg.geometry("ragged26", dc.RES, dc.TS)[1]) == dc.STAGED_TILES
    # the frame as one launch: chunks of 64 samples, batches of 8, 8, 8 and 2 tiles
    o = _staged_plan(scene, spp, 0, spp, chunked)
    assert o.sc == 64 and o.tb == 8 < dc.STAGED_TILES and dc.STAGED_TILES % o.tb != 0 and spp % o.sc != 0
    assert o.ws_bytes < 256 << 20
    assert {pp.name(o), pp.name(o, "vertex"), pp.name(o, "trace"), "wf_scan_kernel", "wf_scatter_kernel", "wf_accumulate_kernel"} == dc.staged_names(scene)
    begin = 0
    for n in passes:  # every pass of the case is several batches with a shorter last one
        o = _staged_plan(scene, spp, begin, n, chunked)
        assert o.sc == min(n, 64) and 1 <= o.tb < dc.STAGED_TILES and dc.STAGED_TILES % o.tb != 0, (begin, n, o.tb)
        assert o.ws_bytes < 256 << 20
        begin += n
    if len(passes) == 1 or chunked:
        assert any(n > 64 and n % 64 for n in passes), "a pass of several sample chunks with a shorter last one"
    if chunked:  # the flush of the first 256-sample chunk falls inside the second pass, inside one of its sample chunks
        assert passes[0] < 256 < passes[0] + passes[1] and (256 - passes[0]) % 64 != 0
        assert o.nchan == 1


def test_the_matrix_frames_of_today_are_single_batch():
    """why STAGED_BATCHES exists: every staged row of the matrix, on every geometry, is one tile batch"""
    for first in dc.wf_configurations():
        row = dc.CASES[first]
        for geometry in ("grid",) + tg.GEOMETRIES:
            ts, n = _tiling(geometry, row)
            o = pp.plan(pp.STAGED, pp.row_input(row, tiling=(ts, n)))
            assert o.rc == 0 and o.tb == n
