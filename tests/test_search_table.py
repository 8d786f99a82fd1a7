"""The compile-time table of the partition search's constants (hl_mbcore.h
kSearchTab): every one of the 41 entries (partitioning j, partition pi,
sub-partition spi) against the geometry restated here -- the partition's
origin and shape (part_x / part_y / sub_x / sub_y, PartGeo), the pass budget,
the raster index of a single-block partition, the four motion-grid cells of
the MV predictor's neighbours A, B, C, D with C's availability in the grid
(nb_motion), and the directional rule of 16x8 / 8x16 partitions -- and the MV
predictor read through the table against the one computed from the
partition's geometry, on random motion grids.  Tolerance: none."""
import ctypes
import random

import pytest

from hl_testlib import emu_lib

# kParts (rdo.c:731-760): num_part, num_sub, sub_w, sub_h, part_w, part_h
PARTS = [(1, 1, 16, 16, 16, 16), (2, 1, 16, 8, 16, 8), (2, 1, 8, 16, 8, 16), (4, 1, 8, 8, 8, 8), (4, 2, 8, 4, 8, 8), (4, 2, 4, 8, 8, 8),
         (4, 4, 4, 4, 8, 8)]
SEARCHES = [(j, pi, spi) for j, p in enumerate(PARTS) for pi in range(p[0]) for spi in range(p[1])]
# a pass of the 512-lane workgroup: 256 (candidate, block) items, at most 32 candidates (kPassItems, kMaxCand)
PASS_ITEMS, MAX_CAND = 256, 32


def _lib():
    lib = emu_lib()
    lib.emu_search_entry.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)]
    lib.emu_search_mvp.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)] * 3
    return lib


def _origin(j, pi, spi):
    """Luma origin and size of the (sub)partition: partitions in raster order
    in the MB, sub-partitions in raster order in their 8x8 partition."""
    num_part, num_sub, sw, sh, pw, ph = PARTS[j]
    per_row = 16 // pw
    x, y = (pi % per_row) * pw, (pi // per_row) * ph
    if num_part == 4:
        sub_row = 8 // sw
        x, y = x + (spi % sub_row) * sw, y + (spi // sub_row) * sh
    return x, y, sw, sh


def _blk_idx(x, y):  # 6.4.3: 8x8 quadrants in raster order, 4x4 blocks in raster order inside
    return 8 * (y // 8) + 4 * (x // 8) + 2 * ((y % 8) // 4) + (x % 8) // 4


def _cells(x, y, w):
    """Cells (row by + 1, column bx + 1 of the 5 x 6 grid) of A (left), B
    (above), C (above right), D (above left) of the partition, and whether C
    lies in the grid: not right of MB C's first column, nor right of the MB
    below its first block row (8.4.1.3.2: not yet decoded)."""
    bx, by, cx = x // 4, y // 4, (x + w) // 4
    c_in = cx <= 4 and not (cx == 4 and by > 0)
    cell = lambda bx_, by_: (by_ + 1) * 6 + bx_ + 1
    return cell(bx - 1, by), cell(bx, by - 1), cell(cx if c_in else bx - 1, by - 1), cell(bx - 1, by - 1), c_in


def test_the_table_has_41_searches():
    assert len(SEARCHES) == 41
    lib, out = _lib(), (ctypes.c_int * 21)()
    n = sum(lib.emu_search_entry(j, pi, spi, out) == 0 and out[12] == 1 for j in range(7) for pi in range(4) for spi in range(4))
    assert n == 41
    assert lib.emu_search_entry(1, 2, 0, out) == 1 and lib.emu_search_entry(4, 0, 2, out) == 1 and lib.emu_search_entry(7, 0, 0, out) == 1


@pytest.mark.parametrize("s", SEARCHES, ids=[f"j{j}_p{pi}_s{spi}" for j, pi, spi in SEARCHES])
def test_entry(s):
    j, pi, spi = s
    lib, out = _lib(), (ctypes.c_int * 21)()
    assert lib.emu_search_entry(j, pi, spi, out) == 0
    e = list(out)
    x, y, w, h = _origin(j, pi, spi)
    nbw, nblk = w // 4, (w // 4) * (h // 4)
    assert e[0:6] == [x, y, w, h, nbw, nblk]
    assert (1 << e[6], 1 << e[7]) == (nbw, nblk)
    assert e[8] == _blk_idx(x, y)
    assert e[9] == min(MAX_CAND, PASS_ITEMS // nblk)  # (every partition chains steps: HL_SPEC_MAX_BLOCKS = 16)
    pw, ph = PARTS[j][4], PARTS[j][5]
    want_dir = {(16, 8, 0): 1, (16, 8, 1): 2, (8, 16, 0): 2, (8, 16, 1): 3}.get((pw, ph, pi), 0)  # B / A / A / C alone when inter-coded
    assert e[10] == want_dir
    a, b, c, d, c_in = _cells(x, y, w)
    assert e[11] == int(c_in) and e[12] == 1
    assert e[13:17] == [a, b, c, d]
    # what nb_motion reads from the partition's geometry: A, B, the third neighbour, and D behind an unavailable C
    assert e[17:19] == [a, b]
    assert e[19] == (c if c_in else d)
    assert e[20] == (d if c_in else -1)
    assert all(0 <= v < 30 for v in e[13:17])


def test_predictor_through_the_table():
    """mvp from the entry against nb_motion + 8.4.1.3 from the geometry, every
    search, grids with every availability pattern of the four neighbours."""
    lib, rng = _lib(), random.Random(8)
    out = (ctypes.c_int * 4)()
    for j, pi, spi in SEARCHES:
        x, y, w, h = _origin(j, pi, spi)
        cells = _cells(x, y, w)[:4]
        for pat in range(81):
            st = [rng.randrange(3) for _ in range(30)]
            for k, cidx in enumerate(cells):
                st[cidx] = (pat // 3 ** k) % 3
            mv = [rng.randrange(-200, 201) for _ in range(60)]
            assert lib.emu_search_mvp(j, pi, spi, (ctypes.c_int * 30)(*st), (ctypes.c_int * 60)(*mv), out) == 0
            assert (out[0], out[1]) == (out[2], out[3]), (j, pi, spi, pat)
