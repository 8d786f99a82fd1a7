// hl_emu_search.hip -- TEST INFRASTRUCTURE.  The translation unit of the host
// emulation (tests/emu/libhl_emu.so): hl_emu_ctl.hip as it is, plus the export
// of the partition search's compile-time table (hl_mbcore.h kSearchTab) beside
// what the search reads through it, so that tests/test_search_table.py checks
// every entry against the geometry restated there.
#include "hl_emu_ctl.hip"

// Entry (j, pi, spi) of kSearchTab as the search uses it.  out[0..12]: the
// PartGeo of part_geo (px, py, pw, ph, nbw, nblk, lbw, lnb, bi), the pass
// budget, the directional rule, c_in, 1 for an entry of a search that
// exists; out[13..16]: the cells A, B, C, D of the entry; out[17..20]: the
// cells nb_motion (the geometry path that skip_mv and the table's derivation
// share) reads for that partition on a grid whose every cell holds its own
// index: A, B, C with every cell inter-coded (D's cell where C lies outside
// the grid), and the third neighbour again with that cell marked unavailable
// (D's cell; -1 where the cell marked was D's own).  Returns 0, or 1 when
// kParts[j] has no such partition.
extern "C" int emu_search_entry(int j, int pi, int spi, int* out)
{
#if !defined(__HIP_DEVICE_COMPILE__)
    if (j < 0 || j > 6) return 1;
    const PartDef& pd = kParts[j];
    if (pi < 0 || pi >= pd.num_part || spi < 0 || spi >= pd.num_sub) return 1;
    const SearchK k = kSearchTab.e[search_slot(j, pi, spi)];
    const PartGeo g = part_geo(k);
    const int geo[13] = {g.px, g.py, g.pw, g.ph, g.nbw, g.nblk, g.lbw, g.lnb, g.bi, (int)((k.geo >> 12) & 63), (int)((k.geo >> 22) & 3),
                         (int)((k.geo >> 24) & 1), (int)((k.geo >> 25) & 1)};
    for (int i = 0; i < 13; ++i) out[i] = geo[i];
    for (int i = 0; i < 4; ++i) out[13 + i] = (int)((k.nbc >> (5 * i)) & 31);
    static Shared* S = (Shared*)calloc(1, sizeof(Shared));
    for (int c = 0; c < 30; ++c) {
        (&S->mvs[0][0])[c] = 2;
        (&S->mvg[0][0])[c] = c;  // mv[0] = the cell's index
    }
    MvN nb[3];
    nb_motion(*S, g.px, g.py, g.pw, nb);
    for (int i = 0; i < 3; ++i) out[17 + i] = nb[i].mv[0];
    (&S->mvs[0][0])[out[19]] = 0;
    nb_motion(*S, g.px, g.py, g.pw, nb);
    out[20] = nb[2].st == 2 ? nb[2].mv[0] : -1;  // (-1: C lay outside the grid, so the cell marked was D's own)
    return 0;
#else
    return 1;
#endif
}

// The MV predictor of a search both ways, on the motion grid st[30] (0 not
// available, 1 intra, 2 inter) / mv[30][2]: out[0..1] from the table entry
// (mvp), out[2..3] from nb_motion and mvp_of with the partition's geometry
// and directional rule computed from kParts[j] here.  Returns 0, or 1.
extern "C" int emu_search_mvp(int j, int pi, int spi, const int* st, const int* mv, int* out)
{
#if !defined(__HIP_DEVICE_COMPILE__)
    if (j < 0 || j > 6) return 1;
    const PartDef& pd = kParts[j];
    if (pi < 0 || pi >= pd.num_part || spi < 0 || spi >= pd.num_sub) return 1;
    static Shared* S = (Shared*)calloc(1, sizeof(Shared));
    for (int c = 0; c < 30; ++c) {
        (&S->mvs[0][0])[c] = (int8_t)st[c];
        (&S->mvg[0][0])[c] = (mv[2 * c] & 0xFFFF) | (int)((uint32_t)mv[2 * c + 1] << 16);
    }
    mvp(*S, kSearchTab.e[search_slot(j, pi, spi)], out);
    int x = part_x(pi, pd.part_w), y = part_y(pi, pd.part_w, pd.part_h), ppw = pd.part_w;
    if (pd.num_part == 4) {
        x += sub_x(spi, pd.sub_w);
        y += sub_y(spi, pd.sub_w, pd.sub_h);
        ppw = pd.sub_w;
    }
    MvN nb[3];
    nb_motion(*S, x, y, ppw, nb);
    const bool p168 = pd.part_w == 16 && pd.part_h == 8, p816 = pd.part_w == 8 && pd.part_h == 16;
    mvp_of(nb, p168 ? (pi == 0 ? 1 : 2) : (p816 ? (pi == 0 ? 2 : 3) : 0), out + 2);
    return 0;
#else
    return 1;
#endif
}
