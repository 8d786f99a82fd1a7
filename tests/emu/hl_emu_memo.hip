// hl_emu_memo.hip -- TEST INFRASTRUCTURE.  The translation unit of the host
// emulation (tests/emu/libhl_emu.so): hl_emu.hip as it is, plus the settings,
// counters and key export of the candidate evaluation's memo (hl_mbcore.h
// kMemoSlots, eval_candidates).  The emulator gets the memo's setting through
// host globals, like g_emu_bad_guess: they hold for the whole process.
#include "hl_emu.hip"

#if !defined(__HIP_DEVICE_COMPILE__)
int hl::g_emu_memo_slots = hl::kMemoSlots;
int hl::g_emu_memo_probe = hl::kMemoProbe;
long long hl::g_emu_memo_stat[hl::MS_COUNT] = {};
int hl::g_emu_memo_mb = -1;
#endif

// Slots in use (a power of two up to the built capacity; 0 = off; -1 = the
// default) and the probe length (1..4; the device's is 4) of every emulator
// of the process.  Returns 0, or 1 for a setting it refuses.
extern "C" int emu_set_memo(int slots, int probe)
{
#if !defined(__HIP_DEVICE_COMPILE__)
    if (slots < 0) slots = kMemoSlots;
    if (slots > kMemoSlots || (slots & (slots - 1)) || probe < 1 || probe > kMemoProbe) return 1;
    g_emu_memo_slots = slots;
    g_emu_memo_probe = probe;
    return 0;
#else
    return 1;
#endif
}
extern "C" int emu_memo_capacity(void) { return kMemoSlots; }

// The memo's counters since the last reset (process-wide), in this order:
// items, hits, bypassed (key does not fit), not inserted (probe window full),
// inserted, most keys of one MB, MBs with a search, passes, passes without a
// miss, 128-item rounds, rounds with a miss, 16-item wave shares of the
// rounds, wave shares with a miss.  Returns how many it wrote.
extern "C" int emu_memo_stats(long long* out, int n, int reset)
{
#if !defined(__HIP_DEVICE_COMPILE__)
    n = n < (int)MS_COUNT ? n : (int)MS_COUNT;
    for (int i = 0; i < n; ++i) out[i] = g_emu_memo_stat[i];
    if (reset) memset(g_emu_memo_stat, 0, sizeof(g_emu_memo_stat));
    return n;
#else
    return 0;
#endif
}

// The memo key of block k (raster in the partition) of the candidate (mvx,
// mvy) of partition (pi, spi) of kParts[j] in MB (mbx, mby) of a W x H
// picture, as put_cand and eval_candidates form it, with what the block's
// quad reads: out = {key (0: bypass), off1 + o, off2 + o, source offset} for
// block row 0.  Returns 0, or 1 when the geometry has no such block.
extern "C" int emu_memo_key(int W, int H, int mbx, int mby, int j, int pi, int spi, int mvx, int mvy, int k, long long* out)
{
#if !defined(__HIP_DEVICE_COMPILE__)
    if (j < 0 || j > 6 || W <= 0 || H <= 0 || (W & 15) || (H & 15) || mbx < 0 || mby < 0 || mbx >= W / 16 || mby >= H / 16) return 1;
    const PartDef& pd = kParts[j];
    if (pi < 0 || pi >= pd.num_part || spi < 0 || spi >= pd.num_sub) return 1;
    static Shared* S = (Shared*)calloc(1, sizeof(Shared));
    FrameArgs F{};
    F.W = W;
    F.H = H;
    F.mbw = W / 16;
    F.mbh = H / 16;
    F.pstride = W + 2 * kPad;
    F.plsz = F.pstride * (H + 2 * kPad);
    Ctx c{F, *S, 0, 1, mby * F.mbw + mbx, mbx, mby, mbx * 16, mby * 16, 0, 0, 0};
    int px = part_x(pi, pd.part_w), py = part_y(pi, pd.part_w, pd.part_h);
    if (pd.num_part == 4) {
        px += sub_x(spi, pd.sub_w);
        py += sub_y(spi, pd.sub_w, pd.sub_h);
    }
    const int nbw = pd.sub_w >> 2, nblk = nbw * (pd.sub_h >> 2);
    if (k < 0 || k >= nblk) return 1;
    const int hx = k % nbw, hy = k / nbw;
    put_cand(c, px, py, pd.sub_w, pd.sub_h, 0, mvx, mvy);
    const CandSlot cs = S->wc[0][0];
    const long long o = (long long)(hy << 2) * F.pstride + (hx << 2);
    const uint32_t kb = (uint32_t)cs.pad >> 4;
    out[0] = kb ? (long long)memo_key(kb, (((py >> 2) + hy) << 2) + (px >> 2) + hx) : 0;
    out[1] = cs.off1 + o;
    out[2] = cs.off2 + o;
    out[3] = (py + (hy << 2)) * 16 + px + (hx << 2);
    return 0;
#else
    return 1;
#endif
}
