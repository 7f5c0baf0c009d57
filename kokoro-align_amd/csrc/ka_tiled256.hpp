// ka_tiled256.hpp — the 256-position tile pipeline (ka_tiled.hpp) with TWO wavefronts per tile: one computes, one feeds.
//
// Why: a lattice's tiles form a chain, so a lone lattice (and a book: its longest chapter) runs at the speed of ONE
// wavefront's frame loop - and a wavefront that is alone on its SIMD issues one instruction every four cycles, whatever
// the instruction.  In the one-wavefront tile of round 2 a block of 32 frames cost ~4000 cycles of frames and ~2700 cycles
// of everything around them: the wait for the staged block, its finiteness sum, the progress store, the poll of the tile
// below, the LDS-DMA requests of the block three ahead, the publish of the block's halo packets
// (profiles/r03_tile_stats_cfg2_one_wave.txt).  None of that depends on the scores.  Here wavefront 1 of the workgroup (the
// FEEDER) does all of it and wavefront 0 (the COMPUTE wavefront) only runs frames; they meet at one s_barrier per block.
//   iteration `it` (both wavefronts, after the barrier):
//     compute:  frames of block it (LDS rows / packets of blocks it and it+1 - the reads run two frames ahead), drops its
//               per-frame packets into staging buffer it & 1, stores the checkpoint if the block ends on one
//     feeder:   polls the tile below for block it+2 and requests it, publishes block it-1's packets (staging buffer
//               (it-1) & 1), sums block it+1 for the finiteness check, works out block it+1's band bookkeeping, then waits
//               for EVERYTHING it has in flight (s_waitcnt vmcnt(0)) and announces block it-1 in the progress word
//   so the compute wavefront finds blocks it+1 and it+2 landed at barrier it+1, the requests have the whole iteration of the
//   compute wavefront (~1.8 us) to land, and a block is announced one iteration after it was computed.
// Hand-off (cdna_hip_programming.md Guideline 16, sc1 payload + drained + sc1 flag; all loads of it sc1): halo packets are
// write-through stores; a tile publishes "slots < n are complete" in its progress word once per 32-frame block, and the tile
// above polls that word once per block, two blocks ahead of use.  Every slot is written once and read once: no ring, no
// back-pressure.  All of it is the feeder's; the compute wavefront's only vector-memory instruction is the checkpoint store.
#pragma once
#include "ka_tiled.hpp"

namespace ka {

// lanes [a, b) of a 64-bit mask, any a, b (clamped to 0..64)
__device__ __forceinline__ uint64_t tp_lane_range(int32_t a, int32_t b)
{
    a = a < 0 ? 0 : (a > 64 ? 64 : a);
    b = b < 0 ? 0 : (b > 64 ? 64 : b);
    if (b <= a) return 0ull;
    const uint32_t n = (uint32_t)(b - a);
    return (n >= 64u ? ~0ull : ((1ull << n) - 1ull)) << a;
}
struct TpMasks {
    uint64_t m0, m1, m2, m3;   // m<k>: lanes whose cell k (position base + 4 lane + k) is inside the band
};
// band [lo, hi) relative to the tile's first position (may be negative / beyond the tile)
__device__ __forceinline__ void tp_masks(TpMasks &mk, int32_t lo_rel, int32_t hi_rel)
{
    lo_rel = lo_rel < -8 ? -8 : (lo_rel > kTpTile + 8 ? kTpTile + 8 : lo_rel);
    hi_rel = hi_rel < -8 ? -8 : (hi_rel > kTpTile + 8 ? kTpTile + 8 : hi_rel);
    // lanes l with lo_rel <= 4 l + k < hi_rel  <=>  l in [ceil((lo_rel - k) / 4), ceil((hi_rel - k) / 4))
    mk.m0 = tp_lane_range((lo_rel + 3) >> 2, (hi_rel + 3) >> 2);
    mk.m1 = tp_lane_range((lo_rel + 2) >> 2, (hi_rel + 2) >> 2);
    mk.m2 = tp_lane_range((lo_rel + 1) >> 2, (hi_rel + 1) >> 2);
    mk.m3 = tp_lane_range((lo_rel + 0) >> 2, (hi_rel + 0) >> 2);
}
// -inf into the cell at tile-relative position rel (0..255): S = {cell 0, 2, 1, 3} of lane rel >> 2.  ONE v_cndmask behind
// a two-level scalar branch INSIDE one asm statement (6 instructions executed; as C++ - four selects on masks picked by
// s_cselect, or a switch whose arms are asm statements - hipcc made 24 to 35 of it, with copies at the merges).
__device__ __forceinline__ void tp_kill(f32x4 &S, uint32_t rel, float NINF)
{
    const uint64_t m = 1ull << (rel >> 2);
    float c0 = S[0], c2 = S[1], c1 = S[2], c3 = S[3];
    asm volatile("s_bitcmp1_b32 %[rel], 1\n\t"
                 "s_cbranch_scc1 .Lka_k23_%=\n\t"
                 "s_bitcmp1_b32 %[rel], 0\n\t"
                 "s_cbranch_scc1 .Lka_k1_%=\n\t"
                 "v_cndmask_b32 %[c0], %[c0], %[ninf], %[m]\n\t"
                 "s_branch .Lka_ke_%=\n"
                 ".Lka_k1_%=:\n\t"
                 "v_cndmask_b32 %[c1], %[c1], %[ninf], %[m]\n\t"
                 "s_branch .Lka_ke_%=\n"
                 ".Lka_k23_%=:\n\t"
                 "s_bitcmp1_b32 %[rel], 0\n\t"
                 "s_cbranch_scc1 .Lka_k3_%=\n\t"
                 "v_cndmask_b32 %[c2], %[c2], %[ninf], %[m]\n\t"
                 "s_branch .Lka_ke_%=\n"
                 ".Lka_k3_%=:\n\t"
                 "v_cndmask_b32 %[c3], %[c3], %[ninf], %[m]\n"
                 ".Lka_ke_%=:"
                 : [c0] "+v"(c0), [c1] "+v"(c1), [c2] "+v"(c2), [c3] "+v"(c3)
                 : [rel] "s"(rel), [m] "s"(m), [ninf] "v"(NINF)
                 : "scc");
    S = f32x4{c0, c2, c1, c3};
}
// state of a lane: S = {cell 0, cell 2, cell 1, cell 3} = {blank, blank, label, label} - the two blanks and the two labels
// are register pairs (v_pk_add_f32 of the emissions), and the four registers as they lie ARE the halo packet
__device__ __forceinline__ void tp_mask_state(f32x4 &S, const TpMasks &mk, float NINF)
{
    S[0] = select_by_mask(NINF, S[0], mk.m0);
    S[2] = select_by_mask(NINF, S[2], mk.m1);
    S[1] = select_by_mask(NINF, S[1], mk.m2);
    S[3] = select_by_mask(NINF, S[3], mk.m3);
}

// sc1 (write-through, agent scope) accesses of the progress words.  The loads are untracked by hipcc like the row loads:
// pair with a counted wait.
__device__ __forceinline__ void tp_prog_store(gu32w_t word /* uniform */, uint32_t value)
{
    uint64_t saved;
    asm volatile("s_nop 4\n\ts_mov_b64 %0, exec\n\ts_and_b64 exec, exec, 1\n\tglobal_store_dword %1, %2, %3 sc1\n\ts_mov_b64 exec, %0"
                 : "=&s"(saved) : "v"(0u), "v"(value), "s"(word) : "memory", "scc");
}
__device__ __forceinline__ void tp_prog_load(uint32_t &dst, gu32w_t word /* uniform */)
{
    asm volatile("s_nop 4\n\tglobal_load_dword %0, %1, %2 sc1" : "+v"(dst) : "v"(0u), "s"(word) : "memory");
}
// progress of the tile below must reach `need` leading slots; polled relaxed with a sleep that grows while far away.
// Bounded by a STALL detector: a tile whose producer has not advanced its progress word for ~4 s of wall clock gives up
// (returns false; the lattice gets KA_ERR_INTERNAL) instead of hanging the GPU - this can only be a bug in the hand-off,
// never an input.  The clock restarts whenever the polled word moves: a tile whose producer is healthy but far behind
// (a long lattice with every tile resident, a queue that is time-sliced with another process) waits as long as it takes.
// Hysteresis: a tile that does have to wait waits for `want` >= need (two blocks more): the poll it carries into a block
// start is a block old, so a tile sitting exactly at the limit would pay a poll round trip (~1 us) at every block;
// after one longer wait it stays ahead of its stale information for as long as it is not faster than its producer.
// (diagnostic counters - number of waits, 100 MHz ticks spent in them - live in two LDS words at `stat_lds`)
__device__ __forceinline__ bool tp_wait_progress(gu32w_t word, uint32_t need, uint32_t want, uint32_t have, uint32_t stat_lds)
{
    if (have >= need) return true;
    const uint64_t t0 = wall_clock64();   // 100 MHz
    uint64_t t_moved = t0;
    __attribute__((address_space(3))) uint32_t *st = (__attribute__((address_space(3))) uint32_t *)(uintptr_t)stat_lds;
    st[0] += 1;
    for (;;) {
        const uint32_t gap = want - have;
        if (gap > 4096u) __builtin_amdgcn_s_sleep(127);
        else if (gap > 256u) __builtin_amdgcn_s_sleep(32);
        else __builtin_amdgcn_s_sleep(4);
        uint32_t v = 0;
        tp_prog_load(v, word);
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(v) : : "memory");
        const uint32_t now_have = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
        const uint64_t now = wall_clock64();
        if (now_have != have) t_moved = now;
        have = now_have;
        if (have >= want) {
            st[1] += (uint32_t)(now - t0);
            return true;
        }
        if (now - t_moved > 400000000ull) return false;
    }
}

// A 256-position tile: four cells per lane
template <int M, bool ZL>
struct TpTile : TileCore<kTpCells> {
    gu32w_t prog_in, prog_out;
    // per lane
    f32x4 S;
    int la0, la1;           // 4 * label of cells 1 and 3
    float vz0, vz1;
};

// One frame, F = its index in the block.  The LDS reads run TWO frames ahead of their use (an LDS read takes longer than
// half a frame of this loop): In.cur = inputs of this frame (emissions E, e0 and H, the three cells below each lane's
// first cell), In.nxt = raw LDS data of frame t+1 (issued a frame ago, landed by now), and the reads for frame t+2 are
// issued here from `r2_*` / `h2` (byte addresses of row / packet t+2 in LDS).  H of frame t+1 is taken at the end, from
// this frame's final scores and the packet of slot t+1.
struct TpIn {
    f32x2 E;      // emissions of the two label cells
    float e0;     // blank emission
    f32x4 hp;     // packet of the tile below: {cell 0, 2, 1, 3} of the lane below lane 0
};
template <int M, bool ZL, bool GUARDED, int F>
__device__ __forceinline__ void tp_frame(TpTile<M, ZL> &c, uint32_t t, float (&H)[3], TpIn &cur, TpIn &nxt, uint32_t r2_l0, uint32_t r2_l1, uint32_t r2_0,
                                         uint32_t h2, float NINF)
{
    const bool live = !GUARDED || ((int32_t)t >= c.t_in && (int32_t)t < c.t_end);
    if (live) {
        const float b0 = c.S[0], b1 = c.S[1], l0 = c.S[2], l1 = c.S[3];
        f32x2 ml, mb;
        ml = label_pair_max<M, ZL>(l1, b1, l0, b0, H[0], H[1], c.vz1, c.vz0);   // {lower, upper}
        mb[1] = cell_blank_max<M>(b1, l0, H[0]);
        mb[0] = cell_blank_max<M>(b0, H[0], H[2]);
        const f32x2 sl = ml + cur.E, sb = mb + f32x2{cur.e0, cur.e0};
        c.S = f32x4{sb[0], sb[1], sl[0], sl[1]};
        // The band is enforced by KILLING single cells, not by masking all of them: a cell above hi collects "leaked" scores
        // from the live cells under it and must hold -inf at the moment it enters the band (rule i: the positions
        // [hi(t), hi(t+1)) are killed after frame t); a cell that has dropped below lo was live in the last frame of the old
        // band, is still computed in the first frame of the new one and must be dead after it (rule ii: the positions
        // [lo(t-1), lo(t)) are killed after frame t) - from then on it only reads cells below itself, which are dead, and
        // stays -inf by itself.  `ev` marks the frames in which either range meets this tile (band_block).
        if (__builtin_expect((c.ev >> F) & 1u, 0)) {
            asm volatile("" ::: "memory");
            // what to kill was worked out for the whole block (band_block): first tile-relative position | count << 16
            const uint32_t k2 = (uint32_t)__builtin_amdgcn_readlane((int)c.KL, F), k1 = (uint32_t)__builtin_amdgcn_readlane((int)c.KE, F + 1);
            for (uint32_t r = k2 & 0xffffu, e = r + (k2 >> 16); r < e; ++r) tp_kill(c.S, r, NINF);   // rule ii: left the band before this frame
            for (uint32_t r = k1 & 0xffffu, e = r + (k1 >> 16); r < e; ++r) tp_kill(c.S, r, NINF);   // rule i: enters it after this frame
        }
    }
    // the three cells below every lane's first cell, for frame t+1 (lane 0: from the packet of the tile below)
    // (the packet's first dword is not needed; it is kept alive up to here so that its register is not recycled - and
    //  the LDS read waited for - earlier)
    asm volatile("" : : "v"(nxt.hp));
    H[0] = wave_shr1(nxt.hp[3], c.S[3]);   // position base + 4 lane - 1 (label)
    H[1] = wave_shr1(nxt.hp[1], c.S[1]);   // - 2 (blank)
    H[2] = wave_shr1(nxt.hp[2], c.S[2]);   // - 3 (label)
    // publish the state after frame t = slot t+1 of the upper boundary (lane 63's four cells)
    // (staged: every lane drops its four cells into this frame's 1-KB row of the LDS staging area - no EXEC change and
    //  no vector-memory instruction per frame; lane 63's go out at the end of the block, tp_publish_block)
    if (live) *(__attribute__((address_space(3))) f32x4 *)(uintptr_t)(c.lds_stage + F * 16) = c.S;
    // LDS reads of frame t+2 (skipped frames read too: they prime the pipeline).  At the END of the frame, behind the branch
    // merge above: hipcc waits with lgkmcnt(0) at every merge (the band visit, the guarded frames), and with the reads at the
    // top of the frame that wait covered reads issued a dozen instructions earlier - every frame stalled for most of an LDS
    // round trip.  Down here the wait of the next frame finds reads that are a whole frame old.
    TpIn far;
    far.E = f32x2{lds_f32(r2_l0), lds_f32(r2_l1)};
    far.e0 = lds_f32(r2_0);
    far.hp = lds_f32x4(h2);
    cur = nxt;
    nxt = far;
}

// the frames of a block.  LDS byte addresses of this block's slot (A[0]) and the next one's (A[1]): row 0 + the lane's
// two label columns, row 0 itself (column 0 = blank), packet 0 - per block, so that a frame adds only an immediate offset
struct TpAddr {
    uint32_t l0, l1, r, h;
};
template <int M, bool ZL, int PITCH, bool GUARDED, int F>
__device__ __forceinline__ void tp_block_frames(TpTile<M, ZL> &c, uint32_t tb, float (&H)[3], TpIn &cur, TpIn &nxt, const TpAddr (&A)[2], float NINF)
{
    // frame t+2 = F+2 of this block, or F+2-16 of the next one
    constexpr int F2 = (F + 2) % kTpBlock, W = (F + 2) / kTpBlock;
    tp_frame<M, ZL, GUARDED, F>(c, tb + F, H, cur, nxt, A[W].l0 + F2 * PITCH, A[W].l1 + F2 * PITCH, A[W].r + F2 * PITCH, A[W].h + F2 * 16, NINF);
    if constexpr (F + 1 < kTpBlock) tp_block_frames<M, ZL, PITCH, GUARDED, F + 1>(c, tb, H, cur, nxt, A, NINF);
}

// end of a block: lane f < kTpBlock fetches what lane 63 staged in frame f and stores it as slot tb + f + 1 (one write-through
// store instruction for the block's packets = 512 contiguous bytes); frames the tile did not compute store nothing
template <int M, bool ZL>
__device__ __forceinline__ void tp_publish_block(TpTile<M, ZL> &c, uint32_t tb, int lane)
{
    const int32_t t = (int32_t)tb + lane;
    if (lane < kTpBlock && t >= c.t_in && t < c.t_end) {
        const f32x4 pk = lds_f32x4(c.lds_packets + (uint32_t)lane * 16u);
        // slot tb of the upper boundary (frame tb + f publishes slot tb + f + 1); worked out here, after the frames: two
        // scalar registers that are not live across them
        const char *out_block = c.halo_out + ((int64_t)tb - (int64_t)c.t_in) * 16;
        tp_slot_store<16>(out_block, (uint32_t)lane * 16u, pk);
    }
}

template <int M, bool ZL>
__device__ __forceinline__ void tp_checkpoint(TpTile<M, ZL> &c, uint32_t t_next /* multiple of 32 */)
{
    const f32x4 v = {c.S[0], c.S[2], c.S[1], c.S[3]};   // cells 0..3 in position order
    asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2\n\ts_nop 1" : : "v"(c.ck_off), "v"(v), "s"(c.ck + ((size_t)(t_next / kCkFrames) - 1) * (size_t)c.ck_pitch) : "memory");
}
// LDS map of a workgroup: kTpRing blocks of rows (TileRows), the ring's packets, the poll words, two publish staging buffers,
// the diagnostic words (ticket at +48), two buffers of band words.  27.1 KB for V = 39 with contiguous rows: FIVE workgroups
// per CU when the engine asks for no more (launches whose tiles outnumber the slots), 39.1 KB otherwise.
template <int PITCH, bool CONTIG>
struct Tp2Lds {
    static constexpr int kSlot = TileRows<PITCH, CONTIG>::kSlot;
    static constexpr int kHalo = kTpRing * kSlot;
    static constexpr int kTicket = kHalo + kTpRing * kTpBlock * 16 + 16 + kTp2StageBytes + 48;
    static constexpr int kTotal = kHalo + kTpRing * kTpBlock * 16 + 16 + kTp2StageBytes + 64 + 2 * kTp2BandBytes;
};
static_assert(Tp2Lds<256, false>::kTotal <= (int)kTpLdsRequest && Tp2Lds<256, true>::kTotal <= (int)kTpLdsRequest, "four workgroups per CU");
static_assert(5 * ((Tp2Lds<156, true>::kTotal + 511) / 512 * 512) <= 160 * 1024, "five workgroups per CU with V = 39");

template <int M, bool ZL, int PITCH, bool CONTIG>
__device__ __forceinline__ void tp2_run_tile(const Lattice &d, const TileTask &tk, int32_t *meta, char *halo, gu32w_t prog, TileAux *aux,
                                             uint32_t lds_rows, uint32_t lds_halo, int verify, TpStats *stats_out)
{
    const int lane = threadIdx.x & 63;
    const bool feeder = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) != 0;
    const uint32_t lds_poll = lds_halo + kTpRing * kTpBlock * 16;
    const uint32_t lds_stage0 = lds_poll + 16;                                  // two staging buffers of kTpStageBytes
    const uint32_t stat_lds = lds_stage0 + kTp2StageBytes;                      // diagnostic words, then two flag words
    const uint32_t lds_band = stat_lds + 64;                                    // two buffers of kTp2BandBytes: the band code's kill words and event mask of a block
    tile_stats_open(stat_lds, verify, !feeder, feeder, lane, stats_out);
    unsigned long long ph = 0;
    auto phase = [&](int w) {
        if (verify & 4) {
            const unsigned long long now = __builtin_amdgcn_s_memtime();
            if (w >= 0) ((lu32_t)(uintptr_t)stat_lds)[w] += (uint32_t)(now - ph);
            ph = now;
        }
    };
    // the compute wavefront is the chain: where it shares a SIMD with feeders and with other kernels' wavefronts it issues first
    if (!feeder) __builtin_amdgcn_s_setprio(3);
    const float NINF = ninf();
    TpTile<M, ZL> c;
    tile_setup(c, d, tk, halo, lane, lds_rows, lds_halo, lds_stage0);
    c.prog_in = prog + tk.prog_in;
    c.prog_out = prog + tk.prog_out;
    static_assert(kTpBlock * 16 + 62 * 16 + (kTpBlock - 1) * 16 + 16 <= kTpStageBytes, "publish staging");
    {
        gci32_t labx = (gci32_t)d.labx + ((size_t)c.base >> 1) + 2 * (size_t)lane;
        c.la0 = labx[0];
        c.la1 = labx[1];
        c.vz0 = (ZL && c.la0 == 0) ? NINF : __builtin_inff();
        c.vz1 = (ZL && c.la1 == 0) ? NINF : __builtin_inff();
    }
    // state before frame t_in: nothing of the tile is live, except the virtual start state (align.py:57-58)
    c.S = f32x4{NINF, NINF, NINF, NINF};
    if (c.base == 0 && c.t_in == 0 && lane == 0) c.S[0] = 0.0f;
    // slot t_in of the upper boundary = the state before the tile's first frame: lane 63's cells, all -inf.  The FEEDER
    // stores it: every store the progress word vouches for is in its own in-order vmcnt history.
    if (feeder) tp_halo_store<0>(c.halo_out, f32x4{NINF, NINF, NINF, NINF}, 1ull << 63);

    const uint32_t last_slot = (uint32_t)c.t_end - 1;     // this tile reads slots t_in .. t_end - 1
    auto ring = [](int32_t k) { return (uint32_t)((k % kTpRing + kTpRing) % kTpRing); };
    constexpr uint32_t kSlot = Tp2Lds<PITCH, CONTIG>::kSlot;     // LDS bytes of a block of rows
    auto issue_block = [&](int32_t k) {    // k >= 0
        const uint32_t slot = ring(k);
        stage_rows<PITCH, CONTIG>(c, k, c.lds_rows + slot * kSlot, lane);
        stage_packets(c, k, c.lds_halo + slot * (kTpBlock * 16), last_slot, lane);
        if (lane == 0) __builtin_amdgcn_global_load_lds((gptr_t)c.prog_in, (lptr_t)(lchar_t)(uintptr_t)(lds_poll + slot * 4), 4, 0, 16);
    };
    bool stale = false;
    auto landed_block = [&](int32_t k) {
        const uint32_t slot = ring(k);
        sum_rows<PITCH, CONTIG>(c, k, c.lds_rows + slot * kSlot, lane);
        if (verify & 1) {
            const int32_t sidx = k * kTpBlock + (lane & (kTpBlock - 1));
            const f32x4 h = lds_f32x4(c.lds_halo + slot * (kTpBlock * 16) + (uint32_t)(lane & (kTpBlock - 1)) * 16u);
            const bool mine = lane < kTpBlock && sidx >= c.t_in && sidx < c.t_end;
            if (__builtin_amdgcn_ballot_w64(mine && tp_sentinel_in(h))) stale = true;
        }
    };
    auto need_for = [&](int32_t k) {
        const uint32_t n = (uint32_t)(k + 1) * kTpBlock;
        return n < (uint32_t)c.t_end ? n : (uint32_t)c.t_end;
    };

    const int32_t kb0 = c.t_in / kTpBlock, kb1 = (c.t_end - 1) / kTpBlock;   // first and last block
    bool fed = true;
    TpIn cur = {f32x2{0.0f, 0.0f}, 0.0f, f32x4{NINF, NINF, NINF, NINF}}, nxt = cur;
    float H[3] = {NINF, NINF, NINF};
    // Iterations kb0-2, kb0-1 prime the feeder's pipeline; iteration kb1+1 publishes the last block.
    for (int32_t it = kb0 - 2; it <= kb1 + 1; ++it) {
        const uint32_t tb = (uint32_t)(it * kTpBlock);              // (wraps in the priming iterations of block 0: not used there)
        if ((verify & 4) && !feeder) {      // the compute wavefront's cycles at the barrier (words 8, 9: as the 128-position tile's)
            const unsigned long long b0 = __builtin_amdgcn_s_memtime();
            tp2_barrier();
            if (it >= kb0 && it <= kb1 + 1) ((lu32_t)(uintptr_t)stat_lds)[8] += (uint32_t)(__builtin_amdgcn_s_memtime() - b0);
        } else
        tp2_barrier();
        if (feeder) {
            phase(-1);
            // block it+2 is requested now (LDS ring slot of block it-2): the tile below must have published its packets (the
            // freshest look at its progress word that has landed came with block it+1)
            if (it + 2 <= kb1 && fed) {
                const uint32_t have = it + 1 >= kb0 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_bit_cast(uint32_t, lds_f32(lds_poll + ring(it + 1) * 4))) : 0u;
                // (no hysteresis here: the one-wavefront tile asks for two blocks more than it needs once it has to wait, so that
                //  its frames are not interrupted by a poll per block; here the frames run in the other wavefront)
                fed = tp_wait_progress(c.prog_in, need_for(it + 2), need_for(it + 2), have, stat_lds);
            }
            phase(5);
            if (it + 2 >= 0 && it + 2 <= kb1 + 1) issue_block(it + 2);
            phase(6);
            // block it-1 is complete in staging buffer (it-1) & 1: lane f < 32 stores the packet of frame f as slot tb-32+f+1
            const bool published = it - 1 >= kb0 && it - 1 <= kb1;
            if (published) {
                c.lds_packets = lds_stage0 + (uint32_t)((it - 1) & 1) * kTpStageBytes;
                tp_publish_block(c, tb - kTpBlock, lane);
            }
            phase(7);
            // block it+1 landed before the last barrier: its finiteness sum
            if (it + 1 >= kb0 && it + 1 <= kb1) landed_block(it + 1);
            // the band bookkeeping of the NEXT block (which positions of the tile enter or leave the band in which frame), for
            // the compute wavefront to pick up after the next barrier: ~60 instructions it does not have to issue
            if (it + 1 >= kb0 && it + 1 <= kb1) {
                band_block(c, tb + kTpBlock, lane);
                const uint32_t bb = lds_band + (uint32_t)((it + 1) & 1) * kTp2BandBytes;
                typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                *(__attribute__((address_space(3))) u32x2 *)(uintptr_t)(bb + (uint32_t)lane * 8u) = u32x2{c.KL, c.KE};
                if (lane == 0) *(lu32_t)(uintptr_t)(bb + 512u) = c.ev;
                band_advance(c);
            }
            phase(4);
            // EVERYTHING this wavefront has in flight is waited for, once per iteration: the requests of block it+2 (the compute
            // wavefront reads its first rows in the next iteration) and the packets just published.  No counted wait: a
            // counted vmcnt orders loads among loads and stores among stores, not one against the other - announcing block
            // it-1 behind "at most the requests are outstanding" would rest on stores retiring before younger loads, which
            // is not something the ISA promises.  The requests have had the whole iteration to land, and the feeder is idle
            // for half of it anyway.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            phase(3);
            // slots <= tb are in memory - but never vouch for more than the tile's own frames have produced: the slots behind
            // t_end are filled (with -inf) after the loop, and the final progress word covers those
            if (published) tp_prog_store(c.prog_out, (tb < (uint32_t)c.t_end ? tb : (uint32_t)c.t_end) + 1);
        } else if (it >= kb0 && it <= kb1) {
            const unsigned long long g0 = (verify & 4) ? __builtin_amdgcn_s_memtime() : 0ull;
            const uint32_t slot = ring(it), nslot = ring(it + 1);
            uint32_t rc = c.lds_rows + slot * kSlot, rn = c.lds_rows + nslot * kSlot;
            uint32_t hc = c.lds_halo + slot * (kTpBlock * 16), hn = c.lds_halo + nslot * (kTpBlock * 16);
            asm volatile("v_mov_b32 %0, %4\n\tv_mov_b32 %1, %5\n\tv_mov_b32 %2, %6\n\tv_mov_b32 %3, %7"
                         : "=&v"(rc), "=&v"(rn), "=&v"(hc), "=&v"(hn) : "s"(rc), "s"(rn), "s"(hc), "s"(hn));
            TpAddr A[2] = {{rc + (uint32_t)c.la0, rc + (uint32_t)c.la1, rc, hc}, {rn + (uint32_t)c.la0, rn + (uint32_t)c.la1, rn, hn}};
            asm volatile("" : "+v"(A[0].l0), "+v"(A[0].l1), "+v"(A[1].l0), "+v"(A[1].l1));
            // where this block's frames drop their packets: lane 63's into the packet row, the others' into scratch behind it
            {
                const uint32_t pk = lds_stage0 + (uint32_t)(it & 1) * kTpStageBytes;
                c.lds_stage = lane == 63 ? pk : pk + kTpBlock * 16 + (uint32_t)lane * 16u;
            }
            if (it == kb0) {
                cur.E = f32x2{lds_f32(A[0].l0), lds_f32(A[0].l1)};
                cur.e0 = lds_f32(A[0].r);
                nxt.E = f32x2{lds_f32(A[0].l0 + PITCH), lds_f32(A[0].l1 + PITCH)};
                nxt.e0 = lds_f32(A[0].r + PITCH);
                nxt.hp = lds_f32x4(A[0].h + 16);
                const f32x4 hp = lds_f32x4(A[0].h);
                H[0] = wave_shr1(hp[3], c.S[3]);
                H[1] = wave_shr1(hp[1], c.S[1]);
                H[2] = wave_shr1(hp[2], c.S[2]);
            }
            {   // this block's band bookkeeping, left by the feeder
                const uint32_t bb = lds_band + (uint32_t)(it & 1) * kTp2BandBytes;
                typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                const u32x2 kk = *(const __attribute__((address_space(3))) u32x2 *)(uintptr_t)(bb + (uint32_t)lane * 8u);
                c.KL = kk[0];
                c.KE = kk[1];
                c.ev = (uint32_t)__builtin_amdgcn_readfirstlane((int)*(const lu32_t)(uintptr_t)(bb + 512u));
            }
            const bool partial = (int32_t)tb < c.t_in || (int32_t)(tb + kTpBlock) > c.t_end;
            const unsigned long long fr0 = (verify & 4) ? __builtin_amdgcn_s_memtime() : 0ull;
            if (!partial) {
                tp_block_frames<M, ZL, PITCH, false, 0>(c, tb, H, cur, nxt, A, NINF);
                if ((tb + kTpBlock) % kCkFrames == 0 && tb + kTpBlock < c.T) tp_checkpoint(c, tb + kTpBlock);
            } else {
                tp_block_frames<M, ZL, PITCH, true, 0>(c, tb, H, cur, nxt, A, NINF);
                if ((tb + kTpBlock) % kCkFrames == 0 && (int32_t)(tb + kTpBlock) <= c.t_end && tb + kTpBlock < c.T) tp_checkpoint(c, tb + kTpBlock);
            }
            if (verify & 4) {
                const unsigned long long now = __builtin_amdgcn_s_memtime();
                // frames + checkpoint of the block | everything of the iteration that is not frames (set-up, checkpoint)
                ((lu32_t)(uintptr_t)stat_lds)[2] += (uint32_t)(now - fr0);
                ((lu32_t)(uintptr_t)stat_lds)[9] += (uint32_t)(fr0 - g0);
            }
        }
    }
    // nothing of this workgroup may still be landing in LDS or in a register when it ends
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    int32_t *m = meta_of(meta, d.idx);
    if (feeder) {
        // ---- flagged before the tile reports itself done (barrier below), so that whoever closes the lattice sees the flag
        if ((!fed || stale) && lane == 0) atomicMin(&m[0], kStatusInternal);
        flag_finiteness(c.absum, d, m, lane);
        // ---- hand the rest of the upper boundary over: after t_end the whole tile is below the band = -inf ----
        const f32x4 dead = {NINF, NINF, NINF, NINF};
        for (int64_t s = (int64_t)c.t_end + 1 + lane; s <= (int64_t)tk.fill_end; s += 64)
            tp_slot_store<0>(c.halo_out, (uint32_t)((s - c.t_in) * 16), dead);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tp_prog_store(c.prog_out, kTpProgDone);
        __threadfence();
    }
    tp2_barrier();
    if (feeder) {
        if ((verify & 4) && lane == 0) {
            const __attribute__((address_space(3))) uint32_t *sw = (const __attribute__((address_space(3))) uint32_t *)(uintptr_t)stat_lds;
            TpStats st;
            st.phase[0] = sw[3] | ((unsigned long long)sw[4] << 32);
            st.phase[1] = sw[5] | ((unsigned long long)sw[6] << 32);
            st.phase[2] = sw[7] | ((unsigned long long)sw[10] << 32);   // (high half: HW_ID of the compute wavefront)
            st.wait_ticks = sw[1] | ((unsigned long long)sw[2] << 32);
            st.extra[0] = sw[8] | ((unsigned long long)sw[2] << 32);    // compute wavefront: cycles at the barrier | cycles inside the frame blocks (+ checkpoint stores)
            st.extra[1] = sw[9];                                         // ... and between a barrier and the block's first frame
            tile_stats_close(st, sw[0], stats_out);
        }
        return;
    }
    // ---- terminal state: the highest live position of frame T-1 over the tiles alive then (close_lattice) ----
    if ((uint32_t)c.t_end == c.T) {
        TpMasks mk;   // (the only full band mask of a tile's life: cells above hi may hold leaked scores)
        uint32_t lo_last, hi_last;
        c.last_band(lo_last, hi_last);
        tp_masks(mk, (int32_t)lo_last - c.base, (int32_t)hi_last - c.base);
        tp_mask_state(c.S, mk, NINF);
        const float cell[4] = {c.S[0], c.S[2], c.S[1], c.S[3]};
        unsigned long long key = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (cell[k] != NINF) key = ((unsigned long long)(uint32_t)(c.base + 4 * lane + k + 1) << 32) | __builtin_bit_cast(uint32_t, cell[k]);
        close_lattice(key, d, aux, m, lane);
    }
}

// One workgroup of TWO wavefronts per tile (40 KB of LDS requested: four workgroups per CU).  The tile a workgroup runs is
// drawn from a ticket counter; tasks are sorted by first frame.
template <int M, int PITCH, bool CONTIG>
__global__ __launch_bounds__(128) void forward_tp2_kernel(const Lattice *__restrict__ lats, const TileTask *__restrict__ tasks, int n_tasks,
                                                          int32_t *meta, char *halo, uint32_t *prog, TileAux *aux, uint32_t *ticket, int verify, TpStats *stats)
{
    typedef Tp2Lds<PITCH, CONTIG> Lds;
    extern __shared__ __attribute__((aligned(16))) char tp_lds[];
    const uint32_t lds_rows = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)&tp_lds[0];
    const uint32_t lds_halo = lds_rows + Lds::kHalo;
    // (the ticket goes through a word of the dynamic LDS block: a static __shared__ variable on top of the request would cost a
    //  workgroup per CU)
    volatile uint32_t *s_ticket = reinterpret_cast<volatile uint32_t *>(&tp_lds[Lds::kTicket]);
    if (threadIdx.x == 0) *s_ticket = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint32_t tix = (uint32_t)__builtin_amdgcn_readfirstlane((int)*s_ticket);
    __syncthreads();
    if (tix >= (uint32_t)n_tasks) return;
    const TileTask &tk = tasks[tix];
    const Lattice &d = lats[__builtin_amdgcn_readfirstlane(tk.lat)];
    const int flags = __builtin_amdgcn_readfirstlane(meta_of(meta, d.idx)[2]);
    if (flags & kFlagZeroLabel)
        tp2_run_tile<M, true, PITCH, CONTIG>(d, tk, meta, halo, (gu32w_t)prog, aux, lds_rows, lds_halo, verify, stats + tix);
    else
        tp2_run_tile<M, false, PITCH, CONTIG>(d, tk, meta, halo, (gu32w_t)prog, aux, lds_rows, lds_halo, verify, stats + tix);
}

}  // namespace ka
