// ka_tiled.hpp — what the two tile pipelines of the tiled forward DP (KA_MODE_TILED) share.
//
// The lattice is cut along the label axis into ABSOLUTE tiles of 64 x CELLS positions: 256 (four cells per lane, two wavefronts
// per tile, progress words: ka_tiled256.hpp) or 128 (two cells per lane, three wavefronts per tile, self-vouching packets:
// ka_tiled128.hpp).  Dependencies only point UP the label axis (cell p reads p .. p-3 of the previous frame, align.py:70-81), so
// tile b may run any number of frames behind tile b-1 and takes the top cells of b-1 from 16-byte halo packets in HBM, one slot
// per frame.  A tile lives from the frame in which the band's upper edge reaches it (t_in) to the frame in which its lower edge
// has passed it (t_end); tiles are drawn from a ticket counter and the host sorts them by t_in.  Log-prob rows and packets are
// staged through LDS in blocks of 32 frames, the band is stepped once per block, and the scores are checkpointed every 32
// frames for backtrace_rc_kernel.  Here: the tile's description and band bookkeeping (TileCore), the staging of rows and
// packets, the finiteness sum, the close of a lattice, the diagnostics, the hand-off stores and the barrier.
#pragma once
#include "ka_device.hpp"

namespace ka {

typedef uint32_t KA_GLOBAL *gu32w_t;
typedef __attribute__((address_space(1))) const void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;
typedef __attribute__((address_space(3))) char *lchar_t;
typedef __attribute__((address_space(3))) uint32_t *lu32_t;

__device__ __forceinline__ float lds_f32(uint32_t addr) { return *(const __attribute__((address_space(3))) float *)(uintptr_t)addr; }
__device__ __forceinline__ f32x4 lds_f32x4(uint32_t addr) { return *(const __attribute__((address_space(3))) f32x4 *)(uintptr_t)addr; }

// sc1 (write-through, agent scope) store of the hand-off.
template <int OFF>
__device__ __forceinline__ void tp_halo_store(const void *block_base /* uniform */, const f32x4 &pk, uint64_t lane_mask)
{
    // one lane stores: EXEC is narrowed to it and put back as it was (never assumed to be "all lanes": the compiler
    // may have structured the surrounding control flow with lanes parked).  A store wider than 64 bits reads its data
    // registers for two more wait states: the EXEC restore and the s_nop are those.
    uint64_t saved;
    asm volatile("s_nop 4\n\ts_mov_b64 %0, exec\n\ts_and_b64 exec, exec, %4\n\tglobal_store_dwordx4 %1, %2, %3 offset:%5 sc1\n\ts_mov_b64 exec, %0\n\ts_nop 0"
                 : "=&s"(saved) : "v"(0u), "v"(pk), "s"(block_base), "s"(lane_mask), "i"(OFF) : "memory", "scc");
}

// write-through store of a halo slot per calling lane: at byte off + OFF of `base`
template <int OFF>
__device__ __forceinline__ void tp_slot_store(const void *base /* uniform */, uint32_t off, const f32x4 &v)
{
    asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 offset:%3 sc1\n\ts_nop 1" : : "v"(off), "v"(v), "s"(base), "i"(OFF) : "memory");
}
// a staged packet that has not been written yet: one of the three words a frame uses is still the sentinel
__device__ __forceinline__ bool tp_sentinel_in(const f32x4 &h)
{
    return __builtin_bit_cast(uint32_t, h[1]) == kTpSentinel || __builtin_bit_cast(uint32_t, h[2]) == kTpSentinel || __builtin_bit_cast(uint32_t, h[3]) == kTpSentinel;
}

// the barrier of a block: each side first finishes what the others are going to look at (LDS writes; LDS-DMA is waited for
// with a counted vmcnt) - NOT the vmcnt(0) of __syncthreads, which would drain the feeder's requests
__device__ __forceinline__ void tp2_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Diagnostics (verify & 4: ka_debug_tile_stats, tools/tile_stats*.py).  At the start: the workgroup's diagnostic words in LDS
// are zeroed, the compute wavefront notes where it runs (word 10), the feeder stamps wall clock (100 MHz) and shader clock.
__device__ __forceinline__ void tile_stats_open(uint32_t stat_lds, int verify, bool compute, bool feeder, int lane, TpStats *stats_out)
{
    if (threadIdx.x < 10) ((lu32_t)(uintptr_t)stat_lds)[threadIdx.x] = 0;
    if ((verify & 4) && compute && lane == 0) {
        uint32_t hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        ((lu32_t)(uintptr_t)stat_lds)[10] = hw & 0xffffu;
    }
    if ((verify & 4) && feeder) {
        stats_out->start_tick = (unsigned long long)wall_clock64();
        stats_out->total_ticks = __builtin_amdgcn_s_memtime();
    }
}
// At the end, the feeder's lane 0: `st` holds the form's own words; the spin count (with where the feeder ran in the high
// half), the shader cycles and the wall-clock ticks since the start complete it.
__device__ __forceinline__ void tile_stats_close(TpStats &st, uint32_t spins, TpStats *stats_out)
{
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    st.spins = spins | ((unsigned long long)((xcc & 0xf) << 16 | (hw & 0xffff))) << 32;
    st.start_tick = __builtin_amdgcn_s_memtime() - stats_out->total_ticks;
    st.total_ticks = wall_clock64() - stats_out->start_tick;
    *stats_out = st;
}

// A staged block of log-prob rows in LDS: LDS-DMA instructions per block and bytes of its slot - as the rows lie in memory when
// they are contiguous (32 x PITCH bytes, rounded up to whole 1-KB instructions: 5 KB for V = 39), else 32 rows of 256 bytes.
template <int PITCH, bool CONTIG>
struct TileRows {
    static_assert(CONTIG || PITCH == kTpRowBytes, "row-by-row staging uses 256-byte rows");
    static constexpr int kRowDmas = !CONTIG ? kTpBlock : (kTpBlock * PITCH + 1023) / 1024;
    static constexpr int kSlot = CONTIG ? kRowDmas * 1024 : kTpSlotBytes;
};

// The wave-uniform description of a tile of 64 x CELLS positions and its lattice, and the per-lane state both forms keep the same.
template <int CELLS>
struct TileCore {
    static constexpr int kPositions = 64 * CELLS;
    uint32_t T, L, B, dq, dr;
    // The band (align.py:64-65) per BLOCK of 32 frames, not per frame: q0 / r0 = floor(L tb / T) and the remainder at the
    // block's first frame tb, advanced by (32 L) / T, (32 L) % T per block; per block the lanes work out, 34 frames at once,
    // which positions of THIS tile enter or leave the band at which frame (KE / KL) and `ev` gets bit F set when frame
    // tb+F has any to kill.  A tile pays nothing at all for the band steps that do not touch it - 3 of 5 for a 1000-wide
    // band, whose edges are inside a 256-position tile for 2 x 256 of the ~1250 steps the tile lives through.  (Rounds 1-2
    // stepped a Bresenham remainder in every frame and ran ~40 scalar instructions at every step, relevant or not: 161 cycles
    // per frame in cfg2 against 105 where the band never moves.)
    uint32_t q0, r0, dq32, dr32, ev;
    uint32_t KL, KE;        // per lane (VGPRs): the cells to kill, lane l <-> the band step after frame tb - 1 + l (band_block)
    float inv_T;
    __device__ __forceinline__ uint32_t lo_of(uint32_t q) const
    {
        const int32_t d = (int32_t)q - (int32_t)(B >> 1);
        return (uint32_t)(d > 0 ? d : 0);
    }
    __device__ __forceinline__ uint32_t hi_of(uint32_t lo) const { return (L - lo < B) ? L : lo + B; }
    // the band [lo, hi) of frame T-1
    __device__ __forceinline__ void last_band(uint32_t &lo, uint32_t &hi) const
    {
        const uint32_t q_last = L - (L + T - 1u) / T;   // floor(L (T-1) / T) = L - ceil(L / T)
        lo = lo_of(q_last);
        hi = hi_of(lo);
    }
    int32_t base, t_in, t_end;
    const char *lp;
    size_t ld;
    uint32_t lane_off;
    const char *halo_in;    // slot j of the lower boundary at halo_in + (j - t_in) * 16
    char *halo_out;         // slot j of the upper boundary at halo_out + (j - t_in) * 16 (the top tile writes to a boundary nobody reads)
    char *ck;               // checkpoint k (scores after frame 32 (k + 1) - 1) at ck + k * ck_pitch
    uint32_t ck_pitch;
    uint32_t ck_off;        // per lane: ((base + CELLS lane) & ck_mask) * 4
    float absum;            // per lane: sum of |log-prob| over the staged blocks (sum_rows)
    // LDS
    uint32_t lds_rows, lds_halo;   // byte addresses of this workgroup's row and packet buffers
    uint32_t lds_stage;            // per lane: where frame 0 of a block drops the lane's cells
    uint32_t lds_packets;          // the publish staging buffer
};

// The core of the tile `tk` of lattice `d`, and the lane's part of it
template <int CELLS>
__device__ __forceinline__ void tile_setup(TileCore<CELLS> &c, const Lattice &d, const TileTask &tk, char *halo, int lane, uint32_t lds_rows, uint32_t lds_halo,
                                           uint32_t lds_packets)
{
    c.T = (uint32_t)__builtin_amdgcn_readfirstlane(d.T);
    c.L = (uint32_t)__builtin_amdgcn_readfirstlane(d.L);
    c.B = (uint32_t)__builtin_amdgcn_readfirstlane(d.beam);
    c.dq = c.L / c.T;
    c.dr = c.L % c.T;
    c.base = __builtin_amdgcn_readfirstlane(tk.tile) * TileCore<CELLS>::kPositions;
    c.t_in = __builtin_amdgcn_readfirstlane(tk.t_in);
    c.t_end = __builtin_amdgcn_readfirstlane(tk.t_end);
    c.lp = reinterpret_cast<const char *>(d.lp);
    c.ld = (size_t)d.ld * 4;
    c.lane_off = (lane < d.V ? (uint32_t)lane : 0u) * 4u;
    c.halo_in = halo + tk.halo_in;
    c.halo_out = halo + tk.halo_out;
    c.ck = reinterpret_cast<char *>(d.bp);
    c.ck_pitch = (uint32_t)d.ck_pitch;
    c.ck_off = (((uint32_t)c.base + (uint32_t)CELLS * (uint32_t)lane) & (uint32_t)d.ck_mask) * 4u;
    c.lds_rows = lds_rows;
    c.lds_halo = lds_halo;
    const auto uni = [](uint64_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v); };
    {
        const uint64_t x = (uint64_t)c.L * (uint64_t)((uint32_t)c.t_in / kTpBlock * kTpBlock);
        c.q0 = uni(x / c.T);
        c.r0 = uni(x % c.T);
        c.dq32 = uni(((uint64_t)c.L * kTpBlock) / c.T);
        c.dr32 = uni(((uint64_t)c.L * kTpBlock) % c.T);
        c.inv_T = 1.0f / (float)c.T;
        c.ev = 0;
        c.KL = c.KE = 0;
    }
    c.absum = 0.0f;
    c.lds_packets = lds_packets;
    c.lds_stage = 0;
}

// Band bookkeeping of the block that starts at frame tb (c.q0 / c.r0 are that frame's floor(L tb / T) and remainder): lane l
// works out floor(L t / T) for frame t = tb - 1 + l (l = 0 .. 33 are used) - x / T for x < 63 T < 2^32 by a float estimate
// and one correction each way, as in backtrace_rc_kernel - and, for the band step between its frame and the next one,
// which positions enter at the top (rule i) or leave at the bottom (rule ii) inside this tile (first position and count,
// packed).  A rule-i step after frame t is dealt with in frame t, a rule-ii step after frame t in frame t+1: bit F of c.ev <=>
// frame tb + F has cells to kill, KL of lane F and KE of lane F+1 say which.  ~45 vector and a dozen scalar instructions per block.
template <int CELLS>
__device__ __forceinline__ void band_block(TileCore<CELLS> &c, uint32_t tb, int lane)
{
    const uint32_t l1 = lane > 0 ? (uint32_t)lane - 1u : 0u;
    const uint32_t x = c.r0 + l1 * c.dr;
    uint32_t qe = (uint32_t)((float)x * c.inv_T);
    qe -= (qe * c.T > x) ? 1u : 0u;
    qe += (x - qe * c.T >= c.T) ? 1u : 0u;
    uint32_t qa = c.q0 + l1 * c.dq + qe;
    const uint32_t q_before = tb == 0 ? c.q0 : (c.r0 >= c.dr ? c.q0 - c.dq : c.q0 - c.dq - 1u);   // frame tb-1 (block 0: no step into frame 0)
    qa = lane == 0 ? q_before : qa;
    // floor(L (t+1) / T): the lane above's value (DPP wave_shl:1; lane 63 keeps its own, it is not used)
    const uint32_t qn = (uint32_t)__builtin_amdgcn_update_dpp((int)qa, (int)qa, 0x130, 0xF, 0xF, false);
    const uint32_t tile_lo = (uint32_t)c.base, tile_hi = (uint32_t)c.base + TileCore<CELLS>::kPositions;
    const uint32_t lo_a = c.lo_of(qa), lo_n = c.lo_of(qn);
    const uint32_t hi_a = c.hi_of(lo_a), hi_n = c.hi_of(lo_n);
    const uint32_t t = tb - 1u + (uint32_t)lane;          // (lane 0 of block 0 wraps: its step is void, q_before == q0)
    // rule ii: [lo(t), lo(t+1)) within the tile, killed after frame t+1 (bit l of ev, word read from lane F of KL)
    const uint32_t la = lo_a > tile_lo ? lo_a : tile_lo, lb = lo_n < tile_hi ? lo_n : tile_hi;
    const bool leave = la < lb;
    c.KL = leave ? (la - tile_lo) | ((lb - la) << 16) : 0u;
    // rule i: [hi(t), hi(t+1)) within the tile, killed after frame t (bit l-1 of ev, word read from lane F+1 of KE)
    const uint32_t ea = hi_a > tile_lo ? hi_a : tile_lo, eb = hi_n < tile_hi ? hi_n : tile_hi;
    const bool enter = ea < eb && t + 1u < c.T;
    c.KE = enter ? (ea - tile_lo) | ((eb - ea) << 16) : 0u;
    const uint64_t b_leave = __builtin_amdgcn_ballot_w64(leave), b_enter = __builtin_amdgcn_ballot_w64(enter);
    c.ev = (uint32_t)b_leave | (uint32_t)(b_enter >> 1);
}
// one block further
template <int CELLS>
__device__ __forceinline__ void band_advance(TileCore<CELLS> &c)
{
    c.q0 += c.dq32;
    c.r0 += c.dr32;
    if (c.r0 >= c.T) { c.r0 -= c.T; ++c.q0; }
}

// bytes of the contiguous block of rows that starts at row `first` (< T): 32 rows, fewer at the end of the array
template <int PITCH>
__device__ __forceinline__ uint32_t block_bytes(uint32_t T, uint32_t first)
{
    return (T - first < (uint32_t)kTpBlock ? T - first : (uint32_t)kTpBlock) * (uint32_t)PITCH;
}

// The log-prob rows of block k (k >= 0) into LDS at `dst`.  PITCH = bytes between two rows of a staged block in LDS.
// CONTIG = false (PITCH 256): rows are staged one by one (lane = column; any row stride of the caller's array; rows behind
// T - 1 repeat it).  CONTIG = true (PITCH = 4 V; the array's rows are contiguous, V columns): the block is copied as it lies in
// memory, 1 KB per LDS-DMA instruction - 4 (V = 64) or 3 (V = 39) instructions per block instead of 32; an LDS-DMA instruction
// costs the wave ~60 cycles to issue whatever it moves.
template <int PITCH, bool CONTIG, int CELLS>
__device__ __forceinline__ void stage_rows(const TileCore<CELLS> &c, int32_t k, uint32_t dst_lds, int lane)
{
    const uint32_t tb = (uint32_t)k * kTpBlock, last_row = c.T - 1;
    lchar_t dst = (lchar_t)(uintptr_t)dst_lds;
    if constexpr (!CONTIG) {
        const char *rp = c.lp + (size_t)(tb < last_row ? tb : last_row) * c.ld;
        if (tb + kTpBlock <= c.T) {
#pragma unroll
            for (int f = 0; f < kTpBlock; ++f) {
                __builtin_amdgcn_global_load_lds((gptr_t)(rp + c.lane_off), (lptr_t)(dst + f * kTpRowBytes), 4, 0, 0);
                rp += c.ld;
            }
        } else {
#pragma unroll
            for (int f = 0; f < kTpBlock; ++f) {
                __builtin_amdgcn_global_load_lds((gptr_t)(rp + c.lane_off), (lptr_t)(dst + f * kTpRowBytes), 4, 0, 0);
                rp += tb + f < last_row ? c.ld : 0;
            }
        }
    } else {
        // The pieces of a block are clamped to the one that holds the block's LAST BYTE.  A block starts on a 16-byte border
        // (the array's base is aligned, 32 rows are a multiple of 16 bytes), so that piece starts on a byte of the lattice and
        // stays inside its page; with V = 39 and T % 4 != 0 it ends up to 12 bytes behind row T - 1, which sum_rows keeps out of
        // the finiteness sum and no frame reads.  (A block behind the last one - the 256-position tile requests one, and
        // nobody reads it - repeats block 0: row T - 1 alone need not start on a 16-byte border.)
        const uint32_t first = tb < c.T ? tb : 0u;
        const uint32_t last_chunk = (block_bytes<PITCH>(c.T, first) - 1u) & ~15u;
        const char *bp = c.lp + (size_t)first * PITCH;
#pragma unroll
        for (int j = 0; j < TileRows<PITCH, CONTIG>::kRowDmas; ++j) {
            uint32_t off = (uint32_t)j * 1024u + (uint32_t)lane * 16u;
            off = off < last_chunk ? off : last_chunk;
            __builtin_amdgcn_global_load_lds((gptr_t)(bp + off), (lptr_t)(dst + j * 1024), 16, 0, 0);
        }
    }
}

// The tile below's packets of block k into LDS at `dst`: slot 32 k + f for frame f, clamped to the slots t_in .. last_slot this
// tile reads (sc1)
template <int CELLS>
__device__ __forceinline__ void stage_packets(const TileCore<CELLS> &c, int32_t k, uint32_t dst_lds, uint32_t last_slot, int lane)
{
    if (lane < kTpBlock) {
        uint32_t s = (uint32_t)k * kTpBlock + (uint32_t)lane;
        s = s < (uint32_t)c.t_in ? (uint32_t)c.t_in : (s > last_slot ? last_slot : s);
        __builtin_amdgcn_global_load_lds((gptr_t)(c.halo_in + (size_t)(s - (uint32_t)c.t_in) * 16), (lptr_t)(lchar_t)(uintptr_t)dst_lds, 16, 0, 16);
    }
}

// |log-prob| of the landed block k of rows (at `rows`) into c.absum: all reads first, then the adds.  Every 16 bytes of the
// slot hold a piece of the block (stage_rows: the ones behind the block's end repeat its last piece) - only a last block of
// V = 39 rows that does not end on a 16-byte border has a last piece with 1 to 3 floats of row T - 1 and then whatever lies
// behind the array: those do not count, in that piece and in its repeats.
template <int PITCH, bool CONTIG, int CELLS>
__device__ __forceinline__ void sum_rows(TileCore<CELLS> &c, int32_t k, uint32_t rows, int lane)
{
    const uint32_t r = rows + (uint32_t)lane * 16u;
    constexpr int kReads = TileRows<PITCH, CONTIG>::kSlot / 1024;
    f32x4 v[kReads];
#pragma unroll
    for (int j = 0; j < kReads; ++j) v[j] = lds_f32x4(r + j * 1024);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (CONTIG && PITCH % 16 != 0) {
        const uint32_t bytes = block_bytes<PITCH>(c.T, (uint32_t)k * kTpBlock);
        if (bytes & 15u) {      // (wave-uniform; at most once in a tile's life)
            const uint32_t last_chunk = bytes & ~15u, floats = (bytes & 15u) >> 2;
#pragma unroll
            for (int j = 0; j < kReads; ++j) {
                const bool last = (uint32_t)j * 1024u + (uint32_t)lane * 16u >= last_chunk;
#pragma unroll
                for (int i = 1; i < 4; ++i) v[j][i] = (last && (uint32_t)i >= floats) ? 0.0f : v[j][i];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kReads; ++j) c.absum += (__builtin_fabsf(v[j][0]) + __builtin_fabsf(v[j][1])) + (__builtin_fabsf(v[j][2]) + __builtin_fabsf(v[j][3]));
}

// Finiteness (as forward_ck: the scores-only form is valid for finite log-probs of sane magnitude), from the lanes' absum: a NaN
// fails the lattice, a magnitude of 1e30 or more sends it to the exact kernels (declines it where the band is too wide for them).
__device__ __forceinline__ void flag_finiteness(float absum, const Lattice &d, int32_t *m, int lane)
{
    const uint32_t abits = __builtin_bit_cast(uint32_t, absum) & 0x7fffffffu;
    if (__builtin_amdgcn_ballot_w64(abits > 0x7f800000u)) {
        if (lane == 0) atomicMin(&m[0], kStatusNaN);
    } else if (__builtin_amdgcn_ballot_w64(abits >= __builtin_bit_cast(uint32_t, 1e30f))) {
        if (lane == 0) atomicOr(&m[2], d.W <= kFastMaxBand ? kFlagExact : kFlagDeclined);
    }
}

// The terminal state: the HIGHEST live position of frame T-1 (align.py:99-101), over the tiles alive then.  `key` per lane:
// (position + 1) << 32 | score bits of the lane's highest live cell in the band of frame T-1, 0 if none.  The wave's maximum goes
// into the lattice's TileAux; the last of its final tiles to arrive writes the end position, the score and the status to `m`.
__device__ __forceinline__ void close_lattice(unsigned long long key, const Lattice &d, TileAux *aux, int32_t *m, int lane)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off);
        key = o > key ? o : key;
    }
    if (lane == 0) {
        TileAux *a = aux + d.idx;
        if (key) atomicMax(&a->best, key);
        __threadfence();
        const uint32_t n = atomicAdd(&a->arrived, 1u) + 1u;
        if (n == (uint32_t)d.n_final) {
            __threadfence();
            const unsigned long long best = atomicMax(&a->best, 0ull);
            const int fl = atomicOr(&m[2], 0);
            if (fl & (kFlagExact | kFlagDeclined)) {
                m[1] = -1;   // declined: the exact kernels redo the lattice (or ka_batch_finish hands it to the generic ones)
            } else if (best == 0) {
                m[1] = -1;
                atomicMin(&m[0], kStatusEmptyBeam);
            } else {
                m[1] = (int32_t)(best >> 32) - 1;
                m[3] = (int32_t)(uint32_t)best;
            }
        }
    }
}

}  // namespace ka
