// ka_determined.hpp — the determined prefix of a resumed best path (ka_ctc_best_path_determined,
// ka_ctc_best_path_tracking_determined): device helpers of ka_determined.hip.
//
// After a forward pass of ka_banded.hpp under the caller's boundary conditions every band cell of every frame holds the code of
// its chosen move j*_t(p).  The walk here follows ALL live cells of the last frame back at once,
//   anc_{T-1} = the live cells after frame T-1,   anc_{t-1} = { p - j*_t(p) : p in anc_t },
// until one cell is left: determined = 1 + max{ t in [-1, T-1] : |anc_t| == 1 }, -1 without such a t (anc_{-1} is a set of
// cells of the start row).  Frames [0, determined) of the path are the same whichever live cell it ends at, and whatever
// frames follow.  An ancestor of a live cell is live, so only codes of live cells are read.
//
// One wavefront per lattice: the set is a bit mask over the ring of 1024 slots, position p at lane (p >> 4) & 63, cell p & 15,
// bit 2 (p & 15), as pres2.  A band is at most kFastMaxBand wide and a move at most 3, so the cells of one frame and their
// ancestors never share a slot: the walk needs no table, and a re-labelled lane needs no care.  One frame back is bit-parallel
// over a lane's sixteen cells; what falls below cell 0 goes to the lane that holds the block below (wave_rol1).
#pragma once
#include "ka_banded.hpp"

namespace ka {

// lane i <- lane i+1, lane 63 <- lane 0 (DPP wave_rol:1): the opposite direction of wave_ror1
__device__ __forceinline__ uint32_t wave_rol1(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x134, 0xF, 0xF, false);
}

// one frame back: `m` the set's cells of this lane's slots (pair-bits), `code` the lane's stored code dword of the frame
__device__ __forceinline__ uint32_t determined_step(uint32_t m, uint32_t code)
{
    const uint32_t mv = ~blank_to_uniform(code);   // move = 3 & ~code, bit-parallel
    const uint32_t lo1 = mv & 0x55555555u, hi1 = (mv >> 1) & 0x55555555u;   // the two bits of every cell's move, at the pair-bit
    const uint32_t sel0 = m & ~lo1 & ~hi1, sel1 = m & lo1 & ~hi1, sel2 = m & ~lo1 & hi1, sel3 = m & lo1 & hi1;
    const uint64_t y = ((uint64_t)sel0 << 32) | (((uint64_t)sel1 << 32) >> 2) | (((uint64_t)sel2 << 32) >> 4) | (((uint64_t)sel3 << 32) >> 6);
    // the high word stays; the low word fell below cell 0: it belongs to the lane below, over the ring (lane 0 hands to lane 63)
    return (uint32_t)(y >> 32) | wave_rol1((uint32_t)y);
}

// exactly one cell in the whole set (wave-uniform)
__device__ __forceinline__ bool determined_single(uint32_t m)
{
    const uint64_t many = __builtin_amdgcn_ballot_w64(__builtin_popcount(m) > 1);
    const uint64_t any = __builtin_amdgcn_ballot_w64(m != 0u);
    return many == 0ull && __builtin_popcountll(any) == 1;
}

// The walk of one lattice by one wavefront; every lane returns `determined`.  `fin` is the last row the forward pass wrote (NaN
// = dead), read at the blocks the ring held in frame T-1.  A lattice whose forward pass did not run to its end (a bad table, a
// +inf start cell, a NaN log-prob) or left a bad label has no live cell: -1, and nothing of it is read.
__device__ __forceinline__ int determined_wave(const BandLattice &d, const float *fin_row, const int32_t *meta)
{
    const int lane = threadIdx.x;
    const int st = __builtin_amdgcn_readfirstlane(meta[4 * (size_t)d.idx]);
    if (st != kStatusOk && st != kStatusEmptyBeam) return kUndetermined;
    const int T = __builtin_amdgcn_readfirstlane(d.T);
    const uint32_t L = (uint32_t)__builtin_amdgcn_readfirstlane(d.L);
    uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane(d.band_lo[T - 1]);
    lo = lo < L ? lo : L - 1u;   // (a table some forward pass used is in range; whatever it holds, no read leaves the row)
    const uint32_t blo = lo >> 4;
    const uint32_t blk = blo + (((uint32_t)lane - blo) & 63u);
    gcu32_t fin = (gcu32_t)reinterpret_cast<const uint32_t *>(fin_row);
    uint32_t m = 0u, row[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {   // (sixteen loads in flight; a cell at or above L reads the row's last cell)
        const uint32_t p = blk * 16u + (uint32_t)k;
        row[k] = fin[p < L ? p : L - 1u];
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool live = blk * 16u + (uint32_t)k < L && row_cell_live(row[k]);
        m |= live ? 1u << (2 * k) : 0u;
    }
    // codes: [t/4][lane][t%4] dwords, one dwordx4 per lane and four frames, the group below in flight
    const u32x4 *bp = reinterpret_cast<const u32x4 *>(d.bp) + lane;
    int g = (T - 1) >> 2;
    u32x4 cur = bp[(size_t)g * 64], nxt = cur;
    int det = kUndetermined;
    bool found = false;
    for (; g >= 0 && !found; --g) {
        if (g > 0) nxt = bp[(size_t)(g - 1) * 64];
#pragma unroll
        for (int dd = 3; dd >= 0; --dd) {
            const int t = 4 * g + dd;
            if (t < T) {   // (wave-uniform, like `found`: the rotate below runs with every lane)
                const bool one = determined_single(m);
                det = one && !found ? t + 1 : det;
                found = found || one;
                m = determined_step(m, dd == 0 ? cur.x : dd == 1 ? cur.y : dd == 2 ? cur.z : cur.w);
            }
        }
        cur = nxt;
    }
    if (!found && determined_single(m)) det = 0;   // the cells of the start row: frame -1
    return det;
}

// The generic form's walk, by a 256-thread workgroup: two position sets over the lattice's columns (the forward pass's two
// liveness columns, free by now), a shared counter.  `lo_t` comes from the table (a tracking call's: the one its forward pass
// wrote).  Every thread returns `determined`.  Not tuned.
__device__ __forceinline__ int determined_generic(const BandLattice &d, const float *fin_row, const int32_t *meta)
{
    __shared__ int s_count;
    const int tid = threadIdx.x;
    const int st = meta[4 * (size_t)d.idx];
    if (st != kStatusOk && st != kStatusEmptyBeam) return kUndetermined;
    const int64_t T = d.T, L = d.L, B = d.beam, W = d.W;
    const int M = d.max_move;
    uint8_t *cur = reinterpret_cast<uint8_t *>(d.col + 2 * L), *prev = cur + L;
    const uint8_t *bp = reinterpret_cast<const uint8_t *>(d.bp);
    const uint32_t *fin = reinterpret_cast<const uint32_t *>(fin_row);
    if (tid == 0) s_count = 0;
    __syncthreads();
    int mine = 0;
    for (int64_t p = tid; p < L; p += 256) {
        const uint8_t live = row_cell_live(fin[p]) ? 1 : 0;
        cur[p] = live;
        prev[p] = 0;
        mine += live;
    }
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    int count = s_count;
    if (count == 0) return kUndetermined;
    // anc_t lies in frame t's band
    for (int64_t t = T - 1; t >= 0; --t) {
        if (count == 1) return (int)t + 1;
        int64_t lo = d.band_lo[t];
        lo = lo < 0 ? 0 : lo < L ? lo : L - 1;   // (in range already: a table some forward pass used)
        const int64_t hi = (L - lo < B) ? L : lo + B;
        __syncthreads();   // every thread has read s_count
        if (tid == 0) s_count = 0;
        for (int64_t p = lo + tid; p < hi; p += 256)
            if (cur[p]) {
                cur[p] = 0;   // (leaves the column clear for the frame after next)
                int64_t q = p - bp[(size_t)t * (size_t)W + (size_t)(p - lo)];
                q = q < 0 ? 0 : q;   // (a live cell's move does not leave the lattice)
                prev[q] = 1;
            }
        __syncthreads();
        const int64_t qlo = lo - (M - 1) > 0 ? lo - (M - 1) : 0;
        mine = 0;
        for (int64_t q = qlo + tid; q < hi; q += 256) mine += prev[q];
        if (mine) atomicAdd(&s_count, mine);
        __syncthreads();
        count = s_count;
        uint8_t *x = cur;
        cur = prev;
        prev = x;
    }
    return count == 1 ? 0 : kUndetermined;
}

}  // namespace ka
