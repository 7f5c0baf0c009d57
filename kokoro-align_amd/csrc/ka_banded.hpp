// ka_banded.hpp — best path over a caller-given band (ka_ctc_best_path_banded[_batch]_f32).
// Included by ka_banded.hip only (it holds non-template kernels).
//
// The recurrence is ka_device.hpp's with ONE change: the band's low end comes from a table,
//   frame t:  lo = band_lo[t], hi = min(lo + B, L)         (align.py:64-65 replaced; everything else align.py:62-107)
// with 0 <= band_lo[t] < L and band_lo[t] <= band_lo[t+1], any step.  prep_banded_kernel checks the table (and the labels)
// before any other kernel reads a value of it; a lattice with a bad table is flagged and skipped by every kernel behind it.
//
// One wavefront per lattice (band <= kFastMaxBand, V <= 64, max_move <= 4): ka_device.hpp's ring, cells, codes and band
// masks as forward_w16 uses them (position p at slot p & 1023, lane (p >> 4) & 63, cell p & 15; 16 x 2-bit codes = one dword
// per lane and frame, stored [t/4][lane][t%4]).  What is new is the band step:
//   * prep writes the table once more, shifted and padded (tab[i] = band_lo[min(i+1, T-1)], whole groups of four plus one
//     group), so the frame loop takes the next four low ends with ONE aligned scalar load, a group ahead of their use, and a
//     frame pays one scalar compare (next lo != lo) and a branch, as it does for the Bresenham step of forward_w16;
//   * a step of one position toggles one lane bit per band edge (band_toggle); any larger step rebuilds the sixteen lane
//     masks from (lo, hi) in closed form (band_rebuild): there is no catch-up loop, so no step is too large for it;
//   * as lo passes blocks of 16 their lanes are re-labelled for the block 64 (or 128, ...) above.  A re-labelled lane starts
//     dead; a lane's halo (the three cells below its block) is valid iff its left neighbour HELD the block below the lane's
//     block in the frame before, which is asked directly (left's old block + 1 == own block): right for a step of a whole
//     block of 16, of more than 64 positions, of the whole ring and past the old hi + max_move - 1, where nothing survives.
//   Cells that enter the band start dead and cells that leave it die through the band masks alone: a frame's cells outside
//   [lo, hi) are written -inf and not live, whatever they held.
// The walk back (backtrace_banded_wave_kernel) reads a window of 8 blocks per 16 frames, the next window in flight while the
// current one is walked, and writes best_path, best_labels and best_scores of those 16 frames together.
//
// Generic form (any band, any V, max_move <= 255): forward_generic_kernel's scheme with the table; not tuned.
#pragma once
#include "ka_device.hpp"

namespace ka {

constexpr int kBandFlagBadTable = 8;   // meta flags: band_lo is not a valid table (status KA_ERR_BAD_ARGS)
constexpr int kBandMinWaves = 4;       // __launch_bounds__ of the one-wavefront forward kernels: wavefronts per SIMD

typedef __attribute__((address_space(4))) const v4i_t *cc4_t;   // constant address space: scalar loads

// ---------------------------------------------------------------------------------------
// preparation: labels (validate, scale by 4, zero-pad), the band table (validate, shift, pad)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_banded_kernel(const BandLattice *__restrict__ lats, int32_t *meta)
{
    const BandLattice &d = lats[blockIdx.x];
    int32_t *m = meta_of(meta, d.idx);
    int bad = 0, zero = 0;
    for (int i = threadIdx.x; i < d.labx_len; i += blockDim.x) {
        int v = 0;
        if (i < d.S) {
            int l = d.labels[i];
            if (l < 0 || l >= d.V) { bad = 1; l = 0; }
            if (l == 0) zero = 1;
            v = l * 4;
        }
        d.labx[i] = v;
    }
    if (bad) atomicMin(&m[0], kStatusBadLabel);
    if (zero) atomicOr(&m[2], kFlagZeroLabel);
    // the table: in range and non-decreasing
    int bad_tab = 0;
    for (int i = threadIdx.x; i < d.T; i += blockDim.x) {
        const int v = d.band_lo[i];
        if (v < 0 || v >= d.L) bad_tab = 1;
        if (i > 0 && d.band_lo[i - 1] > v) bad_tab = 1;
    }
    if (__syncthreads_or(bad_tab)) {
        if (threadIdx.x == 0) {
            atomicMin(&m[0], kStatusBadArgs);
            atomicOr(&m[2], kBandFlagBadTable);
            m[1] = -1;
        }
        return;
    }
    if (d.tab)
        for (int i = threadIdx.x; i < d.tab_len; i += blockDim.x) d.tab[i] = d.band_lo[i + 1 < d.T ? i + 1 : d.T - 1];
}

// ---------------------------------------------------------------------------------------
// forward DP, one wavefront per lattice, every cell's code stored
// ---------------------------------------------------------------------------------------
template <int M, bool ZL>
__device__ __forceinline__ void forward_banded_wave(const BandLattice &d, int32_t *meta)
{
    constexpr int D = kRowDepth;
    const int lane = threadIdx.x;
    const uint32_t T = (uint32_t)__builtin_amdgcn_readfirstlane(d.T);
    const uint32_t L = (uint32_t)__builtin_amdgcn_readfirstlane(d.L);
    const uint32_t B = (uint32_t)__builtin_amdgcn_readfirstlane(d.beam);
    const float NINF = ninf();

    uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane(d.band_lo[0]);   // band of frame 0 (the table is valid: prep)
    uint32_t hi = (L - lo < B) ? L : lo + B;
    uint32_t blo = lo >> 4;
    int blk = (int)blo + ((lane - (int)blo) & 63);   // block of 16 positions this lane currently owns
    int prev_blk = blk;                              // ... and owned before the last re-labelling

    float sc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) sc[k] = NINF;
    // virtual state before frame 0 (align.py:57-58): position 0, which a lane holds only while block 0 is on the ring
    const bool holds0 = blk == 0;
    if (holds0) sc[0] = 0.0f;
    uint32_t pres2 = holds0 ? 1u : 0u;      // bit 2k: cell k holds a live state
    bool pend_reset = false;                // wave-uniform: lanes were re-labelled for this frame
    bool reset_lane = false;                // per lane: this lane was re-labelled

    int la[8];
    float vz[8];
    gci32_t labx = (gci32_t)d.labx;
    load_block_labels(labx, blk, la);
#pragma unroll
    for (int i = 0; i < 8; ++i) vz[i] = (ZL && la[i] == 0) ? NINF : __builtin_inff();

    BandMasks mk;
    band_rebuild(mk, lo, hi);
    uint32_t band2 = band_pairs(lo, hi, blk);

    // lanes >= V read column 0 (a valid address); their value is never selected (labels < V)
    const uint32_t lane_off = (lane < d.V ? (uint32_t)lane : 0u) * 4u;
    const char *lp = reinterpret_cast<const char *>(d.lp);
    const size_t ld = (size_t)d.ld * 4;  // row pitch in bytes
    float rows[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const uint32_t tt = (uint32_t)i < T ? (uint32_t)i : T - 1;
        rows[i] = row_load(lane_off, lp + (size_t)tt * ld);
    }
    // (the counted wait inside the loop assumes the steady-state number of younger operations: land the first rows all)
#pragma unroll
    for (int i = 0; i < D; ++i) row_wait<0>(rows[i]);
    float e[8], e0[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = bperm(la[i], rows[0]);
    e0[0] = first_lane(rows[0]);
    float absum = __builtin_fabsf(rows[0]);   // NaN detector: sum over frames of |lp[t, lane]|

    const uint32_t *bp = reinterpret_cast<const uint32_t *>(d.bp);   // wave-uniform row base
    const uint32_t lane_store_off = (uint32_t)lane * 16u;            // codes: [t/4][lane][t%4] dwords

    // low ends of frames tb+1 .. tb+4, one aligned scalar load per group, the next group's in flight (prep padded the table)
    cc4_t tab = (cc4_t)(uintptr_t)d.tab;
    v4i_t step_next = tab[0];

    const char *row_ahead = lp + (size_t)(D < T ? D : T - 1) * ld;   // row min(t+D, T-1) of the current frame t
    for (uint32_t tb = 0; tb < T; tb += D) {
        const v4i_t step = step_next;
        step_next = tab[(tb >> 2) + 1];
        uint32_t gw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) asm("" : "=v"(gw[i]));
#pragma unroll
        for (int dd = 0; dd < D; ++dd) {
            const uint32_t t = tb + dd;
            if (t < T) {
                // halos of frame t, then the reset of the lanes re-labelled in frame t-1 (they still held the scores of their
                // OLD block, which their right neighbour has just read as its halo)
                float h1 = wave_ror1(sc[15]), h2 = wave_ror1(sc[14]), h3 = wave_ror1(sc[13]);
                if (__builtin_expect(pend_reset, 0)) {
                    asm volatile("" ::: "memory");  // keep this rare block a real branch
                    // a halo is what the left neighbour held in frame t-1: valid iff that was the block below this lane's
                    const int left_old = __builtin_amdgcn_mov_dpp(prev_blk, 0x13C, 0xF, 0xF, false);
                    const bool kill = left_old + 1 != blk;
                    h1 = kill ? NINF : h1;
                    h2 = kill ? NINF : h2;
                    h3 = kill ? NINF : h3;
#pragma unroll
                    for (int k = 0; k < 16; ++k) sc[k] = reset_lane ? NINF : sc[k];
                    pres2 = reset_lane ? 0u : pres2;
                    prev_blk = blk;
                    pend_reset = false;
                }
                // A. band of frame t+1 from the table; re-label the lanes whose block lo has passed
                const uint32_t nlo = (uint32_t)(dd == 0 ? step.x : dd == 1 ? step.y : dd == 2 ? step.z : step.w);
                bool moved = false;
                if (__builtin_expect(nlo != lo, 0)) {   // (prep repeats the last low end behind frame T-1: no step into frame T)
                    asm volatile("" ::: "memory");  // a real branch: the common frame pays a compare and a jump
                    moved = true;
                    if ((nlo >> 4) != blo) {
                        blo = nlo >> 4;
                        const int nb = (int)blo + ((lane - (int)blo) & 63);
                        prev_blk = blk;
                        reset_lane = nb != blk;
                        if (nb != blk) {
                            blk = nb;
                            load_block_labels(labx, blk, la);
                            // consume the loads HERE (see forward_w16): no every-frame s_waitcnt vmcnt(0) at the merge point
#pragma unroll
                            for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(la[i]));
                        }
                        pend_reset = true;
                    }
                }
                // B. row t+1 (its emissions are gathered while frame t is computed); counted wait as in forward_w16: the
                // same vector-memory operations are in flight
                if (dd < D - 1) row_wait<D - 1>(rows[(dd + 1) % D]); else row_wait<D - 2>(rows[(dd + 1) % D]);
                const float rn = rows[(dd + 1) % D];
                e0[(dd + 1) & 1] = first_lane(rn);
                absum += __builtin_fabsf(rn);
                // C. frame t
                uint32_t word = 0;
                frame_cells<M, ZL, 15>(sc, h1, h2, h3, e, vz, e0[dd & 1], mk, NINF, word, la, rn);
                gw[dd] = word;
                pres2 = live_pairs(pres2, word, band2);
                row_reload(rows[dd], lane_off, row_ahead);
                row_ahead += t + D + 1 < T ? ld : 0;
                // D. lane masks of frame t+1
                if (moved) {
                    const uint32_t nhi = (L - nlo < B) ? L : nlo + B;
                    if (nhi - hi <= 1u && nlo - lo <= 1u) {
                        if (nhi != hi) band_toggle(mk, hi);
                        band_toggle(mk, lo);
                    } else {
                        band_rebuild(mk, nlo, nhi);
                    }
                    band2 = band_pairs(nlo, nhi, blk);
                    lo = nlo;
                    hi = nhi;
                    if (ZL && pend_reset) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) vz[i] = la[i] == 0 ? NINF : __builtin_inff();
                    }
                }
            }
        }
        const u32x4 words = {gw[0], gw[1], gw[2], gw[3]};
        // (s_nop 1: a store wider than 64 bits reads its data registers for two more wait states, see forward_ck)
        asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" : : "v"(lane_store_off), "v"(words), "s"(bp + (size_t)tb * 64) : "memory");
    }
    // drain the row prefetches that are still in flight (see forward_w16)
#pragma unroll
    for (int i = 0; i < D; ++i) row_wait<0>(rows[i]);

    int32_t *m = meta_of(meta, d.idx);
    if (__builtin_amdgcn_ballot_w64((__builtin_bit_cast(uint32_t, absum) & 0x7fffffffu) > 0x7f800000u)) {   // a NaN log-prob
        if (lane == 0) {
            m[1] = -1;
            atomicMin(&m[0], kStatusNaN);
        }
        return;
    }
    // terminal state: the HIGHEST live position of frame T-1 (align.py:99-101)
    int best = -1;
    if (pres2) best = blk * 16 + ((31 - __clz((int)pres2)) >> 1);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(best, off);
        best = o > best ? o : best;
    }
    if (best < 0) {
        if (lane == 0) {
            m[1] = -1;
            atomicMin(&m[0], kStatusEmptyBeam);
        }
    } else if ((best >> 4) == blk) {
        float v = sc[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) v = (best & 15) == k ? sc[k] : v;
        m[1] = best;
        m[3] = __builtin_bit_cast(int32_t, v);
    }
}

// Two kernels per max_move over the same lattices, as forward_w16_kernel: ZL = the transcript contains label 0.
template <int M, bool ZL>
__global__ __launch_bounds__(64, kBandMinWaves) void forward_banded_wave_kernel(const BandLattice *__restrict__ lats, int32_t *meta)
{
    const BandLattice &d = lats[blockIdx.x];
    const int flags = __builtin_amdgcn_readfirstlane(meta_of(meta, d.idx)[2]);
    if (flags & kBandFlagBadTable) return;
    if (((flags & kFlagZeroLabel) != 0) != ZL) return;
    forward_banded_wave<M, ZL>(d, meta);
}

// ---------------------------------------------------------------------------------------
// the walk back, one wavefront per lattice: path, labels and scores of 16 frames at a time
//
// A path drops at most 3 positions per frame.  The chunk entered at position p (its last frame) stays within [p - 45, p];
// the chunk below it within [p - 93, p]: its window of 8 blocks from block (p - 96) >> 4 is loaded while the current
// chunk is walked.  Window register r[v]: lane = (f & 7) * 8 + j holds the code dword of frame 8 v + (f & 7), block j.
// ---------------------------------------------------------------------------------------
constexpr int kBandBtChunk = 16;
__device__ __forceinline__ int band_bt_window(int p_entry)
{
    const int lo = p_entry - 6 * kBandBtChunk;
    return (lo > 0 ? lo : 0) >> 4;
}
__device__ __forceinline__ void band_bt_load(uint32_t (&r)[2], gcu32_t bp, int t0, int n, int w0, int lane)
{
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int f = 8 * v + (lane >> 3);
        const int t = t0 + f;
        const size_t at = (size_t)(t >> 2) * 256 + (size_t)((w0 + (lane & 7)) & 63) * 4 + (size_t)(t & 3);
        r[v] = f < n ? bp[at] : 0u;
    }
}
__global__ __launch_bounds__(64) void backtrace_banded_wave_kernel(const BandLattice *__restrict__ lats, const int32_t *meta)
{
    const BandLattice &d = lats[blockIdx.x];
    const int lane = threadIdx.x;
    int p = __builtin_amdgcn_readfirstlane(meta[4 * (size_t)d.idx + 1]);
    if (p < 0) return;   // no path: the status says why
    const int T = __builtin_amdgcn_readfirstlane(d.T);
    gcu32_t bp = (gcu32_t)d.bp;
    gci32_t labx = (gci32_t)d.labx;
    gcf32_t lp = (gcf32_t)d.lp;
    const size_t ld = (size_t)d.ld;
    int t0 = ((T - 1) / kBandBtChunk) * kBandBtChunk;
    int n = T - t0;
    int w = band_bt_window(p + 3 * kBandBtChunk);   // the tail chunk is entered at the end position itself
    uint32_t cur[2], nxt[2] = {0u, 0u};
    band_bt_load(cur, bp, t0, n, w, lane);
    for (;;) {
        const int t1 = t0 - kBandBtChunk;
        const int wn = band_bt_window(p);
        if (t1 >= 0) band_bt_load(nxt, bp, t1, kBandBtChunk, wn, lane);
        const uint32_t c0 = blank_to_uniform(cur[0]), c1 = blank_to_uniform(cur[1]);
        int q = p - 16 * w;   // position relative to the window: 0 .. 127
        int pathv = 0;
#pragma unroll
        for (int f = kBandBtChunk - 1; f >= 0; --f) {
            if (f < n) {
                const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)(f >= 8 ? c1 : c0), (f & 7) * 8 + (q >> 4));
                pathv = lane == f ? q : pathv;
                q -= bp_decode(word >> ((q * 2) & 31));
            }
        }
        if (lane < n) {
            const int pos = pathv + 16 * w;
            const int t = t0 + lane;
            const int lab = (pos & 1) ? (labx[pos >> 1] >> 2) : 0;
            ((gi32_t)d.path)[t] = pos;
            ((gi32_t)d.lab_out)[t] = lab;
            ((gf32_t)d.sc_out)[t] = lp[(size_t)t * ld + (size_t)lab];
        }
        if (t1 < 0) break;
        p = q + 16 * w;
        cur[0] = nxt[0];
        cur[1] = nxt[1];
        w = wn;
        t0 = t1;
        n = kBandBtChunk;
    }
}

// ---------------------------------------------------------------------------------------
// generic form: any band, any V, max_move <= 255.  One 256-thread workgroup per lattice, score columns double-buffered in
// global memory, one byte of back-pointer per band cell (forward_generic_kernel's scheme with the table).  Not tuned.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void forward_banded_generic_kernel(const BandLattice *__restrict__ lats, int32_t *meta)
{
    const BandLattice &d = lats[blockIdx.x];
    const int tid = threadIdx.x;
    int32_t *m = meta_of(meta, d.idx);
    if (m[2] & kBandFlagBadTable) return;
    const int64_t T = d.T, L = d.L, B = d.beam;
    const int M = d.max_move;
    const int64_t W = d.W;
    // a NaN log-prob is an error (found by its bits: the library is built with -fno-honor-nans)
    int nan = 0;
    for (int64_t i = tid; i < T * (int64_t)d.V; i += 256) {
        const uint32_t b = __builtin_bit_cast(uint32_t, d.lp[(size_t)(i / d.V) * (size_t)d.ld + (size_t)(i % d.V)]);
        if ((b & 0x7fffffffu) > 0x7f800000u) nan = 1;
    }
    if (__syncthreads_or(nan)) {
        if (tid == 0) {
            m[1] = -1;
            atomicMin(&m[0], kStatusNaN);
        }
        return;
    }
    float *scA = d.col, *scB = d.col + L;
    uint8_t *prA = reinterpret_cast<uint8_t *>(d.col + 2 * L), *prB = prA + L;
    uint8_t *bp = reinterpret_cast<uint8_t *>(d.bp);
    for (int64_t p = tid; p < L; p += 256) { prA[p] = 0; prB[p] = 0; }
    __syncthreads();
    if (tid == 0) { scA[0] = 0.0f; prA[0] = 1; }
    __syncthreads();
    int64_t plo = 0, phi = 1;
    for (int64_t t = 0; t < T; ++t) {
        const int64_t lo = d.band_lo[t];
        const int64_t hi = (L - lo < B) ? L : lo + B;
        const float *row = d.lp + (size_t)t * (size_t)d.ld;
        for (int64_t p = lo + tid; p < hi; p += 256) {
            const int lab = (p & 1) ? (d.labx[p >> 1] >> 2) : 0;
            const float e = row[lab];
            float best = ninf();
            int bj = 0;
            for (int j = 0; j < M; ++j) {
                const int64_t u = p - j;
                if (u < 0) break;
                const bool pres = (u >= plo && u < phi) ? prA[u] != 0 : false;
                float c = pres ? scA[u] + e : ninf();
                if (j > 0 && (j & 1) == 0 && lab == 0) c = ninf();
                if (j == 0 || c > best) { best = c; bj = j; }
            }
            const int64_t ub = p - bj;
            prB[p] = (ub >= plo && ub < phi) ? prA[ub] : 0;
            scB[p] = best;
            bp[(size_t)t * (size_t)W + (size_t)(p - lo)] = (uint8_t)bj;
        }
        __syncthreads();
        { float *x = scA; scA = scB; scB = x; }
        { uint8_t *x = prA; prA = prB; prB = x; }
        plo = lo;
        phi = hi;
    }
    // highest live position of the last frame
    __shared__ int64_t s_best;
    if (tid == 0) s_best = -1;
    __syncthreads();
    int64_t mine = -1;
    for (int64_t p = plo + tid; p < phi; p += 256)
        if (prA[p]) mine = p;
    if (mine >= 0) atomicMax((long long *)&s_best, (long long)mine);
    __syncthreads();
    if (tid == 0) {
        if (s_best < 0) {
            m[1] = -1;
            atomicMin(&m[0], kStatusEmptyBeam);
        } else {
            m[1] = (int32_t)s_best;
            m[3] = __builtin_bit_cast(int32_t, scA[s_best]);
        }
    }
}

__global__ __launch_bounds__(64) void backtrace_banded_generic_kernel(const BandLattice *__restrict__ lats, const int32_t *meta)
{
    const BandLattice &d = lats[blockIdx.x];
    int64_t p = meta[4 * (size_t)d.idx + 1];
    if (p < 0 || threadIdx.x != 0) return;
    const int64_t T = d.T, W = d.W;
    const uint8_t *bp = reinterpret_cast<const uint8_t *>(d.bp);
    for (int64_t t = T - 1; t >= 0; --t) {
        const int lab = (p & 1) ? (d.labx[p >> 1] >> 2) : 0;
        d.path[t] = (int32_t)p;
        d.lab_out[t] = lab;
        d.sc_out[t] = d.lp[(size_t)t * (size_t)d.ld + (size_t)lab];
        p -= bp[(size_t)t * (size_t)W + (size_t)(p - d.band_lo[t])];
    }
}

}  // namespace ka
