// ka_banded.hpp — best path over a caller-given band (ka_ctc_best_path_banded[_batch]_f32).
// Included by ka_banded.hip, which holds the table's own kernels (preparation, the two walks back), by ka_tracking.hip for
// the self-steering band of ka_ctc_best_path_tracking (section 4.32), by ka_resume.hip for the caller's boundary conditions
// of ka_ctc_best_path_resume (section 4.34) and by ka_tracking_resume.hip for the two together (section 4.35): what they share
// lives here, the table's check and the walks back included.
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

// labels of one lattice: validate, scale by 4, zero-pad (every thread of a 256-thread workgroup)
__device__ __forceinline__ void prep_labels(const BandLattice &d, int32_t *m)
{
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
}

// the band table of one lattice: validate (in range and non-decreasing), shift, pad (every thread of a 256-thread workgroup);
// false, with the lattice flagged, for an invalid table
__device__ __forceinline__ bool prep_band_table(const BandLattice &d, int32_t *m)
{
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
        return false;
    }
    if (d.tab)
        for (int i = threadIdx.x; i < d.tab_len; i += blockDim.x) d.tab[i] = d.band_lo[i + 1 < d.T ? i + 1 : d.T - 1];
    return true;
}

// ---------------------------------------------------------------------------------------
// where the band's low end comes from: the frame loops below ask a policy for the low end of frame t+1 while sc[] / pres2
// hold the cells of frame t-1
// ---------------------------------------------------------------------------------------
// First maximum of the scores over the live cells of a wavefront's ring, in ascending position (np.argmax over the compacted
// live list: ties to the lowest position, -0.0 == +0.0, an all -inf list gives its lowest live position); -1 without a live
// cell.  Per lane a float compare from the top cell down, then six butterfly steps over one orderable 64-bit key: the float's
// order-preserving bits above, ~position below.  The result is a position some lane holds live, whatever the floats are.
__device__ __forceinline__ int wave_best_live(const float (&sc)[16], uint32_t pres2, int blk)
{
    float best = 0.0f;
    int bk = -1;
#pragma unroll
    for (int k = 15; k >= 0; --k) {
        const bool take = ((pres2 >> (2 * k)) & 1u) != 0 && (bk < 0 || sc[k] >= best);
        best = take ? sc[k] : best;
        bk = take ? k : bk;
    }
    uint32_t b = __builtin_bit_cast(uint32_t, best);
    b = b == 0x80000000u ? 0u : b;   // -0.0 orders as +0.0
    uint32_t kh = b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
    uint32_t kl = ~(uint32_t)(blk * 16 + bk);
    kh = bk < 0 ? 0u : kh;   // (a live cell's key is never 0: kl = 0 would be position 2^32 - 1)
    kl = bk < 0 ? 0u : kl;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t oh = (uint32_t)__shfl_xor((int)kh, off), ol = (uint32_t)__shfl_xor((int)kl, off);
        const bool g = oh > kh || (oh == kh && ol > kl);
        kh = g ? oh : kh;
        kl = g ? ol : kl;
    }
    const uint32_t h = (uint32_t)__builtin_amdgcn_readfirstlane((int)kh), l = (uint32_t)__builtin_amdgcn_readfirstlane((int)kl);
    return (h | l) == 0u ? -1 : (int)~l;
}

// the highest live position of a wavefront's ring, -1 without a live cell
__device__ __forceinline__ int wave_highest_live(uint32_t pres2, int blk)
{
    int best = -1;
    if (pres2) best = blk * 16 + ((31 - __clz((int)pres2)) >> 1);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(best, off);
        best = o > best ? o : best;
    }
    return best;
}

// the caller's table: prep shifted and padded it, one aligned scalar load per group of four frames, a group ahead of its use
struct BandFromTable {
    static constexpr bool kTracking = false;
    static constexpr bool kStart = false;   // the lattice's boundary conditions are the reference's (BandResume: the caller's)
    typedef v4i_t Group;   // low ends of the four frames behind a group's first
    cc4_t tab;
    v4i_t step_next;
    static __device__ __forceinline__ uint32_t first_lo(const BandLattice &d) { return (uint32_t)__builtin_amdgcn_readfirstlane(d.band_lo[0]); }
    __device__ __forceinline__ void begin(const BandLattice &d)
    {
        tab = (cc4_t)(uintptr_t)d.tab;
        step_next = tab[0];
    }
    __device__ __forceinline__ Group group(uint32_t tb, uint32_t, uint32_t, int)
    {
        const v4i_t step = step_next;
        step_next = tab[(tb >> 2) + 1];
        return step;
    }
    __device__ __forceinline__ uint32_t next_lo(const Group &step, int dd, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const float (&)[16],
                                                uint32_t, int)
    {
        return (uint32_t)(dd == 0 ? step.x : dd == 1 ? step.y : dd == 2 ? step.z : step.w);
    }
    __device__ __forceinline__ bool end_at_best() const { return false; }
};

// the self-steering band (ka_ctc_best_path_tracking): lo_0 = 0; frame t > 0 with t % period == 0 takes
//   lo_t = min(max(lo_{t-1}, c - B / 2), L - 1),   c = the first maximum of the scores after frame t-2 over the live cells
// (no live cell: lo_{t-1}); every other frame keeps lo_{t-1}.  The lag of two frames is what the loop has at hand where it needs
// the next low end: in step A of frame t-1, sc[] holds the scores after frame t-2.  period is a multiple of 4, so a retarget
// falls on the last frame of a group: a scalar compare per group, nothing in the other three frames, and the four frames of
// a group share one low end, which lanes 0..3 write to the table the call returns (band_lo, here an output).
struct BandTracking {
    static constexpr bool kTracking = true;
    static constexpr bool kStart = false;
    struct Group {};
    uint32_t period, next_rt;
    int end_rule;
    int32_t *out;
    // the retarget rule: the low end behind lo under the scores sc[] / pres2 (wave-uniform)
    static __device__ __forceinline__ uint32_t retarget(uint32_t lo, uint32_t L, uint32_t B, const float (&sc)[16], uint32_t pres2, int blk)
    {
        uint32_t nlo = lo;
        const int c = wave_best_live(sc, pres2, blk);
        if (c >= 0) {
            int v = c - (int)(B >> 1);
            v = v > (int)lo ? v : (int)lo;
            v = v < (int)L - 1 ? v : (int)L - 1;   // unconditional: whatever the floats were, lo stays in [0, L)
            nlo = (uint32_t)v;
        }
        return nlo;
    }
    static __device__ __forceinline__ uint32_t first_lo(const BandLattice &) { return 0u; }
    __device__ __forceinline__ void begin(const BandLattice &d)
    {
        out = const_cast<int32_t *>(d.band_lo);
        next_rt = period;
    }
    __device__ __forceinline__ Group group(uint32_t tb, uint32_t lo, uint32_t T, int lane)
    {
        if (lane < 4 && tb + (uint32_t)lane < T) out[tb + (uint32_t)lane] = (int32_t)lo;
        return Group();
    }
    __device__ __forceinline__ uint32_t next_lo(const Group &, int dd, uint32_t tb, uint32_t lo, uint32_t T, uint32_t L, uint32_t B, const float (&sc)[16],
                                                uint32_t pres2, int blk)
    {
        uint32_t nlo = lo;
        if (dd == kRowDepth - 1 && __builtin_expect(tb + kRowDepth == next_rt, 0)) {
            asm volatile("" ::: "memory");  // a real branch: the common group pays a compare and a jump
            next_rt += period;
            if (tb + kRowDepth < T) nlo = retarget(lo, L, B, sc, pres2, blk);   // (no step into frame T)
        }
        return nlo;
    }
    __device__ __forceinline__ bool end_at_best() const { return end_rule == 1; }
};

// a score row's cell as the kernels hold it: a NaN (found by its bits: the library is built with -fno-honor-nans) is a dead
// cell, which enters sc[] as -inf with its liveness bit clear; -inf is a LIVE cell of score -inf
__device__ __forceinline__ bool row_cell_live(uint32_t bits) { return (bits & 0x7fffffffu) <= 0x7f800000u; }
__device__ __forceinline__ float row_cell_score(uint32_t bits) { return __builtin_bit_cast(float, row_cell_live(bits) ? bits : 0xff800000u); }

// the caller's boundary conditions (ka_ctc_best_path_resume): the state before frame 0 is a score row
// (no band applies to it), the path ends at the reference's cell, the best cell or a given cell, and the live cells after frame
// T-1 go out as a row.  The start row touches the prologue and the re-labelling block of frame 0 (forward_banded_wave), the
// rest the epilogue; the frame loop is that of the band source the rows are combined with (BandResume, BandTrackingResume).
struct BandRows {
    gcu32_t init;   // [L] the start row's bits, or NULL: the virtual state {0: 0.0}
    gf32_t fin;     // [L] the last row (prep filled it with kDeadScoreBits), or NULL
    int end;        // ResumeRows::end, wave-uniform
    // cells of block `blk` before frame 0.  The ring holds the 64 blocks from lo_0 >> 4: every cell frame 0 reads but the three
    // below the lowest block (start_halos), and none at or above L.
    __device__ __forceinline__ uint32_t start_row(float (&sc)[16], int blk, uint32_t L) const
    {
        uint32_t pres2 = 0u;
        if (!init) {
            if (blk == 0) {
                sc[0] = 0.0f;
                pres2 = 1u;
            }
            return pres2;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t p = (uint32_t)blk * 16u + (uint32_t)k;
            if (p < L) {
                const uint32_t b = init[p];
                sc[k] = row_cell_score(b);
                pres2 |= row_cell_live(b) ? 1u << (2 * k) : 0u;
            }
        }
        return pres2;
    }
    // frame 0's halo of the lane that owns the ring's lowest block: its left neighbour holds the block 64 above, not the one
    // below, so the three cells come from the row itself (every other lane's halo is its neighbour's, as in any frame)
    __device__ __forceinline__ void start_halos(float &h1, float &h2, float &h3, int blk, uint32_t blo) const
    {
        if (init && blo > 0u && blk == (int)blo) {
            const uint32_t p = blo * 16u;
            const uint32_t b1 = init[p - 1], b2 = init[p - 2], b3 = init[p - 3];
            h1 = row_cell_score(b1);
            h2 = row_cell_score(b2);
            h3 = row_cell_score(b3);
        }
    }
    __device__ __forceinline__ bool end_at_best() const { return end == -2; }
    __device__ __forceinline__ bool end_given() const { return end >= 0; }
    // the caller's end cell if it is live after the last frame (pres2 of the lane that holds its block), else -1
    __device__ __forceinline__ int end_cell(uint32_t pres2, int blk) const
    {
        const bool live = (end >> 4) == blk && ((pres2 >> (2 * (end & 15))) & 1u) != 0u;
        return __builtin_amdgcn_ballot_w64(live) ? end : -1;
    }
    // the live cells after frame T-1 (a live cell lies in the last band, so below L)
    __device__ __forceinline__ void last_row(const float (&sc)[16], uint32_t pres2, int blk) const
    {
        if (!fin) return;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if ((pres2 >> (2 * k)) & 1u) fin[(size_t)blk * 16 + (size_t)k] = sc[k];
    }
};

// the caller's table under the caller's boundary conditions: the frame loop is BandFromTable's
struct BandResume : BandFromTable, BandRows {
    static constexpr bool kStart = true;
    using BandRows::end_at_best;
};

// the self-steering band under the caller's boundary conditions (ka_ctc_best_path_tracking_resume):
// BandTracking's frame loop from the caller's lo_0, BandRows' prologue and epilogue, and the low end frame T would get, which
// BandTracking declines to compute: here it goes to a cell of the lattice's own, and lo stays.  The chunk that follows takes it
// as its lo_0, so a band steered across a cut at a multiple of the period is the uncut call's.
struct BandTrackingResume : BandTracking, BandRows {
    static constexpr bool kStart = true;
    using BandRows::end_at_best;
    uint32_t lo0;    // lo_0, in [0, L) (the host checked it)
    uint32_t lo_T;   // the retarget that falls on frame T, where T % period == 0 (wave-uniform; last_lo writes it)
    gi32_t next;     // one int32: lo_T
    __device__ __forceinline__ uint32_t first_lo(const BandLattice &) const { return lo0; }
    __device__ __forceinline__ uint32_t next_lo(const Group &, int dd, uint32_t tb, uint32_t lo, uint32_t T, uint32_t L, uint32_t B, const float (&sc)[16],
                                                uint32_t pres2, int blk)
    {
        uint32_t nlo = lo;
        if (dd == kRowDepth - 1 && __builtin_expect(tb + kRowDepth == next_rt, 0)) {
            asm volatile("" ::: "memory");  // a real branch: the common group pays a compare and a jump
            next_rt += period;
            const uint32_t v = retarget(lo, L, B, sc, pres2, blk);
            if (tb + kRowDepth < T) nlo = v;
            else lo_T = v;   // T % period == 0: frame T's low end, not walked here
        }
        return nlo;
    }
    // behind the frame loop, one lane: frame T's low end; T % period != 0 keeps the last frame's.  (Not stored from next_lo's
    // branch: a per-lane store there makes the frame loop's scalar values cross divergent control flow.)
    __device__ __forceinline__ void last_lo(uint32_t lo, uint32_t T) const
    {
        if (threadIdx.x == 0) *next = (int32_t)(T % period != 0u ? lo : lo_T);
    }
};

// ---------------------------------------------------------------------------------------
// forward DP, one wavefront per lattice, every cell's code stored
// ---------------------------------------------------------------------------------------
template <int M, bool ZL, class Src>
__device__ __forceinline__ void forward_banded_wave(const BandLattice &d, int32_t *meta, Src src)
{
    constexpr int D = kRowDepth;
    const int lane = threadIdx.x;
    const uint32_t T = (uint32_t)__builtin_amdgcn_readfirstlane(d.T);
    const uint32_t L = (uint32_t)__builtin_amdgcn_readfirstlane(d.L);
    const uint32_t B = (uint32_t)__builtin_amdgcn_readfirstlane(d.beam);
    const float NINF = ninf();

    uint32_t lo = src.first_lo(d);   // band of frame 0 (a table is valid: prep; a caller's lo_0: the host)
    uint32_t hi = (L - lo < B) ? L : lo + B;
    uint32_t blo = lo >> 4;
    int blk = (int)blo + ((lane - (int)blo) & 63);   // block of 16 positions this lane currently owns
    int prev_blk = blk;                              // ... and owned before the last re-labelling

    float sc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) sc[k] = NINF;
    uint32_t pres2;                         // bit 2k: cell k holds a live state
    if constexpr (Src::kStart) {
        pres2 = src.start_row(sc, blk, L);  // the caller's state before frame 0
    } else {
        // virtual state before frame 0 (align.py:57-58): position 0, which a lane holds only while block 0 is on the ring
        const bool holds0 = blk == 0;
        if (holds0) sc[0] = 0.0f;
        pres2 = holds0 ? 1u : 0u;
    }
    // wave-uniform: lanes were re-labelled for this frame.  A start row takes frame 0 through that block, with no lane reset:
    // it kills the wrapped halo of the lane that owns the lowest block and puts the row's own three cells there.
    bool pend_reset = Src::kStart;
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

    // low ends of frames tb+1 .. tb+4: the table's, one aligned scalar load per group, the next group's in flight (prep padded
    // the table), or the tracking band's
    src.begin(d);

    const char *row_ahead = lp + (size_t)(D < T ? D : T - 1) * ld;   // row min(t+D, T-1) of the current frame t
    for (uint32_t tb = 0; tb < T; tb += D) {
        const typename Src::Group step = src.group(tb, lo, T, lane);
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
                    if constexpr (Src::kStart) {
                        if (dd == 0 && tb == 0) src.start_halos(h1, h2, h3, blk, blo);
                    }
#pragma unroll
                    for (int k = 0; k < 16; ++k) sc[k] = reset_lane ? NINF : sc[k];
                    pres2 = reset_lane ? 0u : pres2;
                    prev_blk = blk;
                    pend_reset = false;
                }
                // A. band of frame t+1 from its source; re-label the lanes whose block lo has passed
                const uint32_t nlo = src.next_lo(step, dd, tb, lo, T, L, B, sc, pres2, blk);
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
    if constexpr (Src::kStart) {
        if (m[0] == kStatusOk) src.last_row(sc, pres2, blk);   // (a lattice with a bad label keeps the row prep wrote: all dead)
    }
    if constexpr (Src::kTracking && Src::kStart) src.last_lo(lo, T);   // (lo is lo_{T-1}: no step into frame T)
    // terminal state: the HIGHEST live position of frame T-1 (align.py:99-101), or on request the tracking call's best one,
    // or the resumed call's given one
    int best;
    if ((Src::kTracking || Src::kStart) && src.end_at_best()) {
        best = wave_best_live(sc, pres2, blk);
    } else if constexpr (Src::kStart) {
        best = src.end_given() ? src.end_cell(pres2, blk) : wave_highest_live(pres2, blk);
    } else {
        best = wave_highest_live(pres2, blk);
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
    forward_banded_wave<M, ZL>(d, meta, BandFromTable());
}

// ... and the same pair over the self-steering band: no table to check, period and end rule are the call's
template <int M, bool ZL>
__global__ __launch_bounds__(64, kBandMinWaves) void forward_tracking_wave_kernel(const BandLattice *__restrict__ lats, int32_t *meta,
                                                                                  uint32_t period, int end_rule)
{
    const BandLattice &d = lats[blockIdx.x];
    const int flags = __builtin_amdgcn_readfirstlane(meta_of(meta, d.idx)[2]);
    if (((flags & kFlagZeroLabel) != 0) != ZL) return;
    BandTracking src;
    src.period = period;
    src.end_rule = end_rule;
    forward_banded_wave<M, ZL>(d, meta, src);
}


// ---------------------------------------------------------------------------------------
// generic form: any band, any V, max_move <= 255.  One 256-thread workgroup per lattice, score columns double-buffered in
// global memory, one byte of back-pointer per band cell (forward_generic_kernel's scheme with the table).  Not tuned.
// ---------------------------------------------------------------------------------------
// First maximum of a score column over its live cells in ascending position, as wave_best_live: the largest key
// (order-preserving float bits, ~position), 0 without a live cell.  All 256 threads; `key` is shared memory.
__device__ __forceinline__ unsigned long long block_best_live(const float *sc, const uint8_t *pr, int64_t plo, int64_t phi,
                                                              unsigned long long *key)
{
    if (threadIdx.x == 0) *key = 0ull;
    __syncthreads();
    unsigned long long mine = 0ull;
    for (int64_t p = plo + threadIdx.x; p < phi; p += 256)
        if (pr[p]) {
            uint32_t b = __builtin_bit_cast(uint32_t, sc[p]);
            b = b == 0x80000000u ? 0u : b;
            const uint32_t kh = b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
            const unsigned long long k = ((unsigned long long)kh << 32) | (uint32_t)~(uint32_t)p;
            mine = k > mine ? k : mine;
        }
    if (mine) atomicMax(key, mine);
    __syncthreads();
    return *key;
}

// kTrack: the self-steering band of BandTracking instead of the table.  The arg-max of frame t-2 is taken at the end of frame
// t-2, when its column is the current one, and held in shared memory for two frames; thread 0 writes the table.
// kStart: the resumed call's boundary conditions (BandRows', `rr` the lattice's rows): the start row goes into the first
// column with every position open, the last row comes out of the last column's band.  Both: BandTrackingResume.
template <bool kTrack, bool kStart = false>
__device__ __forceinline__ void forward_banded_generic(const BandLattice &d, int32_t *meta, int period, int end_rule,
                                                       const ResumeRows *rr = nullptr)
{
    const int tid = threadIdx.x;
    int32_t *m = meta_of(meta, d.idx);
    if ((!kTrack || kStart) && (m[2] & kBandFlagBadTable)) return;   // a bad table, or a +inf cell in the start row
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
    int64_t plo = 0, phi = 1;
    if (kStart && rr->init) {
        const uint32_t *init = reinterpret_cast<const uint32_t *>(rr->init);
        for (int64_t p = tid; p < L; p += 256) {
            const uint32_t b = init[p];
            scA[p] = row_cell_score(b);
            prA[p] = row_cell_live(b) ? 1 : 0;
        }
        phi = L;
    } else if (tid == 0) {
        scA[0] = 0.0f;
        prA[0] = 1;
    }
    __syncthreads();
    __shared__ unsigned long long s_key;
    int64_t lo_track = 0;
    if constexpr (kTrack && kStart) lo_track = rr->first_lo;   // the caller's lo_0, in [0, L) (the host checked it)
    for (int64_t t = 0; t < T; ++t) {
        if (kTrack) {
            if (t > 0 && t % period == 0 && s_key != 0ull) {
                const int64_t c = (int64_t)(uint32_t)~(uint32_t)s_key;
                int64_t v = c - B / 2;
                v = v > lo_track ? v : lo_track;
                lo_track = v < L - 1 ? v : L - 1;   // unconditional: whatever the floats were, lo stays in [0, L)
            }
            if (tid == 0) const_cast<int32_t *>(d.band_lo)[t] = (int32_t)lo_track;
        }
        const int64_t lo = kTrack ? lo_track : (int64_t)d.band_lo[t];
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
        // (with a start row also for frame T, whose low end goes to the chunk that follows)
        if (kTrack && (t + 2 < T || (kStart && t + 2 == T)) && (t + 2) % period == 0) block_best_live(scA, prA, plo, phi, &s_key);
    }
    if constexpr (kTrack && kStart) {   // the low end frame T would get: BandTrackingResume's cell
        if (T % period == 0 && s_key != 0ull) {
            const int64_t c = (int64_t)(uint32_t)~(uint32_t)s_key;
            int64_t v = c - B / 2;
            v = v > lo_track ? v : lo_track;
            lo_track = v < L - 1 ? v : L - 1;
        }
        if (tid == 0) rr->entry[1] = (int32_t)lo_track;
        __syncthreads();   // (s_key is used again below)
    }
    if constexpr (kStart) {
        if (rr->fin && m[0] == kStatusOk)   // (a lattice with a bad label keeps the row prep wrote: all dead)
            for (int64_t p = plo + tid; p < phi; p += 256)
                if (prA[p]) rr->fin[p] = scA[p];
    }
    // highest live position of the last frame (the tracking call's end rule 1 and the resumed call's end -2: the best one; the
    // resumed call's end >= 0: that cell if it is live)
    __shared__ int64_t s_best;
    if (kStart && rr->end >= 0) {
        const int64_t q = rr->end;
        if (tid == 0) s_best = (q >= plo && q < phi && prA[q]) ? q : -1;
    } else if ((kTrack && end_rule == 1) || (kStart && rr->end == -2)) {
        const unsigned long long k = block_best_live(scA, prA, plo, phi, &s_key);
        if (tid == 0) s_best = k ? (int64_t)(uint32_t)~(uint32_t)k : -1;
    } else {
        if (tid == 0) s_best = -1;
        __syncthreads();
        int64_t mine = -1;
        for (int64_t p = plo + tid; p < phi; p += 256)
            if (prA[p]) mine = p;
        if (mine >= 0) atomicMax((long long *)&s_best, (long long)mine);
    }
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


// ---------------------------------------------------------------------------------------
// the walk back, one wavefront per lattice: path, labels and scores of 16 frames at a time.  Returns the position
// before frame 0 (the cell of the start state the path left from), -1 without a path.
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
__device__ __forceinline__ int backtrace_banded_wave(const BandLattice &d, const int32_t *meta)
{
    const int lane = threadIdx.x;
    int p = __builtin_amdgcn_readfirstlane(meta[4 * (size_t)d.idx + 1]);
    if (p < 0) return -1;   // no path: the status says why
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
        p = q + 16 * w;
        if (t1 < 0) break;
        cur[0] = nxt[0];
        cur[1] = nxt[1];
        w = wn;
        t0 = t1;
        n = kBandBtChunk;
    }
    return p;
}

// the generic form's walk back, by thread 0, which returns the position before frame 0 (every other thread, and a lattice
// without a path: -1)
__device__ __forceinline__ int64_t backtrace_banded_generic(const BandLattice &d, const int32_t *meta)
{
    int64_t p = meta[4 * (size_t)d.idx + 1];
    if (p < 0 || threadIdx.x != 0) return -1;
    const int64_t T = d.T, W = d.W;
    const uint8_t *bp = reinterpret_cast<const uint8_t *>(d.bp);
    for (int64_t t = T - 1; t >= 0; --t) {
        const int lab = (p & 1) ? (d.labx[p >> 1] >> 2) : 0;
        d.path[t] = (int32_t)p;
        d.lab_out[t] = lab;
        d.sc_out[t] = d.lp[(size_t)t * (size_t)d.ld + (size_t)lab];
        p -= bp[(size_t)t * (size_t)W + (size_t)(p - d.band_lo[t])];
    }
    return p;
}

}  // namespace ka
