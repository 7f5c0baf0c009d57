// ka_mea.hpp — the maximum-expected-accuracy alignment (posterior-decoded path): the one path s_0 ... s_{T-1} of the band that
// ends at a caller-given terminal s* and maximises sum over t of gamma_t(s_t), that sum (the expected number of correctly
// placed frames), and Z = alpha_{T-1}(s*).  Included by ka_mea.hip and ka_mea_banded.hip only.
//
// Same lattice, band, moves, veto, statuses and form split as ka_occupancy.hpp (DESIGN.md sections 4.18 and 4.26): the
// driver of ka_fb_ck.hpp with MeaOut, which recomputes every block as the occupancy does and runs a Viterbi recursion over
// every cell's gamma - the float the state posteriors write (fb_gamma) - backwards, as the driver hands the frames out:
//   W_{T-1}(p) = gamma_{T-1}(p) if p = s*, else -inf
//   W_t(p)     = gamma_t(p) + max over j in [0, max_move), p + j in band t+1, not fb_vetoed(j, lab'[p + j]) of W_{t+1}(p + j)
//   c_t(p)     = the smallest j that attains the maximum (0 where every successor is -inf: such a cell is never walked)
// in float64, one add per cell: the maximum is exact, so W has no order dependence and equals a sequential float64 loop over
// the rows of ka_ctc_state_posteriors, bit for bit.  After frame 0 the path is walked forward from the virtual state 0:
//   s_0 = the smallest j < max_move in band 0 (which a table may start above 0), not fb_vetoed(j, lab'[j]), that maximises W_0(j);  s_{t+1} = s_t + c_t(s_t)
//   expected_accuracy = W_0(s_0)
//
// W columns.  Fast form: two LDS rings (position p at the form's column slot, p & 1023), W_{t+1} and W_t, swapped per frame.
// A frame's cells read the ring of t+1 only inside [lo_{t+1}, hi_{t+1}) - at most 1009 positions, so no two of them share a
// slot - and write the ring of t, whose previous content (W_{t+2}) has no reader left: a live slot of the t+1 ring is never
// written during the frame that reads it, and what lies outside a band (an older frame's, or another lattice's) is never
// read, so the rings need no clearing.  An entry carries the sign of mea_ring_entry below.  One wavefront's LDS operations execute in order and the driver's fence() stands in
// front of every frame's cells.  Generic form: two more columns of the slot at absolute positions, ordered from frame to
// frame by the barrier of the frame's reduction (as the working columns are).
//
// Back-pointers are kept for the whole lattice (the walk runs forward, after the last block).  Fast form: 2 bits per cell;
// a lane's 16 cells lo + lane + 64 k go into one dword, bits [2k, 2k + 2): 256 bytes per frame, one coalesced plain store.
// Generic form: a byte per cell, [T][cw].
//
// Ordering of the walk.  Fast form: lane l stores dword l of every frame's codes and, in the walk, lane l loads that same dword
// back - every 32 frames the wavefront copies the block's rows (8 KB, 32 independent loads per lane, each of an address the
// lane itself stored with a plain store) into working column 0, which the finished backward pass no longer needs.  A lane's own
// store followed by its own load of the same address needs nothing but program order.  Only then do the codes cross lanes, in
// LDS, behind post_wave_sync: one wavefront's LDS operations execute in order.  So the T-step dependent chain of the walk runs
// on LDS, and nothing leans on how the caches treat another lane's stores.  Generic form: every frame ended in the barrier of
// its reduction, frame 0 included (frame_end runs behind it), and one more barrier opens the walk; the codes are read from
// global memory across threads - a correctness path, as the form is.
// The path is staged in LDS a block at a time and written as 128-byte rows by 32 consecutive threads.
//
// LDS: four working columns, the log-prob row, the two rings, the offsets and the row of the path: 49.9 KB in the fast form,
// the duration kernel's figure, so three workgroups share a CU and a launch of 769 to 1536 fast lattices runs in two
// rounds; launch_fb_ck's grid rule is left as it is.
#pragma once
#include "ka_fb_ck.hpp"

namespace ka {

// A ring entry of the fast form carries its cell's veto with it: W is >= 0 or -inf, so a cell whose label value is 0 stores -W
// (-0.0 for 0), and a reader that arrives by a skipping move (an even j >= 2) takes any entry with the sign bit set - a
// label-0 cell, or a dead one - as -inf.  The cells then read no label but their own, which the driver hands them: a label load
// of the successor inside the cells would be a global load that the frame's W waits for, and with it for the log-prob row
// prefetched for the next frame.
__device__ __forceinline__ double mea_ring_entry(double w, int32_t lab) { return (lab == 0 && w != post_dninf()) ? -w : w; }
__device__ __forceinline__ double mea_ring_value(double v, bool skip)
{
    if (skip) return __builtin_signbit(v) ? post_dninf() : v;
    return v == post_dninf() ? v : __builtin_fabs(v);
}

// fb_ck's policy.  The forms differ in where W and the codes live (above); a position's place in W is the form's column slot.
template <class Form_, class Band>
struct MeaOut {
    using Form = Form_;
    using Desc = MeaLattice;
    struct Lds : FbRings<Form::kWave> {   // W_{t+1} and W_t
        int32_t tile[kPostCk];
    };
    static constexpr int NT = Form::NT;
    const MeaLattice &d;
    Form &f;
    double *wn, *wc;      // W_{t+1} and W_t
    int32_t *tile;        // kPostCk positions of the path (LDS)
    int64_t nlo, nhi;     // the band of frame t + 1
    uint32_t word;        // fast form: the codes of this lane's cells of the frame
    const int32_t *tab;   // the caller's table (BandTable), which the forward walk steps as the passes did
    template <class D>
    __device__ __forceinline__ MeaOut(const D &d_, Form &f_, Lds &lds)
        : d(d_), f(f_), wn(Form::kWave ? lds.ring(0) : d_.wcol), wc(Form::kWave ? lds.ring(1) : d_.wcol + d_.L), tile(lds.tile), nlo(0), nhi(0), word(0),
          tab(fb_table(d_))
    {
    }
    // a lattice without a result: -1 over [0, T) of the path, NaN as the expected accuracy, and the status and
    // log-likelihood of fb_fail_result
    __device__ __forceinline__ void fail(PostResult *res, int status)
    {
        for (int64_t t = threadIdx.x; t < d.T; t += NT) d.path[t] = -1;
        if (threadIdx.x == 0) *reinterpret_cast<uint64_t *>(d.ea) = kNaN64;
        fb_fail_result(d, res, status);
    }
    __device__ __forceinline__ bool recompute(int64_t) const { return true; }
    __device__ __forceinline__ auto cells(int64_t t, int64_t lo)
    {
        const bool last = t == (int64_t)d.T - 1;
        const int64_t sstar = d.terminal, slo = nlo, shi = nhi;
        const double *rn = wn;
        double *rc = wc;
        uint8_t *brow = Form::kWave ? nullptr : reinterpret_cast<uint8_t *>(d.bp) + (size_t)t * (size_t)d.cw;
        uint32_t *wd = &word;
        const MeaLattice *dd = &d;
        return [=](int64_t p, int32_t lab, auto arg) {
            const double g = (double)fb_gamma(arg());
            double best = post_dninf();
            int c = 0;
            if (last) {
                best = (p == sstar) ? 0.0 : best;
            } else if constexpr (Form::kWave) {
#pragma unroll
                for (int j = 0; j < Form::kMoves; ++j) {
                    const int64_t u = p + j;
                    const bool ok = u >= slo && u < shi;
                    const double x = ok ? mea_ring_value(rn[Form::cslot(u)], fb_skip(j)) : post_dninf();
                    c = x > best ? j : c;
                    best = x > best ? x : best;
                }
            } else {
                const int M = dd->max_move;
                for (int j = 0; j < M; ++j) {
                    const int64_t u = p + j;
                    if (u < slo || u >= shi || fb_vetoed(j, fb_lab(*dd, u))) continue;
                    const double x = rn[Form::cslot(u)];
                    c = x > best ? j : c;
                    best = x > best ? x : best;
                }
            }
            const double w = g + best;   // (-inf stays -inf: g is finite)
            rc[Form::cslot(p)] = Form::kWave ? mea_ring_entry(w, lab) : w;
            if constexpr (Form::kWave) *wd |= (uint32_t)c << (2 * (int)((p - lo) >> 6));
            else brow[p - lo] = (uint8_t)c;
        };
    }
    __device__ __forceinline__ void cells_done() {}
    __device__ __forceinline__ void frame_end(int64_t t, int64_t lo, int64_t hi)
    {
        if constexpr (Form::kWave) {
            reinterpret_cast<uint32_t *>(d.bp)[(size_t)t * 64 + threadIdx.x] = word;
            word = 0;
        }
        { double *x = wn; wn = wc; wc = x; }
        nlo = lo;
        nhi = hi;
        if (t == 0) walk();
    }

    // The forward walk, behind frame 0 (wn holds W_0, over the band of frame 0).
    // Invariant: W_t(s_t) is finite at every frame.  The lattice passed the zero-mass check, so with finite log-probs some
    // band path of finite score ends at s*; its first state is an allowed start j with W_0(j) finite (W sums non-negative
    // finite gammas along the best continuation, and is -inf only where no allowed continuation reaches s*), so the maximum
    // over the starts is finite and s_0 attains it.  If W_t(p) is finite and t < T-1, the maximum over p's allowed successors
    // is finite and c_t(p) names one that attains it, so W_{t+1}(s_{t+1}) is finite.  A finite W_{T-1} is at s* alone, so the
    // walk ends there, never follows the code of a dead cell, and every s_t lies in the band of its frame.
    __device__ __forceinline__ void walk()
    {
        const int tid = threadIdx.x;
        const int64_t T = d.T;
        f.sync();   // frame 0's W (and, generic form, every frame's codes), stored by the threads that own the cells, before the thread that walks
        // the band every frame's codes were stored under: a code lies at p - lo_t, so the walk takes lo_t from the driver's own
        // Band.  A table was accepted by the forward pass (start(), a whole-workgroup step): here it is only seated, by every
        // thread alike, and thread 0 alone steps it.
        Band bw(d.L, d.beam, T, tab);
        if constexpr (Band::kTable) bw.seek(0);
        int32_t s = 0;
        if (tid == 0) {
            int64_t lo, hi;
            bw.band(lo, hi);
            const int M = d.max_move;
            double best = post_dninf();
            for (int j = 0; j < M; ++j) {
                if (j < lo || j >= hi || fb_vetoed(j, fb_lab(d, j))) continue;
                const double x = Form::kWave ? mea_ring_value(wn[Form::cslot(j)], false) : wn[Form::cslot(j)];
                s = x > best ? j : s;
                best = x > best ? x : best;
            }
            *d.ea = best;
        }
        uint32_t *stage = reinterpret_cast<uint32_t *>(f.col(0));   // fast form: the block's codes, [kPostCk][64] dwords
        for (int64_t t0 = 0; t0 < T; t0 += kPostCk) {
            const int64_t t1 = (t0 + kPostCk < T) ? t0 + kPostCk : T;
            if constexpr (Form::kWave) {
                const uint32_t *src = reinterpret_cast<const uint32_t *>(d.bp) + (size_t)t0 * 64 + tid;
#pragma unroll 8
                for (int r = 0; r < kPostCk; ++r)
                    if (t0 + r < t1) stage[r * 64 + tid] = src[(size_t)r * 64];
                f.sync();
            }
            if (tid == 0) {
                for (int64_t t = t0; t < t1; ++t) {   // bw stands at t
                    tile[t - t0] = s;
                    int64_t lo, hi;
                    bw.band(lo, hi);
                    bw.next();
                    const int64_t o = (int64_t)s - lo;
                    if constexpr (Form::kWave) s += (int32_t)((stage[(t - t0) * 64 + (o & 63)] >> (2 * (int)(o >> 6))) & 3u);
                    else s += (int32_t) reinterpret_cast<const uint8_t *>(d.bp)[(size_t)t * (size_t)d.cw + (size_t)o];
                }   // (frame T-1's code is 0)
            }
            f.sync();   // the row of the path before the threads that write it out
            if (tid < kPostCk && t0 + tid < t1) d.path[t0 + tid] = tile[tid];
            f.sync();   // the row, and the staged codes, before the next block rewrites them
        }
    }
};

template <class Band>
void launch_mea_path(const BandDesc<MeaLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<MeaOut, Band>(lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
