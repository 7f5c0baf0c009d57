// ka_quantile.hpp — exact boundary-time quantiles: for every cut position c_k of the blank-expanded labels and every level
// q_m the first frame at which the posterior mass at or above the cut reaches the level, over the band's paths that end at a
// caller-given terminal s*, and Z = alpha_{T-1}(s*).  Included by ka_quantile.hip and ka_quantile_banded.hip only.
//   tau_c = the first frame whose state is >= c; paths only move up, so P(tau_c <= t) = P(state_t >= c) = sum_{s >= c} gamma_t(s)
//   F_t(c) = 2^32 where c <= lo_t, 0 where c >= hi_t, else the sum over p in [c, hi_t) of occ_fix of the cell: an unsigned
//            32.32 fixed-point integer, so it does not depend on the order of the adds and is defined bit for bit by the rows
//            that ka_ctc_state_posteriors writes
//   quantile[k, m] = the smallest t in [0, T) with F_t(c_k) >= thr_m, T if there is none
//
// Same lattice, band, moves, veto, statuses and form split as ka_duration.hpp (DESIGN.md sections 4.18 and 4.28): the driver
// of ka_fb_ck.hpp with QuantOut, which recomputes every block.  Its work is a scan across the band once a frame, where the
// durations accumulate per position over time:
//   cells        a cell's occ_fix goes to the frame's row of 64-bit integers: in the fast form an LDS ring (position p at
//                qring(p): the column slot p & 1023, padded by one word per 16 so that a lane's 16 consecutive slots fall on
//                banks of their own), in the generic form a per-slot workspace row at p - lo.  The recurrences call the cell for
//                every position of [lo, hi): a frame overwrites the whole of its band, and nothing else is read.
//   frame_end    one inclusive prefix sum of the row over [lo, hi), written back in place: every thread sums a run of
//                consecutive positions (16 in the fast form), the runs' totals are scanned across the wavefront (and, in the
//                generic form, across the workgroup's four).  Then the cuts inside the band, lo < c_k < hi - a contiguous run
//                [ka, kb) of cut indices whose two ends only move down as the sweep goes back, kept as running indices - get
//                F = total - prefix[c_k - 1], and for every level that F reaches, quantile[k, m] = t.  The levels ascend, so
//                the first level that fails ends a cut's loop.
// The sweep runs T-1 ... 0, so the last store to a word is the minimum over the frames whose band holds the cut.  The frames
// whose band lies at or above the cut (F = 2^32) are those from the first t with lo_t >= c_k on: the planner's closed form,
// uploaded beside the cuts (start), is the value a cut's words hold before the sweep - T where there is no such frame.
// Under a caller's table (BandTable) there is no closed form and the table may lie in device memory: the same value, the first
// t with tab[t] >= c_k or T, is a lower-bound search of the non-decreasing table by the cut's owner thread, in begin() - behind
// the forward pass, whose start() accepted the table, and before the sweep's first store.  A cut at or below lo_0 so starts at 0.
// Ownership: cut k belongs to thread k mod NT in every frame (the run's low end is rounded down to a multiple of NT), and that
// thread also writes the start value and, for a failed lattice, the -1: all stores to one output word come from one thread in
// program order, and no ring of candidates or retire step is needed.
#pragma once
#include "ka_fb_ck.hpp"
#include "ka_occupancy.hpp"

namespace ka {

constexpr int kQuantRing = 1024 + 64;   // the fast form's row: 1024 column slots and a word of padding per 16
// where position p lives in the fast form's row
__device__ __forceinline__ int qring(int64_t p)
{
    const int s = (int)(p & 1023);
    return s + (s >> 4);
}
__device__ __forceinline__ unsigned long long quant_wave_scan(unsigned long long x)   // inclusive, across the wavefront's lanes
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long y = __shfl_up(x, off);
        x += lane >= off ? y : 0ull;
    }
    return x;
}

// fb_ck's policy.  The forms differ in where the frame's row lives and in how wide the scan is.
template <class Form_, class Band>
struct QuantOut {
    using Form = Form_;
    using Desc = QuantLattice;
    struct Lds {   // the fast form's ring, or the generic form's totals of its wavefronts
        unsigned long long w[Form::kWave ? kQuantRing : Form::NT / 64];
    };
    static constexpr int NT = Form::NT;
    const QuantLattice &d;
    unsigned long long *row;    // fast form: the LDS ring; generic: the slot's workspace row
    unsigned long long *part;   // generic form: the four wavefronts' totals (LDS)
    unsigned long long thr[kMaxLevels];   // the thresholds; those past M can never be reached
    int64_t ka, kb;             // the cuts inside the band of the frame last seen: indices [ka, kb)
    bool dna, dnb;              // this lane's look below ka and kb for the frame in flight (asked for before the frame's cells)
    const int32_t *tab;         // the caller's table (BandTable): where begin() finds the cuts' start frames
    template <class D>
    __device__ __forceinline__ QuantOut(const D &d_, Form &, Lds &lds)
        : d(d_), row(Form::kWave ? lds.w : d_.frow), part(lds.w), ka(d_.K), kb(d_.K), dna(false), dnb(false), tab(fb_table(d_))
    {
#pragma unroll
        for (int m = 0; m < kMaxLevels; ++m) thr[m] = m < d.M ? d.thr[m] : ~0ull;
        if constexpr (!Band::kTable)
            for (int64_t k = threadIdx.x; k < d.K; k += NT) fill(k, d.start[k]);
    }
    // fb_ck's opt-in hook behind the forward pass: under a table, every cut's start frame from the accepted table - the first t
    // with tab[t] >= c_k, T if there is none - stored by the cut's owner.  (The diagonal's came from the host, in the constructor.)
    __device__ __forceinline__ void begin() const
    {
        if constexpr (Band::kTable)
            for (int64_t k = threadIdx.x; k < d.K; k += NT) {
                const int64_t c = d.cuts[k];
                int32_t a = 0, b = d.T;   // tab[t] < c below a, tab[t] >= c from b on
                while (a < b) {
                    const int32_t mid = a + ((b - a) >> 1);
                    if ((int64_t)tab[mid] >= c) b = mid;
                    else a = mid + 1;
                }
                fill(k, a);
            }
    }
    __device__ __forceinline__ void fill(int64_t k, int32_t v) const
    {
        int32_t *q = d.quant + k * d.ld_out;
        for (int m = 0; m < d.M; ++m) q[m] = v;
    }
    // a lattice without a result: -1 over [K, M] (from the threads that own the cuts), and the status and log-likelihood of
    // fb_fail_result
    __device__ __forceinline__ void fail(PostResult *res, int status)
    {
        for (int64_t k = threadIdx.x; k < d.K; k += NT) fill(k, -1);
        fb_fail_result(d, res, status);
    }
    __device__ __forceinline__ bool recompute(int64_t) const { return true; }
    // this lane's look at the cut `lane` below a running end: does the end move below it?  (`above`: the bound the cut must
    // reach or pass to leave the run - cuts[k] >= hi at the high end, cuts[k] > lo at the low one)
    __device__ __forceinline__ bool below(int64_t end, int64_t bound) const
    {
        const int64_t k = end - 1 - (threadIdx.x & 63);
        return k >= 0 && d.cuts[k] >= bound;
    }
    // a running end moved down past every cut that is >= bound; `dn` this lane's look, taken before (the cuts ascend, so the
    // lanes that say yes are the lowest ones)
    __device__ __forceinline__ int64_t lower(int64_t end, int64_t bound, bool dn) const
    {
        for (;;) {
            const int n = __popcll(__ballot(dn));
            end -= n;
            if (n < 64) return end;
            dn = below(end, bound);
        }
    }
    __device__ __forceinline__ auto cells(int64_t, int64_t lo)
    {
        const int64_t hi = (d.L - lo < d.beam) ? (int64_t)d.L : lo + d.beam;   // hi_t from lo_t, as post_band forms it
        dnb = below(kb, hi);        // (global loads a frame's cells ahead of their use in frame_end)
        dna = below(ka, lo + 1);
        unsigned long long *r = row;
        return [=](int64_t p, int32_t, auto arg) {
            const unsigned long long f = occ_fix(arg());
            if constexpr (Form::kWave) r[qring(p)] = f;
            else r[p - lo] = f;
        };
    }
    __device__ __forceinline__ void cells_done() {}
    // the frame's prefix sum in place; returns the row's total.  Fast form: lane l owns positions lo + 16 l ... + 15.
    __device__ __forceinline__ unsigned long long scan_fast(int64_t lo, int64_t hi)
    {
        const int64_t base = lo + 16 * (int64_t)threadIdx.x;
        unsigned long long v[16], sum = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            v[i] = base + i < hi ? row[qring(base + i)] : 0ull;
            sum += v[i];
        }
        const unsigned long long inc = quant_wave_scan(sum);
        unsigned long long run = inc - sum;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            run += v[i];
            if (base + i < hi) row[qring(base + i)] = run;
        }
        return __shfl(inc, 63);
    }
    // generic form: thread i owns the positions lo + i per ... + per - 1, per = ceil((hi - lo) / NT); ends behind a barrier
    __device__ __forceinline__ unsigned long long scan_gen(int64_t lo, int64_t hi)
    {
        const int64_t n = hi - lo, per = (n + NT - 1) / NT;
        const int64_t j0 = (int64_t)threadIdx.x * per, j1 = j0 + per < n ? j0 + per : n;
        unsigned long long sum = 0;
        for (int64_t j = j0; j < j1; ++j) sum += row[j];
        const unsigned long long inc = quant_wave_scan(sum);
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 63) part[wave] = inc;
        __syncthreads();
        unsigned long long run = inc - sum, total = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) {
            run += w < wave ? part[w] : 0ull;
            total += part[w];
        }
        for (int64_t j = j0; j < j1; ++j) {
            run += row[j];
            row[j] = run;
        }
        __syncthreads();
        return total;
    }
    __device__ __forceinline__ void frame_end(int64_t t, int64_t lo, int64_t hi)
    {
        kb = lower(kb, hi, dnb);
        ka = lower(ka, lo + 1, dna);
        unsigned long long total;
        if constexpr (Form::kWave) {
            post_wave_sync();   // the frame's cells, stored by the lanes that own them, before the lanes that sum them
            total = scan_fast(lo, hi);
            post_wave_sync();
        } else {
            total = scan_gen(lo, hi);   // (the reduction's barrier closed the frame's cells)
        }
        const int32_t tt = (int32_t)t;
        for (int64_t k = (ka & ~(int64_t)(NT - 1)) + threadIdx.x; k < kb; k += NT) {
            if (k < ka) continue;
            const int64_t c = d.cuts[k];   // lo < c < hi
            const unsigned long long F = total - (Form::kWave ? row[qring(c - 1)] : row[c - 1 - lo]);
            int32_t *q = d.quant + k * d.ld_out;
#pragma unroll
            for (int m = 0; m < kMaxLevels; ++m) {
                if (F < thr[m]) break;
                q[m] = tt;
            }
        }
        if (!Form::kWave) __syncthreads();   // the row is read before the next frame's cells overwrite it
    }
};

template <class Band>
void launch_boundary_quantiles(const BandDesc<QuantLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<QuantOut, Band>(lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
