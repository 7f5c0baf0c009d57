// ka_posterior_common.hpp — the forward-backward core under all six calls, which reach it through the form policy of
// ka_fb_form.hpp: ka_posterior.hpp (best-path posteriors) and ka_fb_ck.hpp (the checkpointed pass of label occupancy, state
// posteriors, state durations, sampled paths and the MEA path).  Base-2 log-sum-exp, the band and its walk, status flags, wave
// and block reductions, and the frame recurrences themselves, one forward and one backward per form (fb_fast_fwd / fb_fast_bwd,
// fb_gen_fwd / fb_gen_bwd), which FbFast<M> and FbGen wrap as their fwd / bwd.
// The callers differ only in where a cell's label comes from (the form's label policy) and what they do with a cell once it is
// computed; both are template arguments, so each recurrence exists once and every caller runs the same expressions on the same
// operands.  What a call does with a finished cell of the checkpointed pass is its Out policy's business (ka_fb_ck.hpp).
#pragma once
#include "ka_types.hpp"

namespace ka {

constexpr double kLog2e64 = 1.44269504088896340736;
constexpr double kLn2 = 0.693147180559945309417;

__device__ __forceinline__ float post_ninf() { return -__builtin_inff(); }
// (integer tests on the bits, hidden from the optimiser: the library is built with -fno-honor-nans, under which a test of a
//  float's bits may be folded as a floating-point class test that assumes no NaN)
__device__ __forceinline__ int post_bad_bits(float x)
{
    uint32_t b = __builtin_bit_cast(uint32_t, x);
    asm volatile("" : "+v"(b));
    return ((b & 0x7fffffffu) > 0x7f800000u ? 1 : 0) | (b == 0x7f800000u ? 2 : 0);   // 1: NaN, 2: +inf
}
// (fmax, not fmaxf: HIP declares fmaxf for floats only, and a double maximum taken through it is rounded to float32 - harmless
//  while the cells stay within exp2's range of it, fatal for a frame 2^37 nats below its neighbours)
__device__ __forceinline__ double post_wave_max(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = fmax(x, __shfl_xor(x, off));
    return x;
}
// One wavefront: its LDS operations execute in program order, so a frame hand-off needs no s_barrier (whose fence would also
// wait for the global loads prefetched for the next frame), only a compiler fence that keeps the accesses in order.
__device__ __forceinline__ void post_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ double post_dninf() { return -__builtin_inf(); }
// log2(sum 2^x_j) from the running maximum; all -inf -> -inf (never 2^(-inf - -inf))
__device__ __forceinline__ double post_lse2(const double *x, int n, double mx)
{
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += exp2(x[j] - mx);
    return mx == post_dninf() ? post_dninf() : mx + log2(s);
}
// band of align.py:64-65 from q = floor(L t / T)
__device__ __forceinline__ void post_band(int64_t q, int64_t L, int64_t B, int64_t &lo, int64_t &hi)
{
    lo = q - B / 2;
    lo = lo < 0 ? 0 : lo;
    hi = (L - lo < B) ? L : lo + B;
}
// The band as a policy of the passes above (posterior_lattice, fb_ck_forward, fb_ck_recompute, fb_ck), two of them, both
// built as Band(L, beam, T, table):
//   start()        before frame 0 and before any use of the band: is the band valid?  The walk then stands at frame 0.
//   seek(t)        stand at frame t, any t in [0, T]
//   next(), prev() one frame on or back; the passes step one frame past either end (to T from T-1, to -1 from 0)
//   band(lo, hi)   the band of the frame the walk stands at
//   kTable         does the band come from a caller's table (positions below lo_0 are then held by no band)?
// BandWalk: the reference's diagonal, q = floor(L t / T) of frame t, stepped one frame at a time (Bresenham: q + r / T = L t / T
// with 0 <= r < T)
struct BandWalk {
    static constexpr bool kTable = false;
    int64_t q, r, dq, dr, T, L, B;
    __device__ __forceinline__ BandWalk(int64_t L_, int64_t B_, int64_t T_, const int32_t * = nullptr)   // (no table to walk)
        : q(0), r(0), dq(L_ / T_), dr(L_ % T_), T(T_), L(L_), B(B_)
    {
    }
    __device__ __forceinline__ bool start() const { return true; }
    __device__ __forceinline__ void seek(int64_t t)
    {
        q = (L * t) / T;
        r = (L * t) % T;
    }
    __device__ __forceinline__ void next()
    {
        q += dq;
        r += dr;
        if (r >= T) { r -= T; ++q; }
    }
    __device__ __forceinline__ void prev()
    {
        q -= dq;
        r -= dr;
        if (r < 0) { r += T; --q; }
    }
    __device__ __forceinline__ void band(int64_t &lo, int64_t &hi) const { post_band(q, L, B, lo, hi); }
};
// BandTable: the caller's table, lo_t = tab[t], hi_t = min(lo_t + B, L) (post_band's rule for hi).  A valid table holds
// 0 <= tab[t] < L, non-decreasing, any step; start() checks all of it with the whole workgroup before a value is used.
// The walk keeps the values of frames t-1, t and t+1; a step moves them along and loads the one that enters, so the value a
// frame's band is formed from was asked for a whole frame earlier.  The loads are scalar (constant address space: the table
// does not change under the kernel) and so count against lgkmcnt, not against the vmcnt of the row a form prefetches.
// No index leaves [0, T): frames past either end read the end's entry (at), which is what the passes' steps past the ends,
// fb_ck_recompute's seek(t0); prev() and fb_ck's seek(t1) with t1 = T come down to.
typedef __attribute__((address_space(4))) const int32_t *cci32_t;
struct BandTable {
    static constexpr bool kTable = true;
    const int32_t *const src;
    const cci32_t tab;
    const int32_t T, L, B;
    int32_t t, vp, v, vn;   // the frame the walk stands at; tab at t-1, t, t+1
    __device__ __forceinline__ BandTable(int64_t L_, int64_t B_, int64_t T_, const int32_t *tab_)
        : src(tab_), tab((cci32_t)(uintptr_t)tab_), T((int32_t)T_), L((int32_t)L_), B((int32_t)B_), t(0), vp(0), v(0), vn(0)
    {
    }
    __device__ __forceinline__ int32_t at(int32_t i) const { return tab[i < 0 ? 0 : (i < T ? i : T - 1)]; }
    __device__ __forceinline__ bool start()
    {
        int bad = 0;
        for (int32_t i = threadIdx.x; i < T; i += blockDim.x) {
            const int32_t x = src[i];
            bad |= (x < 0 || x >= L) ? 1 : 0;
            bad |= (i > 0 && src[i - 1] > x) ? 1 : 0;
        }
        if (__syncthreads_or(bad)) return false;
        seek(0);
        return true;
    }
    __device__ __forceinline__ void seek(int64_t t_)
    {
        t = (int32_t)t_;
        vp = at(t - 1);
        v = at(t);
        vn = at(t + 1);
    }
    __device__ __forceinline__ void next()
    {
        ++t;
        vp = v;
        v = vn;
        vn = at(t + 1);
    }
    __device__ __forceinline__ void prev()
    {
        --t;
        vn = v;
        v = vp;
        vp = at(t - 1);
    }
    __device__ __forceinline__ void band(int64_t &lo, int64_t &hi) const
    {
        lo = v;
        hi = ((int64_t)L - lo < B) ? (int64_t)L : lo + B;
    }
};
// the table a descriptor brings: none for a call's own descriptor (BandWalk), Banded<>::band_lo (BandTable).  The one place
// where a kernel's body meets the band.
__device__ __forceinline__ const int32_t *fb_table(const FbLattice &) { return nullptr; }
template <class Desc>
__device__ __forceinline__ const int32_t *fb_table(const Banded<Desc> &d)
{
    return d.band_lo;
}
// error flags -> status: a bad label is reported before anything runs; then NaN, +inf, a path value outside [0, L)
__device__ __forceinline__ int post_status_of(int flags)
{
    return (flags & 1) ? kStatusNaN : (flags & 2) ? kStatusNonFinite : (flags & 4) ? kStatusBadArgs : kStatusOk;
}
// the OR of every thread's error flags (__syncthreads_or is a predicate: it answers 0 or 1)
__device__ __forceinline__ int post_block_flags(int flags)
{
    return (__syncthreads_or(flags & 1) ? 1 : 0) | (__syncthreads_or(flags & 2) ? 2 : 0) | (__syncthreads_or(flags & 4) ? 4 : 0);
}
// a lattice without a result: log-likelihood NaN, or -inf for kStatusZeroMass (stored as bits: the library is built with
// -fno-honor-nans, under which a NaN constant is undefined); each caller also fills its output with NaN
constexpr uint64_t kNaN64 = 0x7ff8000000000000ull, kNinf64 = 0xfff0000000000000ull;
__device__ __forceinline__ void fb_fail_result(const FbLattice &d, PostResult *res, int status)
{
    if (threadIdx.x == 0) {
        res[d.idx].status = status;
        *reinterpret_cast<uint64_t *>(&res[d.idx].log_likelihood) = status == kStatusZeroMass ? kNinf64 : kNaN64;
    }
}
__device__ __forceinline__ bool fb_labels_bad(const FbLattice &d)
{
    int bad = 0;
    for (int i = threadIdx.x; i < d.S; i += blockDim.x) {
        const int l = d.labels[i];
        bad |= (l < 0 || l >= d.V) ? 1 : 0;
    }
    return __syncthreads_or(bad) != 0;
}
// lab'[p]: blanks at even positions, the caller's labels at odd ones
__device__ __forceinline__ int32_t fb_lab(const FbLattice &d, int64_t p) { return (p & 1) ? d.labels[p >> 1] : 0; }
// posterior of one frame from its two halves (log2 units), clamped to a probability
__device__ __forceinline__ float post_value(double cb, float dt, double D, double w, double Z)
{
    const double l2 = (cb + (double)dt) + (D + w) - Z;
    const double p = exp2(l2);
    return (float)(p < 1.0 ? p : 1.0);
}

// Z of a terminal as ka_posterior.hpp forms it (the block offset plus the float-stored relative alpha), in nats: the value the
// path-posterior call returns for a path that ends at s*
__device__ __forceinline__ double fb_reported_z(double cb, double ca, double us)
{
    return (cb + (double)(float)((ca - cb) + us)) * kLn2;
}

__device__ __forceinline__ double post_block_max(double x, double *red)   // red: 4 values of this frame's parity
{
    x = post_wave_max(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// sums in a fixed order (a butterfly; then the four wavefronts' sums from the first to the last), so that every thread holds the
// same bits and a lattice's do not depend on what ran before it
__device__ __forceinline__ double post_wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ double post_block_sum(double x, double *red)   // red: 4 values of this frame's parity
{
    x = post_wave_sum(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------------------
// the frame recurrences, with lab'[s] the label of position s:
//   forward:  u_t(s) = lse2_j u_{t-1}(s-j) - m_{t-1} + e_t(s)          j in [0, max_move), s-j in band t-1, not vetoed
//   backward: w_t(s) = lse2_j G_{t+1}(s+j) - n_{t+1},  G_t(s) = w_t(s) + e_t(s)
// A move of an even j >= 2 skips a label; it may not land on a cell whose label VALUE is 0 (align.py:80-81).  The backward
// pass reads such a move's source from the vetoable copy of G, -inf where the label value is 0.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool fb_skip(int j) { return j >= 2 && (j & 1) == 0; }
__device__ __forceinline__ bool fb_vetoed(int j, int32_t lab) { return fb_skip(j) && lab == 0; }

// fast form: one wavefront, position p at slot p & 1023 of an LDS column, row = the frame's log-probs in log2 units.
// lab_at(p): the cell's label; cell(p, val): the caller's use of u_t(p).  Returns the lane's maximum.
template <int M, class LabAt, class Cell>
__device__ __forceinline__ double fb_fast_fwd(int64_t lo, int64_t hi, int64_t plo, int64_t phi, const double *prev, double *cur,
                                              const double *row, double mprev, LabAt lab_at, Cell cell)
{
    const double NINF = post_dninf();
    double mymax = NINF;
    for (int64_t p = lo + threadIdx.x; p < hi; p += 64) {
        const int32_t lab = lab_at(p);
        const double e = row[lab];
        double x[M];
        double mx = NINF;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int64_t u = p - j;
            const bool ok = u >= plo && u < phi && !fb_vetoed(j, lab);
            x[j] = ok ? prev[u & 1023] : NINF;
            mx = fmax(mx, x[j]);
        }
        const double val = post_lse2(x, M, mx) + (e - mprev);
        cur[p & 1023] = val;
        cell(p, val);
        mymax = fmax(mymax, val);
    }
    return mymax;
}
// w_{T-1}(p) of a backward pass, by the End the pass is given: a terminal s* (an int64_t), beta_{T-1} = {s*: 0}; or an FbEndRow,
// the caller's row (nats, absolute) in log2 units relative to its maximum d0, or its terminal where the row is NULL
struct FbEndRow {
    const double *row;
    double d0;
    int64_t sstar;
};
__device__ __forceinline__ double fb_end_w(int64_t sstar, int64_t p) { return (p == sstar) ? 0.0 : post_dninf(); }
__device__ __forceinline__ double fb_end_w(const FbEndRow &e, int64_t p) { return e.row ? e.row[p] * kLog2e64 - e.d0 : fb_end_w(e.sstar, p); }

// G_t over [lo, hi) from G_{t+1} (gn, its vetoable copy vn) over [nlo, nhi) into gc / vc.  last: t = T-1 of a pass that
// starts there, beta_{T-1} = fb_end_w(end, .).  cell(p, lab, w): the caller's use of w_t(p).  Returns the lane's maximum of G_t.
template <int M, class End, class LabAt, class Cell>
__device__ __forceinline__ double fb_fast_bwd(int64_t lo, int64_t hi, int64_t nlo, int64_t nhi, const double *gn, const double *vn,
                                              double *gc, double *vc, const double *row, double nprev, bool last, End end,
                                              LabAt lab_at, Cell cell)
{
    const double NINF = post_dninf();
    double mymax = NINF;
    for (int64_t p = lo + threadIdx.x; p < hi; p += 64) {
        const int32_t lab = lab_at(p);
        double w;
        if (last) {
            w = fb_end_w(end, p);
        } else {
            double x[M];
            double mx = NINF;
#pragma unroll
            for (int j = 0; j < M; ++j) {
                const int64_t u = p + j;
                const bool ok = u >= nlo && u < nhi;
                const double g = fb_skip(j) ? vn[u & 1023] : gn[u & 1023];
                x[j] = ok ? g : NINF;
                mx = fmax(mx, x[j]);
            }
            w = post_lse2(x, M, mx) - nprev;
        }
        const double g = w + row[lab];   // (read here, not before the branch: a global label load stays behind the lse)
        gc[p & 1023] = g;
        vc[p & 1023] = lab == 0 ? NINF : g;
        mymax = fmax(mymax, g);
        cell(p, lab, w);
    }
    return mymax;
}

// generic form: one 256-thread workgroup, columns at absolute positions, labels and the log-prob row lrow read where they lie,
// M = d.max_move at run time.  The same contracts as the fast form's.
template <class Cell>
__device__ __forceinline__ double fb_gen_fwd(const FbLattice &d, const float *lrow, int64_t lo, int64_t hi, int64_t plo, int64_t phi,
                                             const double *prev, double *cur, double mprev, Cell cell)
{
    const int M = d.max_move;
    const double NINF = post_dninf();
    double mymax = NINF;
    for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
        const int32_t lab = fb_lab(d, p);
        const double e = (double)lrow[lab] * kLog2e64;
        auto in = [&](int j) {
            const int64_t u = p - j;
            return u >= plo && u < phi && !fb_vetoed(j, lab);
        };
        double mx = NINF;
        for (int j = 0; j < M && j <= p; ++j)
            if (in(j)) mx = fmax(mx, prev[p - j]);
        double s = 0.0;
        for (int j = 0; j < M && j <= p; ++j)
            if (in(j)) s += exp2(prev[p - j] - mx);
        const double l = mx == NINF ? NINF : mx + log2(s);
        const double val = l + (e - mprev);
        cur[p] = val;
        cell(p, val);
        mymax = fmax(mymax, val);
    }
    return mymax;
}
template <class End, class Cell>
__device__ __forceinline__ double fb_gen_bwd(const FbLattice &d, const float *lrow, int64_t lo, int64_t hi, int64_t nlo, int64_t nhi,
                                             const double *gn, const double *vn, double *gc, double *vc, double nprev, bool last,
                                             End end, Cell cell)
{
    const int M = d.max_move;
    const double NINF = post_dninf();
    double mymax = NINF;
    for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
        const int32_t lab = fb_lab(d, p);
        const double e = (double)lrow[lab] * kLog2e64;
        double w;
        if (last) {
            w = fb_end_w(end, p);
        } else {
            auto g = [&](int j) { return fb_skip(j) ? vn[p + j] : gn[p + j]; };
            double mx = NINF;
            for (int j = 0; j < M; ++j)
                if (p + j >= nlo && p + j < nhi) mx = fmax(mx, g(j));
            double s = 0.0;
            for (int j = 0; j < M; ++j)
                if (p + j >= nlo && p + j < nhi) s += exp2(g(j) - mx);
            w = (mx == NINF ? NINF : mx + log2(s)) - nprev;
        }
        const double g = w + e;
        gc[p] = g;
        vc[p] = lab == 0 ? NINF : g;
        mymax = fmax(mymax, g);
        cell(p, lab, w);
    }
    return mymax;
}

}  // namespace ka
