// ka_sample.hpp — alignments sampled from the band posterior (forward filter, backward sample): n_samples <= 64 whole paths
// s_0 ... s_{T-1} per lattice, drawn from the posterior over the band's paths that end at a caller-given terminal s*, and
// Z = alpha_{T-1}(s*).  Included by ka_sample.hip and ka_sample_banded.hip only.
//
// Same lattice, band, moves, veto, statuses, Z and form split as ka_occupancy.hpp (DESIGN.md sections 4.18 and 4.24).  The
// forward pass with its checkpoints and the recompute of a block's alpha into the slab are those of ka_fb_ck.hpp
// (fb_ck_forward, fb_ck_recompute: the functions its driver calls); there is no beta pass.  Walking the blocks last to
// first, lane (thread) k owns sample k: its state is one integer in a register, and for t = T-1 ... 1 it draws s_{t-1} given
// p = s_t from
//   x_j = u_{t-1}(p - j) for j in [0, max_move) with p - j in band t-1 and the move not vetoed, else -inf;  w_j = 2^(x_j - max x)
//   tot = w_0 + ... + w_{M-1} (ascending j, float64);  r = U(k, t-1) tot;  j* = the smallest j with w_0 + ... + w_j > r
//   (none, by rounding: the largest j with w_j > 0);  s_{t-1} = p - j*;  U(k, t) = (mix64(seed, k T + t) >> 11) 2^-53
// u_{t-1} is read from the slab row of t-1, and for t = t0 > 0 (the block's first frame) from checkpoint column k, which is
// alpha of t0 - 1 over the band of t0 - 1.  A path's probability is its share of Z.
//
// Ordering.  The slab is global memory; the cells of a row were stored by the lanes that own them in that frame, and the walk
// reads them from whichever lane holds the sample: across lanes, unlike fb_ck's beta step, which reads a cell from the
// lane that wrote it.  One wavefront (fast form): every frame of the recompute ends in FbFast's fence(), post_wave_sync: a
// sequentially consistent fence at wavefront scope over every address space - what the driver of ka_fb_ck.hpp already places between the
// slab's stores and its loads.  At that scope it costs no instruction: a wavefront issues its vector memory operations in
// order to the one L1 of its CU, which its own stores write through, so a later load of the wavefront sees them whichever
// lane issued them; the fence keeps the compiler from moving the accesses.  This leans on the slab's stores being plain ones:
// were they ever made non-temporal, or given another cache policy, the walk would need s_waitcnt vmcnt(0) (and the matching
// cache action) between the recompute and its first load.  Nothing but bit-equality to the reference tests it.  The next
// block's recompute overwrites the slab only after the walk has used every value it loaded (the last state of the block goes
// to the LDS tile before the tile is written out).
// Generic form: the barrier that ends fb_ck_recompute (FbGen's sync()), and the one behind the tile's write-out.
//
// Output.  A block's positions are staged in LDS, [64 samples][32 frames] int32 (rows padded by one word: lane k writes row
// k, and 32-word rows would put all 64 lanes on one bank), and written after the block's walk, each sample's 32 frames as
// one 128-byte row: lanes 0-31 of a wavefront write one sample's row, lanes 32-63 the next one's.
#pragma once
#include "ka_fb_ck.hpp"

namespace ka {

constexpr int kSampleTilePitch = kPostCk + 1;

// a lattice without a result: -1 over [0, T) of each of its n_samples rows, and the status and log-likelihood of fb_fail_result
template <int NT>
__device__ __forceinline__ void sample_fail(const SampleLattice &d, PostResult *res, int status)
{
    for (int k = 0; k < d.n_samples; ++k)
        for (int64_t t = threadIdx.x; t < d.T; t += NT) d.paths[(size_t)k * (size_t)d.ld_out + t] = -1;
    fb_fail_result(d, res, status);
}

// U(k, t): a 53-bit uniform in [0, 1) that depends on the lattice's seed, the sample and the frame alone - not on the batch,
// nor on how many samples are asked for
__device__ __forceinline__ double sample_uniform(const SampleLattice &d, int k, int64_t t)
{
    return (double)(mix64(d.seed, (uint64_t)k * (uint64_t)d.T + (uint64_t)t) >> 11) * 0x1p-53;
}

// The conditional draw of s_{t-1} given p = s_t.  alpha_at(u): u_{t-1}(u) for u in [plo, phi), the band of t-1; M: max_move.
// Invariant: u_t(s_t) is finite for every frame of every sample.  It holds at T-1: s_{T-1} = s*, which passed the zero-mass
// check.  If u_t(p) is finite, some allowed predecessor has a finite u_{t-1} (u_t(p) is their log-sum plus the emission), so
// mx is finite, the predecessor that attains it has w = 2^0 = 1 and tot >= 1.  A predecessor with w_j = 0 is never chosen:
// the running sum does not move at it, so it cannot be the first to exceed r, and the fallback takes a j with w_j > 0.  The
// chosen u_{t-1}(p - j*) is therefore above -inf, and below +inf as every alpha is.  (sample_pick and sample_draw below.)
// The draw itself from the M weights' exponents x (fast form: M <= 4 registers, each weight exponentiated once).  The two
// draws are two on purpose, and the walk takes the one of its form.
template <int M>
__device__ __forceinline__ int32_t sample_pick(int32_t p, const double (&x)[M], double u01)
{
    double mx = post_dninf();
#pragma unroll
    for (int j = 0; j < M; ++j) mx = fmax(mx, x[j]);
    double w[M];
    double tot = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        w[j] = exp2(x[j] - mx);
        tot += w[j];
    }
    const double r = u01 * tot;
    double c = 0.0;
    int jstar = -1, jlast = 0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        jlast = w[j] > 0.0 ? j : jlast;
        c += w[j];
        if (jstar < 0 && c > r) jstar = j;
    }
    return p - (jstar >= 0 ? jstar : jlast);
}
template <int M, class AlphaAt>
__device__ __forceinline__ int32_t sample_draw_small(int32_t p, int32_t lab, int64_t plo, int64_t phi, double u01, AlphaAt alpha_at)
{
    double x[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const int64_t u = (int64_t)p - j;
        x[j] = (u >= plo && u < phi && !fb_vetoed(j, lab)) ? alpha_at(u) : post_dninf();
    }
    return sample_pick<M>(p, x, u01);
}
// generic form: M = max_move at run time, up to 255, so nothing is kept: three passes over the predecessors (the maximum, the
// total, the running sum), the same expressions in the same order as sample_pick - a correctness path, as the form is
template <class AlphaAt>
__device__ __forceinline__ int32_t sample_draw(int M, int32_t p, int32_t lab, int64_t plo, int64_t phi, double u01, AlphaAt alpha_at)
{
    const double NINF = post_dninf();
    auto x_of = [&](int j) {
        const int64_t u = (int64_t)p - j;
        return (u >= plo && u < phi && !fb_vetoed(j, lab)) ? alpha_at(u) : NINF;
    };
    double mx = NINF;
    for (int j = 0; j < M; ++j) mx = fmax(mx, x_of(j));
    double tot = 0.0;
    for (int j = 0; j < M; ++j) tot += exp2(x_of(j) - mx);
    const double r = u01 * tot;
    double c = 0.0;
    int jstar = -1, jlast = 0;
    for (int j = 0; j < M; ++j) {
        const double w = exp2(x_of(j) - mx);
        jlast = w > 0.0 ? j : jlast;
        c += w;
        if (jstar < 0 && c > r) jstar = j;
    }
    return p - (jstar >= 0 ? jstar : jlast);
}

// the block's tile to the output: row k of the tile holds sample k's positions at frames [t0, t1); NT / 32 rows at a time,
// each by 32 consecutive threads
template <int NT>
__device__ __forceinline__ void sample_flush(const SampleLattice &d, int64_t t0, int64_t t1, const int32_t (*tile)[kSampleTilePitch])
{
    const int f = threadIdx.x & 31;
    for (int k = threadIdx.x >> 5; k < d.n_samples; k += NT / 32)
        if (t0 + f < t1) d.paths[(size_t)k * (size_t)d.ld_out + (size_t)(t0 + f)] = tile[k][f];
}

// The block walk, once over the form: thread k < n_samples owns sample k (a lane of the one wavefront, or one of the first 64
// threads of the workgroup).  The form's working columns 0 and 1 serve the forward pass and every recompute.  Band: the band
// of the forward pass, every recompute and every draw (BandWalk, or BandTable on `tab`, the caller's table).
template <class Form, class Band>
__device__ __forceinline__ void sample_walk(Form &f, const SampleLattice &d, PostResult *res, int32_t (*tile)[kSampleTilePitch],
                                            const int32_t *tab)
{
    const int tid = threadIdx.x;
    const int64_t T = d.T;
    Band bw(d.L, d.beam, T, tab);
    double Z, Zr;
    const int status = fb_ck_forward(f, bw, Z, Zr);   // (ends behind f.sync())
    if (status != kStatusOk) {
        sample_fail<Form::NT>(d, res, status);
        return;
    }
    const bool mine = tid < d.n_samples;
    int32_t p = d.terminal;   // s_{T-1} = s*
    for (int64_t k = (T - 1) / kPostCk; k >= 0; --k) {
        const int64_t t0 = k * kPostCk, t1 = (t0 + kPostCk < T) ? t0 + kPostCk : T;
        fb_ck_recompute(f, k, t0, t1, bw, f.col(0), f.col(1), [](int64_t, double) {});
        // (the recompute ended in the fast form's fence, or behind the generic form's barrier: the slab's stores are ordered
        //  before the loads below)
        const double *ckc = d.ckcol + k * f.cw();
        for (int64_t t = t1 - 1; t >= t0; --t) {   // bw stands at t + 1
            bw.prev();
            if (mine) tile[tid][t - t0] = p;
            if (t == 0) break;
            bw.prev();
            int64_t plo, phi;
            bw.band(plo, phi);   // the band of t - 1, which the slab row and the checkpoint column are both laid out by: the
                                 // walk's own frame t - 1 (a table's entry t - 1, also across a block's edge), never one formed from t
            bw.next();
            const double *al = t > t0 ? d.slab + (t - 1 - t0) * f.cw() : ckc;
            if (mine) {
                const double u01 = sample_uniform(d, tid, t - 1);
                auto alpha_at = [&](int64_t u) { return al[Form::slot(u, plo)]; };
                if constexpr (Form::kWave) p = sample_draw_small<Form::kMoves>(p, fb_lab(d, p), plo, phi, u01, alpha_at);
                else p = sample_draw(d.max_move, p, fb_lab(d, p), plo, phi, u01, alpha_at);
            }
        }
        f.sync();   // the tile's rows, written by the threads that own the samples, before the threads that write them out
        sample_flush<Form::NT>(d, t0, t1, tile);
        f.sync();   // the tile, and the slab, before the next block rewrites them
    }
    if (tid == 0) {
        res[d.idx].status = kStatusOk;
        res[d.idx].log_likelihood = Zr;
    }
}

template <class Form, class Band>
__global__ __launch_bounds__(Form::NT) void sample_kernel(const BandDesc<SampleLattice, Band> *__restrict__ lats, int n, PostResult *res)
{
    __shared__ typename Form::template Shared<2> sh;
    __shared__ int32_t tile[kMaxSamples][kSampleTilePitch];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        Form f(lats[i], sh);
        sample_walk<Form, Band>(f, lats[i], res, tile, fb_table(lats[i]));
        f.sync();
    }
}

// launch_fb_ck's form split, grid and slots over the sampler's five kernels of a band
template <class Band>
void launch_sample_paths(const BandDesc<SampleLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    using Desc = BandDesc<SampleLattice, Band>;
    launch_fb_slots<Desc>({sample_kernel<FbFast<1>, Band>, sample_kernel<FbFast<2>, Band>, sample_kernel<FbFast<3>, Band>,
                           sample_kernel<FbFast<4>, Band>},
                          sample_kernel<FbGen<>, Band>, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
