// ka_fb_form.hpp — the two forms of the checkpointed forward-backward (ka_fb_ck.hpp) as a policy: FbFast<M> and FbGen own
// what differs between a one-wavefront and a workgroup pass, and every layer above them is written once.
//                      FbFast<M>: band <= kFastMaxBand, V <= 64, M = max_move <= 4    FbGen: any band, any V, max_move <= 255
//   threads            NT = 64, one wavefront (kWave)                                 NT = 256
//   sync()             post_wave_sync                                                 __syncthreads
//   fence()            post_wave_sync: the frame hand-off, before a frame's cells     nothing: the barrier inside max() orders
//                      and after its bookkeeping                                      the frames
//   max(x)             post_wave_max                                                  post_block_max on red[ph], ph its state
//   col(k)             LDS column k, position p at cslot(p) = p & 1023                d.col + k L, position p at cslot(p) = p
//   slot(p, lo), cw()  checkpoint and slab: p & 1023 of 1024                          p - lo of d.cw, lo the frame's low end
//   ck_store, ck_load  all 1024 slots                                                 [plo, phi) of the column's band
//   row_prefetch(t),   a float of row t per lane, loaded a frame ahead; row() puts    nothing; row() points at d.lp + t ld, read
//   row(t, tn, more)   it into LDS in log2 units and loads row tn if `more`           in place
//   row(..., true)     returns the bad bits of the prefetched value                   returns those of a strided loop over the row
//   fwd, bwd           fb_fast_fwd<M>, fb_fast_bwd<M>                                 fb_gen_fwd, fb_gen_bwd
// A form is built per lattice from the kernel's `__shared__ typename Form::template Shared<N>` (N working columns).  The
// recurrences stay the two pairs of ka_posterior_common.hpp, which the path-posterior kernels (ka_posterior.hpp) call directly:
// they sum their log-sum-exp terms in differently written loops, and a form's outputs keep the bits they have.
#pragma once
#include "ka_posterior_common.hpp"

namespace ka {

template <int M>
struct FbFast {
    static constexpr int NT = 64, kMoves = M;
    static constexpr bool kWave = true;
    template <int N>
    struct Shared {
        double col[N][1024];
        double row[64];
    };
    const FbCkLattice &d;
    double (*const cols)[1024];
    double *const lds_row;
    float rv;   // this lane's entry of the prefetched row
    template <int N>
    __device__ __forceinline__ FbFast(const FbCkLattice &d_, Shared<N> &sh) : d(d_), cols(sh.col), lds_row(sh.row), rv(0.0f) {}

    __device__ __forceinline__ void sync() const { post_wave_sync(); }
    __device__ __forceinline__ void fence() const { post_wave_sync(); }
    __device__ __forceinline__ double max(double x) { return post_wave_max(x); }

    __device__ __forceinline__ double *col(int k) const { return cols[k]; }
    __device__ __forceinline__ static int64_t cslot(int64_t p) { return p & 1023; }
    __device__ __forceinline__ static int64_t slot(int64_t p, int64_t) { return p & 1023; }
    __device__ __forceinline__ int64_t cw() const { return 1024; }
    __device__ __forceinline__ void ck_store(int64_t k, const double *c, int64_t, int64_t) const
    {
        for (int s = threadIdx.x; s < 1024; s += 64) d.ckcol[k * 1024 + s] = c[s];
    }
    __device__ __forceinline__ void ck_load(int64_t k, double *c, int64_t, int64_t) const
    {
        for (int s = threadIdx.x; s < 1024; s += 64) c[s] = d.ckcol[k * 1024 + s];
    }

    __device__ __forceinline__ void row_prefetch(int64_t t)
    {
        const int lane = threadIdx.x;
        rv = lane < (int64_t)d.V ? d.lp[(size_t)t * (size_t)d.ld + lane] : 0.0f;
    }
    __device__ __forceinline__ int row(int64_t, int64_t tn, bool more, bool check = false)
    {
        const int lane = threadIdx.x;
        const int64_t V = d.V;
        int bad = 0;
        if (lane < V) {
            if (check) bad = post_bad_bits(rv);
            lds_row[lane] = (double)rv * kLog2e64;
        }
        if (more && lane < V) rv = d.lp[(size_t)tn * (size_t)d.ld + lane];
        return bad;
    }

    template <class Cell>
    __device__ __forceinline__ double fwd(int64_t lo, int64_t hi, int64_t plo, int64_t phi, const double *prev, double *cur, double mprev,
                                          Cell cell) const
    {
        return fb_fast_fwd<M>(lo, hi, plo, phi, prev, cur, lds_row, mprev, [this](int64_t p) { return fb_lab(d, p); }, cell);
    }
    template <class Cell>
    __device__ __forceinline__ double bwd(int64_t lo, int64_t hi, int64_t nlo, int64_t nhi, const double *gn, const double *vn, double *gc,
                                          double *vc, double nprev, bool last, int64_t sstar, Cell cell) const
    {
        return fb_fast_bwd<M>(lo, hi, nlo, nhi, gn, vn, gc, vc, lds_row, nprev, last, sstar, [this](int64_t p) { return fb_lab(d, p); },
                              cell);
    }
};

// A correctness path, not tuned.
struct FbGen {
    static constexpr int NT = 256;
    static constexpr bool kWave = false;
    template <int N>
    struct Shared {
        double red[2][4];
    };
    const FbCkLattice &d;
    double (*const red)[4];
    int ph;              // parity of the reduction slots
    const float *lrow;   // the frame's log-prob row
    template <int N>
    __device__ __forceinline__ FbGen(const FbCkLattice &d_, Shared<N> &sh) : d(d_), red(sh.red), ph(0), lrow(nullptr) {}

    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ void fence() const {}
    __device__ __forceinline__ double max(double x)
    {
        const double m = post_block_max(x, red[ph]);
        ph ^= 1;
        return m;
    }

    __device__ __forceinline__ double *col(int k) const { return d.col + k * (int64_t)d.L; }
    __device__ __forceinline__ static int64_t cslot(int64_t p) { return p; }
    __device__ __forceinline__ static int64_t slot(int64_t p, int64_t lo) { return p - lo; }
    __device__ __forceinline__ int64_t cw() const { return d.cw; }
    __device__ __forceinline__ void ck_store(int64_t k, const double *c, int64_t plo, int64_t phi) const
    {
        for (int64_t p = plo + threadIdx.x; p < phi; p += 256) d.ckcol[k * cw() + (p - plo)] = c[p];
    }
    __device__ __forceinline__ void ck_load(int64_t k, double *c, int64_t plo, int64_t phi) const
    {
        for (int64_t p = plo + threadIdx.x; p < phi; p += 256) c[p] = d.ckcol[k * cw() + (p - plo)];
    }

    __device__ __forceinline__ void row_prefetch(int64_t) {}
    __device__ __forceinline__ int row(int64_t t, int64_t, bool, bool check = false)
    {
        lrow = d.lp + (size_t)t * (size_t)d.ld;
        int bad = 0;
        if (check)
            for (int64_t v = threadIdx.x; v < d.V; v += 256) bad |= post_bad_bits(lrow[v]);
        return bad;
    }

    template <class Cell>
    __device__ __forceinline__ double fwd(int64_t lo, int64_t hi, int64_t plo, int64_t phi, const double *prev, double *cur, double mprev,
                                          Cell cell) const
    {
        return fb_gen_fwd(d, lrow, lo, hi, plo, phi, prev, cur, mprev, cell);
    }
    template <class Cell>
    __device__ __forceinline__ double bwd(int64_t lo, int64_t hi, int64_t nlo, int64_t nhi, const double *gn, const double *vn, double *gc,
                                          double *vc, double nprev, bool last, int64_t sstar, Cell cell) const
    {
        return fb_gen_bwd(d, lrow, lo, hi, nlo, nhi, gn, vn, gc, vc, nprev, last, sstar, cell);
    }
};

}  // namespace ka
