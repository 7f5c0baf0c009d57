// ka_fb_form.hpp — the two forms of the forward-backward as a policy: FbFast<M> and FbGen own what differs between a
// one-wavefront and a workgroup pass, and every layer above them is written once: the checkpointed pass of ka_fb_ck.hpp on an
// FbCkLattice (the default descriptor) and the path-posterior kernel of ka_posterior.hpp on a PostLattice.
//                      FbFast<M>: band <= kFastMaxBand, V <= 64, M = max_move <= 4    FbGen: any band, any V, max_move <= 255
//   threads            NT = 64, one wavefront (kWave)                                 NT = 256
//   sync()             post_wave_sync                                                 __syncthreads
//   fence()            post_wave_sync: the frame hand-off, before a frame's cells     nothing: the barrier inside max() orders
//                      and after its bookkeeping                                      the frames
//   max(x)             post_wave_max                                                  post_block_max on red[ph], ph its state
//   sum(x)             post_wave_sum: a butterfly, every lane the same bits           post_block_sum on red[ph]: the four wavefronts' sums in order
//   col(k)             LDS column k, position p at cslot(p) = p & 1023                d.col + k L, position p at cslot(p) = p
//   slot(p, lo), cw()  checkpoint and slab: p & 1023 of 1024                          p - lo of d.cw, lo the frame's low end
//   ck_store, ck_load  all 1024 slots                                                 [plo, phi) of the column's band
//   row_prefetch(t),   a float of row t per lane, loaded a frame ahead; row() puts    nothing; row() points at d.lp + t ld, read
//   row(t, tn, more)   it into LDS in log2 units and loads row tn if `more`           in place
//   row(..., true)     returns the bad bits of the prefetched value                   returns those of a strided loop over the row
//   lab                the label source, LabDirect or LabRing (below)                 LabDirect
//   fwd, bwd           fb_fast_fwd<M>, fb_fast_bwd<M> with lab as their lab_at        fb_gen_fwd, fb_gen_bwd
// slot, cw, ck_store and ck_load touch what only an FbCkLattice has; like every member of a class template they are compiled
// where they are called, so a form on a PostLattice does without them.
// A form is built per lattice from the kernel's `__shared__ typename Form::template Shared<N>` (N working columns).  The
// recurrences stay the two pairs of ka_posterior_common.hpp: they sum their log-sum-exp terms in differently written loops,
// and a form's outputs keep the bits they have.
#pragma once
#include "ka_posterior_common.hpp"

namespace ka {

// Where a cell's label comes from: a member `lab` of the form, called as lab(p), with a hook at every place of a pass where a
// source that runs ahead of the band has work to do.  LabDirect reads the label where it lies; its hooks are empty.
struct LabDirect {
    struct Store {};
    const FbLattice &d;
    __device__ __forceinline__ LabDirect(const FbLattice &d_, Store &) : d(d_) {}
    __device__ __forceinline__ int32_t operator()(int64_t p) const { return fb_lab(d, p); }
    __device__ __forceinline__ void fill() {}
    __device__ __forceinline__ void fwd_request(int64_t) {}
    __device__ __forceinline__ void fwd_commit() {}
    __device__ __forceinline__ void turn(int64_t) {}
    __device__ __forceinline__ void bwd_request(int64_t, bool) {}
    __device__ __forceinline__ void bwd_commit() {}
};
// LabRing (fast form only): the labels of 1024 consecutive positions in LDS, position p at slot p & 1023, refilled as the band
// slides: [lfill - 1024, lfill) on the way forward, [lbot, lbot + 1024) on the way back.  A frame asks for what the next
// frame's band needs before its own fence (64 global loads, a frame ahead of their use) and stores it after its cells; a band
// that moved more than 64 positions (L > 64 T) is caught up with in the commit.
struct LabRing {
    struct Store {
        int32_t ring[1024];
    };
    const FbLattice &d;
    int32_t *const ring;
    int64_t lfill, lbot;
    int64_t want, np;   // the request in flight: the end the ring has to reach, this lane's position
    int32_t nlab;       // and its label
    __device__ __forceinline__ LabRing(const FbLattice &d_, Store &st) : d(d_), ring(st.ring), lfill(0), lbot(0), want(0), np(0), nlab(0) {}
    __device__ __forceinline__ int32_t operator()(int64_t p) const { return ring[p & 1023]; }

    __device__ __forceinline__ void fill()   // before frame 0
    {
        lfill = d.L < 1024 ? d.L : 1024;
        for (int64_t p = threadIdx.x; p < lfill; p += 64) ring[p] = fb_lab(d, p);
    }
    __device__ __forceinline__ void fwd_request(int64_t lon)   // lon: the low end of the next frame's band
    {
        want = (lon + 1024 < d.L) ? lon + 1024 : d.L;
        np = lfill + threadIdx.x;
        nlab = np < want ? fb_lab(d, np) : 0;
    }
    __device__ __forceinline__ void fwd_commit()
    {
        if (np < want) ring[np & 1023] = nlab;
        lfill = (lfill + 64 < want) ? lfill + 64 : (want > lfill ? want : lfill);
        for (int64_t p = lfill + threadIdx.x; lfill < want; p = lfill + threadIdx.x) {
            if (p < want) ring[p & 1023] = fb_lab(d, p);
            lfill = (lfill + 64 < want) ? lfill + 64 : want;
        }
    }
    __device__ __forceinline__ void turn(int64_t lo)   // between the passes; lo: the low end of frame T-1's band, which must be in
    {
        lbot = lfill - 1024 > 0 ? lfill - 1024 : 0;
        for (int64_t p = lo + threadIdx.x; p < lbot && p < lo + 1024; p += 64) ring[p & 1023] = fb_lab(d, p);
        if (lo < lbot) lbot = lo;
    }
    __device__ __forceinline__ void bwd_request(int64_t lon, bool more)   // lon: the low end of the previous frame's band, if `more`
    {
        want = more ? lon : lbot;
        np = lbot - 1 - threadIdx.x;
        nlab = np >= want ? fb_lab(d, np) : 0;
    }
    __device__ __forceinline__ void bwd_commit()
    {
        if (np >= want) ring[np & 1023] = nlab;
        lbot = (lbot - 64 > want) ? lbot - 64 : (want < lbot ? want : lbot);
        for (int64_t p = lbot - 1 - threadIdx.x; lbot > want; p = lbot - 1 - threadIdx.x) {
            if (p >= want) ring[p & 1023] = fb_lab(d, p);
            lbot = (lbot - 64 > want) ? lbot - 64 : want;
        }
    }
};

template <int M, class Desc = FbCkLattice, class Lab = LabDirect>
struct FbFast {
    static constexpr int NT = 64, kMoves = M;
    static constexpr bool kWave = true;
    template <int N>
    struct Shared : Lab::Store {   // (an empty Store adds no byte)
        double col[N][1024];
        double row[64];
    };
    const Desc &d;
    double (*const cols)[1024];
    double *const lds_row;
    float rv;   // this lane's entry of the prefetched row
    Lab lab;
    template <int N>
    __device__ __forceinline__ FbFast(const Desc &d_, Shared<N> &sh) : d(d_), cols(sh.col), lds_row(sh.row), rv(0.0f), lab(d_, sh) {}

    __device__ __forceinline__ void sync() const { post_wave_sync(); }
    __device__ __forceinline__ void fence() const { post_wave_sync(); }
    __device__ __forceinline__ double max(double x) { return post_wave_max(x); }
    __device__ __forceinline__ double sum(double x) { return post_wave_sum(x); }

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
        return fb_fast_fwd<M>(lo, hi, plo, phi, prev, cur, lds_row, mprev, lab, cell);
    }
    template <class End, class Cell>
    __device__ __forceinline__ double bwd(int64_t lo, int64_t hi, int64_t nlo, int64_t nhi, const double *gn, const double *vn, double *gc,
                                          double *vc, double nprev, bool last, End end, Cell cell) const
    {
        return fb_fast_bwd<M>(lo, hi, nlo, nhi, gn, vn, gc, vc, lds_row, nprev, last, end, lab, cell);
    }
};

// A correctness path, not tuned.
template <class Desc = FbCkLattice>
struct FbGen {
    static constexpr int NT = 256;
    static constexpr bool kWave = false;
    template <int N>
    struct Shared : LabDirect::Store {
        double red[2][4];
    };
    const Desc &d;
    double (*const red)[4];
    int ph;              // parity of the reduction slots
    const float *lrow;   // the frame's log-prob row
    LabDirect lab;       // (the recurrences read fb_lab themselves; here for its hooks)
    template <int N>
    __device__ __forceinline__ FbGen(const Desc &d_, Shared<N> &sh) : d(d_), red(sh.red), ph(0), lrow(nullptr), lab(d_, sh) {}

    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ void fence() const {}
    __device__ __forceinline__ double max(double x)
    {
        const double m = post_block_max(x, red[ph]);
        ph ^= 1;
        return m;
    }
    __device__ __forceinline__ double sum(double x)
    {
        const double m = post_block_sum(x, red[ph]);
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
    template <class End, class Cell>
    __device__ __forceinline__ double bwd(int64_t lo, int64_t hi, int64_t nlo, int64_t nhi, const double *gn, const double *vn, double *gc,
                                          double *vc, double nprev, bool last, End end, Cell cell) const
    {
        return fb_gen_bwd(d, lrow, lo, hi, nlo, nhi, gn, vn, gc, vc, nprev, last, end, cell);
    }
};

}  // namespace ka
