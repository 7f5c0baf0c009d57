// ka_engine_fb.hip — the forward-backward calls of the C ABI: best-path posteriors (ka_posterior.hpp), label occupancy
// (ka_occupancy.hpp), state posteriors at chosen frames (ka_state_posterior.hpp), expected state durations (ka_duration.hpp),
// state visit probabilities (ka_visit.hpp), exact boundary-time quantiles (ka_quantile.hpp), alignments sampled from the band
// posterior (ka_sample.hpp), the maximum-expected-accuracy alignment (ka_mea.hpp) and the posteriors under the caller's boundary
// conditions (ka_fb_resume.hpp); and, through the same driver, fb_impl, the best-path margins from max-marginals (ka_margin.hpp)
// and their resumed form (ka_margin_resume.hpp), which are max-plus and no forward-backward.  The first eight also run over a
// caller-given band (ka_ctc_*_banded_*: fb_impl<Call, ka::BandTable>, the same driver on Banded<Desc> descriptors).  Host code
// only.  They use the engine's workspace and pinned buffer, with their own kernels and workspace layout, whatever the engine's
// mode, and run to the end inside the call: no batch stays in flight.  (The best path over a band: ka_engine_band.hip.)
#include "ka_engine.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

namespace {

using namespace ka::host;
using ka::plan::align_up;

// ---- best-path posteriors (ka_posterior.hpp), label occupancy (ka_occupancy.hpp), state posteriors at chosen frames
// (ka_state_posterior.hpp) and expected state durations (ka_duration.hpp): their own kernels and workspace layout, whatever the
// engine's mode.  One driver, fb_impl; a call (PostCall, OccCall, StateCall, QuantCall, SampleCall, MeaCall, and PairCall as
// DurCall and VisitCall) brings what differs: its own arrays and their checks, its planner and its launch (launch<Band>, one
// for either band), the descriptor fields beyond FbLattice, its own staging (upload: host buffers only; stage: every memory
// mode), what two statuses mean, and kBandedGranule, the bytes a lattice's Banded<Desc> descriptor is carved as.
struct FbArgs : LatticeArgs {
    double *log_likelihood;
    int32_t *status;
    const int32_t *const *band_lo;   // NULL: the reference's diagonal band; else a table per lattice ([T] int32, where `mem` says)
};

// an optional array's entry: NULL where the array is
template <class P>
P at(P const *arr, int32_t i) { return arr ? arr[i] : nullptr; }

// why a lattice's k query frames are refused (StateCall, MarginResumeCall), or nullptr
const char *bad_frames(const int64_t *frames, int64_t k, int64_t T)
{
    if (k > 0 && !frames) return ": NULL frames";
    for (int64_t j = 0; j < k; ++j) {
        if (frames[j] < 0 || frames[j] >= T) return ": a frame outside [0, T)";
        if (j > 0 && frames[j] <= frames[j - 1]) return ": frames not strictly increasing";
    }
    return nullptr;
}

// whether one of a lattice's two output rows lies over one of its two input rows (2S+1 doubles each; any may be NULL): the
// resumed kernels read an input row again behind the store of an output row
bool rows_overlap(int64_t S, const double *out0, const double *out1, const double *in0, const double *in1)
{
    const size_t row = (size_t)(2 * S + 1) * sizeof(double);
    auto overlap = [row](const double *x, const double *y) {
        return x && y && reinterpret_cast<uintptr_t>(x) < reinterpret_cast<uintptr_t>(y) + row &&
               reinterpret_cast<uintptr_t>(y) < reinterpret_cast<uintptr_t>(x) + row;
    };
    return overlap(out0, in0) || overlap(out0, in1) || overlap(out1, in0) || overlap(out1, in1);
}

struct PostCall {
    using Desc = ka::PostLattice;
    static constexpr size_t kBandedGranule = ka::kBandedDescBytes;
    using Carve = ka::plan::PostCarve;
    static constexpr const char *kName = "posteriors";
    static constexpr const char *kBadArgs = ": a best-path position outside [0, 2S+1)";
    static constexpr const char *kZeroMass = ": no path of finite score reaches the best path's terminal";
    const int32_t *const *best_path;
    float *const *posteriors;

    bool arrays() const { return best_path && posteriors; }
    const char *bad_lattice(const FbArgs &, int32_t) const { return nullptr; }
    bool buffers(int32_t i) const { return best_path[i] && posteriors[i]; }
    static constexpr auto plan = ka::plan::posterior_workspace;
    template <class Band>
    static constexpr auto launch = ka::launch_posteriors<Band>;
    void fill(Desc &d, const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        if (a.mem == KA_MEM_HOST) {
            d.path = reinterpret_cast<const int32_t *>(ws + c.path);
            d.post = reinterpret_cast<float *>(ws + c.post);
        } else {
            d.path = best_path[i];
            d.post = posteriors[i];
        }
        d.ck = reinterpret_cast<double *>(ws + c.ck);
        d.col = reinterpret_cast<double *>(ws + c.col);
    }
    int upload(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        KA_HIP(hipMemcpyAsync(ws + c.path, best_path[i], (size_t)a.T[i] * 4, hipMemcpyHostToDevice, a.stream));
        return KA_OK;
    }
    int stage(const Carve &, const FbArgs &, int32_t, char *) const { return KA_OK; }
    int download(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        KA_HIP(hipMemcpyAsync(posteriors[i], ws + c.post, (size_t)a.T[i] * 4, hipMemcpyDeviceToHost, a.stream));
        return KA_OK;
    }
};

// the FbCkLattice fields that the slot calls (OccCall, StateCall, DurCall, SampleCall) fill alike: the lattice's slot, its
// terminal, the column stride
void fill_slot(ka::FbCkLattice &d, const ka::plan::SlotCarve &c, int64_t terminal, char *ws)
{
    d.ck = reinterpret_cast<double *>(ws + c.slot + c.parts.ck);
    d.ckcol = reinterpret_cast<double *>(ws + c.slot + c.parts.ckcol);
    d.slab = reinterpret_cast<double *>(ws + c.slot + c.parts.slab);
    d.col = reinterpret_cast<double *>(ws + c.slot + c.parts.col);
    d.terminal = (terminal >= 0 && terminal <= INT32_MAX) ? (int32_t)terminal : -1;
    d.cw = c.parts.cw;
}

struct OccCall {
    using Desc = ka::OccLattice;
    static constexpr size_t kBandedGranule = ka::kBandedDescBytes;
    using Carve = ka::plan::OccCarve;
    static constexpr const char *kName = "label posteriors";
    static constexpr const char *kBadArgs = ": terminal outside [0, 2S+1)";
    static constexpr const char *kZeroMass = ": no path of finite score reaches the terminal";
    const int64_t *terminal;
    float *const *occupancy;
    const int64_t *ld_out;

    bool arrays() const { return terminal && occupancy && ld_out; }
    const char *bad_lattice(const FbArgs &a, int32_t i) const { return ld_out[i] < a.V ? ": ld_out < V" : nullptr; }
    bool buffers(int32_t i) const { return occupancy[i] != nullptr; }
    static constexpr auto plan = ka::plan::label_posterior_workspace;
    template <class Band>
    static constexpr auto launch = ka::launch_label_posteriors<Band>;
    void fill(Desc &d, const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        if (a.mem == KA_MEM_HOST) {
            d.occ = reinterpret_cast<float *>(ws + c.occ);
            d.ld_out = a.V;
        } else {
            d.occ = occupancy[i];
            d.ld_out = ld_out[i];
        }
        fill_slot(d, c, terminal[i], ws);
        d.gbin = reinterpret_cast<unsigned long long *>(ws + c.slot + c.parts.gbin);
    }
    int upload(const Carve &, const FbArgs &, int32_t, char *) const { return KA_OK; }
    int stage(const Carve &, const FbArgs &, int32_t, char *) const { return KA_OK; }
    int download(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        KA_HIP(hipMemcpy2DAsync(occupancy[i], (size_t)ld_out[i] * 4, ws + c.occ, (size_t)a.V * 4, (size_t)a.V * 4, (size_t)a.T[i],
                                hipMemcpyDeviceToHost, a.stream));
        return KA_OK;
    }
};

struct StateCall {
    using Desc = ka::StateLattice;
    static constexpr size_t kBandedGranule = ka::kBandedDescBytes;
    using Carve = ka::plan::StateCarve;
    static constexpr const char *kName = "state posteriors";
    static constexpr const char *kBadArgs = ": terminal outside [0, 2S+1)";
    static constexpr const char *kZeroMass = ": no path of finite score reaches the terminal";
    const int64_t *terminal;
    const int64_t *const *frames;   // host arrays in both memory modes
    const int64_t *K;
    float *const *gamma;
    const int64_t *ld_out;
    int64_t *const *band_lo;

    bool arrays() const { return terminal && frames && K && gamma && ld_out && band_lo; }
    const char *bad_lattice(const FbArgs &a, int32_t i) const
    {
        if (const char *why = bad_frames(frames[i], K[i], a.T[i])) return why;
        const int64_t W = std::max<int64_t>(1, std::min<int64_t>(a.beam_size, 2 * a.S[i] + 1));
        return ld_out[i] < W ? ": ld_out < min(beam_size, 2S+1)" : nullptr;
    }
    bool buffers(int32_t i) const { return K[i] == 0 || (gamma[i] && band_lo[i]); }
    size_t plan(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam, int32_t max_move, bool host, Carve *cv,
                size_t *off_res) const
    {
        return ka::plan::state_posterior_workspace(n, T, S, K, V, beam, max_move, host, cv, off_res);   // (0 for K < 0 or K > T)
    }
    template <class Band>
    static constexpr auto launch = ka::launch_state_posteriors<Band>;
    void fill(Desc &d, const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        if (a.mem == KA_MEM_HOST) {
            d.gamma = reinterpret_cast<float *>(ws + c.gamma);
            d.band_lo = reinterpret_cast<int64_t *>(ws + c.band_lo);
            d.ld_out = c.W;
        } else {
            d.gamma = gamma[i];
            d.band_lo = band_lo[i];
            d.ld_out = ld_out[i];
        }
        fill_slot(d, c, terminal[i], ws);
        d.frames = reinterpret_cast<const int64_t *>(ws + c.frames);
        d.K = (int32_t)K[i];
        d.W = c.W;
    }
    int upload(const Carve &, const FbArgs &, int32_t, char *) const { return KA_OK; }
    int stage(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        if (K[i] > 0) KA_HIP(hipMemcpyAsync(ws + c.frames, frames[i], (size_t)K[i] * 8, hipMemcpyHostToDevice, a.stream));
        return KA_OK;
    }
    int download(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        if (K[i] == 0) return KA_OK;
        KA_HIP(hipMemcpy2DAsync(gamma[i], (size_t)ld_out[i] * 4, ws + c.gamma, (size_t)c.W * 4, (size_t)c.W * 4, (size_t)K[i],
                                hipMemcpyDeviceToHost, a.stream));
        KA_HIP(hipMemcpyAsync(band_lo[i], ws + c.band_lo, (size_t)K[i] * 8, hipMemcpyDeviceToHost, a.stream));
        return KA_OK;
    }
};

// The expected state durations and the state visit probabilities: one call over what differs, the descriptor's type, the
// launch and the error texts.  Both take a terminal and two output arrays of 2S+1 doubles, the second optional.
struct DurKind {
    using Desc = ka::DurLattice;
    static constexpr const char *kName = "state durations";
    static constexpr const char *kBadArgs = ": terminal outside [0, 2S+1)";
    static constexpr const char *kZeroMass = ": no path of finite score reaches the terminal";
    template <class Band>
    static constexpr auto launch = ka::launch_state_durations<Band>;
};
struct VisitKind {
    using Desc = ka::VisitLattice;
    static constexpr const char *kName = "state visits";
    static constexpr const char *kBadArgs = ": terminal outside [0, 2S+1)";
    static constexpr const char *kZeroMass = ": no path of finite score reaches the terminal";
    template <class Band>
    static constexpr auto launch = ka::launch_state_visits<Band>;
};
template <class Kind>
struct PairCall {
    using Desc = typename Kind::Desc;
    static constexpr size_t kBandedGranule = ka::kBandedDescBytes;
    using Carve = ka::plan::PairCarve;
    static constexpr const char *kName = Kind::kName;
    static constexpr const char *kBadArgs = Kind::kBadArgs;
    static constexpr const char *kZeroMass = Kind::kZeroMass;
    const int64_t *terminal;
    double *const *sum;    // duration, or visit
    double *const *tsum;   // time_sum, or exit_time: NULL, or an array in which any entry may be NULL: no time moment for that lattice

    bool arrays() const { return terminal && sum; }
    const char *bad_lattice(const FbArgs &, int32_t) const { return nullptr; }
    bool buffers(int32_t i) const { return sum[i] != nullptr; }
    bool moment(int32_t i) const { return tsum && tsum[i]; }
    static constexpr auto plan = ka::plan::pair_sum_workspace;
    template <class Band>
    static constexpr auto launch = Kind::template launch<Band>;
    void fill(Desc &d, const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        if (a.mem == KA_MEM_HOST) {
            d.sum = reinterpret_cast<double *>(ws + c.sum);
            d.tsum = moment(i) ? reinterpret_cast<double *>(ws + c.tsum) : nullptr;
        } else {
            d.sum = sum[i];
            d.tsum = moment(i) ? tsum[i] : nullptr;
        }
        fill_slot(d, c, terminal[i], ws);
    }
    int upload(const Carve &, const FbArgs &, int32_t, char *) const { return KA_OK; }
    int stage(const Carve &, const FbArgs &, int32_t, char *) const { return KA_OK; }
    int download(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        const size_t bytes = (size_t)(2 * a.S[i] + 1) * sizeof(double);
        KA_HIP(hipMemcpyAsync(sum[i], ws + c.sum, bytes, hipMemcpyDeviceToHost, a.stream));
        if (moment(i)) KA_HIP(hipMemcpyAsync(tsum[i], ws + c.tsum, bytes, hipMemcpyDeviceToHost, a.stream));
        return KA_OK;
    }
};
using DurCall = PairCall<DurKind>;
using VisitCall = PairCall<VisitKind>;

struct QuantCall {
    using Desc = ka::QuantLattice;
    static constexpr size_t kBandedGranule = ka::kBandedQuantDescBytes;   // (ka_boundary_quantile_band_table_workspace_bytes)
    using Carve = ka::plan::QuantCarve;
    static constexpr const char *kName = "boundary quantiles";
    static constexpr const char *kBadArgs = ": terminal outside [0, 2S+1)";
    static constexpr const char *kZeroMass = ": no path of finite score reaches the terminal";
    const int64_t *terminal;
    const int64_t *const *cuts;   // host arrays in both memory modes
    const int64_t *K;
    int32_t *const *quantile;
    const int64_t *ld_q;
    int32_t M;
    unsigned long long thr[ka::kMaxLevels];   // the levels as thresholds (quant_thresholds)
    mutable std::vector<std::vector<char>> staged;   // per lattice: its cuts and, behind them (the diagonal only), their start frames, until the call's end

    bool arrays() const { return terminal && cuts && K && quantile && ld_q; }
    const char *bad_lattice(const FbArgs &a, int32_t i) const
    {
        const int64_t k = K[i], L = 2 * a.S[i] + 1;
        if (k > 0 && !cuts[i]) return ": NULL cuts";
        for (int64_t j = 0; j < k; ++j) {
            if (cuts[i][j] < 0 || cuts[i][j] > L) return ": a cut outside [0, 2S+1]";
            if (j > 0 && cuts[i][j] <= cuts[i][j - 1]) return ": cuts not strictly increasing";
        }
        return ld_q[i] < M ? ": ld_q < M" : nullptr;
    }
    bool buffers(int32_t i) const { return K[i] == 0 || quantile[i] != nullptr; }
    size_t plan(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam, int32_t max_move, bool host, Carve *cv,
                size_t *off_res) const
    {
        return ka::plan::boundary_quantile_workspace(n, T, S, K, M, V, beam, max_move, host, cv, off_res);   // (0 for K < 0 or K > 2S+2)
    }
    template <class Band>
    static constexpr auto launch = ka::launch_boundary_quantiles<Band>;
    void fill(Desc &d, const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        if (a.mem == KA_MEM_HOST) {
            d.quant = reinterpret_cast<int32_t *>(ws + c.quant);
            d.ld_out = M;
        } else {
            d.quant = quantile[i];
            d.ld_out = ld_q[i];
        }
        fill_slot(d, c, terminal[i], ws);
        d.cuts = reinterpret_cast<const int64_t *>(ws + c.cuts);
        d.start = reinterpret_cast<const int32_t *>(ws + c.start);
        d.thr = reinterpret_cast<const unsigned long long *>(ws + c.thr);
        d.frow = reinterpret_cast<unsigned long long *>(ws + c.frow);
        d.K = (int32_t)K[i];
        d.M = M;
    }
    int upload(const Carve &, const FbArgs &, int32_t, char *) const { return KA_OK; }
    int stage(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        if (i == 0) {
            staged.assign((size_t)a.n, {});
            KA_HIP(hipMemcpyAsync(ws + c.thr, thr, sizeof(thr), hipMemcpyHostToDevice, a.stream));
        }
        const size_t k = (size_t)K[i];
        if (k == 0) return KA_OK;
        std::vector<char> &buf = staged[(size_t)i];
        const bool table = a.band_lo != nullptr;   // a table's start frames are the kernel's to find (QuantOut::begin): cuts only
        buf.resize(table ? k * 8 : k * 12);
        std::memcpy(buf.data(), cuts[i], k * 8);
        int32_t *start = reinterpret_cast<int32_t *>(buf.data() + k * 8);
        for (size_t j = 0; j < k && !table; ++j)
            start[j] = (int32_t)ka::plan::quantile_start_frame(cuts[i][j], a.T[i], 2 * a.S[i] + 1, a.beam_size);
        KA_HIP(hipMemcpyAsync(ws + c.cuts, buf.data(), buf.size(), hipMemcpyHostToDevice, a.stream));
        return KA_OK;
    }
    int download(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        if (K[i] == 0) return KA_OK;
        KA_HIP(hipMemcpy2DAsync(quantile[i], (size_t)ld_q[i] * 4, ws + c.quant, (size_t)M * 4, (size_t)M * 4, (size_t)K[i], hipMemcpyDeviceToHost,
                                a.stream));
        return KA_OK;
    }
};
// the levels of a boundary-quantile call as thresholds: thr_m = ceil(levels[m] 2^32), for 1 <= M <= kMaxLevels strictly increasing
// levels in [2^-10, 1 - 2^-10]; else the reason they are refused
const char *quant_thresholds(const double *levels, int32_t M, unsigned long long *thr)
{
    if (M < 1 || M > ka::kMaxLevels) return "boundary quantiles: M outside [1, 8]";
    if (!levels) return "boundary quantiles: NULL levels";
    const double lim = 1.0 / 1024.0;
    for (int32_t m = 0; m < ka::kMaxLevels; ++m) thr[m] = ~0ull;
    for (int32_t m = 0; m < M; ++m) {
        // (a NaN is found by its bits, hidden from the optimiser: the library is built with -fno-honor-nans)
        uint64_t b;
        std::memcpy(&b, &levels[m], sizeof(b));
        asm volatile("" : "+r"(b));
        if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return "boundary quantiles: a level is NaN";
        if (!(levels[m] >= lim && levels[m] <= 1.0 - lim)) return "boundary quantiles: a level outside [2^-10, 1 - 2^-10]";
        if (m > 0 && !(levels[m] > levels[m - 1])) return "boundary quantiles: levels not strictly increasing";
        thr[m] = (unsigned long long)std::ceil(levels[m] * 4294967296.0);
    }
    return nullptr;
}

struct SampleCall {
    using Desc = ka::SampleLattice;
    static constexpr size_t kBandedGranule = ka::kBandedDescBytes;
    using Carve = ka::plan::SampleCarve;
    static constexpr const char *kName = "sample paths";
    static constexpr const char *kBadArgs = ": terminal outside [0, 2S+1)";
    static constexpr const char *kZeroMass = ": no path of finite score reaches the terminal";
    const int64_t *terminal;
    const int32_t *n_samples;
    const uint64_t *seed;
    int32_t *const *paths;
    const int64_t *ld_paths;

    bool arrays() const { return terminal && n_samples && seed && paths && ld_paths; }
    const char *bad_lattice(const FbArgs &a, int32_t i) const
    {
        if (n_samples[i] < 1 || n_samples[i] > ka::kMaxSamples) return ": n_samples outside [1, 64]";
        return ld_paths[i] < a.T[i] ? ": ld_paths < T" : nullptr;
    }
    bool buffers(int32_t i) const { return paths[i] != nullptr; }
    size_t plan(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam, int32_t max_move, bool host, Carve *cv,
                size_t *off_res) const
    {
        return ka::plan::sample_paths_workspace(n, T, S, n_samples, V, beam, max_move, host, cv, off_res);
    }
    template <class Band>
    static constexpr auto launch = ka::launch_sample_paths<Band>;
    void fill(Desc &d, const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        if (a.mem == KA_MEM_HOST) {
            d.paths = reinterpret_cast<int32_t *>(ws + c.paths);
            d.ld_out = a.T[i];
        } else {
            d.paths = paths[i];
            d.ld_out = ld_paths[i];
        }
        fill_slot(d, c, terminal[i], ws);
        d.seed = seed[i];
        d.n_samples = n_samples[i];
    }
    int upload(const Carve &, const FbArgs &, int32_t, char *) const { return KA_OK; }
    int stage(const Carve &, const FbArgs &, int32_t, char *) const { return KA_OK; }
    int download(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        KA_HIP(hipMemcpy2DAsync(paths[i], (size_t)ld_paths[i] * 4, ws + c.paths, (size_t)a.T[i] * 4, (size_t)a.T[i] * 4, (size_t)n_samples[i],
                                hipMemcpyDeviceToHost, a.stream));
        return KA_OK;
    }
};

struct MeaCall {
    using Desc = ka::MeaLattice;
    static constexpr size_t kBandedGranule = ka::kBandedDescBytes;
    using Carve = ka::plan::MeaCarve;
    static constexpr const char *kName = "mea path";
    static constexpr const char *kBadArgs = ": terminal outside [0, 2S+1)";
    static constexpr const char *kZeroMass = ": no path of finite score reaches the terminal";
    const int64_t *terminal;
    int32_t *const *path;
    double *expected_accuracy;   // host array in both memory modes, as log_likelihood is; may be NULL

    bool arrays() const { return terminal && path; }
    const char *bad_lattice(const FbArgs &, int32_t) const { return nullptr; }
    bool buffers(int32_t i) const { return path[i] != nullptr; }
    static constexpr auto plan = ka::plan::mea_path_workspace;
    template <class Band>
    static constexpr auto launch = ka::launch_mea_path<Band>;
    void fill(Desc &d, const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        d.path = a.mem == KA_MEM_HOST ? reinterpret_cast<int32_t *>(ws + c.path) : path[i];
        fill_slot(d, c, terminal[i], ws);
        d.ea = reinterpret_cast<double *>(ws + c.ea);
        d.bp = ws + c.bp;
        d.wcol = reinterpret_cast<double *>(ws + c.wcol);
    }
    int upload(const Carve &, const FbArgs &, int32_t, char *) const { return KA_OK; }
    int stage(const Carve &, const FbArgs &, int32_t, char *) const { return KA_OK; }
    int download(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        KA_HIP(hipMemcpyAsync(path[i], ws + c.path, (size_t)a.T[i] * 4, hipMemcpyDeviceToHost, a.stream));
        return KA_OK;
    }
};

// The best-path margins (ka_margin.hpp): fb_impl on the diagonal's descriptors, with the table a field the call fills itself,
// since one batch mixes lattices that bring a table with lattices that do not.  The score rides in PostResult::log_likelihood.
struct MarginCall {
    using Desc = ka::MarginLattice;
    static constexpr size_t kBandedGranule = ka::kBandedDescBytes;   // (never carved: no Banded<> sibling)
    using Carve = ka::plan::MarginCarve;
    static constexpr const char *kName = "path margins";
    static constexpr const char *kBadArgs = ": a path value outside [0, 2S+1), or band_lo does not hold non-decreasing values in [0, 2S+1)";
    static constexpr const char *kZeroMass = ": no path of finite score reaches the path's last state";
    const int32_t *const *band_lo;   // NULL, or an array in which any entry may be NULL: that lattice runs on the diagonal
    const int32_t *const *path;
    int32_t unit;
    double *const *through;
    double *const *alt;
    int32_t *const *runner_up;       // NULL, or an array in which any entry may be NULL

    bool arrays() const { return path && through && alt; }
    const char *bad_lattice(const FbArgs &, int32_t) const { return nullptr; }
    bool buffers(int32_t i) const { return path[i] && through[i] && alt[i]; }
    const int32_t *table(int32_t i) const { return band_lo ? band_lo[i] : nullptr; }
    int32_t *runner(int32_t i) const { return runner_up ? runner_up[i] : nullptr; }
    static constexpr auto plan = ka::plan::path_margin_workspace;
    template <class Band>
    static constexpr auto launch = ka::launch_path_margins;
    void fill(Desc &d, const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        if (a.mem == KA_MEM_HOST) {
            d.band_lo = table(i) ? reinterpret_cast<const int32_t *>(ws + c.tab) : nullptr;
            d.path = reinterpret_cast<const int32_t *>(ws + c.path);
            d.through = reinterpret_cast<double *>(ws + c.through);
            d.alt = reinterpret_cast<double *>(ws + c.alt);
            d.runner = runner(i) ? reinterpret_cast<int32_t *>(ws + c.runner) : nullptr;
        } else {
            d.band_lo = table(i);
            d.path = path[i];
            d.through = through[i];
            d.alt = alt[i];
            d.runner = runner(i);
        }
        d.unit = unit;
        fill_slot(d, c, -1, ws);
    }
    int upload(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        KA_HIP(hipMemcpyAsync(ws + c.path, path[i], (size_t)a.T[i] * 4, hipMemcpyHostToDevice, a.stream));
        if (table(i)) KA_HIP(hipMemcpyAsync(ws + c.tab, table(i), (size_t)a.T[i] * 4, hipMemcpyHostToDevice, a.stream));
        return KA_OK;
    }
    int stage(const Carve &, const FbArgs &, int32_t, char *) const { return KA_OK; }
    int download(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        const size_t T = (size_t)a.T[i];
        KA_HIP(hipMemcpyAsync(through[i], ws + c.through, T * sizeof(double), hipMemcpyDeviceToHost, a.stream));
        KA_HIP(hipMemcpyAsync(alt[i], ws + c.alt, T * sizeof(double), hipMemcpyDeviceToHost, a.stream));
        if (runner(i)) KA_HIP(hipMemcpyAsync(runner(i), ws + c.runner, T * 4, hipMemcpyDeviceToHost, a.stream));
        return KA_OK;
    }
};

// The best-path margins under the caller's boundary conditions, with rows of m at chosen frames (ka_margin_resume.hpp):
// MarginCall's arrays, every one of them optional here, and beside them two rows in, two rows out and the query frames with
// their rows.  Like MarginCall it runs as fb_impl on the diagonal's descriptors and fills the table itself.
struct MarginResumeCall {
    using Desc = ka::MarginResumeLattice;
    static constexpr size_t kBandedGranule = ka::kBandedDescBytes;   // (never carved: no Banded<> sibling)
    using Carve = ka::plan::MarginResumeCarve;
    static constexpr const char *kName = "margins resume";
    static constexpr const char *kBadArgs =
        ": a path value or the terminal outside [0, 2S+1), a NaN or +inf in d_in or e_in, or band_lo does not hold non-decreasing values in [0, 2S+1)";
    static constexpr const char *kZeroMass = ": no path of finite score joins the start row to the end";
    const int32_t *const *band_lo;
    const double *const *d_in;
    const double *const *e_in;
    const int64_t *terminal;         // NULL: all -1 (path[T-1])
    const int32_t *const *path;
    int32_t unit;
    double *const *through;
    double *const *alt;
    int32_t *const *runner_up;
    const int64_t *const *frames;    // host arrays in both memory modes
    const int64_t *K;                // NULL: no query frames
    double *const *rows;
    const int64_t *ld_rows;
    int64_t *const *rows_lo;
    double *const *d_out;
    double *const *e_out;

    int64_t k(int32_t i) const { return K ? K[i] : 0; }
    int64_t term(int32_t i) const { return terminal ? terminal[i] : -1; }
    bool arrays() const { return true; }
    const char *bad_lattice(const FbArgs &a, int32_t i) const
    {
        const int64_t n = k(i);
        if (const char *why = bad_frames(at(frames, i), n, a.T[i])) return why;
        if (n > 0 && (!at(rows, i) || !at(rows_lo, i) || !ld_rows)) return ": state rows asked for without rows, ld_rows or rows_lo";
        const int64_t W = std::max<int64_t>(1, std::min<int64_t>(a.beam_size, 2 * a.S[i] + 1));
        if (n > 0 && ld_rows[i] < W) return ": ld_rows < min(beam_size, 2S+1)";
        if ((at(through, i) || at(alt, i) || at(runner_up, i)) && !at(path, i)) return ": through, alt or runner_up without path";
        if (term(i) < -1) return ": terminal must be -1 (the path's last state) or a position";
        if (!at(e_in, i) && term(i) == -1 && !at(path, i)) return ": neither e_in, a terminal nor a path says where the lattice ends";
        // (the kernel reads d_in again behind the store of d_out, and e_in behind it)
        return rows_overlap(a.S[i], at(d_out, i), at(e_out, i), at(d_in, i), at(e_in, i)) ? ": an output row overlaps an input row" : nullptr;
    }
    bool buffers(int32_t) const { return true; }
    size_t plan(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam, int32_t max_move, bool host, Carve *cv,
                size_t *off_res) const
    {
        return ka::plan::margins_resume_workspace(n, T, S, K, V, beam, max_move, host, cv, off_res);   // (0 for K < 0 or K > T)
    }
    template <class Band>
    static constexpr auto launch = ka::launch_margins_resume;
    void fill(Desc &d, const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        const bool host = a.mem == KA_MEM_HOST;
        auto dbl = [&](const double *p, size_t off) { return !p ? nullptr : host ? reinterpret_cast<double *>(ws + off) : const_cast<double *>(p); };
        d.band_lo = !at(band_lo, i) ? nullptr : host ? reinterpret_cast<const int32_t *>(ws + c.tab) : band_lo[i];
        d.path = !at(path, i) ? nullptr : host ? reinterpret_cast<const int32_t *>(ws + c.path) : path[i];
        d.through = dbl(at(through, i), c.through);
        d.alt = dbl(at(alt, i), c.alt);
        d.runner = !at(runner_up, i) ? nullptr : host ? reinterpret_cast<int32_t *>(ws + c.runner) : runner_up[i];
        d.unit = unit;
        d.d_in = dbl(at(d_in, i), c.rows[0]);
        d.e_in = dbl(at(e_in, i), c.rows[1]);
        d.d_out = dbl(at(d_out, i), c.rows[2]);
        d.e_out = dbl(at(e_out, i), c.rows[3]);
        fill_slot(d, c, -1, ws);
        d.terminal = term(i) < 0 ? -1 : (int32_t)std::min<int64_t>(term(i), INT32_MAX);   // (a position past the lattice is the kernel's to refuse)
        d.K = (int32_t)k(i);
        d.W = c.W;
        d.frames = reinterpret_cast<const int64_t *>(ws + c.frames);
        if (d.K > 0) {
            d.rows = host ? reinterpret_cast<double *>(ws + c.qrows) : rows[i];
            d.rows_lo = host ? reinterpret_cast<int64_t *>(ws + c.qlo) : rows_lo[i];
            d.ld_rows = host ? c.W : ld_rows[i];
        }
    }
    int upload(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        const size_t row = (size_t)(2 * a.S[i] + 1) * sizeof(double);
        if (at(path, i)) KA_HIP(hipMemcpyAsync(ws + c.path, path[i], (size_t)a.T[i] * 4, hipMemcpyHostToDevice, a.stream));
        if (at(band_lo, i)) KA_HIP(hipMemcpyAsync(ws + c.tab, band_lo[i], (size_t)a.T[i] * 4, hipMemcpyHostToDevice, a.stream));
        if (at(d_in, i)) KA_HIP(hipMemcpyAsync(ws + c.rows[0], d_in[i], row, hipMemcpyHostToDevice, a.stream));
        if (at(e_in, i)) KA_HIP(hipMemcpyAsync(ws + c.rows[1], e_in[i], row, hipMemcpyHostToDevice, a.stream));
        return KA_OK;
    }
    int stage(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        if (k(i) > 0) KA_HIP(hipMemcpyAsync(ws + c.frames, frames[i], (size_t)k(i) * 8, hipMemcpyHostToDevice, a.stream));
        return KA_OK;
    }
    int download(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        const size_t T = (size_t)a.T[i], row = (size_t)(2 * a.S[i] + 1) * sizeof(double);
        if (at(through, i)) KA_HIP(hipMemcpyAsync(through[i], ws + c.through, T * sizeof(double), hipMemcpyDeviceToHost, a.stream));
        if (at(alt, i)) KA_HIP(hipMemcpyAsync(alt[i], ws + c.alt, T * sizeof(double), hipMemcpyDeviceToHost, a.stream));
        if (at(runner_up, i)) KA_HIP(hipMemcpyAsync(runner_up[i], ws + c.runner, T * 4, hipMemcpyDeviceToHost, a.stream));
        if (at(d_out, i)) KA_HIP(hipMemcpyAsync(d_out[i], ws + c.rows[2], row, hipMemcpyDeviceToHost, a.stream));
        if (at(e_out, i)) KA_HIP(hipMemcpyAsync(e_out[i], ws + c.rows[3], row, hipMemcpyDeviceToHost, a.stream));
        if (k(i) > 0) {
            KA_HIP(hipMemcpy2DAsync(rows[i], (size_t)ld_rows[i] * 8, ws + c.qrows, (size_t)c.W * 8, (size_t)c.W * 8, (size_t)k(i),
                                    hipMemcpyDeviceToHost, a.stream));
            KA_HIP(hipMemcpyAsync(rows_lo[i], ws + c.qlo, (size_t)k(i) * 8, hipMemcpyDeviceToHost, a.stream));
        }
        return KA_OK;
    }
};

// Forward-backward posteriors under the caller's boundary conditions (ka_fb_resume.hpp): OccCall's slots with up to four rows, a
// path and two more outputs per lattice, every one of them optional (a NULL array, or a NULL entry).  Banded only.
struct ResumeFbCall {
    using Desc = ka::ResumeFbLattice;
    static constexpr size_t kBandedGranule = ka::kBandedResumeFbDescBytes;
    using Carve = ka::plan::ResumeFbCarve;
    static constexpr const char *kName = "posteriors resume";
    static constexpr const char *kBadArgs = ": terminal outside [0, 2S+1), or a NaN or +inf in alpha_in or beta_in";
    static constexpr const char *kZeroMass = ": no path of finite score joins the start row to the end";
    const double *const *alpha_in;
    const double *const *beta_in;
    const int64_t *terminal;         // may be NULL: every lattice then needs a beta_in
    const int32_t *const *path;
    float *const *occupancy;
    const int64_t *ld_out;           // required with occupancy
    float *const *path_post;
    double *const *alpha_out;
    double *const *beta_out;

    bool arrays() const { return !occupancy || ld_out; }
    const char *bad_lattice(const FbArgs &a, int32_t i) const
    {
        if (at(occupancy, i) && ld_out[i] < a.V) return ": ld_out < V";
        if (at(path_post, i) && !at(path, i)) return ": path_post without path";
        // (the kernel reads alpha_in again behind the store of alpha_out, and beta_in behind it)
        return rows_overlap(a.S[i], at(alpha_out, i), at(beta_out, i), at(alpha_in, i), at(beta_in, i)) ? ": an output row overlaps an input row"
                                                                                                       : nullptr;
    }
    bool buffers(int32_t) const { return true; }
    static constexpr auto plan = ka::plan::posteriors_resume_workspace;
    template <class Band>
    static constexpr auto launch = ka::launch_posteriors_resume<Band>;
    void fill(Desc &d, const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        const bool host = a.mem == KA_MEM_HOST;
        auto dbl = [&](const double *p, int k) { return !p ? nullptr : host ? reinterpret_cast<double *>(ws + c.rows[k]) : const_cast<double *>(p); };
        d.occ = !at(occupancy, i) ? nullptr : host ? reinterpret_cast<float *>(ws + c.occ) : occupancy[i];
        d.ld_out = !at(occupancy, i) ? 0 : host ? a.V : ld_out[i];
        d.alpha_in = dbl(at(alpha_in, i), 0);
        d.beta_in = dbl(at(beta_in, i), 1);
        d.alpha_out = dbl(at(alpha_out, i), 2);
        d.beta_out = dbl(at(beta_out, i), 3);
        d.path = !at(path, i) ? nullptr : host ? reinterpret_cast<const int32_t *>(ws + c.path) : path[i];
        d.path_post = !at(path_post, i) ? nullptr : host ? reinterpret_cast<float *>(ws + c.ppost) : path_post[i];
        fill_slot(d, c, terminal ? terminal[i] : -1, ws);
        d.gbin = reinterpret_cast<unsigned long long *>(ws + c.slot + c.parts.gbin);
    }
    int upload(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        const size_t row = (size_t)(2 * a.S[i] + 1) * sizeof(double);
        if (at(alpha_in, i)) KA_HIP(hipMemcpyAsync(ws + c.rows[0], alpha_in[i], row, hipMemcpyHostToDevice, a.stream));
        if (at(beta_in, i)) KA_HIP(hipMemcpyAsync(ws + c.rows[1], beta_in[i], row, hipMemcpyHostToDevice, a.stream));
        if (at(path, i)) KA_HIP(hipMemcpyAsync(ws + c.path, path[i], (size_t)a.T[i] * 4, hipMemcpyHostToDevice, a.stream));
        return KA_OK;
    }
    int stage(const Carve &, const FbArgs &, int32_t, char *) const { return KA_OK; }
    int download(const Carve &c, const FbArgs &a, int32_t i, char *ws) const
    {
        const size_t row = (size_t)(2 * a.S[i] + 1) * sizeof(double);
        if (at(occupancy, i))
            KA_HIP(hipMemcpy2DAsync(occupancy[i], (size_t)ld_out[i] * 4, ws + c.occ, (size_t)a.V * 4, (size_t)a.V * 4, (size_t)a.T[i],
                                    hipMemcpyDeviceToHost, a.stream));
        if (at(path_post, i)) KA_HIP(hipMemcpyAsync(path_post[i], ws + c.ppost, (size_t)a.T[i] * 4, hipMemcpyDeviceToHost, a.stream));
        if (at(alpha_out, i)) KA_HIP(hipMemcpyAsync(alpha_out[i], ws + c.rows[2], row, hipMemcpyDeviceToHost, a.stream));
        if (at(beta_out, i)) KA_HIP(hipMemcpyAsync(beta_out[i], ws + c.rows[3], row, hipMemcpyDeviceToHost, a.stream));
        return KA_OK;
    }
};

// what a call reads back per lattice besides PostResult, in both memory modes, enqueued behind the launch: nothing, but for
// the expected accuracies of MeaCall (one double per lattice, consecutive from lattice 0's)
template <class Call>
int fb_readback(const Call &, const typename Call::Carve *, const FbArgs &, char *)
{
    return KA_OK;
}
int fb_readback(const MeaCall &call, const ka::plan::MeaCarve *cv, const FbArgs &a, char *ws)
{
    if (call.expected_accuracy)
        KA_HIP(hipMemcpyAsync(call.expected_accuracy, ws + cv[0].ea, (size_t)a.n * sizeof(double), hipMemcpyDeviceToHost, a.stream));
    return KA_OK;
}

// A call with a table (FbArgs::band_lo) runs as fb_impl<Call, ka::BandTable>: the same steps on Banded<Desc> descriptors, which
// lie with the staged tables behind the sibling's workspace (plan::band_table_workspace), and the kernels of
// Call::launch<ka::BandTable>.  Call::launch<Band> is the call's one launch; a band whose unit does not exist does not link.
template <class Call, class Band = ka::BandWalk>
int fb_impl(ka_engine *e, const FbArgs &a, const Call &call)
{
    constexpr bool kBanded = std::is_same_v<Band, ka::BandTable>;
    using Desc = ka::BandDesc<typename Call::Desc, Band>;
    static_assert(sizeof(Desc) <= Call::kBandedGranule || !kBanded, "descriptor sizes");
    const int32_t n = a.n, V = a.V;
    const hipStream_t stream = a.stream;
    const bool host = a.host();
    int rc = refuse_call(e, a, Call::kName, call.arrays() && (!kBanded || a.band_lo));
    if (rc != KA_OK || n == 0) return rc;
    std::vector<typename Call::Carve> cv(n);
    size_t off_res = 0;
    size_t total = call.plan(n, a.T, a.S, V, a.beam_size, a.max_move, host, cv.data(), &off_res);
    if (total == 0) return fail(KA_ERR_BAD_ARGS, std::string(Call::kName) + ": unsupported T/S/V/beam_size/max_move");
    size_t off_desc = 0;            // the descriptors: at the head of the workspace, a banded call's behind the sibling's bytes
    std::vector<size_t> off_tab;    // banded, host buffers: the staged tables
    if (kBanded) {
        off_desc = total = align_up(total);
        off_tab.resize((size_t)n);
        total += ka::plan::band_table_workspace(n, a.T, host, off_tab.data(), Call::kBandedGranule);
    }
    for (int32_t i = 0; i < n; ++i) {
        if (a.ld[i] < V) return fail(KA_ERR_BAD_ARGS, "lattice " + std::to_string(i) + ": ld < V");
        if (const char *why = call.bad_lattice(a, i)) return fail(KA_ERR_BAD_ARGS, "lattice " + std::to_string(i) + why);
        if (!a.log_probs[i] || !call.buffers(i) || (a.S[i] > 0 && !a.labels[i]) || (kBanded && !a.band_lo[i]))
            return fail(KA_ERR_BAD_ARGS, "lattice " + std::to_string(i) + ": NULL buffer");
    }
    DeviceGuard guard;
    KA_HIP(guard.enter(e->device));
    const size_t desc_bytes = align_up((size_t)n * sizeof(Desc));
    if ((rc = begin_call(e, total, desc_bytes + (size_t)n * sizeof(ka::PostResult), stream)) != KA_OK) return rc;
    Desc *h = reinterpret_cast<Desc *>(e->res.pin);
    ka::PostResult *h_res = reinterpret_cast<ka::PostResult *>(e->res.pin + desc_bytes);
    SlotOrder order(cv.data(), n);
    const int32_t n_fast = order.n_fast;
    for (int32_t i = 0; i < n; ++i) {
        const auto &c = cv[i];
        Desc &d = h[order.next(c.fast)];
        fill_head(d, c, a, i, e->res.ws);
        call.fill(d, c, a, i, e->res.ws);
        if constexpr (kBanded)
            d.band_lo = host ? reinterpret_cast<const int32_t *>(e->res.ws + off_desc + off_tab[(size_t)i]) : a.band_lo[i];
    }
    if (host)
        for (int32_t i = 0; i < n; ++i) {
            if ((rc = stage_lattice(cv[i], a, i, e->res.ws)) != KA_OK) return rc;
            if ((rc = call.upload(cv[i], a, i, e->res.ws)) != KA_OK) return rc;
            if (kBanded)
                KA_HIP(hipMemcpyAsync(e->res.ws + off_desc + off_tab[(size_t)i], a.band_lo[i], (size_t)a.T[i] * 4, hipMemcpyHostToDevice, stream));
        }
    for (int32_t i = 0; i < n; ++i)
        if ((rc = call.stage(cv[i], a, i, e->res.ws)) != KA_OK) return rc;
    Desc *d_lats = reinterpret_cast<Desc *>(e->res.ws + off_desc);
    ka::PostResult *d_res = reinterpret_cast<ka::PostResult *>(e->res.ws + off_res);
    KA_HIP(hipMemcpyAsync(d_lats, h, (size_t)n * sizeof(Desc), hipMemcpyHostToDevice, stream));
    Call::template launch<Band>(d_lats, n_fast, n - n_fast, a.max_move, d_res, stream);
    KA_HIP(hipGetLastError());
    KA_HIP(hipMemcpyAsync(h_res, d_res, (size_t)n * sizeof(ka::PostResult), hipMemcpyDeviceToHost, stream));
    if ((rc = fb_readback(call, cv.data(), a, e->res.ws)) != KA_OK) return rc;
    if (host)
        for (int32_t i = 0; i < n; ++i)
            if ((rc = call.download(cv[i], a, i, e->res.ws)) != KA_OK) return rc;
    KA_HIP(hipStreamSynchronize(stream));
    int first_bad = KA_OK;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t st = h_res[i].status;
        if (a.status) a.status[i] = st;
        if (a.log_likelihood) a.log_likelihood[i] = h_res[i].log_likelihood;
        if (st != KA_OK && first_bad == KA_OK) {
            first_bad = st;
            g_err = "lattice " + std::to_string(i) + status_message(st, {nullptr, nullptr, ": a log-prob is +inf", Call::kBadArgs, Call::kZeroMass});
            if (kBanded && st == KA_ERR_BAD_ARGS) g_err += ", or band_lo does not hold non-decreasing values in [0, 2S+1)";
        }
    }
    return first_bad;
}


}  // namespace

extern "C" {

int ka_ctc_path_posteriors_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                     const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                     const int32_t *const *best_path, float *const *posteriors, double *log_likelihood, int32_t *status,
                                     int32_t mem, void *stream)
{
    return fb_impl(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status},
                   PostCall{best_path, posteriors});
}

int ka_ctc_path_posteriors_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                               int32_t beam_size, int32_t max_move, const int32_t *best_path, float *posteriors, double *log_likelihood,
                               int32_t mem, void *stream)
{
    return fb_impl(e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr},
                   PostCall{&best_path, &posteriors});
}

size_t ka_posterior_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move, int32_t mem)
{
    if (!countable(n, mem, {T, S})) return 0;
    return ka::plan::posterior_workspace(n, T, S, V, beam_size, max_move, mem == KA_MEM_HOST, nullptr, nullptr);
}

int ka_ctc_label_posteriors_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                      const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                      const int64_t *terminal, float *const *occupancy, const int64_t *ld_out, double *log_likelihood,
                                      int32_t *status, int32_t mem, void *stream)
{
    return fb_impl(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status},
                   OccCall{terminal, occupancy, ld_out});
}

int ka_ctc_label_posteriors_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                int32_t beam_size, int32_t max_move, int64_t terminal, float *occupancy, int64_t ld_out,
                                double *log_likelihood, int32_t mem, void *stream)
{
    return fb_impl(e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr},
                   OccCall{&terminal, &occupancy, &ld_out});
}

size_t ka_label_posterior_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move,
                                          int32_t mem)
{
    if (!countable(n, mem, {T, S})) return 0;
    return ka::plan::label_posterior_workspace(n, T, S, V, beam_size, max_move, mem == KA_MEM_HOST, nullptr, nullptr);
}

int ka_ctc_state_posteriors_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                      const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                      const int64_t *terminal, const int64_t *const *frames, const int64_t *K, float *const *gamma,
                                      const int64_t *ld_out, int64_t *const *band_lo, double *log_likelihood, int32_t *status, int32_t mem,
                                      void *stream)
{
    return fb_impl(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status},
                   StateCall{terminal, frames, K, gamma, ld_out, band_lo});
}

int ka_ctc_state_posteriors_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                int32_t beam_size, int32_t max_move, int64_t terminal, const int64_t *frames, int64_t K, float *gamma,
                                int64_t ld_out, int64_t *band_lo, double *log_likelihood, int32_t mem, void *stream)
{
    return fb_impl(e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr},
                   StateCall{&terminal, &frames, &K, &gamma, &ld_out, &band_lo});
}

size_t ka_state_posterior_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, const int64_t *K, int32_t V, int32_t beam_size,
                                          int32_t max_move, int32_t mem)
{
    if (!countable(n, mem, {T, S, K})) return 0;
    return ka::plan::state_posterior_workspace(n, T, S, K, V, beam_size, max_move, mem == KA_MEM_HOST, nullptr, nullptr);
}

int ka_ctc_state_durations_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                     const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                     const int64_t *terminal, double *const *duration, double *const *time_sum, double *log_likelihood,
                                     int32_t *status, int32_t mem, void *stream)
{
    return fb_impl(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status},
                   DurCall{terminal, duration, time_sum});
}

int ka_ctc_state_durations_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                               int32_t beam_size, int32_t max_move, int64_t terminal, double *duration, double *time_sum,
                               double *log_likelihood, int32_t mem, void *stream)
{
    return fb_impl(e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr},
                   DurCall{&terminal, &duration, &time_sum});
}

size_t ka_state_duration_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move,
                                         int32_t mem)
{
    if (!countable(n, mem, {T, S})) return 0;
    return ka::plan::pair_sum_workspace(n, T, S, V, beam_size, max_move, mem == KA_MEM_HOST, nullptr, nullptr);
}

// ---- the four calls over a caller-given band: their siblings' arguments with band_lo behind max_move ----
int ka_ctc_path_posteriors_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                            const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                            int32_t max_move, const int32_t *const *band_lo, const int32_t *const *best_path,
                                            float *const *posteriors, double *log_likelihood, int32_t *status, int32_t mem, void *stream)
{
    if (n > 0 && !band_lo) return fail(KA_ERR_BAD_ARGS, "posteriors: NULL band_lo");
    return fb_impl<PostCall, ka::BandTable>(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status, band_lo},
                                   PostCall{best_path, posteriors});
}

int ka_ctc_path_posteriors_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                      int32_t beam_size, int32_t max_move, const int32_t *band_lo, const int32_t *best_path,
                                      float *posteriors, double *log_likelihood, int32_t mem, void *stream)
{
    return fb_impl<PostCall, ka::BandTable>(
        e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr, &band_lo},
        PostCall{&best_path, &posteriors});
}

int ka_ctc_label_posteriors_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                             const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                             int32_t max_move, const int32_t *const *band_lo, const int64_t *terminal,
                                             float *const *occupancy, const int64_t *ld_out, double *log_likelihood, int32_t *status,
                                             int32_t mem, void *stream)
{
    if (n > 0 && !band_lo) return fail(KA_ERR_BAD_ARGS, "label posteriors: NULL band_lo");
    return fb_impl<OccCall, ka::BandTable>(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status, band_lo},
                                  OccCall{terminal, occupancy, ld_out});
}

int ka_ctc_label_posteriors_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                       int32_t beam_size, int32_t max_move, const int32_t *band_lo, int64_t terminal, float *occupancy,
                                       int64_t ld_out, double *log_likelihood, int32_t mem, void *stream)
{
    return fb_impl<OccCall, ka::BandTable>(
        e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr, &band_lo},
        OccCall{&terminal, &occupancy, &ld_out});
}

int ka_ctc_state_posteriors_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                             const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                             int32_t max_move, const int32_t *const *band_table, const int64_t *terminal,
                                             const int64_t *const *frames, const int64_t *K, float *const *gamma, const int64_t *ld_out,
                                             int64_t *const *band_lo, double *log_likelihood, int32_t *status, int32_t mem, void *stream)
{
    if (n > 0 && !band_table) return fail(KA_ERR_BAD_ARGS, "state posteriors: NULL band table");
    return fb_impl<StateCall, ka::BandTable>(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status, band_table},
                                    StateCall{terminal, frames, K, gamma, ld_out, band_lo});
}

int ka_ctc_state_posteriors_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                       int32_t beam_size, int32_t max_move, const int32_t *band_table, int64_t terminal, const int64_t *frames,
                                       int64_t K, float *gamma, int64_t ld_out, int64_t *band_lo, double *log_likelihood, int32_t mem,
                                       void *stream)
{
    return fb_impl<StateCall, ka::BandTable>(
        e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr, &band_table},
        StateCall{&terminal, &frames, &K, &gamma, &ld_out, &band_lo});
}

int ka_ctc_state_durations_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                            const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                            int32_t max_move, const int32_t *const *band_lo, const int64_t *terminal,
                                            double *const *duration, double *const *time_sum, double *log_likelihood, int32_t *status,
                                            int32_t mem, void *stream)
{
    if (n > 0 && !band_lo) return fail(KA_ERR_BAD_ARGS, "state durations: NULL band_lo");
    return fb_impl<DurCall, ka::BandTable>(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status, band_lo},
                                  DurCall{terminal, duration, time_sum});
}

int ka_ctc_state_durations_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                      int32_t beam_size, int32_t max_move, const int32_t *band_lo, int64_t terminal, double *duration,
                                      double *time_sum, double *log_likelihood, int32_t mem, void *stream)
{
    return fb_impl<DurCall, ka::BandTable>(
        e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr, &band_lo},
        DurCall{&terminal, &duration, &time_sum});
}

int ka_ctc_posteriors_resume_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                       const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                       const int32_t *const *band_lo, const double *const *alpha_in, const double *const *beta_in,
                                       const int64_t *terminal, const int32_t *const *path, float *const *occupancy, const int64_t *ld_out,
                                       float *const *path_post, double *const *alpha_out, double *const *beta_out, double *log_likelihood,
                                       int32_t *status, int32_t mem, void *stream)
{
    if (n > 0 && !band_lo) return fail(KA_ERR_BAD_ARGS, "posteriors resume: NULL band_lo");
    return fb_impl<ResumeFbCall, ka::BandTable>(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status, band_lo},
                                                ResumeFbCall{alpha_in, beta_in, terminal, path, occupancy, ld_out, path_post, alpha_out, beta_out});
}

int ka_ctc_posteriors_resume_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                 int32_t beam_size, int32_t max_move, const int32_t *band_lo, const double *alpha_in, const double *beta_in,
                                 int64_t terminal, const int32_t *path, float *occupancy, int64_t ld_out, float *path_post, double *alpha_out,
                                 double *beta_out, double *log_likelihood, int32_t mem, void *stream)
{
    return fb_impl<ResumeFbCall, ka::BandTable>(
        e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr, &band_lo},
        ResumeFbCall{&alpha_in, &beta_in, &terminal, &path, &occupancy, &ld_out, &path_post, &alpha_out, &beta_out});
}

size_t ka_posteriors_resume_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move,
                                            int32_t mem)
{
    if (!countable(n, mem, {T, S})) return 0;
    const size_t own = ka::plan::posteriors_resume_workspace(n, T, S, V, beam_size, max_move, mem == KA_MEM_HOST, nullptr, nullptr);
    const size_t tab = ka::plan::band_table_workspace(n, T, mem == KA_MEM_HOST, nullptr, ka::kBandedResumeFbDescBytes);
    return own && tab ? align_up(own) + tab : 0;
}

size_t ka_band_table_workspace_bytes(int32_t n, const int64_t *T, int32_t mem)
{
    if (!countable(n, mem, {T})) return 0;
    return ka::plan::band_table_workspace(n, T, mem == KA_MEM_HOST, nullptr);
}

size_t ka_boundary_quantile_band_table_workspace_bytes(int32_t n, const int64_t *T, int32_t mem)
{
    if (!countable(n, mem, {T})) return 0;
    return ka::plan::band_table_workspace(n, T, mem == KA_MEM_HOST, nullptr, ka::kBandedQuantDescBytes);
}

int ka_ctc_state_visits_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                  const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                  const int64_t *terminal, double *const *visit, double *const *exit_time, double *log_likelihood,
                                  int32_t *status, int32_t mem, void *stream)
{
    return fb_impl(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status},
                   VisitCall{terminal, visit, exit_time});
}

int ka_ctc_state_visits_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                            int32_t beam_size, int32_t max_move, int64_t terminal, double *visit, double *exit_time, double *log_likelihood,
                            int32_t mem, void *stream)
{
    return fb_impl(e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr},
                   VisitCall{&terminal, &visit, &exit_time});
}

size_t ka_state_visit_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move, int32_t mem)
{
    if (!countable(n, mem, {T, S})) return 0;
    return ka::plan::pair_sum_workspace(n, T, S, V, beam_size, max_move, mem == KA_MEM_HOST, nullptr, nullptr);
}

int ka_ctc_boundary_quantiles_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                        const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                        const int64_t *terminal, const int64_t *const *cuts, const int64_t *K, const double *levels, int32_t M,
                                        int32_t *const *quantile, const int64_t *ld_q, double *log_likelihood, int32_t *status, int32_t mem,
                                        void *stream)
{
    QuantCall call{terminal, cuts, K, quantile, ld_q, M, {}, {}};
    if (const char *why = quant_thresholds(levels, M, call.thr)) return fail(KA_ERR_BAD_ARGS, why);
    return fb_impl(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status}, call);
}

int ka_ctc_boundary_quantiles_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                  int32_t beam_size, int32_t max_move, int64_t terminal, const int64_t *cuts, int64_t K, const double *levels,
                                  int32_t M, int32_t *quantile, int64_t ld_q, double *log_likelihood, int32_t mem, void *stream)
{
    QuantCall call{&terminal, &cuts, &K, &quantile, &ld_q, M, {}, {}};
    if (const char *why = quant_thresholds(levels, M, call.thr)) return fail(KA_ERR_BAD_ARGS, why);
    return fb_impl(e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr}, call);
}

size_t ka_boundary_quantile_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, const int64_t *K, int32_t M, int32_t V,
                                            int32_t beam_size, int32_t max_move, int32_t mem)
{
    if (!countable(n, mem, {T, S, K})) return 0;
    return ka::plan::boundary_quantile_workspace(n, T, S, K, M, V, beam_size, max_move, mem == KA_MEM_HOST, nullptr, nullptr);
}

int ka_ctc_sample_paths_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                  const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                  const int64_t *terminal, const int32_t *n_samples, const uint64_t *seed, int32_t *const *paths,
                                  const int64_t *ld_paths, double *log_likelihood, int32_t *status, int32_t mem, void *stream)
{
    return fb_impl(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status},
                   SampleCall{terminal, n_samples, seed, paths, ld_paths});
}

int ka_ctc_sample_paths_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                            int32_t beam_size, int32_t max_move, int64_t terminal, int32_t n_samples, uint64_t seed, int32_t *paths,
                            int64_t ld_paths, double *log_likelihood, int32_t mem, void *stream)
{
    return fb_impl(e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr},
                   SampleCall{&terminal, &n_samples, &seed, &paths, &ld_paths});
}

size_t ka_sample_paths_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, const int32_t *n_samples, int32_t V, int32_t beam_size,
                                       int32_t max_move, int32_t mem)
{
    if (!countable(n, mem, {T, S, n_samples})) return 0;
    for (int32_t i = 0; i < n; ++i)
        if (n_samples[i] < 1 || n_samples[i] > ka::kMaxSamples) return 0;
    return ka::plan::sample_paths_workspace(n, T, S, n_samples, V, beam_size, max_move, mem == KA_MEM_HOST, nullptr, nullptr);
}

int ka_ctc_mea_path_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                              const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move, const int64_t *terminal,
                              int32_t *const *path, double *expected_accuracy, double *log_likelihood, int32_t *status, int32_t mem,
                              void *stream)
{
    return fb_impl(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status},
                   MeaCall{terminal, path, expected_accuracy});
}

int ka_ctc_mea_path_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                        int32_t beam_size, int32_t max_move, int64_t terminal, int32_t *path, double *expected_accuracy,
                        double *log_likelihood, int32_t mem, void *stream)
{
    return fb_impl(e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr},
                   MeaCall{&terminal, &path, expected_accuracy});
}

size_t ka_mea_path_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move, int32_t mem)
{
    if (!countable(n, mem, {T, S})) return 0;
    return ka::plan::mea_path_workspace(n, T, S, V, beam_size, max_move, mem == KA_MEM_HOST, nullptr, nullptr);
}

// ---- and the other four over a caller-given band ----
int ka_ctc_state_visits_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                         const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                         const int32_t *const *band_lo, const int64_t *terminal, double *const *visit,
                                         double *const *exit_time, double *log_likelihood, int32_t *status, int32_t mem, void *stream)
{
    if (n > 0 && !band_lo) return fail(KA_ERR_BAD_ARGS, "state visits: NULL band_lo");
    return fb_impl<VisitCall, ka::BandTable>(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status, band_lo}, VisitCall{terminal, visit, exit_time});
}

int ka_ctc_state_visits_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                   int32_t beam_size, int32_t max_move, const int32_t *band_lo, int64_t terminal, double *visit,
                                   double *exit_time, double *log_likelihood, int32_t mem, void *stream)
{
    return fb_impl<VisitCall, ka::BandTable>(e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr, &band_lo}, VisitCall{&terminal, &visit, &exit_time});
}

int ka_ctc_boundary_quantiles_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                               const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                               int32_t max_move, const int32_t *const *band_lo, const int64_t *terminal,
                                               const int64_t *const *cuts, const int64_t *K, const double *levels, int32_t M,
                                               int32_t *const *quantile, const int64_t *ld_q, double *log_likelihood, int32_t *status,
                                               int32_t mem, void *stream)
{
    QuantCall call{terminal, cuts, K, quantile, ld_q, M, {}, {}};
    if (const char *why = quant_thresholds(levels, M, call.thr)) return fail(KA_ERR_BAD_ARGS, why);
    if (n > 0 && !band_lo) return fail(KA_ERR_BAD_ARGS, "boundary quantiles: NULL band_lo");
    return fb_impl<QuantCall, ka::BandTable>(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status, band_lo}, call);
}

int ka_ctc_boundary_quantiles_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels,
                                         int64_t S, int32_t beam_size, int32_t max_move, const int32_t *band_lo, int64_t terminal,
                                         const int64_t *cuts, int64_t K, const double *levels, int32_t M, int32_t *quantile, int64_t ld_q,
                                         double *log_likelihood, int32_t mem, void *stream)
{
    QuantCall call{&terminal, &cuts, &K, &quantile, &ld_q, M, {}, {}};
    if (const char *why = quant_thresholds(levels, M, call.thr)) return fail(KA_ERR_BAD_ARGS, why);
    return fb_impl<QuantCall, ka::BandTable>(e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr, &band_lo}, call);
}

int ka_ctc_sample_paths_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                         const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                         const int32_t *const *band_lo, const int64_t *terminal, const int32_t *n_samples,
                                         const uint64_t *seed, int32_t *const *paths, const int64_t *ld_paths, double *log_likelihood,
                                         int32_t *status, int32_t mem, void *stream)
{
    if (n > 0 && !band_lo) return fail(KA_ERR_BAD_ARGS, "sample paths: NULL band_lo");
    return fb_impl<SampleCall, ka::BandTable>(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status, band_lo}, SampleCall{terminal, n_samples, seed, paths, ld_paths});
}

int ka_ctc_sample_paths_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                   int32_t beam_size, int32_t max_move, const int32_t *band_lo, int64_t terminal, int32_t n_samples,
                                   uint64_t seed, int32_t *paths, int64_t ld_paths, double *log_likelihood, int32_t mem, void *stream)
{
    return fb_impl<SampleCall, ka::BandTable>(e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr, &band_lo}, SampleCall{&terminal, &n_samples, &seed, &paths, &ld_paths});
}

int ka_ctc_mea_path_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                     const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                     const int32_t *const *band_lo, const int64_t *terminal, int32_t *const *path,
                                     double *expected_accuracy, double *log_likelihood, int32_t *status, int32_t mem, void *stream)
{
    if (n > 0 && !band_lo) return fail(KA_ERR_BAD_ARGS, "mea path: NULL band_lo");
    return fb_impl<MeaCall, ka::BandTable>(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, status, band_lo}, MeaCall{terminal, path, expected_accuracy});
}

int ka_ctc_mea_path_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                               int32_t beam_size, int32_t max_move, const int32_t *band_lo, int64_t terminal, int32_t *path,
                               double *expected_accuracy, double *log_likelihood, int32_t mem, void *stream)
{
    return fb_impl<MeaCall, ka::BandTable>(e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, log_likelihood, nullptr, &band_lo}, MeaCall{&terminal, &path, expected_accuracy});
}

// ---- best-path margins from max-marginals (ka_margin.hpp) ----
int ka_ctc_path_margins_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                  const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                  const int32_t *const *band_lo, const int32_t *const *path, int32_t unit, double *const *through,
                                  double *const *alt, int32_t *const *runner_up, double *score, int32_t *status, int32_t mem, void *stream)
{
    if (unit != 0 && unit != 1) return fail(KA_ERR_BAD_ARGS, "path margins: unit must be 0 (state) or 1 (text index)");
    return fb_impl(e, {{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, score, status},
                   MarginCall{band_lo, path, unit, through, alt, runner_up});
}

int ka_ctc_path_margins_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                            int32_t beam_size, int32_t max_move, const int32_t *band_lo, const int32_t *path, int32_t unit, double *through,
                            double *alt, int32_t *runner_up, double *score, int32_t mem, void *stream)
{
    if (unit != 0 && unit != 1) return fail(KA_ERR_BAD_ARGS, "path margins: unit must be 0 (state) or 1 (text index)");
    return fb_impl(e, {{1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, score, nullptr},
                   MarginCall{&band_lo, &path, unit, &through, &alt, &runner_up});
}

size_t ka_path_margin_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move, int32_t mem)
{
    if (!countable(n, mem, {T, S})) return 0;
    return ka::plan::path_margin_workspace(n, T, S, V, beam_size, max_move, mem == KA_MEM_HOST, nullptr, nullptr);
}

// ---- best-path margins under the caller's boundary conditions, rows of max-marginals at chosen frames (ka_margin_resume.hpp) ----
int ka_ctc_margins_resume_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                    const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                    const int32_t *const *band_lo, const double *const *d_in, const double *const *e_in, const int64_t *terminal,
                                    const int32_t *const *path, int32_t unit, double *const *through, double *const *alt,
                                    int32_t *const *runner_up, const int64_t *const *frames, const int64_t *K, double *const *rows,
                                    const int64_t *ld_rows, int64_t *const *rows_lo, double *const *d_out, double *const *e_out, double *score,
                                    int32_t *status, int32_t mem, void *stream)
{
    if (unit != 0 && unit != 1) return fail(KA_ERR_BAD_ARGS, "margins resume: unit must be 0 (state) or 1 (text index)");
    return fb_impl(e, FbArgs{{n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, score, status, nullptr},
                   MarginResumeCall{band_lo, d_in, e_in, terminal, path, unit, through, alt, runner_up, frames, K, rows, ld_rows, rows_lo, d_out,
                                    e_out});
}

int ka_ctc_margins_resume_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                              int32_t beam_size, int32_t max_move, const int32_t *band_lo, const double *d_in, const double *e_in,
                              int64_t terminal, const int32_t *path, int32_t unit, double *through, double *alt, int32_t *runner_up,
                              const int64_t *frames, int64_t K, double *rows, int64_t ld_rows, int64_t *rows_lo, double *d_out, double *e_out,
                              double *score, int32_t mem, void *stream)
{
    return ka_ctc_margins_resume_batch_f32(e, 1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, &band_lo, &d_in, &e_in, &terminal, &path,
                                           unit, &through, &alt, &runner_up, &frames, &K, &rows, &ld_rows, &rows_lo, &d_out, &e_out, score,
                                           nullptr, mem, stream);
}

size_t ka_margins_resume_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, const int64_t *K, int32_t V, int32_t beam_size,
                                         int32_t max_move, int32_t mem)
{
    if (!countable(n, mem, {T, S})) return 0;
    return ka::plan::margins_resume_workspace(n, T, S, K, V, beam_size, max_move, mem == KA_MEM_HOST, nullptr, nullptr);
}

}  // extern "C"
