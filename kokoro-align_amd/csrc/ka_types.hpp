// ka_types.hpp — structs and constants shared by the host side (ka_engine.hip) and every device translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace ka {

// Pointers read from a descriptor in memory are generic ("flat") to the compiler; everything
// here lives in HBM, so say so: global_load/global_store instead of flat_* (which also tie
// up lgkmcnt).
#define KA_GLOBAL __attribute__((address_space(1)))
typedef KA_GLOBAL const float *gcf32_t;
typedef KA_GLOBAL float *gf32_t;
typedef KA_GLOBAL const int32_t *gci32_t;
typedef KA_GLOBAL int32_t *gi32_t;
typedef KA_GLOBAL const uint32_t *gcu32_t;
typedef KA_GLOBAL uint32_t *gu32_t;
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef KA_GLOBAL const v4i_t *gci4_t;

// the 64-bit hash generator of the synthetic inputs and of the path sampler's uniforms (definition: include/kokoro_align_amd.h)
__device__ __forceinline__ uint64_t mix64(uint64_t seed, uint64_t idx)
{
    uint64_t z = (seed * 0x9E3779B97F4A7C15ull + idx + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr int kStatusOk = 0;
constexpr int kStatusEmptyBeam = -1;
constexpr int kStatusBadLabel = -5;
constexpr int kStatusInternal = -8;  // a tile of the tiled form was never fed by the tile below it (a bug, not an input)
constexpr int kStatusNaN = -6;      // a log-prob is NaN (the reference's np.argmax would treat it as a maximum: not reproduced)
constexpr int kFlagZeroLabel = 1;   // meta flags: a transcript label is 0
constexpr int kFlagExact = 2;       // meta flags: the checkpointed path declined this lattice (non-finite log-probs)
constexpr int kFlagDeclined = 4;    // meta flags: declined, and too wide for the exact kernels' ring: no result (KA_ERR_NONFINITE)
constexpr int kFlagAllNeg = 8;      // meta flags: every log-prob has its sign bit set (forward_ck; a +0.0 clears it): the keyed backtrace is exact

constexpr int kSlots = 1024;        // 64 lanes x 16 cells
constexpr int kFastMaxBand = 1009;  // kSlots - 15: widest band the w16 layout can hold
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int kCkFrames = 32;       // checkpointed path: frames between stored score rings
constexpr int kRowDepth = 4;        // log-prob rows in flight per wave
static_assert(kRowDepth == 4, "the frame loop is unrolled by the 4 frames of a back-pointer group");

struct Lattice {
    const float *lp;        // [T, ld] log-probs (device)
    const int32_t *labels;  // [S] caller labels (device)
    int32_t *labx;          // [labx_len] 4*label of odd position 2i+1, zero padded (workspace)
    void *bp;               // w16: uint32 [ceil(T/4)][64 blocks][4 frames]; generic: uint8 [T][W]
    float *col;             // generic only: 2 x L float scores followed by 2 x L present bytes
    int32_t *path;          // [T] outputs (device)
    int32_t *lab_out;
    float *sc_out;
    int64_t ld;
    int32_t T, S, L, V;
    int32_t beam, max_move;
    int32_t labx_len, W;    // W = min(beam, L)
    int32_t idx;            // index of this lattice in the caller's batch
    int32_t n_final;        // tiled form: number of tiles alive in the last frame
    // checkpointed forms: the scores after frame 32 (k+1) - 1 are row k of `bp`; position p sits at float index
    // p & ck_mask of its row (one-wavefront form: the 1024-slot ring, mask 1023, pitch 4096; tiled form: a ring that
    // holds every tile the band can touch, or the whole label axis)
    uint32_t ck_mask;
    int32_t ck_pitch;       // bytes
    // chunk-parallel backtrace (ka_parallel_bt.hpp), rows addressed like the checkpoints (position p at p & ck_mask):
    uint8_t *map0;          // [chunk c][ck_pitch / 4]: how far the best path into position p of frame 32c+31 has risen since frame 32c-1
    uint16_t *map1;         // [super-chunk s][ck_pitch / 4]: the same over the 32 chunks of a super-chunk
    int32_t *entry;         // [chunks]: best-path position at the last frame of every chunk, then [super-chunks]: of every super-chunk
    int64_t chunk0;         // index of this lattice's chunk 0 among the chunks of the launch's chunk-parallel lattices
    int32_t par;            // 1: walked back by the chunk-parallel kernels, 0: by one wavefront (backtrace_rc_kernel<.., false>)
    int32_t pad_;
};

// The status record of one lattice, 16 bytes.  The host reads its copy of the records through this struct; device code
// addresses the same words as meta[4*idx + {0,1,2,3}] (meta_of).
struct LatticeMeta {
    int32_t status;     // kStatus* (the public header's KA_OK / KA_ERR_*)
    int32_t end;        // end position of the best path
    int32_t flags;      // kFlag* (bit0: a transcript label is 0)
    float score;        // total score
};
static_assert(sizeof(LatticeMeta) == 16, "four 32-bit words per lattice, as the kernels index them");
__device__ __forceinline__ int32_t *meta_of(int32_t *meta, int idx) { return meta + 4 * (size_t)idx; }

// ---- tiled forms (ka_tiled.hpp, ka_tiled256.hpp, ka_tiled128.hpp) ----
constexpr int kTpCells = 4;                    // cells per lane
constexpr int kTpTile = 64 * kTpCells;         // positions per tile
constexpr int kTpBlock = 32;                   // frames per staging block (= the checkpoint interval)
constexpr int kTpRing = 4;                     // LDS staging slots: the block being computed, the next one (landed), two more in flight
constexpr int kTpRowBytes = 256;               // LDS pitch of a staged row in the row-by-row staging mode (64 columns)
constexpr int kTpSlotBytes = kTpBlock * 256;   // LDS bytes of a staged block of rows (any mode)
constexpr int kTpStageBytes = 2048;            // publish staging: 512 B of lane 63's packets + the other lanes' scratch
constexpr uint32_t kTpSentinel = 0x7fc0deadu;  // verification fill of the halo region (a NaN: no score is ever NaN)
constexpr uint32_t kTpProgDone = 0x7fffffffu;  // progress word of a finished tile / of "no tile below"
static_assert(kCkFrames % kTpBlock == 0 && kTpBlock <= 32, "checkpoints fall on block ends; a block's packets are published by lanes 0..kTpBlock-1");

struct TileTask {
    int32_t lat;        // index into the launch's Lattice array
    int32_t tile;       // positions [256 tile, 256 tile + 256)
    int32_t t_in;       // first frame whose band reaches into the tile (hi(t) > 256 tile)
    int32_t t_end;      // first frame whose band has left it (lo(t) >= 256 (tile + 1)), or T
    int64_t halo_in;    // halo region byte offset of slot t_in of the boundary BELOW this tile (tile 0: the -inf region)
    int64_t halo_out;   // byte offset of slot t_in of the boundary ABOVE this tile (the top tile has one too: nobody reads it)
    int32_t fill_end;   // last slot of the upper boundary that the tile above reads (its t_end - 1)
    int32_t prog_in;    // progress word of the tile below (word 0 holds kTpProgDone: nothing below tile 0)
    int32_t prog_out;   // progress word of this tile
    int32_t below_end;  // t_end of the tile below (tile 0: INT32_MAX): the slots behind it hold -inf by construction (ka_tiled128.hpp uses it)
};
// per lattice, zeroed before every launch: terminal state by 64-bit atomicMax, arrival counter of the last-frame tiles
struct TileAux {
    unsigned long long best;   // (end position + 1) << 32 | score bits; 0 = no live state
    uint32_t arrived;
    uint32_t pad;
};

struct TpStats {
    unsigned long long phase[3];   // shader cycles: (wait | check+sum << 32), (progress | requests << 32), (publish+checkpoint)
    unsigned long long wait_ticks, total_ticks, spins, start_tick;   // 100 MHz ticks (ka_engine_set_verify(4): ka_debug_tile_stats)
    unsigned long long extra[2];   // 128-position tiles: (compute wavefront's cycles at the barrier | cycles in its frame blocks << 32), look-up wavefront's busy cycles
};

constexpr unsigned kTpLdsRequest = 40 * 1024;   // used: 32 KB rows + 2 KB packets + 2 KB publish staging
constexpr int kTp2BandBytes = 64 * 8 + 16;           // per block: KL, KE of 64 lanes + the event mask (worked out by the feeder, band_block)
constexpr int kTp2StageBytes = 2 * kTpStageBytes;   // publish staging, double-buffered (the feeder reads block it-1's while block it's is written)
constexpr int kTnCells = 2;
constexpr int kTnTile = 64 * kTnCells;
constexpr int kTgPairBytes = kTpBlock * 64 * 8;   // a block of emission pairs of a 128-position tile (ka_tiled128.hpp)

constexpr int kCuSlots = 2048;      // entries of a per-CU table indexed by cu_slot() (ka_device.hpp): XCC_ID (3 bits) | HW_ID's se, sh, cu (8 bits)

// ---- chunk-parallel backtrace (ka_parallel_bt.hpp) ----
constexpr int kCmCells = 8;                      // cells per lane
constexpr int kCmSpan = 64 * kCmCells;           // positions a wavefront recomputes
constexpr int kCmWarm = 96;                      // lowest positions of the window: warm-up only (3 positions x 32 frames)
constexpr int kCmOut = 408;                      // positions a wavefront delivers (a multiple of 8, <= kCmSpan - kCmWarm - 7)
constexpr int kCmCellsWide = 18;                 // ... and the wide form (round 4): 1152 positions recomputed,
constexpr int kCmOutWide = 64 * kCmCellsWide - kCmWarm - 8;   // 1048 delivered: the reference's band of 1000 in ONE wavefront
// which form a launch's map kernel takes, from the widest band among its chunk-parallel lattices: positions a wavefront delivers
inline int cm_out_for(int64_t max_w) { return max_w + 7 <= kCmOut ? kCmOut : kCmOutWide; }
constexpr int kSuperChunks = 32;                 // chunks per super-chunk
static_assert(kCmWarm == 3 * kCkFrames && kCmOut % 8 == 0 && kCmOut + kCmWarm <= kCmSpan, "window geometry");

// ---- the log-prob producer (ka_lstm.hpp) ----
constexpr int kLstmH = 128;
constexpr int kLstmTile = 16;          // sequences per workgroup
constexpr int kLstmIn = 40;           // input features of layer 0 (MFCC coefficients)

// ---- best-path posteriors and lattice log-likelihood (ka_posterior.hpp) ----
constexpr int kStatusBadArgs = -2;     // a best-path position outside [0, L)
constexpr int kStatusNonFinite = -7;   // a log-prob is +inf
constexpr int kStatusZeroMass = -9;    // no path of finite score ends at the best path's terminal
constexpr int kPostCk = 32;            // frames per forward offset checkpoint
// what every forward-backward call describes of a lattice; the shared device code (ka_posterior_common.hpp) takes this part
struct FbLattice {
    const float *lp;         // [T, ld] log-probs (device)
    const int32_t *labels;   // [S] caller labels (device)
    int64_t ld;
    int32_t T, S, L, V;
    int32_t beam, max_move;
    int32_t idx;             // index of this lattice in the caller's batch (its PostResult)
};
struct PostLattice : FbLattice {
    const int32_t *path;     // [T] the best path the posteriors are asked for (device)
    float *post;             // [T] output; between the two passes: log2 alpha at the path, relative to ck[t / kPostCk]
    double *ck;              // [(T - 1) / kPostCk + 1] the forward pass's log2 offset at the first frame of every block (workspace)
    double *col;             // generic form only: 4 x L doubles, two score columns and two vetoable copies (workspace)
};
struct PostResult {
    int32_t status;
    int32_t pad_;
    double log_likelihood;   // nats
};

// ---- label occupancy posteriors (ka_occupancy.hpp) ----
constexpr int kOccFastSlots = 1024;    // fast-form lattices resident at once (four wavefronts per CU): per-slot workspace
constexpr int kOccGenericSlots = 512;  // generic-form workgroups of one launch, each walking its lattices in turn
constexpr int kOccLdsBins = 2048;      // generic form: V up to this bins in LDS, above it in a workspace row
// what the checkpointed forward-backward (ka_fb_ck.hpp) reads of a lattice: its slot and terminal
struct FbCkLattice : FbLattice {
    double *ck;                   // [nblk][2] forward offset C and frame maximum m before the first frame of every block (slot)
    double *ckcol;                // [nblk][cw] alpha column before the first frame of every block, relative to its offset (slot)
    double *slab;                 // [kPostCk][cw] alpha of the block being walked back (slot)
    double *col;                  // generic form only: 4 x L doubles, the working columns (slot)
    int64_t ld_out;
    int32_t terminal;             // s*, or -1 for a value outside int32
    int32_t cw;                   // column stride of ckcol / slab: 1024 (fast form, slot = position & 1023) or the band width
};
struct OccLattice : FbCkLattice {
    float *occ;                   // [T, ld_out] output, V columns written
    unsigned long long *gbin;     // generic form, V > kOccLdsBins only: [V] fixed-point bins (slot)
};
// ---- state posteriors at chosen frames (ka_state_posterior.hpp): the occupancy's slots and form split ----
struct StateLattice : FbCkLattice {
    float *gamma;                 // [K, ld_out] output, W columns written
    int64_t *band_lo;             // [K] output: the band's low end at every query frame
    const int64_t *frames;        // [K] query frames, strictly increasing in [0, T) (workspace)
    int32_t K;
    int32_t W;                    // widest band: max(1, min(beam, L))
};
// ---- expected state durations (ka_duration.hpp): the occupancy's slots and form split ----
// and state visit probabilities (ka_visit.hpp): both sum a value e_t(s) of every band cell and its first time moment per
// position (ka_pair_acc.hpp), so they share the descriptor and differ in the type alone
struct PairLattice : FbCkLattice {
    double *sum;                  // [L] output: sum over t of e_t(s)
    double *tsum;                 // [L] output, or NULL: sum over t of t e_t(s)
};
struct DurLattice : PairLattice {};     // e = gamma_t(s): D(s) and B(s)
struct VisitLattice : PairLattice {};   // e = gamma_t(s) r_t(s): V(s), the probability of passing through s, and X(s)
// ---- exact boundary-time quantiles (ka_quantile.hpp): the occupancy's slots and form split ----
constexpr int kMaxLevels = 8;     // levels per call
struct QuantLattice : FbCkLattice {
    int32_t *quant;               // [K, ld_out] output, M columns written: the first frame at which F_t(cuts[k]) reaches thr[m]
    const int64_t *cuts;          // [K] cut positions, strictly increasing in [0, L] (workspace)
    const int32_t *start;         // [K] the first frame whose band lies at or above the cut, T if none: what the output starts from (workspace)
    const unsigned long long *thr;   // [M] the levels as 32.32 fixed-point thresholds, ascending (workspace, one array per call)
    unsigned long long *frow;     // generic form only: [cw] the frame's fixed-point row, then its prefix sums (slot)
    int32_t K, M;
};
// ---- alignments sampled from the band posterior (ka_sample.hpp): the occupancy's slots and form split ----
constexpr int kMaxSamples = 64;   // samples per lattice and call: one per lane of the fast form
struct SampleLattice : FbCkLattice {
    int32_t *paths;               // [n_samples, ld_out] output: row k is sample k's position at every frame, T columns written
    uint64_t seed;                // the lattice's own seed: U(k, t) = (mix64(seed, k T + t) >> 11) 2^-53
    int32_t n_samples;            // in [1, kMaxSamples]
    int32_t pad_;
};
// ---- the maximum-expected-accuracy alignment (ka_mea.hpp): the occupancy's slots and form split ----
struct MeaLattice : FbCkLattice {
    int32_t *path;                // [T] output: the path's position at every frame
    double *ea;                   // one double: sum over t of gamma_t(path[t]) (workspace; the host copies it out)
    void *bp;                     // back-pointers of every cell: uint32 [T][64] (fast form, 2 bits per cell) or uint8 [T][cw] (slot)
    double *wcol;                 // generic form only: 2 x L doubles, W of frame t+1 and of frame t (slot)
};
static_assert(sizeof(MeaLattice) == 136, "descriptor sizes");
// ---- best-path margins from max-marginals (ka_margin.hpp): the occupancy's slots and form split; no Banded<> sibling, the
// table is a field of its own because one call mixes lattices with a table and lattices on the diagonal ----
struct MarginLattice : FbCkLattice {
    const int32_t *band_lo;       // [T] the caller's table (device): lo_t; NULL: the reference's diagonal
    const int32_t *path;          // [T] the path the margins are asked for (device)
    double *through;              // [T] output: m_t(path[t])
    double *alt;                  // [T] output: the best m_t(p) outside the path's group
    int32_t *runner;              // [T] output, or NULL: the lowest p attaining alt[t]
    int32_t unit;                 // a group is p >> unit: 0 a state, 1 a text index
    int32_t pad_;
};
static_assert(sizeof(MarginLattice) == 152, "descriptor sizes");
// ---- best-path margins under the caller's boundary conditions and rows of max-marginals at chosen frames
// (ka_margin_resume.hpp): a descriptor of its own, so that MarginLattice and the workspace figures of
// ka_ctc_path_margins stay as they are.  path, through, alt and runner may each be NULL here; FbCkLattice::terminal is the
// end state where e_in is NULL, -1 for path[T-1].  The rows are [L] doubles, absolute, -inf = no path ----
struct MarginResumeLattice : MarginLattice {
    const double *d_in;           // D of the row before frame 0; NULL: the virtual state {0: 0.0}
    const double *e_in;           // E of frame T-1; NULL: {terminal: 0.0}
    double *d_out;                // output, or NULL: D of frame T-1 over its band, -inf elsewhere
    double *e_out;                // output, or NULL: E of the row before frame 0
    const int64_t *frames;        // [K] query frames, strictly increasing in [0, T) (workspace)
    double *rows;                 // [K, ld_rows] output, W columns written: m at every query frame, from the band's low end
    int64_t *rows_lo;             // [K] output: the band's low end at every query frame
    int64_t ld_rows;
    int32_t K;
    int32_t W;                    // widest band: max(1, min(beam, L))
};
static_assert(sizeof(MarginResumeLattice) == 224, "descriptor sizes");
// the workspace planners (ka_plan.hpp) carve n descriptors: their sizes are part of the published workspace byte counts
static_assert(sizeof(PostLattice) == 88 && sizeof(FbCkLattice) == 104 && sizeof(OccLattice) == 120 && sizeof(StateLattice) == 136 &&
                  sizeof(DurLattice) == 120 && sizeof(SampleLattice) == 128 && sizeof(VisitLattice) == 120 &&
                  sizeof(QuantLattice) == 152,
              "descriptor sizes");

// ---- the forward-backward calls over a caller-given band: a call's descriptor and, behind it, the caller's table.  Only the
// banded kernels read these; the descriptors above keep their sizes ----
template <class Desc>
struct Banded : Desc {
    const int32_t *band_lo;   // [T] the caller's table (device): lo_t
};
// the band policies of the device code (ka_posterior_common.hpp: the reference's diagonal, a caller's table) name the
// descriptor a kernel and its launch take
struct BandWalk;
struct BandTable;
template <class Desc, class Band>
using BandDesc = std::conditional_t<std::is_same_v<Band, BandTable>, Banded<Desc>, Desc>;
constexpr size_t kBandedDescBytes = 144;   // the largest of them but the quantiles': what ka_band_table_workspace_bytes reserves per lattice
constexpr size_t kBandedQuantDescBytes = 160;   // ... and ka_boundary_quantile_band_table_workspace_bytes, for Banded<QuantLattice>
static_assert(sizeof(Banded<PostLattice>) == 96 && sizeof(Banded<OccLattice>) == 128 && sizeof(Banded<StateLattice>) == kBandedDescBytes &&
                  sizeof(Banded<DurLattice>) == 128 && sizeof(Banded<VisitLattice>) == 128 && sizeof(Banded<SampleLattice>) == 136 &&
                  sizeof(Banded<MeaLattice>) == kBandedDescBytes && sizeof(Banded<QuantLattice>) == kBandedQuantDescBytes,
              "descriptor sizes");

// ---- forward-backward posteriors under the caller's boundary conditions (ka_fb_resume.hpp): the
// occupancy's descriptor, slots and form split; run over a caller's table only (Banded<ResumeFbLattice>).  The rows are [L]
// doubles in nats, absolute, -inf = no mass ----
struct ResumeFbLattice : OccLattice {   // occ may be NULL
    const double *alpha_in;       // ln alpha of the row before frame 0; NULL: the virtual state {0: 0}
    const double *beta_in;        // ln beta of frame T-1; NULL: {terminal: 0}
    double *alpha_out;            // output, or NULL: ln alpha of frame T-1
    double *beta_out;             // output, or NULL: ln beta of the row before frame 0
    const int32_t *path;          // [T] the path path_post is asked for, or NULL
    float *path_post;             // [T] output, or NULL: gamma at (t, path[t])
};
constexpr size_t kBandedResumeFbDescBytes = 176;   // what ka_posteriors_resume_workspace_bytes reserves per lattice
static_assert(sizeof(ResumeFbLattice) == 168 && sizeof(Banded<ResumeFbLattice>) == kBandedResumeFbDescBytes, "descriptor sizes");

// ---- best path over a caller-given band (ka_banded.hpp) ----
struct BandLattice {
    const float *lp;          // [T, ld] log-probs (device)
    const int32_t *labels;    // [S] caller labels (device)
    const int32_t *band_lo;   // [T] the caller's table (device): lo_t
    int32_t *labx;            // [labx_len] 4*label of odd position 2i+1, zero padded (workspace)
    int32_t *tab;             // one-wavefront form: [tab_len] band_lo[min(i+1, T-1)], 16-byte aligned (workspace); generic: NULL
    void *bp;                 // one-wavefront form: uint32 [ceil(T/4)][64 lanes][4 frames]; generic: uint8 [T][W]
    float *col;               // generic only: 2 x L float scores followed by 2 x L present bytes
    int32_t *path;            // [T] outputs (device)
    int32_t *lab_out;
    float *sc_out;
    int64_t ld;
    int32_t T, S, L, V;
    int32_t beam, max_move;
    int32_t labx_len, W;      // W = max(1, min(beam, L))
    int32_t tab_len;          // 4 ceil(T/4) + 4
    int32_t idx;              // index of this lattice in the caller's batch (its LatticeMeta)
};
static_assert(sizeof(BandLattice) == 128, "descriptor sizes");

// ---- ... resumed (ka_ctc_best_path_resume): what the call adds to a lattice, one entry per descriptor
// and in the descriptors' order ----
constexpr uint32_t kDeadScoreBits = 0x7fc00000u;   // the quiet NaN a dead cell of a score row holds
struct ResumeRows {
    const float *init;   // [L] the score row before frame 0 (device), NaN = dead; NULL: the virtual state {0: 0.0}
    float *fin;          // [L] the score row after frame T-1 (device), NaN = dead; NULL: not wanted
    int32_t *entry;      // one int32 (device, preset to -1): the cell of the start row the path left from; under a self-steering
                         // band (ka_ctc_best_path_tracking_resume, section 4.35) two: entry[1] (preset to -1) the low end of frame T
    int32_t end;         // -1: the highest live cell, -2: the best live cell, p >= 0: that cell
    int32_t first_lo;    // self-steering band only: the low end of frame 0, in [0, L); else 0
};
static_assert(sizeof(ResumeRows) == 32, "descriptor sizes");
// ---- ... and its determined prefix (ka_ctc_best_path_determined): the walk of ka_determined.hpp reads
// ResumeRows::fin, which the engine then always sets (a row of its own where the caller wants none), and writes one int32 per
// lattice of the batch ----
constexpr int32_t kUndetermined = -1;   // the live cells trace back to more than one start cell, or no cell is live

}  // namespace ka
