"""References of the audio front end's stages (kokoro_align_amd/preprocess.py, csrc/ka_frontend.hpp) in plain NumPy, and the
same stages with one deliberate fault each.  Nothing here imports the product or the oracle.

The references say what a stage must write: ``stft_frames`` in float32 (one multiply, one rounding: the kernel has to match
it bit for bit), the others in float64.  A cell that no segment owns holds the NaN-payload sentinel (float32) or NaN
(float64).

A faulted variant (``fault=...``) models a kernel, an entry point or the slab loop of ``mfcc_segments`` that is wrong in one
specific way; a cell a faulted kernel never writes keeps the sentinel / NaN.  tests/test_frontend_cpu.py holds every GPU
case's reference against every fault that applies to it: if the two did not differ, by more than the case's tolerance, the
case would be too small to see that fault on the device.

  first_pass_only              a kernel without its stride loop: rows (stft) or cells (power, dB) past the first pass of the
                               grid are never written; ``grid`` = rows or cells of one pass, as the entry point sizes it
  reflect_right_off_by_one     2*len-1-i in place of 2*(len-1)-i past the end of a segment
  ld_is_n_fft                  frame rows written n_fft apart whatever ``ld`` says
  frame_off_ignored            frame rows of the segments written densely from row 0
  segmax_first_pass_only       every level converted, the segment maximum taken over the first pass only
  slab_offset_zero             every slab of mfcc_segments writes from row 0 of ``out``
  segmax_shared_across_slabs   slot j of the segment maxima is not reset between slabs
"""
import numpy as np

SENTINEL = 0x7FC0BEEF           # tests/test_lstm_kernels_gpu.py's NAN_FILL: a quiet NaN with a payload
STFT_GRID_ROWS = 4096           # ka_entry_misc.hip: min(max_frames, 4096) blocks of one frame row each
POWER_GRID_CELLS = 65536 * 256  # ka_misc.hip launch_power: at most 65536 blocks of 256 cells
DB_GRID_CELLS = 256 * 256       # ka_entry_misc.hip: min(ceil(max_frames * cols / 256), 256) blocks of 256 cells per segment
SLAB_ROWS = 1 << 21
SLAB_SEGMENTS = 65535


def stft_grid(max_frames):
    """frame rows one pass of stft_frames_kernel covers per segment, as ka_stft_frames_f32 sizes its grid"""
    return min(int(max_frames), STFT_GRID_ROWS)


def db_grid(max_frames, cols):
    """cells one pass of power_to_db_kernel / db_floor_kernel covers per segment, as ka_power_to_db_f32 sizes its grid"""
    return min(-(-int(max_frames) * cols // 256) * 256, DB_GRID_CELLS)


def sentinels(shape):
    """float32 array of the given shape, every cell the sentinel"""
    return np.full(shape, SENTINEL, dtype=np.uint32).view(np.float32)


def is_sentinel(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) == SENTINEL


# ----------------------------------------------------------------------------------------
# constants of the transform, float64
# ----------------------------------------------------------------------------------------
def hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def mel_filters(n_freqs=257, n_mels=40, sample_rate=22050):
    """[n_freqs, n_mels]: triangles on the HTK mel scale over 0 .. sample_rate//2, peak 1"""
    top = sample_rate // 2
    freqs = np.linspace(0, top, n_freqs)
    edges = 700.0 * (10.0 ** (np.linspace(0.0, 2595.0 * np.log10(1.0 + top / 700.0), n_mels + 2) / 2595.0) - 1.0)
    fb = np.zeros((n_freqs, n_mels))
    for m in range(n_mels):
        lo, mid, hi = edges[m], edges[m + 1], edges[m + 2]
        fb[:, m] = np.maximum(0.0, np.minimum((freqs - lo) / (mid - lo), (hi - freqs) / (hi - mid)))
    return fb


def dct2_ortho(n_mfcc=40, n_mels=40):
    """[n_mels, n_mfcc]: orthonormal DCT-II"""
    n = np.arange(n_mels)[:, None]
    k = np.arange(n_mfcc)[None, :]
    d = np.cos(np.pi / n_mels * (n + 0.5) * k) * np.sqrt(2.0 / n_mels)
    d[:, 0] *= np.sqrt(0.5)
    return d


# ----------------------------------------------------------------------------------------
# ka_stft_frames_f32
# ----------------------------------------------------------------------------------------
def stft_owned(seg_len, frame_off, n_fft, hop, rows, ld):
    """bool [rows, ld]: the cells some segment owns (1 + len // hop rows of n_fft cells from its frame_off)"""
    own = np.zeros((rows, ld), dtype=bool)
    for n, f0 in zip(seg_len, frame_off):
        own[int(f0):int(f0) + 1 + int(n) // hop, :n_fft] = True
    return own


def stft_frames(y32, seg_start, seg_len, frame_off, n_fft, hop, window32, rows, ld, fault=None, grid=STFT_GRID_ROWS, dtype=np.float32):
    """float32 [rows, ld]: row frame_off[s] + f holds window32[k] * y32[seg_start[s] + reflect(f * hop - n_fft // 2 + k)] for
    f < 1 + seg_len[s] // hop, the product taken in float32; every other cell holds the sentinel.  (``dtype=np.float64``: the
    same cells with the product in float64 and NaN elsewhere, for the comparison with the float64 transform.)"""
    y = np.asarray(y32, dtype=dtype)
    w = np.asarray(window32, dtype=dtype)
    out = sentinels(rows * ld) if dtype == np.float32 else np.full(rows * ld, np.nan, dtype=dtype)
    row_stride = n_fft if fault == "ld_is_n_fft" else ld
    counts = 1 + np.asarray(seg_len, dtype=np.int64) // hop
    first_rows = np.concatenate([[0], np.cumsum(counts)[:-1]]) if fault == "frame_off_ignored" else np.asarray(frame_off, dtype=np.int64)
    half = n_fft // 2
    k = np.arange(n_fft, dtype=np.int64)[None, :]
    for start, n, f0, nfr in zip(seg_start, seg_len, first_rows, counts):
        start, n, f0 = int(start), int(n), int(f0)
        f = np.arange(min(int(nfr), grid) if fault == "first_pass_only" else int(nfr), dtype=np.int64)[:, None]
        i = np.abs(f * hop - half + k)
        mirror = 2 * n - 1 if fault == "reflect_right_off_by_one" else 2 * (n - 1)
        i = np.where(i >= n, mirror - i, i)
        out[(f0 + f) * row_stride + k] = w[None, :] * y[start + i]
    return out.reshape(rows, ld)


# ----------------------------------------------------------------------------------------
# ka_power_f32, ka_power_to_db_f32
# ----------------------------------------------------------------------------------------
def power(reim32, nf, fault=None, grid=POWER_GRID_CELLS):
    """float64 [n, nf] = re^2 + im^2 of rows stored (nf real parts | nf imaginary parts | padding)"""
    r = np.asarray(reim32)
    re, im = r[:, :nf].astype(np.float64), r[:, nf:2 * nf].astype(np.float64)
    out = re * re + im * im
    if fault == "first_pass_only":
        out.reshape(-1)[grid:] = np.nan
    return out


def power_to_db(x, frame_off, top_db=80.0, fault=None, grid=DB_GRID_CELLS, return_max=False):
    """float64, per segment s = rows frame_off[s] .. frame_off[s + 1] of x [rows, cols]: 10 log10(max(x, 1e-10)), floored at
    the segment's own maximum - top_db.  Rows outside every segment come back NaN.  With return_max also the maxima [nseg]
    (-inf for a segment without rows)."""
    x = np.asarray(x)
    out = np.full(x.shape, np.nan, dtype=np.float64)
    maxima = np.full(len(frame_off) - 1, -np.inf)
    for s in range(len(frame_off) - 1):
        a, b = int(frame_off[s]), int(frame_off[s + 1])
        if a == b:
            continue
        raw = x[a:b].astype(np.float64).reshape(-1)
        db = 10.0 * np.log10(np.maximum(raw, 1e-10))
        if fault == "first_pass_only":
            maxima[s] = db[:grid].max()
            lev = raw.copy()                                         # past the first pass: still the power that came in
            lev[:grid] = np.maximum(db[:grid], maxima[s] - top_db)
        else:
            maxima[s] = db[:grid].max() if fault == "segmax_first_pass_only" else db.max()
            lev = np.maximum(db, maxima[s] - top_db)
        out[a:b] = lev.reshape(b - a, -1)
    return (out, maxima) if return_max else out


# ----------------------------------------------------------------------------------------
# mfcc_segments
# ----------------------------------------------------------------------------------------
def slabs(frame_off, slab_rows=SLAB_ROWS, slab_segments=SLAB_SEGMENTS):
    """How mfcc_segments cuts a recording: whole segments, in order; a slab takes segments while it stays within slab_rows
    frame rows and slab_segments segments, and always at least one.  -> [(first segment, one past the last, what closed it:
    "rows" | "segments" | "end")]"""
    nseg = len(frame_off) - 1
    cut, s0 = [], 0
    while s0 < nseg:
        s1, why = s0 + 1, "end"
        while s1 < nseg:
            if frame_off[s1 + 1] - frame_off[s0] > slab_rows:
                why = "rows"
                break
            if s1 - s0 >= slab_segments:
                why = "segments"
                break
            s1 += 1
        cut.append((s0, s1, why))
        s0 = s1
    return cut


def _mel_power_of_padded(padded, n_frames, n_fft, hop, sample_rate, n_mels):
    """padded [nseg, len + n_fft] float64 -> [nseg * n_frames, n_mels]"""
    idx = np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :]
    spec = np.fft.rfft(padded[:, idx] * hann(n_fft), axis=-1)
    p = spec.real ** 2 + spec.imag ** 2
    return p.reshape(-1, p.shape[-1]) @ mel_filters(n_fft // 2 + 1, n_mels, sample_rate)


def mel_power_segments(y, ends, n_fft=512, hop=256, sample_rate=22050, n_mels=40):
    """float64 [frames, n_mels] of the segments y[0:ends[0]], y[ends[0]:ends[1]], ... one after the other, and their
    frame_off [nseg + 1]"""
    y = np.asarray(y, dtype=np.float64)
    parts, a = [], 0
    for e in ends:
        seg = np.pad(y[a:e], n_fft // 2, mode="reflect")[None, :]
        parts.append(_mel_power_of_padded(seg, 1 + (e - a) // hop, n_fft, hop, sample_rate, n_mels))
        a = e
    return np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])])


def mel_power_equal_segments(y, nseg, seg_len, n_fft=512, hop=256, sample_rate=22050, n_mels=40, chunk=4096):
    """the same of nseg segments of seg_len samples each, 4096 segments per transform call"""
    segs = np.asarray(y[:nseg * seg_len]).reshape(nseg, seg_len)
    n_frames = 1 + seg_len // hop
    parts = []
    for c in range(0, nseg, chunk):
        padded = np.pad(segs[c:c + chunk].astype(np.float64), ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
        parts.append(_mel_power_of_padded(padded, n_frames, n_fft, hop, sample_rate, n_mels))
    return np.concatenate(parts), np.arange(nseg + 1) * n_frames


def floor_margin(mel, frame_off, top_db=80.0):
    """min over the segments of (lowest level) - (highest level - top_db): how far every level stays above its floor, dB"""
    db = 10.0 * np.log10(np.maximum(mel, 1e-10))
    lo = np.minimum.reduceat(db.min(axis=1), frame_off[:-1])
    hi = np.maximum.reduceat(db.max(axis=1), frame_off[:-1])
    return float((lo - (hi - top_db)).min())


def mfcc_from_mel(mel, frame_off, top_db=80.0, n_mfcc=40, fault=None, slab_rows=SLAB_ROWS, slab_segments=SLAB_SEGMENTS,
                  grid=POWER_GRID_CELLS, nf=257):
    """float64 [frames, n_mfcc]: dB per segment with its own floor, then the DCT, slab by slab as mfcc_segments goes.  Every
    segment has at least one frame.  A row a faulted variant never writes, or computes from power cells it never wrote, is
    NaN (of a row that straddles the end of the power kernel's first pass only the cells past it are lost, and the filters
    give the last of them no weight: such a row counts as written)."""
    frame_off = np.asarray(frame_off, dtype=np.int64)
    dct = dct2_ortho(n_mfcc, mel.shape[1])
    out = np.full((len(mel), n_mfcc), np.nan)
    shared = np.full(min(slab_segments, len(frame_off) - 1), -np.inf)
    for s0, s1, _ in slabs(frame_off, slab_rows, slab_segments):
        r0, r1 = int(frame_off[s0]), int(frame_off[s1])
        db = 10.0 * np.log10(np.maximum(mel[r0:r1], 1e-10))
        if fault == "first_pass_only":
            db[-(-grid // nf):] = np.nan
        rel = frame_off[s0:s1] - r0
        with np.errstate(invalid="ignore"):
            top = np.fmax.reduceat(np.fmax.reduce(db, axis=1), rel)
        if fault == "segmax_shared_across_slabs":
            top = shared[:s1 - s0] = np.maximum(shared[:s1 - s0], top)
        db = np.maximum(db, np.repeat(top, np.diff(frame_off[s0:s1 + 1]))[:, None] - top_db)
        if fault == "slab_offset_zero":
            out[0:r1 - r0] = db @ dct
        else:
            out[r0:r1] = db @ dct
    return out


def mfcc_segments(y, ends, **kw):
    """float64 MFCC [frames, 40] of the segments between the given ends, and the cumulative frame counts"""
    mel, frame_off = mel_power_segments(y, ends)
    return mfcc_from_mel(mel, frame_off, **kw), frame_off[1:]


def mfcc_equal_segments(y, nseg, seg_len, **kw):
    """float64 MFCC [nseg * (1 + seg_len // 256), 40] of nseg segments of seg_len samples each"""
    mel, frame_off = mel_power_equal_segments(y, nseg, seg_len)
    return mfcc_from_mel(mel, frame_off, **kw)
