"""Audio front end, CPU side: the oracle's restatement of the reference's silence
splitting against the goldens made by the reference itself (tests/golden/make_golden.py g6), and consistency
checks of the MFCC restatement (which has no reference output to be pinned to: torchaudio is not in the image)."""
import functools

import numpy as np
import pytest

import frontend_cases as C
import frontend_ref as R
from golden_util import g6
from oracle import frontend_oracle as F


def test_silent_ranges_match_the_reference():
    for c in g6()["silent_ranges"]:
        v = np.array([ch == "1" for ch in c["mask"]])
        if "raises" in c:
            with pytest.raises(Exception):
                F.silent_ranges(v)
        else:
            assert F.silent_ranges(v).tolist() == c["ranges"], c["mask"]


def test_split_points_match_the_reference():
    g = g6()
    par = g["parameters"]
    assert par == F.split_parameters(g["sample_rate"], 512)
    for c in g["cases"]:
        x = F.hash_waveform(c["n"], c["seed"], c["pieces"])
        if c["status"] == 1:
            with pytest.raises(ValueError, match="cannot be split"):
                F.split_points(x, **par)
            continue
        got = F.split_points(x, **par)
        assert [int(v) for v in got] == c["split_points"], c["name"]


def test_mfcc_restatement_is_self_consistent():
    """Independent formulations of the pieces: the DCT matrix is orthonormal, a pure tone lands in the mel filter
    that contains it, scaling the input by 10 moves every un-clamped mel level by 20 dB, the frame count follows
    center=True framing, and the top_db floor holds."""
    d = F.dct_matrix(40, 40)
    assert np.allclose(d.T @ d, np.eye(40), atol=1e-12)
    fb = F.mel_filterbank(257, 40, 22050)
    assert fb.shape == (257, 40) and (fb >= 0).all() and fb.max() <= 1.0 + 1e-12
    sr, n = 22050, 22050
    t = np.arange(n) / sr
    tone = 0.5 * np.sin(2 * np.pi * 1000.0 * t)
    m = F.mfcc(tone)
    assert m.shape == (1 + n // 256, 40)
    db = m @ F.dct_matrix(40, 40).T                       # back to mel dB (orthonormal DCT)
    k = int(np.argmax(db[40]))
    centre = np.argmax(fb[:, k]) * (sr // 2) / 256.0
    assert abs(centre - 1000.0) < 150.0
    assert db.min() >= db.max() - 80.0 - 1e-9
    rng = np.random.default_rng(0)
    y = rng.standard_normal(5000) * 0.1
    a = F.mfcc(y) @ F.dct_matrix(40, 40).T
    b = F.mfcc(10.0 * y) @ F.dct_matrix(40, 40).T
    assert np.allclose(b - a, 20.0, atol=1e-9)            # nothing near the floor for white noise


def test_product_merge_of_short_pieces_is_the_reference_order():
    """kokoro_align_amd.preprocess replaces the reference's quadratic merge loop (preprocess.py:81-95) by a heap over a
    linked list; the removals must be the same, ties included (host logic: no GPU needed)."""
    import importlib
    P = importlib.import_module("kokoro_align_amd.preprocess")

    def loop(points, num_frames, m):          # the loop as oracle/frontend_oracle.py restates it
        points = np.asarray(points)
        while len(points):
            dist = np.append(points, num_frames) - np.insert(points, 0, 0)
            i = np.argmin(dist)
            if dist[i] > m:
                break
            if i == 0:
                points = np.delete(points, i)
            elif i == len(points):
                points = np.delete(points, len(points) - 1)
            elif dist[i - 1] < dist[i + 1]:
                points = np.delete(points, i - 1)
            else:
                points = np.delete(points, i)
        return points

    rng = np.random.default_rng(8)
    for _ in range(1500):
        k = int(rng.integers(0, 60))
        n = int(rng.integers(k + 1, 500))
        pts = np.sort(rng.choice(np.arange(1, n), size=min(k, n - 1), replace=False)) if k else np.array([], dtype=np.int64)
        m = float(rng.uniform(0, 80))
        assert list(loop(pts, n, m)) == list(P._merge_short_pieces(pts, n, m))


# ----------------------------------------------------------------------------------------
# tests/frontend_ref.py: the references of the GPU stage tests agree with what the suite already trusts, the product's
# constants agree with independent formulations, and every GPU case is large enough to tell every fault apart
# ----------------------------------------------------------------------------------------
def test_reference_frames_then_the_float64_transform_reproduce_the_oracle_mfcc():
    """R.stft_frames (reflection, frame rows at frame_off, rows ld apart) followed by rfft, mel, dB and DCT in float64 is
    F.mfcc to 1e-9, on three segments of one waveform laid out with gaps.  That bound is below what a float32 product allows
    (one rounding of 2^-24 per sample moves a level by some 1e-6 dB; the figure is printed), so it is held by the float64
    form of the same function, and the float32 form - the one the kernel is compared with - is held to be that float64
    product rounded once, bit for bit: a float32 times a float32 is exact in float64."""
    y = C._speechlike(60000, 3)
    seg_start, seg_len = np.array([0, 30000, 30300]), np.array([30000, 300, 29700])
    counts = 1 + seg_len // 256
    frame_off = np.array([3, 3 + counts[0] + 2, 3 + counts[0] + 2 + counts[1] + 1])
    rows, ld = int(frame_off[2] + counts[2] + 1), 520
    args = (seg_start, seg_len, frame_off, 512, 256)
    f64 = R.stft_frames(y, *args, F.hann_periodic(512), rows, ld, dtype=np.float64)
    owned = R.stft_owned(seg_len, frame_off, 512, 256, rows, ld)
    assert np.array_equal(np.isnan(f64), ~owned)

    def mfcc_of(frames):
        power = np.abs(np.fft.rfft(frames[:, :512], axis=1)) ** 2
        db = 10.0 * np.log10(np.maximum(power @ F.mel_filterbank(257, 40, 22050), 1e-10))
        return np.maximum(db, db.max() - 80.0) @ F.dct_matrix(40, 40)

    w32 = F.hann_periodic(512).astype(np.float32)
    f32 = R.stft_frames(y, *args, w32, rows, ld)
    assert f32.dtype == np.float32 and np.array_equal(R.is_sentinel(f32), ~owned)
    once = R.stft_frames(y, *args, w32.astype(np.float64), rows, ld, dtype=np.float64).astype(np.float32)
    assert np.array_equal(f32.view(np.uint32)[owned], once.view(np.uint32)[owned])
    for s in range(3):
        want = F.mfcc(y[seg_start[s]:seg_start[s] + seg_len[s]])
        a, b = frame_off[s], frame_off[s] + counts[s]
        print(f"segment {s}: float64 frames {np.abs(mfcc_of(f64[a:b]) - want).max():.3g}, float32 frames "
              f"{np.abs(mfcc_of(f32[a:b].astype(np.float64)) - want).max():.3g}")
        assert np.abs(mfcc_of(f64[a:b]) - want).max() <= 1e-9


@functools.lru_cache(maxsize=None)
def _short():
    y, nseg, seg_len = C.short_segments()
    mel, frame_off = R.mel_power_equal_segments(y, nseg, seg_len)
    return y, nseg, seg_len, mel, frame_off, R.mfcc_from_mel(mel, frame_off)


@functools.lru_cache(maxsize=None)
def _recording():
    y, ends = C.recording()
    mel, frame_off = R.mel_power_segments(y, ends)
    return y, ends, mel, frame_off, R.mfcc_from_mel(mel, frame_off)


def test_reference_mfcc_of_equal_segments_is_the_oracle_mfcc_segment_by_segment():
    y, nseg, seg_len, _, _, want = _short()
    assert nseg == 65537 and want.shape == (2 * nseg, 40)
    assert np.abs(want[:16] - R.mfcc_equal_segments(y, 8, seg_len)).max() <= 1e-12
    for s in (0, 65534, 65535, 65536):
        assert np.abs(want[2 * s:2 * s + 2] - F.mfcc(y[s * seg_len:(s + 1) * seg_len])).max() <= 1e-12
    y, ends, _, frame_off, want = _recording()
    assert len(ends) == 86 and frame_off[-1] == 70042
    for s in (0, 41, 85):
        assert np.abs(want[frame_off[s]:frame_off[s + 1]] - F.mfcc(y[(ends[s - 1] if s else 0):ends[s]])).max() <= 1e-12


def test_product_constants_against_independent_formulations():
    """host only: the DFT basis against NumPy's transform, window, mel filters and DCT against the oracle's bit for bit"""
    import importlib
    P = importlib.import_module("kokoro_align_amd.preprocess")
    frames = np.random.default_rng(5).standard_normal((50, 512))
    spec = np.fft.rfft(frames, axis=1)
    assert np.abs(frames @ P._dft_basis(512) - np.concatenate([spec.real, spec.imag], axis=1)).max() <= 1e-9
    assert np.array_equal(P._hann_periodic(512), F.hann_periodic(512))
    assert np.array_equal(P._mel_filterbank(257, 40, 22050), F.mel_filterbank(257, 40, 22050))
    assert np.array_equal(P._dct_ortho(40, 40), F.dct_matrix(40, 40))
    assert (P._SLAB_ROWS, P._SLAB_SEGMENTS) == (R.SLAB_ROWS, R.SLAB_SEGMENTS) == C.RECORDING_RUNS["A"]


def _told_apart(want, faulted, owned=None, tol=None):
    """does the faulted output differ from the reference in a cell a segment owns - in its bits (tol None) or by more than
    tol (a cell the fault left unwritten, NaN, differs)"""
    differs = want.view(np.uint32) != faulted.view(np.uint32) if tol is None else ~(np.abs(faulted - want) <= tol)
    return bool((differs if owned is None else differs & owned).any())


STFT_FAULTS = ("first_pass_only", "reflect_right_off_by_one", "ld_is_n_fft", "frame_off_ignored")


@pytest.mark.parametrize("max_frames", ["true", 1])
def test_stft_case_tells_every_fault_apart(max_frames):
    c = C.stft_main()
    assert c.max_frames == 4098 and c.frame_off[0] == 3 and c.ld > c.n_fft
    grid = R.stft_grid(c.max_frames if max_frames == "true" else max_frames)
    assert grid == (4096 if max_frames == "true" else 1)
    args = (c.y, c.seg_start, c.seg_len, c.frame_off, c.n_fft, c.hop, c.window, c.rows, c.ld)
    want = R.stft_frames(*args)
    owned = R.stft_owned(c.seg_len, c.frame_off, c.n_fft, c.hop, c.rows, c.ld)
    assert owned.any(axis=1).sum() < c.rows and np.array_equal(R.is_sentinel(want), ~owned)      # rows nobody owns; no NaN read
    prod = np.abs(want[owned])
    assert prod[prod > 0].min() >= 2.0 ** -126                                                    # no subnormal product
    for fault in STFT_FAULTS:
        assert _told_apart(want, R.stft_frames(*args, fault=fault, grid=grid), owned), fault


def test_small_stft_case_tells_the_faults_that_apply_apart():
    """n_fft 64, hop 16, rows 64 apart, 63 frames at the most: one pass and no padding, so the two faults about those are
    not faults here"""
    c = C.stft_small()
    assert (c.n_fft, c.hop, c.ld, c.max_frames) == (64, 16, 64, 63) and c.seg_len.min() == c.n_fft // 2 + 1
    args = (c.y, c.seg_start, c.seg_len, c.frame_off, c.n_fft, c.hop, c.window, c.rows, c.ld)
    want = R.stft_frames(*args)
    owned = R.stft_owned(c.seg_len, c.frame_off, c.n_fft, c.hop, c.rows, c.ld)
    assert np.array_equal(R.is_sentinel(want), ~owned)
    for fault in ("reflect_right_off_by_one", "frame_off_ignored"):
        assert _told_apart(want, R.stft_frames(*args, fault=fault, grid=R.stft_grid(c.max_frames)), owned), fault
    for fault in ("first_pass_only", "ld_is_n_fft"):
        assert not _told_apart(want, R.stft_frames(*args, fault=fault, grid=R.stft_grid(c.max_frames)))


def test_power_case_tells_a_missing_second_pass_apart():
    n, nf = 65290, 257
    x = C.power_input(n)
    want = R.power(x, nf)
    assert want.shape == (n, nf) and n * nf - R.POWER_GRID_CELLS == 2314
    assert want.min() >= 2.0 ** -100 and want.max() < 2.0 ** 120 and np.isnan(x[:, 2 * nf:]).all()
    assert _told_apart(want, R.power(x, nf, fault="first_pass_only"), tol=3 * 2.0 ** -24 * want)
    small = C.power_input(3)
    assert not _told_apart(R.power(small, nf), R.power(small, nf, fault="first_pass_only"), tol=0.0)


@pytest.mark.parametrize("max_frames", ["true", 1])
def test_db_case_tells_every_fault_apart(max_frames):
    c = C.db_input()
    grid = R.db_grid(c.max_frames if max_frames == "true" else max_frames, c.cols)
    assert grid == (65536 if max_frames == "true" else 256)
    x = c.x[:, :c.cols]
    want, top = R.power_to_db(x, c.frame_off, return_max=True)
    s, tol = 7, 4 * 2.0 ** -17
    a = c.frame_off[s]
    assert 1690 * c.cols >= 65536 and np.argmax(want[a:c.frame_off[s + 1]].max(axis=1)) == 1690
    assert want[a + 1695, 5] == top[s] - 80.0 and 10.0 * np.log10(x[a + 1695, 5]) == pytest.approx(top[s] - 90.0)
    for fault in ("first_pass_only", "segmax_first_pass_only"):
        got, gtop = R.power_to_db(x, c.frame_off, fault=fault, grid=grid, return_max=True)
        assert _told_apart(want, got, ~np.isnan(want), tol), fault
        assert abs(gtop[s] - top[s]) > tol, fault


@pytest.mark.parametrize("run", sorted(C.RECORDING_RUNS))
def test_recording_tells_the_faults_of_its_run_apart(run):
    _, _, mel, frame_off, want = _recording()
    rows, segments = C.RECORDING_RUNS[run]
    assert R.floor_margin(mel, frame_off) >= 18.0
    closed = [why for _, _, why in R.slabs(frame_off, rows, segments)]
    faults = {"A": ("first_pass_only",), "B": ("slab_offset_zero",), "C": ("slab_offset_zero",), "D": ("slab_offset_zero",)}[run]
    assert {"A": closed == ["end"], "B": len(closed) == 13 and set(closed[:-1]) == {"segments"},
            "C": len(closed) == 86 and set(closed[:-1]) == {"rows"}, "D": set(closed[:-1]) == {"rows", "segments"}}[run], closed
    for fault in faults:
        assert _told_apart(want, R.mfcc_from_mel(mel, frame_off, fault=fault, slab_rows=rows, slab_segments=segments), tol=1e-4), fault


def test_short_segments_tell_their_faults_apart():
    _, nseg, _, mel, frame_off, want = _short()
    assert R.floor_margin(mel, frame_off) >= 18.0
    assert [(s1 - s0, why) for s0, s1, why in R.slabs(frame_off)] == [(65535, "segments"), (2, "end")]
    for fault in ("first_pass_only", "slab_offset_zero"):
        assert _told_apart(want, R.mfcc_from_mel(mel, frame_off, fault=fault), tol=1e-4), fault


def test_a_quiet_segment_in_a_later_slab_tells_a_shared_maximum_apart():
    """In the recording every segment's maximum lies within a few dB of the others', and the two segments of the second slab
    of the 65537 are loud like the two whose slots they would share: neither input can show a maximum that survives from
    one slab into the next.  This one can: a segment 60 dB below the one before it, one segment per slab."""
    for (mel, frame_off, want), rows in ((_recording()[2:], 100), (_short()[3:], R.SLAB_ROWS)):
        assert not _told_apart(want, R.mfcc_from_mel(mel, frame_off, fault="segmax_shared_across_slabs", slab_rows=rows), tol=1e-4)
    y, ends = C.quiet_between_loud()
    mel, frame_off = R.mel_power_segments(y, ends)
    want = R.mfcc_from_mel(mel, frame_off)
    assert R.floor_margin(mel, frame_off) >= 18.0 and np.array_equal(want, R.mfcc_from_mel(mel, frame_off, slab_segments=1))
    for fault in ("segmax_shared_across_slabs", "slab_offset_zero"):
        assert _told_apart(want, R.mfcc_from_mel(mel, frame_off, fault=fault, slab_segments=1), tol=1e-4), fault
