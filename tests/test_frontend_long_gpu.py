"""mfcc_segments on inputs as long as the ones it was built for: a 13.5-minute recording (70042 frames: power_kernel takes a
second pass) cut into slabs in four ways, and 65537 segments in one call (two slabs with the shipped constants, the first a
launch at gridDim.y = 65535).  Against the float64 references of tests/frontend_ref.py, which tests/test_frontend_cpu.py ties
to oracle/frontend_oracle.py, within the project's 1e-4 for speech-like material (tests/test_frontend_gpu.py; measured worst
2.3e-5): that bound rests on no level lying near its segment's max - 80 dB floor, so every test asserts on its reference
that the lowest level of every segment stays 18 dB above it.  tests/test_frontend_cpu.py shows which faults each input tells
apart.  The runs need not be bit-equal to each other: the library GEMM may choose differently by shape."""
from types import SimpleNamespace

import numpy as np
import pytest

import frontend_cases as C
import frontend_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _reference(y, mel, frame_off):
    import torch
    assert torch.cuda.is_available(), "the GPU tests need a device"
    return SimpleNamespace(y=torch.from_numpy(y).cuda(), frame_off=frame_off, margin=R.floor_margin(mel, frame_off),
                           want=R.mfcc_from_mel(mel, frame_off))


@pytest.fixture(scope="module")
def recording():
    y, ends = C.recording()
    ref = _reference(y, *R.mel_power_segments(y, ends))
    ref.ends = ends
    return ref


def _worst_per_segment(ref, ends):
    """mfcc_segments against the reference: max |device - float64| of every segment"""
    from kokoro_align_amd import preprocess as P
    assert ref.margin >= 18.0
    got, indices = P.mfcc_segments(ref.y, ends)
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref.want.shape
    assert indices.dtype == np.int64 and np.array_equal(indices, ref.frame_off[1:])
    err = np.abs(got - ref.want)
    err[np.isnan(err)] = np.inf                                             # a row never written
    return np.maximum.reduceat(err.max(axis=1), ref.frame_off[:-1])


def _check(ref, ends, call):
    """the worst of them printed and recorded, then held"""
    C.record(call, _worst_per_segment(ref, ends).max(), TOL)


@pytest.mark.parametrize("run", sorted(C.RECORDING_RUNS))
def test_mfcc_of_a_long_recording_slab_by_slab(recording, monkeypatch, run):
    """86 segments of 3 to 15 s, 70042 frames.  A: as shipped, one slab of 18 000 794 power cells, 1 223 578 of them in the
    kernel's second pass.  B: slabs of seven segments.  C: one segment per slab, each over the row limit.  D: slabs closed by
    the row limit and slabs closed by the segment limit."""
    from kokoro_align_amd import preprocess as P
    assert (P._SLAB_ROWS, P._SLAB_SEGMENTS) == C.RECORDING_RUNS["A"]
    assert len(recording.ends) == 86 and recording.frame_off[-1] == 70042
    rows, segments = C.RECORDING_RUNS[run]
    monkeypatch.setattr(P, "_SLAB_ROWS", rows)
    monkeypatch.setattr(P, "_SLAB_SEGMENTS", segments)
    _check(recording, recording.ends, f"mfcc_segments[recording, run {run}: slabs of {rows} rows, {segments} segments]")


@pytest.fixture(scope="module")
def short():
    """one call of mfcc_segments with the shipped constants: 65535 segments, then 2"""
    from kokoro_align_amd import preprocess as P
    assert (P._SLAB_ROWS, P._SLAB_SEGMENTS) == C.RECORDING_RUNS["A"]
    y, nseg, seg_len = C.short_segments()
    ref = _reference(y, *R.mel_power_equal_segments(y, nseg, seg_len))
    return _worst_per_segment(ref, np.arange(1, nseg + 1, dtype=np.int64) * seg_len), np.abs(ref.want[:, 0]).reshape(nseg, -1).max(axis=1)


@pytest.mark.parametrize("which", ["loud", "quiet"])
def test_mfcc_of_65537_short_segments(short, which):
    """257 samples each (131074 frames), a third of them scaled by 1e-3; every segment within 1e-4, the loud ones and the quiet
    ones (the last two segments, the second slab, are loud) held apart because they err for different reasons.  The zeroth
    coefficient of a quiet segment is 0.158 * the sum of 40 levels near -70 dB: 370 in the median, up to 515, where one
    float32 ulp is 3.1e-5 to 6.1e-5.  With the DCT as a float32 product this test found the 19 705 quiet ones at 1.66e-4,
    355 of them over 1e-4 (on the host, a float32 DCT of the exact levels: 1.49e-4); mfcc_segments now takes that one
    product in float64 and rounds once.  MI355X: loud worst 5.5e-5, quiet worst 4.7e-5."""
    worst, c0 = short
    quiet = C.short_segments_quiet()
    mine = quiet if which == "quiet" else ~quiet
    assert not quiet[-2:].any()
    C.record(f"mfcc_segments[65537 segments of 257 samples, the {which} ones]", worst[mine].max(), TOL,
             segments=int(mine.sum()), segments_over_bound=int((worst[mine] > TOL).sum()), largest_c0=float(c0[mine].max()))


def test_mfcc_of_a_quiet_segment_in_a_slab_after_a_loud_one(monkeypatch):
    """One segment per slab, the second 60 dB below the first: floored against a maximum left over from the slab before, most
    of it would come out flat.  Neither input above can show that: their maxima lie too close together."""
    from kokoro_align_amd import preprocess as P
    y, ends = C.quiet_between_loud()
    ref = _reference(y, *R.mel_power_segments(y, ends))
    monkeypatch.setattr(P, "_SLAB_SEGMENTS", 1)
    _check(ref, ends, "mfcc_segments[quiet segment after a loud one, one segment per slab]")
