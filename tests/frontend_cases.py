"""Inputs of tests/test_frontend_stages_gpu.py and tests/test_frontend_long_gpu.py, NumPy only: the GPU tests run them on the
device, tests/test_frontend_cpu.py proves on the host that they are large enough to tell every fault of frontend_ref apart."""
import json
import os
from types import SimpleNamespace

import numpy as np

import frontend_ref as R
from test_frontend_edges_gpu import _speechlike


def record(call, worst, bound, **more):
    """Prints one measured figure (the worst error of a call, in the unit of its bound) and, with KA_ACCURACY_OUT=<file>,
    appends it to that file as a JSON line like fb_harness.record (the source of profiles/frontend_accuracy.json); then holds
    it against the bound.  The figure is out before the assertion, so a run that fails still measures."""
    rec = dict(test=os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], call=call, worst=float(worst), bound=bound, **more)
    print(json.dumps(rec))
    path = os.environ.get("KA_ACCURACY_OUT")
    if path:
        with open(path, "at") as f:
            f.write(json.dumps(rec) + "\n")
    assert worst <= bound, rec


def _lay_out(rng, lens, order, gaps, first_row, row_gaps, n_fft, hop, ld):
    """segments of the given lengths in a waveform, in ``order``, NaN before, between and after them (gaps[i] samples before
    the i-th placed); frame rows from first_row on with row_gaps[s] rows nobody owns after segment s"""
    seg_start = np.zeros(len(lens), dtype=np.int64)
    at = 0
    for g, s in zip(gaps, order):
        seg_start[s] = at + g
        at += g + lens[s]
    y = np.full(at + gaps[-1], np.nan, dtype=np.float32)
    for s, n in enumerate(lens):
        y[seg_start[s]:seg_start[s] + n] = 0.3 * rng.standard_normal(n, dtype=np.float32)
    counts = 1 + np.asarray(lens, dtype=np.int64) // hop
    frame_off = first_row + np.concatenate([[0], np.cumsum(counts + np.asarray(row_gaps))[:-1]])
    rows = int(frame_off[-1] + counts[-1] + row_gaps[-1])
    return SimpleNamespace(y=y, seg_start=seg_start, seg_len=np.asarray(lens, dtype=np.int64), frame_off=frame_off.astype(np.int64),
                           n_fft=n_fft, hop=hop, ld=ld, rows=rows, max_frames=int(counts.max()),
                           window=R.hann(n_fft).astype(np.float32))


def stft_main():
    """n_fft 512, hop 256, rows 520 apart.  257: the shortest legal segment; 768: a multiple of hop, the last frame centres on
    the end and its whole right half is reflected; 4097 * 256 samples: 4098 frames, two of them past the 4096 blocks."""
    return _lay_out(np.random.default_rng(31), [257, 511, 512, 513, 768, 4097 * 256], order=[3, 5, 0, 4, 1, 2],
                    gaps=[7, 300, 1, 64, 513, 19, 5], first_row=3, row_gaps=[1, 2, 1, 3, 1, 2], n_fft=512, hop=256, ld=520)


def stft_small():
    """n_fft 64, hop 16, rows 64 apart (no padding): 33 is the shortest legal segment"""
    return _lay_out(np.random.default_rng(32), [33, 64, 1000], order=[2, 0, 1], gaps=[3, 40, 1, 9], first_row=2, row_gaps=[2, 1, 1],
                    n_fft=64, hop=16, ld=64)


def power_input(n, nf=257, ld_in=520):
    """float32 [n, ld_in]: N(0, 1) scaled by exp(U(-20, 20)) in the 2 * nf columns of the transform, NaN in the padding"""
    rng = np.random.default_rng(41 + n)
    x = np.full((n, ld_in), np.nan, dtype=np.float32)
    x[:, :2 * nf] = rng.standard_normal((n, 2 * nf), dtype=np.float32) * np.exp(rng.uniform(-20.0, 20.0, (n, 2 * nf)).astype(np.float32))
    return x


def db_input():
    """The launch of test_power_to_db_segment_maximum_when_every_level_is_negative (test_frontend_edges_gpu.py) with one more
    segment of 1700 rows: its maximum (50 dB) in row 1690, in row 1695 a cell 90 dB below it; the other cells within +-13 dB.
    Two rows nobody owns before the first segment and after the last, sentinels there and in the padding columns."""
    rng = np.random.default_rng(9)
    cols, ld = 40, 44
    nrows = [300, 5, 257, 64, 1, 0, 33, 1700]
    frame_off = (2 + np.concatenate([[0], np.cumsum(nrows)])).astype(np.int64)
    x = R.sentinels((int(frame_off[-1]) + 2, ld))
    gen = [lambda n: np.exp(rng.uniform(0.1, 12.0, (n, cols))),            # all above 0 dB
           lambda n: np.exp(rng.uniform(-12.0, 12.0, (n, cols))),          # mixed
           lambda n: np.exp(rng.uniform(-20.0, -0.1, (n, cols))),          # all negative
           lambda n: np.zeros((n, cols)),                                  # all at the clamp
           lambda n: np.exp(rng.uniform(-30.0, -25.0, (n, cols))),         # one row, negative, some below the clamp
           lambda n: np.zeros((n, cols)),
           lambda n: np.exp(rng.uniform(-9.0, -8.0, (n, cols))),
           lambda n: np.exp(rng.uniform(-3.0, 3.0, (n, cols)))]
    for s, g in enumerate(gen):
        x[frame_off[s]:frame_off[s + 1], :cols] = g(nrows[s])
    x[frame_off[2] + 7, 3] = 0.0                                           # far below the all-negative segment's floor
    x[frame_off[7] + 1690, 17] = 1e5
    x[frame_off[7] + 1695, 5] = 1e-4
    return SimpleNamespace(x=x, frame_off=frame_off, cols=cols, ld=ld, nrows=nrows, max_frames=max(nrows))


def recording():
    """13.5 minutes: 70000 * 256 samples of speech-like material cut into segments of 3 to 15 s (86 segments, 70042 frames;
    the last one is what the others leave, 5.9 s)"""
    n = 70000 * 256
    rng = np.random.default_rng(2)
    ends, at = [], 0
    while True:
        at += int(rng.integers(3 * 22050, 15 * 22050))
        if at >= n:
            break
        ends.append(at)
    ends.append(n)
    return _speechlike(n, 12), np.asarray(ends, dtype=np.int64)


# _SLAB_ROWS, _SLAB_SEGMENTS of the runs over the recording.  A: as shipped, one slab, the power kernel takes a second pass.
# B: 13 slabs, every one closed by the segment limit (seven segments are 9044 rows at the most).  C: every segment exceeds
# the row limit and sits alone.  D: 13 slabs, 9 closed by the row limit and 3 by the segment limit.
RECORDING_RUNS = {"A": (R.SLAB_ROWS, R.SLAB_SEGMENTS), "B": (30000, 7), "C": (100, R.SLAB_SEGMENTS), "D": (6000, 7)}


def quiet_between_loud():
    """test_mfcc_of_a_quiet_segment_whose_levels_are_all_negative's recording: the middle segment 60 dB below its neighbours.
    Cut into one slab per segment, the quiet one's maximum shares its slot with a loud one's."""
    y = np.concatenate([_speechlike(40000, 1), _speechlike(50000, 2, amp=1e-3), _speechlike(30011, 3)])
    return y, np.asarray([40000, 90000, len(y)], dtype=np.int64)


def short_segments():
    """65537 segments of 257 samples, a third of them scaled by 1e-3"""
    nseg, seg_len = 65537, 257
    y = (_speechlike(nseg * seg_len, 8) * np.repeat(np.where(short_segments_quiet(), 1e-3, 1.0), seg_len)).astype(np.float32)
    return y, nseg, seg_len


def short_segments_quiet():
    """bool [65537]: the segments of short_segments() that are scaled by 1e-3"""
    return np.random.default_rng(7).random(65537) < 0.3
