"""Edges of the audio front end's dB stage that tests/test_frontend_gpu.py does not reach: segments whose levels are all
negative (the maximum of a segment then goes through the atomicMin branch of the kernel's float maximum) or all at the
1e-10 clamp, the shortest legal segment, many short segments in one launch.  MFCCs against oracle/frontend_oracle.py in
float64 with that file's tolerances: 1e-4 on speech-like material, 5e-4 where a segment holds digital silence."""
import numpy as np
import pytest

from oracle import frontend_oracle as F

pytestmark = pytest.mark.gpu


def _speechlike(n, seed, amp=0.3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    x = np.convolve(x, np.ones(8) / 8.0, mode="same") + 0.02 * rng.standard_normal(n)
    env = np.repeat(rng.uniform(0.05, 1.0, size=n // 2000 + 1), 2000)[:n]
    return (amp * x * env).astype(np.float32)


def _mel_db(y):
    """the levels F.mfcc floors and transforms, float64 [frames, 40]"""
    y = np.asarray(y, dtype=np.float64)
    yp = np.pad(y, (256, 256), mode="reflect")
    idx = np.arange(1 + len(y) // 256)[:, None] * 256 + np.arange(512)[None, :]
    power = np.abs(np.fft.rfft(yp[idx] * F.hann_periodic(512)[None, :], axis=1)) ** 2
    return 10.0 * np.log10(np.maximum(power @ F.mel_filterbank(257, 40, 22050), 1e-10))


def _compare(y, ends):
    """-> list of max |device - float64| per segment"""
    from kokoro_align_amd import preprocess as P
    got, idx = P.mfcc_segments(y, np.asarray(ends, dtype=np.int64))
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and np.isfinite(got).all()
    worst, k, a = [], 0, 0
    for e, stop in zip(list(ends), idx.tolist()):
        want = F.mfcc(y[a:e])
        assert stop - k == want.shape[0] == 1 + (e - a) // 256
        worst.append(float(np.abs(got[k:stop] - want).max()))
        k, a = stop, e
    return worst


def test_mfcc_of_a_quiet_segment_whose_levels_are_all_negative():
    y = np.concatenate([_speechlike(40000, 1), _speechlike(50000, 2, amp=1e-3), _speechlike(30011, 3)])
    ends = [40000, 90000, len(y)]
    assert _mel_db(y[40000:90000]).max() < 0.0 < _mel_db(y[:40000]).max()
    worst = _compare(y, ends)
    print("quiet segment between loud ones: max |device - float64| per segment =", worst)
    assert max(worst) < 1e-4
    # ... and alone in its call, and as the first and the last segment
    w2 = _compare(y[40000:90000], [50000]) + _compare(y[40000:], [50000, len(y) - 40000]) + _compare(y[:90000], [40000, 90000])
    print("quiet segment alone / first / last:", w2)
    assert max(w2) < 1e-4


def test_mfcc_of_a_segment_of_digital_silence_between_loud_ones():
    """every level of the middle segment sits at the 1e-10 clamp: -100 dB, its own maximum, nothing to floor"""
    y = np.concatenate([_speechlike(30000, 4), np.zeros(20000, np.float32), _speechlike(30000, 5)])
    ends = [30000, 50000, len(y)]
    assert np.all(_mel_db(y[30000:50000]) == -100.0)
    worst = _compare(y, ends)
    print("silent segment between loud ones: max |device - float64| per segment =", worst)
    assert worst[0] < 1e-4 and worst[2] < 1e-4 and worst[1] < 5e-4
    w2 = _compare(np.zeros(9000, np.float32), [3000, 9000])
    print("a recording of nothing but silence:", w2)
    assert max(w2) < 5e-4


def test_mfcc_of_the_shortest_legal_segment_and_of_many_short_ones():
    from kokoro_align_amd import preprocess as P
    y = _speechlike(257, 6)
    assert max(_compare(y, [257])) < 1e-4
    with pytest.raises(ValueError):
        P.mfcc_segments(y[:256], np.array([256]))
    rng = np.random.default_rng(7)
    lens = rng.integers(257, 700, size=400)
    lens[::7] = 257
    amp = np.repeat(np.where(rng.random(400) < 0.3, 1e-3, 1.0), lens)          # a third of them quiet: negative levels
    y = (_speechlike(int(lens.sum()), 8) * amp).astype(np.float32)
    worst = _compare(y, np.cumsum(lens).tolist())
    print("400 short segments: worst", max(worst))
    assert max(worst) < 1e-4


def test_power_to_db_segment_maximum_when_every_level_is_negative():
    """ka_power_to_db_f32 through the C ABI: segments that are all positive, mixed, all negative, all at the clamp, one row
    and empty, in one launch, padded rows; levels and the returned maxima against float64.  Bound: the levels are up to 100
    in magnitude, where a float32 ulp is 7.6e-6; log10f is good to 2 ulp and the product and the floor's subtraction round
    once each: 4 ulp = 3.1e-5."""
    import torch
    from kokoro_align_amd import _lib
    lib = _lib.load_library()
    rng = np.random.default_rng(9)
    cols, ld = 40, 44
    nrows = [300, 5, 257, 64, 1, 0, 33]
    foff = np.concatenate([[0], np.cumsum(nrows)]).astype(np.int64)
    x = np.full((int(foff[-1]), ld), np.nan, dtype=np.float32)
    gen = [lambda n: np.exp(rng.uniform(0.1, 12.0, (n, cols))),            # all above 0 dB
           lambda n: np.exp(rng.uniform(-12.0, 12.0, (n, cols))),          # mixed
           lambda n: np.exp(rng.uniform(-20.0, -0.1, (n, cols))),          # all negative
           lambda n: np.zeros((n, cols)),                                  # all at the clamp
           lambda n: np.exp(rng.uniform(-30.0, -25.0, (n, cols))),         # one row, negative, some below the clamp
           lambda n: np.zeros((n, cols)),
           lambda n: np.exp(rng.uniform(-9.0, -8.0, (n, cols)))]
    for s, g in enumerate(gen):
        x[foff[s]:foff[s + 1], :cols] = g(nrows[s])
    x[foff[2] + 7, 3] = 0.0                                                # far below the all-negative segment's floor
    d_x = torch.from_numpy(x).cuda()
    d_off = torch.from_numpy(foff).cuda()
    segmax = torch.full((len(nrows),), float("-inf"), dtype=torch.float32, device="cuda")
    assert lib.ka_power_to_db_f32(d_x.data_ptr(), ld, cols, d_off.data_ptr(), len(nrows), max(nrows), 80.0, segmax.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got, got_max = d_x.cpu().numpy(), segmax.cpu().numpy()
    assert np.isnan(got[:, cols:]).all()
    tol = 4 * 7.6e-6
    for s in range(len(nrows)):
        if nrows[s] == 0:
            assert np.isneginf(got_max[s])
            continue
        db = 10.0 * np.log10(np.maximum(x[foff[s]:foff[s + 1], :cols].astype(np.float64), 1e-10))
        want = np.maximum(db, db.max() - 80.0)
        print(f"segment {s}: maximum {got_max[s]} (float64 {db.max()}), worst level error {np.abs(got[foff[s]:foff[s + 1], :cols] - want).max():.3g}")
        assert abs(float(got_max[s]) - db.max()) <= tol
        assert np.abs(got[foff[s]:foff[s + 1], :cols] - want).max() <= tol
    assert got_max[2] < 0 and got_max[3] < 0 and got_max[4] < 0 and got_max[6] < 0
