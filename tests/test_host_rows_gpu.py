"""Host rows handed over as they lie: a [:, :V] view of a wider buffer gives every ``_batch`` call the bits its contiguous copy
gives.  The other columns of the buffer hold NaN: a kernel that read them would answer KA_ERR_NAN.  The staging code (one 2-D
copy with the row pitch) is the same for the fast and the generic kernel form, so one shape is enough."""
import numpy as np
import pytest

import band_cases as C

pytestmark = pytest.mark.gpu

T, S, V, LD, BEAM, MM = 70, 40, 39, 111, 24, 4
L = 2 * S + 1


def bits(x):
    """a result (arrays, floats, lists and tuples of them) as nested tuples of bytes"""
    if isinstance(x, (list, tuple)):
        return tuple(bits(y) for y in x)
    return np.asarray(x).dtype.str, np.asarray(x).shape, np.asarray(x).tobytes()


@pytest.fixture(scope="module")
def rows():
    import torch
    assert torch.cuda.is_available()
    lp, labels = C.random_lattice(7040, T, S, V)
    buf = np.full((T, LD), np.nan, np.float32)
    buf[:, :V] = lp
    view = buf[:, :V]
    assert view.strides == (4 * LD, 4) and lp.flags.c_contiguous and np.isnan(buf[:, V:]).all()
    return view, lp, labels


CALLS = dict(
    best_path=lambda ka, lp, labels: ka.ctc_best_path_batch([lp], [labels], BEAM, MM, return_status=True),
    label_posteriors=lambda ka, lp, labels: ka.ctc_label_posteriors_batch([lp], [labels], [L - 1], BEAM, MM, return_status=True),
    label_posteriors_banded=lambda ka, lp, labels: ka.ctc_label_posteriors_batch([lp], [labels], [L - 1], BEAM, MM, return_status=True,
                                                                                 band_lo=[ka.diagonal_band(T, L, BEAM)]),
    mea_path=lambda ka, lp, labels: ka.ctc_mea_path_batch([lp], [labels], [L - 1], BEAM, MM, return_status=True))


@pytest.mark.parametrize("call", CALLS)
def test_a_wide_view_gives_the_bits_of_its_copy(rows, call):
    import kokoro_align_amd as ka
    view, lp, labels = rows
    got = CALLS[call](ka, view, labels)
    want = CALLS[call](ka, lp, labels)
    assert list(got[1]) == [0] and list(want[1]) == [0], (got[1], want[1])      # statuses
    assert bits(got) == bits(want)                                              # outputs, log-likelihood or totals, statuses
