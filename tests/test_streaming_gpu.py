"""StreamingAligner on the GPU: the self-steering band fed in chunks of 64 frames, committing frames as
soon as ka_ctc_best_path_tracking_determined says they are final.  T = 512, S = 60, beam 48, period 8; one case ends in a ragged
chunk.  The commits concatenated are the uncut ctc_best_path_tracking call's, bit for bit, after every push a prefix of it; a
peaked input commits long before its last push; a chunk costs at most two forward passes.
"""
import sys

import numpy as np
import pytest

import resume_ref as RR
import track_cases as TC
from oracle import oracle as O

pytestmark = pytest.mark.gpu

T_FULL, S, BEAM, PERIOD, CHUNK = 512, 60, 48, 8, 64


def peaked_with_a_pause(T):
    """a planted path that climbs a position every third frame and waits for 100 frames in the middle"""
    t = np.arange(T)
    read = np.where(t < 200, t, np.where(t < 300, 200, t - 100))
    true = np.minimum(read // 3, 2 * S)
    return TC.planted(91, T, S, true)


def hashed(T):
    return O.hash_logprobs(T, 39, 92), O.hash_labels(S, 39, 92)


INPUTS = {"peaked": peaked_with_a_pause, "hash": hashed}
_uncut = {}


@pytest.fixture(scope="module")
def ka():
    import torch
    assert torch.cuda.is_available()
    import kokoro_align_amd as ka
    assert hasattr(ka, "StreamingAligner") and hasattr(ka, "ctc_best_path_tracking_determined")
    return ka


def uncut(ka, kind, T, end):
    key = (kind, T, end)
    if key not in _uncut:
        lp, lab = INPUTS[kind](T)
        _uncut[key] = ka.ctc_best_path_tracking(lp, lab, BEAM, 4, PERIOD, end)
    return _uncut[key]


def stream(ka, kind, T, end, tensor=False):
    """push the input in chunks; returns (the commits of every push and of finish, the aligner)"""
    lp, lab = INPUTS[kind](T)
    if tensor:
        import torch
        lp = torch.from_numpy(lp).cuda()
    al = ka.StreamingAligner(lab, BEAM, 4, PERIOD, end)
    commits = [al.push(lp[a:a + CHUNK]) for a in range(0, T, CHUNK)]
    commits.append(al.finish())
    return commits, al


def host(a):
    return np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a)


@pytest.mark.parametrize("kind,T,end", [("peaked", 512, "highest"), ("hash", 512, "highest"), ("peaked", 500, "highest"), ("hash", 500, "best"),
                                        ("peaked", 512, "best")])
def test_commits_are_the_uncut_call_and_never_change(ka, kind, T, end):
    want = uncut(ka, kind, T, end)
    commits, al = stream(ka, kind, T, end)
    assert all(len(c) == 4 for c in commits)
    done = 0
    for c in commits:   # after every push the commits so far are a prefix of the uncut call's answer: no frame is ever taken back
        n = c[0].shape[0]
        assert all(x.shape[0] == n for x in c)
        assert all(RR.same_bits(x, w[done:done + n]) and x.dtype == w.dtype for x, w in zip(c, want)), (kind, T, end, done)
        done += n
    assert done == T == al.frames_committed == al.frames_pushed
    if kind == "peaked":   # committed while it was fed: something is final before the last push
        assert any(c[0].shape[0] for c in commits[:-2])


def test_device_tensors_stay_on_the_device(ka):
    want = uncut(ka, "peaked", 512, "highest")
    commits, _ = stream(ka, "peaked", 512, "highest", tensor=True)
    assert all(x.is_cuda for c in commits for x in c)
    import torch
    got = [torch.cat([c[i] for c in commits]) for i in range(4)]
    assert all(RR.same_bits(host(g), w) for g, w in zip(got, want))


@pytest.mark.parametrize("kind", ["peaked", "hash"])
def test_at_most_two_forward_passes_per_chunk(ka, kind, monkeypatch):
    mod = sys.modules["kokoro_align_amd.align"]
    first, second = [], []
    run_det, run_resume = mod.ctc_best_path_tracking_determined, mod.ctc_best_path_resume

    def det(lp, *a, **k):
        first.append(id(lp))
        return run_det(lp, *a, **k)

    def resume(lp, *a, **k):
        second.append(id(lp))
        return run_resume(lp, *a, **k)
    monkeypatch.setattr(mod, "ctc_best_path_tracking_determined", det)
    monkeypatch.setattr(mod, "ctc_best_path_resume", resume)
    lp, lab = INPUTS[kind](T_FULL)
    chunks = [lp[a:a + CHUNK] for a in range(0, T_FULL, CHUNK)]
    al = ka.StreamingAligner(lab, BEAM, 4, PERIOD)
    for c in chunks:
        al.push(c)
    al.finish()
    ids = [id(c) for c in chunks]
    assert first == ids                                              # one pass with the walk per chunk, in order
    assert set(second) <= set(ids) and all(second.count(i) <= 1 for i in ids)   # and at most one pass that closes it
    assert ids[-1] not in second                                     # (the last chunk is closed by its own first pass)


def test_chunk_lengths(ka):
    lp, lab = INPUTS["hash"](100)
    al = ka.StreamingAligner(lab, BEAM, 4, PERIOD)
    al.push(lp[:64])
    al.push(lp[64:100])          # ragged: must be the last
    with pytest.raises(ValueError):
        al.push(lp[:64])
    out = al.finish()
    assert al.frames_committed == al.frames_pushed == 100 and out[0].shape[0] <= 100
    with pytest.raises(ValueError):
        al.finish()
    with pytest.raises(ValueError):
        ka.StreamingAligner(lab, BEAM, 4, 6)
    with pytest.raises(ValueError):
        ka.StreamingAligner(lab, BEAM, 4, PERIOD, end=3)
