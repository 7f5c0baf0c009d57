"""Float64 label occupancy of the band's paths that end at a terminal: the reference the occupancy kernels are tested against.

occ[t, v] = sum over s in [lo_t, hi_t) with lab'[s] = v of gamma_t(s), gamma from posterior_ref.forward_backward(..., full=True)
with the terminal as the path's last state.  Also a brute-force enumeration for tiny lattices and a
dense banded alpha recursion in torch whose autograd gradient of Z is the occupancy.
"""
import itertools

import numpy as np

import posterior_ref as R


def occupancy(log_probs, labels, terminal, beam_size=1000, max_move=4):
    """dict(status, occ float64 [T, V], ll, last_max, fb); occ NaN for a failed lattice; fb is the forward_backward(full=True)
    the occupancy was summed from, which posterior_ref.label_ratio takes."""
    lp = np.asarray(log_probs, dtype=np.float64)
    T, V = lp.shape
    lab = R.expand(labels)
    got = R.forward_backward(lp, labels, np.full(T, int(terminal), np.int64), beam_size, max_move, full=True)
    if got["status"] != R.OK:
        return dict(status=got["status"], occ=np.full((T, V), np.nan), ll=got["ll"], last_max=got["last_max"], fb=got)
    occ = np.zeros((T, V))
    for t, (lo, g) in enumerate(got["gamma"]):
        np.add.at(occ[t], lab[lo:lo + len(g)], g)
    return dict(status=R.OK, occ=occ, ll=got["ll"], last_max=got["last_max"], fb=got)


def brute_force(log_probs, labels, terminal, beam_size=1000, max_move=4):
    """(occ, ll) by enumerating every path of the band that ends at the terminal (tiny lattices only)."""
    lp = np.asarray(log_probs, dtype=np.float64)
    T, V = lp.shape
    lab = R.expand(labels)
    lo, hi = R.windows(T, len(lab), beam_size)
    total = 0.0
    occ = np.zeros((T, V))
    for moves in itertools.product(range(max_move), repeat=T):
        s, score, states, ok = 0, 0.0, [], True
        for t, j in enumerate(moves):
            s += j
            if not (lo[t] <= s < hi[t]) or (j >= 2 and j % 2 == 0 and lab[s] == 0):
                ok = False
                break
            score += lp[t, lab[s]]
            states.append(s)
        if not ok or states[-1] != terminal:
            continue
        p = np.exp(score)
        total += p
        occ[np.arange(T), lab[states]] += p
    with np.errstate(divide="ignore", invalid="ignore"):
        return occ / total, (np.log(total) if total > 0 else -np.inf)


def torch_z(lp, labels, terminal, beam_size=1000, max_move=4):
    """Z of a dense banded alpha recursion over all L states (torch float64, differentiable in ``lp``).  -inf is carried as
    -1e30 (exp of it minus any live score is exactly 0), so unreachable states give zero gradients rather than NaN."""
    import torch
    NEG = -1e30
    T, V = lp.shape
    lab = R.expand(labels)
    L = len(lab)
    lo, hi = R.windows(T, L, beam_size)
    idx = torch.as_tensor(lab)
    zero = torch.as_tensor(lab == 0)
    neg = torch.tensor(NEG, dtype=torch.float64)
    x = torch.clamp(lp, min=NEG)
    s = torch.arange(L)
    prev = torch.where(s == 0, torch.zeros((), dtype=torch.float64), neg)
    for t in range(T):
        cands = []
        for j in range(max_move):
            sh = torch.full((L,), NEG, dtype=torch.float64)
            if j < L:
                sh = torch.cat([sh[:j], prev[:L - j]])
            if j >= 2 and j % 2 == 0:
                sh = torch.where(zero, neg, sh)
            cands.append(sh)
        a = torch.logsumexp(torch.stack(cands), 0) + x[t, idx]
        prev = torch.where((s >= int(lo[t])) & (s < int(hi[t])), a, neg)
    return prev[int(terminal)]
