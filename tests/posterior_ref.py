"""Float64 NumPy forward-backward over the band of the best-path DP: the reference the posterior kernels are tested against.

Definition (include/kokoro_align_amd.h): lab'[2i] = 0, lab'[2i+1] = labels[i], L = 2S+1; window
[lo_t, hi_t) with lo_t = max(0, L t // T - beam // 2), hi_t = min(lo_t + beam, L); moves j in [0, max_move), a move with
j >= 2, j even, into a state whose label is 0 vetoed; virtual state 0 with score 0 before frame 0.
    alpha_t(s) = logsumexp_j alpha_{t-1}(s-j) + lp[t, lab'[s]]
    Z          = alpha_{T-1}(s*), s* = path[T-1]
    beta_t(s)  = logsumexp_j beta_{t+1}(s+j) + lp[t+1, lab'[s+j]],  beta_{T-1} = {s*: 0}
    post[t]    = exp(alpha_t(p_t) + beta_t(p_t) - Z)
Vectorised per frame; raw log domain (float64 holds ~1e5 to 1e-11).
"""
import itertools

import numpy as np

OK, BAD_ARGS, BAD_LABEL, NAN, NONFINITE, ZERO_MASS = 0, -2, -5, -6, -7, -9


def windows(T, L, beam):
    t = np.arange(T, dtype=np.int64)
    lo = np.maximum(0, (L * t) // T - beam // 2)
    hi = np.minimum(lo + beam, L)
    return lo, hi


def expand(labels):
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    lab = np.zeros(2 * len(labels) + 1, np.int64)
    lab[1::2] = labels
    return lab


def _lse(stack):
    m = np.max(stack, axis=0)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), safe + np.log(np.sum(np.exp(stack - safe), axis=0)), -np.inf)


def forward_backward(log_probs, labels, path, beam_size=1000, max_move=4, full=False):
    """Returns dict(status, post float64 [T], ll, gamma) - gamma (list of (lo, array over the window)) only with full=True."""
    lp = np.asarray(log_probs, dtype=np.float64)
    T, V = lp.shape
    lab = expand(labels)
    L = len(lab)
    path = np.asarray(path, dtype=np.int64).reshape(-1)
    nan = np.full(T, np.nan)
    if np.any((lab < 0) | (lab >= V)):
        return dict(status=BAD_LABEL, post=nan, ll=np.nan, gamma=None)
    if np.isnan(lp).any():
        return dict(status=NAN, post=nan, ll=np.nan, gamma=None)
    if np.isposinf(lp).any():
        return dict(status=NONFINITE, post=nan, ll=np.nan, gamma=None)
    if len(path) != T or np.any((path < 0) | (path >= L)):
        return dict(status=BAD_ARGS, post=nan, ll=np.nan, gamma=None)
    lo, hi = windows(T, L, beam_size)
    zero = lab == 0
    alpha_at = np.full(T, -np.inf)
    alphas = []
    plo, prev = 0, np.zeros(1)
    for t in range(T):
        s = np.arange(lo[t], hi[t])
        cands = []
        for j in range(max_move):
            u = s - j
            ok = (u >= plo) & (u < plo + len(prev))
            if j >= 2 and j % 2 == 0:
                ok &= ~zero[s]
            c = np.full(len(s), -np.inf)
            c[ok] = prev[u[ok] - plo]
            cands.append(c)
        a = (_lse(np.array(cands)) if len(s) else np.zeros(0)) + lp[t, lab[s]]
        if lo[t] <= path[t] < hi[t]:
            alpha_at[t] = a[path[t] - lo[t]]
        if full:
            alphas.append(a)
        plo, prev = lo[t], a
    ll = alpha_at[T - 1]
    last_max = float(np.max(prev)) if len(prev) else -np.inf     # the last frame's best cell
    if ll == -np.inf:
        return dict(status=ZERO_MASS, post=nan, ll=-np.inf, gamma=None, last_max=last_max)
    post = np.zeros(T)
    post[T - 1] = 1.0
    sstar = path[T - 1]
    nxt = np.where(np.arange(lo[T - 1], hi[T - 1]) == sstar, 0.0, -np.inf)   # beta over window T-1
    gamma = [None] * T
    if full:
        gamma[T - 1] = (lo[T - 1], np.exp(alphas[T - 1] + nxt - ll))
    for t in range(T - 2, -1, -1):
        s = np.arange(lo[t], hi[t])
        nlo, nhi = lo[t + 1], hi[t + 1]
        g = nxt + lp[t + 1, lab[nlo:nhi]]
        cands = []
        for j in range(max_move):
            u = s + j
            ok = (u >= nlo) & (u < nhi)
            if j >= 2 and j % 2 == 0:
                ok &= ~zero[np.minimum(u, L - 1)]
            c = np.full(len(s), -np.inf)
            c[ok] = g[u[ok] - nlo]
            cands.append(c)
        b = _lse(np.array(cands)) if len(s) else np.zeros(0)
        if lo[t] <= path[t] < hi[t]:
            post[t] = np.exp(alpha_at[t] + b[path[t] - lo[t]] - ll)
        if full:
            gamma[t] = (lo[t], np.exp(alphas[t] + b - ll))
        nxt = b
    return dict(status=OK, post=post, ll=float(ll), gamma=gamma if full else None, last_max=last_max)


def brute_force(log_probs, labels, path, beam_size=1000, max_move=4):
    """(post, ll) by enumerating every path of the band (tiny lattices only)."""
    lp = np.asarray(log_probs, dtype=np.float64)
    T, V = lp.shape
    lab = expand(labels)
    L = len(lab)
    lo, hi = windows(T, L, beam_size)
    path = np.asarray(path, dtype=np.int64)
    total = 0.0
    on_path = np.zeros(T)
    for moves in itertools.product(range(max_move), repeat=T):
        s, score, states, ok = 0, 0.0, [], True
        for t, j in enumerate(moves):
            s += j
            if not (lo[t] <= s < hi[t]) or (j >= 2 and j % 2 == 0 and lab[s] == 0):
                ok = False
                break
            score += lp[t, lab[s]]
            states.append(s)
        if not ok or states[-1] != path[T - 1]:
            continue
        p = np.exp(score)
        total += p
        on_path += p * (np.array(states) == path)
    with np.errstate(divide="ignore", invalid="ignore"):
        return on_path / total, (np.log(total) if total > 0 else -np.inf)
