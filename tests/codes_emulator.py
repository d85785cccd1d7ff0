"""Numpy restatements of the two code ops (include/aewavenet.h: aew_code_lookup_t, aew_code_runs_t).  Both ops move
bytes and count: the device results must equal these bit for bit."""
import numpy as np


def lookup(emb, ind, d_pitch=None):
    """(zq fp32 [Q][d_pitch], bad): zq[q][:d] = emb[ind[q]], pad channels zero; an index outside [0, K) is not followed -
    a zero row, counted in bad."""
    emb, ind = np.asarray(emb, np.float32), np.asarray(ind, np.int64).reshape(-1)
    K, d = emb.shape
    d_pitch = d if d_pitch is None else d_pitch
    zq = np.zeros((ind.size, d_pitch), np.float32)
    ok = (ind >= 0) & (ind < K)
    zq[ok, :d] = emb[ind[ok]]
    return zq, int((~ok).sum())


def code_runs(ind):
    """ind int64 [B][N] -> (units int64 [B][N], lengths int32 [B][N], n_runs int32 [B]): position t starts a run iff t == 0
    or ind[b][t] != ind[b][t - 1]; -1 / 0 behind the last run."""
    ind = np.asarray(ind, np.int64)
    B, N = ind.shape
    units = np.full((B, N), -1, np.int64)
    lengths = np.zeros((B, N), np.int32)
    n_runs = np.zeros(B, np.int32)
    for b in range(B):
        start = np.ones(N, bool)
        start[1:] = ind[b, 1:] != ind[b, :-1]
        pos = np.flatnonzero(start)
        n = pos.size
        units[b, :n] = ind[b, pos]
        lengths[b, :n] = np.diff(np.append(pos, N))
        n_runs[b] = n
    return units, lengths, n_runs


def boundary_rows(N, chunk=1024, wave=64):
    """Rows of N codes that stress the kernel's seams, as an int64 [5][N] array:
    0  a run straddles every wave and chunk boundary (the code changes 3 positions behind each multiple of `wave`)
    1  a run starts exactly at each multiple of `wave` (and so of `chunk`)
    2  all equal (1 run)            3  all distinct (N runs)
    4  random short runs."""
    t = np.arange(N)
    rs = np.random.RandomState(N)
    rows = [(t + wave - 3) // wave, t // wave + 1000, np.full(N, 7), 5 * t + 1,
            np.repeat(rs.randint(0, 50, N), rs.randint(1, 6, N))[:N]]
    assert chunk % wave == 0
    return np.stack(rows).astype(np.int64)
