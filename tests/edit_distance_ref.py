"""A numpy restatement of the edit-distance rule of include/loco_asr.h ("error rates"), written from the definition and not from
the kernel; the checker of tests/test_edit_distance_ref.py and tests/test_gpu_edit_distance.py, never the product.

A cell is the pair (cost, S) compared lexicographically,
    D[i][0] = (i, 0)    D[0][j] = (j, 0)
    D[i][j] = min(D[i-1][j-1] + (a[i-1] == b[j-1] ? (0,0) : (1,1)),  D[i-1][j] + (1,0),  D[i][j-1] + (1,0)),
here packed as cost << 32 | S in one int64 (one integer min is the lexicographic min) and swept one anti-diagonal i + j = d at a
time: the three neighbours of a cell lie on the two diagonals before it, so a whole diagonal is one vector expression.
"""
import numpy as np

K = 1 << 32  # one unit of cost in a packed key


def edit_key(a, b) -> int:
    """(cost << 32 | S) of D[n][m] for the reference ``a`` and the hypothesis ``b``."""
    a, b = np.asarray(a, dtype=np.int64).ravel(), np.asarray(b, dtype=np.int64).ravel()
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return max(n, m) * K
    # diagonals indexed by the row i; only the entries max(0, d - m) .. min(n, d) of diagonal d mean anything
    prev2, prev1, cur = (np.zeros(n + 1, dtype=np.int64) for _ in range(3))
    prev1[0] = prev1[1] = K  # d = 1: D[0][1] and D[1][0]; prev2 is d = 0: D[0][0] = 0
    for d in range(2, n + m + 1):
        lo, hi = max(1, d - m), min(n, d - 1)  # the rows of the interior cells (i >= 1, j = d - i >= 1)
        i = np.arange(lo, hi + 1)
        sub = prev2[lo - 1:hi] + np.where(a[lo - 1:hi] == b[d - i - 1], 0, K + 1)
        dele = prev1[lo - 1:hi] + K
        ins = prev1[lo:hi + 1] + K
        cur[lo:hi + 1] = np.minimum(sub, np.minimum(dele, ins))
        if d <= m:
            cur[0] = d * K
        if d <= n:
            cur[d] = d * K
        prev2, prev1, cur = prev1, cur, prev2
    return int(prev1[n])


def edit_counts(a, b):
    """(S, D, I, hits): D - I = n - m and D + I = cost - S; hits = n - S - D."""
    n, m = len(a), len(b)
    key = edit_key(a, b)
    cost, S = key >> 32, key & (K - 1)
    D, I = (cost - S + n - m) // 2, (cost - S - n + m) // 2
    return S, D, I, n - S - D


def edit_cost(a, b) -> int:
    return edit_key(a, b) >> 32


def nbest_pairs(N):
    """The pairs (i < j) of an N-best list in row-major order: the order of a group's rows in the kernel's ``counts``."""
    return [(i, j) for i in range(N) for j in range(i + 1, N)]


def nbest_risk(hyps, weights=None):
    """(risk list, best index) of one n-best list.  risk[h] = (sum over h' != h, ascending, of w[h'] * cost(h, h')) / (sum over h',
    ascending, of w[h']), in double: every product and every sum is one rounded Python float operation, in that order.  best = the
    first index of least risk."""
    N = len(hyps)
    w = [1.0] * N if weights is None else [float(x) for x in weights]
    cost = {}
    for i, j in nbest_pairs(N):
        cost[i, j] = cost[j, i] = float(edit_cost(hyps[i], hyps[j]))
    den = 0.0
    for j in range(N):
        den = den + w[j]
    risk = []
    for h in range(N):
        num = 0.0
        for j in range(N):
            if j != h:
                num = num + w[j] * cost[h, j]
        risk.append(num / den)
    best = min(range(N), key=lambda h: (risk[h], h))
    return risk, best
