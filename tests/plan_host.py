"""The batch plan on the host, in plain numpy: what every device plan builder (njode_plan.h,
njode_planner.hip, njode_gen.hip) has to produce for a batch ``(B, K, time_ptr, obs_idx, k_jump)``.

The plan is integer data and a function of the batch and the schedule alone, so it is stated here
once and compared exactly (tests/test_hip_plan_arrays.py); tests/test_plan_host.py holds this file
to a per-path Python loop.  Conventions of include/njode_hip.h: the rows are sorted by time, then
path; ``time_ptr`` are the CSR offsets of the time slices; within a slice a path has at most one
row; ``k_jump[i]`` Euler steps are complete when slice ``i`` jumps.
"""
import numpy as np


def excl_cumsum(x):
    x = np.asarray(x, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(x)[:-1]]) if len(x) else x


def plan(B, K, time_ptr, obs_idx, k_jump):
    """Every array of the plan, as a dict of int64 arrays."""
    time_ptr = np.asarray(time_ptr, dtype=np.int64)
    obs_idx = np.asarray(obs_idx, dtype=np.int64)
    k_jump = np.asarray(k_jump, dtype=np.int64)
    nt, n = len(k_jump), int(time_ptr[-1])
    assert len(time_ptr) == nt + 1 and len(obs_idx) == n
    rows = np.arange(n)
    t_of_row = np.repeat(np.arange(nt), np.diff(time_ptr))
    # the (path, time) sort: the rows are in time order, so a stable sort by path is all it takes
    row_by_path = np.argsort(obs_idx, kind='stable')
    path_sorted = obs_idx[row_by_path]
    starts = np.ones(n, dtype=bool)
    starts[1:] = path_sorted[1:] != path_sorted[:-1]
    ends = np.ones(n, dtype=bool)
    ends[:-1] = starts[1:]
    prev = np.full(n, -1, dtype=np.int64)
    nxt = np.full(n, -1, dtype=np.int64)
    if n:
        prev[row_by_path[~starts]] = row_by_path[np.flatnonzero(~starts) - 1]
        nxt[row_by_path[~ends]] = row_by_path[np.flatnonzero(~ends) + 1]
    first_j = np.full(B, -1, dtype=np.int64)
    first_row = np.full(B, -1, dtype=np.int64)
    last_row = np.full(B, -1, dtype=np.int64)
    first_j[path_sorted[starts]] = np.flatnonzero(starts)
    first_row[path_sorted[starts]] = row_by_path[starts]
    last_row[path_sorted[ends]] = row_by_path[ends]
    kend = k_jump[t_of_row]
    kbeg = np.where(prev >= 0, kend[np.maximum(prev, 0)], 0)
    length = kend - kbeg
    order = np.argsort(-length, kind='stable')      # descending length, equal lengths in row order
    len_hist = np.bincount(length, minlength=K + 1)[:K + 1]
    cnt = n - np.cumsum(len_hist)                   # cnt_s = #{len > s}, s = 0 .. K
    tail_key = np.where(last_row >= 0, np.clip(kend[np.maximum(last_row, 0)] if n else 0, 0, K), 0)
    n_tiles = (n + 15) // 16
    tile_len = length[order[::16]]                  # a tile's first item is its longest
    assert len(tile_len) == n_tiles
    return dict(
        n=n, t_of_row=t_of_row, row_by_path=row_by_path, path_sorted=path_sorted, first_j=first_j,
        first_row=first_row, last_row=last_row, item_prev=prev, item_next=nxt, item_kbeg=kbeg, item_len=length,
        order=order, len_hist=len_hist, cnt=cnt, base_s=excl_cumsum(cnt), base16_s=excl_cumsum((cnt + 15) & ~15),
        tail_key=tail_key, jlo=np.searchsorted(k_jump, np.arange(K + 2), side='left'),
        tile_len=tile_len, tile_base=np.concatenate([excl_cumsum(tile_len), [tile_len.sum()]]), rows=rows)


class SplitCost:
    """The split-point cost of k_traj_layout's comment (njode_planner.hip), in float64.

    The tiles of 16 items are sorted by length; the T longest go to ``ns`` four-wave blocks, a
    tile-step ``r`` times faster than the ``nw`` single-wave workers do the rest:

        cost(T) = max( max(L_0, H(T) / ns) / r ,  max(L_T, (S - H(T)) / nw) )

    with L_t the length of tile t, H its prefix sum and S = H(n_tiles).  A side without tiles
    (T = 0: the four-wave side, T = n_tiles: the workers) costs nothing, a side with tiles and no
    blocks is infinite.  ``v``: 0 backward, 1 forward kernel."""

    def __init__(self, tile_len, ns, nw, r):
        self.L = np.asarray(tile_len, dtype=np.float64)
        self.n_tiles = len(self.L)
        self.H = np.concatenate([[0.0], np.cumsum(self.L)])
        self.ns, self.nw, self.r = list(ns), list(nw), [float(x) for x in r]

    def cost(self, T, v):
        cs = cw = 0.0
        if T > 0:
            cs = max(self.L[0], self.H[T] / self.ns[v]) / self.r[v] if self.ns[v] > 0 else np.inf
        if T < self.n_tiles:
            cw = max(self.L[T], (self.H[-1] - self.H[T]) / self.nw[v]) if self.nw[v] > 0 else np.inf
        return max(cs, cw)

    def costs(self, v):
        return np.array([self.cost(T, v) for T in range(self.n_tiles + 1)])


# ---- the yardstick's yardstick: one path at a time, no numpy ----------------------------------------
def plan_loops(B, K, time_ptr, obs_idx, k_jump):
    """The same plan by brute force (lists and loops; tests/test_plan_host.py)."""
    nt, n = len(k_jump), int(time_ptr[-1])
    t_of_row = [0] * n
    for i in range(nt):
        for r in range(int(time_ptr[i]), int(time_ptr[i + 1])):
            t_of_row[r] = i
    rows_of = [[r for r in range(n) if int(obs_idx[r]) == b] for b in range(B)]     # in time order
    prev, nxt, kbeg, length = [-1] * n, [-1] * n, [0] * n, [0] * n
    first_row, last_row, first_j, tail_key = [-1] * B, [-1] * B, [-1] * B, [0] * B
    path_sorted, row_by_path = [], []
    for b in range(B):
        k = 0
        if rows_of[b]:
            first_j[b] = len(path_sorted)
            first_row[b], last_row[b] = rows_of[b][0], rows_of[b][-1]
        for q, r in enumerate(rows_of[b]):
            path_sorted.append(b)
            row_by_path.append(r)
            prev[r] = rows_of[b][q - 1] if q else -1
            nxt[r] = rows_of[b][q + 1] if q + 1 < len(rows_of[b]) else -1
            kbeg[r] = k
            length[r] = int(k_jump[t_of_row[r]]) - k
            k = int(k_jump[t_of_row[r]])
        tail_key[b] = min(max(k, 0), K)
    order = []
    for s in range(K, -1, -1):
        order += [r for r in range(n) if length[r] == s]
    len_hist = [sum(1 for r in range(n) if length[r] == s) for s in range(K + 1)]
    cnt = [sum(1 for r in range(n) if length[r] > s) for s in range(K + 1)]
    base_s = [sum(cnt[:s]) for s in range(K + 1)]
    base16_s = [sum((c + 15) // 16 * 16 for c in cnt[:s]) for s in range(K + 1)]
    jlo = [next((i for i in range(nt) if int(k_jump[i]) >= k), nt) for k in range(K + 2)]
    tile_len = [max(length[r] for r in order[t:t + 16]) for t in range(0, n, 16)]
    tile_base = [sum(tile_len[:t]) for t in range(len(tile_len) + 1)]
    return dict(n=n, t_of_row=t_of_row, row_by_path=row_by_path, path_sorted=path_sorted, first_j=first_j,
                first_row=first_row, last_row=last_row, item_prev=prev, item_next=nxt, item_kbeg=kbeg,
                item_len=length, order=order, len_hist=len_hist, cnt=cnt, base_s=base_s, base16_s=base16_s,
                tail_key=tail_key, jlo=jlo, tile_len=tile_len, tile_base=tile_base)


def random_case(rng, B_max=9, nt_max=7, K_max=12):
    """A tiny random batch: empty slices, paths without rows, repeated k_jump values, a jump at
    step 0; the schedule ends at its last observation."""
    B, nt = int(rng.randint(1, B_max + 1)), int(rng.randint(1, nt_max + 1))
    K = int(rng.randint(1, K_max + 1))
    k_jump = np.sort(rng.randint(0, K + 1, size=nt))
    k_jump[-1] = K
    obs, counts = [], []
    for i in range(nt):
        m = int(rng.randint(0, B + 1)) if rng.rand() < 0.8 else 0
        paths = np.sort(rng.choice(B, size=m, replace=False))
        obs += paths.tolist()
        counts.append(m)
    if not obs:
        obs, counts[-1] = [int(rng.randint(B))], 1
    return B, K, np.concatenate([[0], np.cumsum(counts)]), np.array(obs), k_jump
