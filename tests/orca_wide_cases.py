"""Batches and the numpy restatement of the selection for the robot's ORCA solve on more than 32 observation rows
(tests/test_robot_orca_wide_cpu.py asserts what the batches cover, on the oracle alone; tests/test_robot_orca_wide_gpu.py
holds orca_robot_wide_kernel to the oracle on the same batches).

The oracle takes at most 64 rows.  Above that the yardstick is the REDUCTION PROPERTY: RVO2 keeps the max_neighbors
nearest rows in range (Agent::insertAgentNeighbor: float32 distSq, strict <, ties in row order), so the solve of an env
equals, bit for bit, the solve of the env that holds only those rows, in their original order (humans before static
rows).  select() is that rule in numpy, reduced_batch() the env of the selected rows; the CPU test checks the property on
the oracle wherever the oracle can take the full batch."""
import numpy as np

from helpers import _blank_batch, orca_branch_batch, orca_case_params

TILE = 32  # rows per lane group: orca_robot_kernel's limit, and the stride of a lane's rows in the wide kernel
SAFETIES = (0.0, 0.15)
# (humans, static rows) checked against the oracle on the full batch (<= 64 rows) ...
ORACLE_CASES = [(32, 1), (1, 32), (14, 30), (33, 31), (3, 61)]
# ... and through the reduction (65 .. 128 rows; (33, 32) is the first shape past the oracle, (33, 95) and (1, 127) fill
# the handle)
REDUCED_CASES = [(33, 32), (20, 76), (33, 94), (33, 95), (1, 127)]
PARAM_SETS = ("default", "mn3-nd2")
# "all" once: it moves the handle's safety space (the humans') off the robot's, and the time step and the horizon
ORACLE_RUNS = [(c, ps) for c in ORACLE_CASES for ps in PARAM_SETS] + [((14, 30), "all")]
TIES_ROWS = (40, 100)

_batches = {}


def _force_rows(b, e, n, ns):
    """Env e keeps its first n humans and ns static rows (unused slots cleared, as _clear_unused leaves them)."""
    b.n_humans[e], b.n_static[e] = n, ns
    for k in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref"):
        getattr(b, k)[e, n:] = 0
    for k in ("spx", "spy", "sradius"):
        getattr(b, k)[e, ns:] = 0


def wide_batch(N, S):
    """orca_branch_batch for 32-lane groups with the robot inside the crowd.  Its ragged envs draw their row counts at
    random; five of them are set by hand, so that every wide shape has an env with no row, with one row, with at most 32
    rows, with static rows only and with humans only.  In a sixth env, one with every row, the rows of index below 32 are
    moved 40 m away, out of everyone's range: its selection lies wholly at row 32 or above."""
    if (N, S) not in _batches:
        b = orca_branch_batch(91000 + 100 * N + S, N, 32, S=S, robot_inside=True)
        ragged = list(range(2, b.n, 3))
        step = len(ragged) // 5
        e0, e1, e32, es, eh = ragged[0], ragged[step], ragged[2 * step], ragged[3 * step], ragged[4 * step]
        _force_rows(b, e0, 0, 0)
        _force_rows(b, e1, 1, 0)
        _force_rows(b, e32, min(N, 9), min(S, 23))
        _force_rows(b, es, 0, S)
        _force_rows(b, eh, N, 0)
        behind = 1  # of crowd(4): not ragged
        assert b.n_humans[behind] == N and b.n_static[behind] == S
        b.px[behind, :min(N, TILE)] += 40.0
        b.spx[behind, :max(TILE - N, 0)] += 40.0
        b.forced = dict(none=e0, one=e1, narrow=e32, static_only=es, humans_only=eh, behind=behind)
        _batches[N, S] = b
    return _batches[N, S]


def ties_batch(R):
    """Robot at the origin; one env per pair of rows (lo, hi) at (x, y) and (-x, -y): equal float32 distSq.  Nine rows
    lie nearer than the pair (behind the robot; one row of the pair stands on its way to the goal) and every other row
    farther, in range, so the pair stands at ranks 9 and 10 and exactly its lower index is selected (max_neighbors = 10).  Every coordinate is a multiple of 1/8: exact in float32.  lo < 32 <=
    hi in every env at R = 40; at R = 100 pairs also straddle row 64, in one lane (5, 37: rows of lane 5) and across
    lanes."""
    if ("ties", R) in _batches:
        return _batches["ties", R]
    N = {40: 14, 100: 33}[R]
    S = R - N
    pairs = [(31, 32), (5, 37), (0, 39), (13, 33), (14, 38)]
    if R > 64:
        pairs += [(63, 64), (40, 90), (10, 70), (31, 99), (64, 96), (35, 67)]
    rs = np.random.RandomState(7700 + R)
    b = _blank_batch(len(pairs), N, S)
    b.robot[:] = [0.0, 0.0, 0.25, 0.125, 0.25, 0.0, 4.0, 1.0, np.pi / 2]
    grid = np.array([(x, y) for x in np.arange(-6, 6.01, 0.125) for y in np.arange(-6, 6.01, 0.125)])
    d = (grid ** 2).sum(1)
    # the pair: one row on the robot's way to its goal (0, 4), the other behind it; the nine nearer rows stand behind the
    # robot, so which of the pair is selected decides whether the way ahead is blocked
    pair_xy = np.array([0.25, 1.75])  # distSq 3.125
    near_pool, far_pool = grid[(d > 0.5) & (d < 3.0) & (grid[:, 1] <= -0.5)], grid[(d > 3.5) & (d < 60.0)]
    for e, (lo, hi) in enumerate(pairs):
        pos = np.zeros((R, 2))
        others = [r for r in range(R) if r not in (lo, hi)]
        near = rs.choice(others, 9, replace=False)
        while True:  # nine nearer rows at nine different distances
            pts = near_pool[rs.choice(len(near_pool), 9, replace=False)]
            if len(set((pts ** 2).sum(1))) == 9:
                break
        pos[near] = pts
        far = [r for r in others if r not in set(near)]
        pos[far] = far_pool[rs.choice(len(far_pool), len(far), replace=False)]
        pos[lo], pos[hi] = pair_xy, -pair_xy
        if e % 2:  # the mirrored pair: the selected row is the one at (-x, -y)
            pos[lo], pos[hi] = -pair_xy, pair_xy
        vel = rs.randint(-4, 5, (R, 2)) / 8.0
        b.px[e], b.py[e] = pos[:N].T
        b.vx[e], b.vy[e] = vel[:N].T
        b.gx[e], b.gy[e] = -pos[:N].T
        b.spx[e], b.spy[e] = pos[N:].T
    b.radius[:], b.v_pref[:], b.sradius[:] = 0.125, 1.0, 0.125
    b.pairs = pairs
    _batches["ties", R] = b
    return b


def sim_batch(rs, E, N, S):
    """Scenes for the persistent simulator at more than 32 rows: every human and static row with a radius of its own,
    N - 1 or N humans and S - 1 or S static rows per env (so restarts meet other row counts, and as often the same), the
    robot walking up through the crowd."""
    b = _blank_batch(E, N, S)
    b.n_humans[:] = rs.randint(N - 1, N + 1, E)
    b.n_static[:] = rs.randint(S - 1, S + 1, E)
    for e in range(E):
        k, m = int(b.n_humans[e]), int(b.n_static[e])
        for key in ("px", "py", "gx", "gy"):
            getattr(b, key)[e, :k] = rs.uniform(-4, 4, k)
        b.vx[e, :k], b.vy[e, :k] = rs.uniform(-0.5, 0.5, k), rs.uniform(-0.5, 0.5, k)
        b.radius[e, :k], b.v_pref[e, :k] = rs.uniform(0.1, 0.5, k), rs.uniform(0.3, 1.2, k)
        b.type[e, :k] = np.sort(rs.randint(0, 3, k))
        b.spx[e, :m], b.spy[e, :m], b.sradius[e, :m] = rs.uniform(-4, 4, m), rs.uniform(-4, 4, m), rs.uniform(0.1, 0.4, m)
        b.robot[e] = [rs.uniform(-1, 1), -3.0, 0, 0, 0.3, 0.0, 3.0, 0.7, np.pi / 2]
    return b


def rows_of(b, e):
    """[rows, 5] px, py, vx, vy, radius of the observation of env e: its humans, then its static rows at velocity 0, one
    after the other as the policy is given them (row r of the kernels); and the row indices, 0 .. rows - 1."""
    n, ns = int(b.n_humans[e]), int(b.n_static[e]) if b.S else 0
    hum = np.stack([b.px[e, :n], b.py[e, :n], b.vx[e, :n], b.vy[e, :n], b.radius[e, :n]], 1)
    sta = np.stack([b.spx[e, :ns], b.spy[e, :ns], np.zeros(ns), np.zeros(ns), b.sradius[e, :ns]], 1)
    return np.concatenate([hum, sta]), np.arange(n + ns)


def select(b, params):
    """Agent::insertAgentNeighbor per env in numpy: float32 dx * dx + dy * dy (one rounding per operation), in range iff
    < neighbor_dist^2, sorted by (distSq, row), the first max_neighbors.  -> [(selected positions into rows_of(b, e),
    ascending; rows in range)] per env."""
    f = np.float32
    range_sq = f(params.orca_neighbor_dist) * f(params.orca_neighbor_dist)
    out = []
    for e in range(b.n):
        rows, _ = rows_of(b, e)
        dx = f(b.robot[e, 0]) - rows[:, 0].astype(f)
        dy = f(b.robot[e, 1]) - rows[:, 1].astype(f)
        d = dx * dx + dy * dy
        assert d.dtype == f
        near = np.flatnonzero(d < range_sq)
        order = near[np.lexsort((near, d[near]))]
        out.append((np.sort(order[:min(int(params.orca_max_neighbors), 10)]), len(near)))
    return out


def reduced_batch(b, params):
    """The batch whose env e holds only the selected rows of env e of `b`, in their order, under the same robot."""
    sel = select(b, params)
    picks = []
    for e in range(b.n):
        _, idx = rows_of(b, e)
        chosen, n = idx[sel[e][0]], int(b.n_humans[e])
        picks.append((chosen[chosen < n], chosen[chosen >= n] - n))
    N = max(1, max(len(h) for h, _ in picks))
    S = max(len(s) for _, s in picks)
    r = _blank_batch(b.n, N, S)
    r.robot[:] = b.robot
    r.n_humans[:] = [len(h) for h, _ in picks]
    r.n_static[:] = [len(s) for _, s in picks]
    for e, (h, s) in enumerate(picks):
        for k in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type"):
            getattr(r, k)[e, :len(h)] = getattr(b, k)[e, h]
        for k in ("spx", "spy", "sradius"):
            if S:
                getattr(r, k)[e, :len(s)] = getattr(b, k)[e, s]
    return r


_refs = {}


def oracle_robot_orca(b, params, safety, library=None):
    from oracle import oracle
    o = oracle.OracleEnv(params, b.n, b.N, b.S, library=library)
    o.reset(b)
    return o.robot_orca(safety)


def reduced_reference(key, b, ps, safety):
    """robot_orca(safety) of the oracle on the reduced batch of `b` under parameter set ps, once per session."""
    k = (key, ps, safety)
    if k not in _refs:
        params = orca_case_params(0, ps)
        _refs[k] = oracle_robot_orca(reduced_batch(b, params), params, safety)
        _refs[k].flags.writeable = False
    return _refs[k]


def full_reference(N, S, ps, safety):
    """robot_orca(safety) of the oracle on wide_batch(N, S) itself (N + S <= 64), once per session."""
    k = ("full", N, S, ps, safety)
    if k not in _refs:
        _refs[k] = oracle_robot_orca(wide_batch(N, S), orca_case_params(0, ps), safety)
        _refs[k].flags.writeable = False
    return _refs[k]
