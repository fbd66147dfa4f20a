"""Where the ROWS role of orca_step_kernel stores its rows: every shape of its store pattern, between canaries (-m gpu).

A ROWS wave stores the rotated rows of its envs, [env][row][T] floats at a 4 T-byte stride, in two parts per env (rows
[n, R) before the humans' velocities are in, rows [0, n) after); an env of more than 64 rows goes in passes.  A row is
only 4-byte aligned, and the lanes of a wave store 16 and 4 bytes at a time.  What can go wrong is where a store
lands, so here
  - obs_rotated (and ob) are interior views of a larger buffer filled with a canary, starting 0, 1, 2 and 3 floats past
    a 16-byte boundary (ob: 0 and 1 doubles), the inside poisoned: both canaries are intact and every element is written;
  - E is 1, 3 and 25 (at 25 the eight env classes are 4 envs, the seventh clipped to 1, the eighth empty);
  - (N, S, T) is (1, 0, 13), (5, 0, 13), (3, 2, 17), (10, 8, 17) and (33, 95, 17): one row per env and 64 envs per wave,
    the bench workload's 18 rows, and 128 rows, the most the library accepts (two passes);
  - n_humans is ragged with 0 included and n_static is ragged, so that padding rows move and a part can be empty;
  - the rows equal the float32 rule of tests/rows_cases.py in every bit, with the frame each env's probe row reports (an
    env without humans has no probe: it is a copy of env 0 without its humans, the robot and its actions included, and
    takes env 0's frame), and are the same bytes at every offset and from the host-location call.
(Written for a form of the role that staged the rows in LDS and stored them as whole 16-byte chunks of the destination;
that form measured slower and is not in the library — DESIGN.md section 3, item 20 — the net stays.)"""
import numpy as np
import pytest

from ebcsim import _abi
from helpers import _close
from rows_cases import bits, frame_of, place, probe_batch, robot_actions, row_types, rows_params, rule_rows
from test_gpu_parity import _env

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0, 13), (5, 0, 13), (3, 2, 17), (10, 8, 17), (33, 95, 17)]
ENVS = (1, 3, 25)
STEPS = 2
CANARY, POISON, PAD = 0xB6, 0xA5, 64 << 10


def no_humans(E):
    """The envs that are env 0 without its humans."""
    return [e for e in (2, 13, 24) if e < E]


def flat_batch(E, N, S, T):
    b = probe_batch(np.random.RandomState(700 + 31 * E + N + S + T), E, N, S)
    ns = b.n_static.copy()
    for e in no_humans(E):
        place(b, 0, e)
        b.n_humans[e] = 0
        for k in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type"):
            getattr(b, k)[e] = 0
        if S:  # its own ragged static rows: some of env 0's, the rest padding
            b.n_static[e] = ns[e] if e != 2 else S // 2
    return b


class Interior:
    """A view `off` bytes past a 16-byte boundary inside a buffer of canary bytes, the inside poisoned."""

    def __init__(self, shape, dtype, off):
        import torch
        self.shape, self.np_dtype = shape, torch.empty((), dtype=dtype).numpy().dtype
        self.nbytes = int(np.prod(shape)) * self.np_dtype.itemsize
        self.raw = torch.full((2 * PAD + self.nbytes + 16,), CANARY, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 16 == 0
        self.start = PAD + off
        self.raw[self.start:self.start + self.nbytes].fill_(POISON)
        self.t = self.raw[self.start:self.start + self.nbytes].view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == off

    def check(self, tag):
        b = self.raw.cpu().numpy()
        lo, inside, hi = b[:self.start], b[self.start:self.start + self.nbytes], b[self.start + self.nbytes:]
        bad = np.nonzero(lo != CANARY)[0]
        assert not len(bad), "%s: write %d bytes before the view" % (tag, self.start - bad[0])
        bad = np.nonzero(hi != CANARY)[0]
        assert not len(bad), "%s: write %d bytes past the end of the view" % (tag, bad[-1] + 1)
        item = self.np_dtype.itemsize
        untouched = (inside.reshape(-1, item) == POISON).all(1)
        assert not untouched.any(), "%s: %d elements not written, the first %d" % (tag, int(untouched.sum()), int(np.argmax(untouched)))
        return inside.view(self.np_dtype).reshape(self.shape).copy()


def assert_rule(b, robot, raw, got, T, tag):
    """Every bit of got [E, R, T] against rule_rows with the frames the probe rows report."""
    E, twins = b.n, no_humans(b.n)
    probes = np.array([e not in twins for e in range(E)])
    assert (raw[probes, 0, 2] == 1.0).all() and (raw[probes, 0, 3] == 0.0).all(), tag + ": the probe's velocity is not (1, 0)"
    c, s = frame_of(got)
    for e in twins:
        assert robot[e].tobytes() == robot[0].tobytes(), tag
        c[e], s[e] = c[0], s[0]
    assert np.isfinite(c).all() and np.isfinite(s).all(), tag
    types, n_rows = row_types(b)
    want = rule_rows(robot, raw, types, T, False, c, s, None, n_rows)
    bad = np.argwhere(bits(got) != bits(want))
    assert not len(bad), "%s: %d values differ from the rule, the first at %s: %r, the rule %r" % (
        tag, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("E", ENVS)
@pytest.mark.parametrize("N,S,T", SHAPES, ids=lambda v: str(v))
def test_rows_land_where_they_belong(N, S, T, E):
    import torch
    params = rows_params(T, 0)
    b = flat_batch(E, N, S, T)
    R = N + S
    acts = robot_actions(STEPS, E, 0)
    for e in no_humans(E):
        acts[:, e] = acts[:, 0]
    g = _env(params, E, N, S)
    g.reset(b)
    host = [g.step(robot_action=acts[t], human_policy=_abi.HUMAN_ORCA) for t in range(STEPS)]
    host = [dict(ob=np.array(o["ob"]), obs_rotated=np.array(o["obs_rotated"])) for o in host]
    acts_t = torch.tensor(acts, dtype=torch.float64, device="cuda")
    for off in range(4):
        g.reset(b)
        for t in range(STEPS):
            tag = "E%d N%d S%d T%d offset %d step %d" % (E, N, S, T, off, t)
            rot = Interior((E, R, T), torch.float32, 4 * off)
            ob = Interior((E, R, 5), torch.float64, 8 * (off & 1))
            g.step_device(dict(ob=ob.t, obs_rotated=rot.t), robot_action=acts_t[t], human_policy=_abi.HUMAN_ORCA,
                          robot_policy=_abi.ROBOT_EXTERNAL)
            g.synchronize()
            got, raw = rot.check(tag + " obs_rotated"), ob.check(tag + " ob")
            assert_rule(b, g.get_state()["robot"], raw, got, T, tag)
            assert got.tobytes() == host[t]["obs_rotated"].tobytes(), tag + ": not the host-location call's rows"
            assert raw.tobytes() == host[t]["ob"].tobytes(), tag + ": not the host-location call's raw rows"
    _close(g)
