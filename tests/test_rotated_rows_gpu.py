"""The rotated observation rows of the device, every site that writes them, held to the float32 rule bit for bit (-m gpu).

The rows are the input of every value network, and until here every comparison of them with the oracle was
atol = rtol = 1e-5, because the device's atan2f / cosf / sinf are not glibc's.  Under that bar a subtraction done in
double before the cast, a contracted multiply-add, a frame built from the old velocity or a swapped operand all pass:
each moves a value by about one float32 ulp.  tests/rows_cases.py splits the error in two.  A probe row (velocity exactly
(1, 0)) makes every frame report its own c and s, and then
(a) every other value of every row must equal rule_rows in every bit, the sign of zero included, padding rows +0 —
    observe_kernel, step_kernel, the ROWS role of orca_step_kernel, phase C of lookahead_kernel at every shape of its
    flat copy, and the three sites of rollout_kernel, at T = 13 and 17, holonomic and unicycle;
(b) the frame itself (c, s and, under rotate_unicycle, column 2) is held to float64 within 4 x what glibc shows on the
    same frames;
(c) the raw rows are the oracle's bytes under HUMAN_EXTERNAL and HUMAN_ORCA, within 1e-9 under HUMAN_LINEAR (cos / sin);
(d) the forms agree byte for byte; (e) the look-ahead writes every requested element and nothing else, at every shape;
(f) a scene's rows do not depend on its place in the batch; (g) the look-ahead's cached linear velocities are the step's.

tests/test_rotated_rows_cpu.py proves the rule, the probe and the table on the oracle."""
import numpy as np
import pytest

from ebcsim import _abi
from helpers import Guarded, _close, oracle_env
from rows_cases import (FORM_SHAPE, LA_CASES, LA_E, POLICY_NAME, ROW_FORMS, WIDTHS, assert_rows_equal_rule, copy_split,
                        form_batch, form_lookahead, frame_error, frame_of, la_actions, la_batch, la_case_id, place,
                        probe_batch, robot_actions, rows_params, run_form)
from test_gpu_parity import _env

pytestmark = pytest.mark.gpu

ROWS_BAR = 1e-5  # the project's bar for rotated rows against the oracle (tests/test_gpu_parity.py)
FORM_CASES = [(form, T, uni) for form in ROW_FORMS for T in WIDTHS for uni in (0, 1)]
LA_KEYS = ("reward", "done", "info", "dmin", "next_ob", "rows_rotated")

_runs = {}


def form_run(form, T, unicycle):
    """(params, the device's records, the oracle's) of a form, once per session."""
    key = (form, T, unicycle)
    if key not in _runs:
        params, dev = run_form(_env, form, T, unicycle)
        _runs[key] = (params, dev, run_form(oracle_env, form, T, unicycle)[1])
    return _runs[key]


def la_run(case):
    """The same for a shape of the look-ahead's table (HUMAN_LINEAR: phase A computes and caches the velocities)."""
    if case not in _runs:
        A, N, S, T, uni = case
        params, b = rows_params(T, uni), la_batch(case)
        kw = dict(A=A, policies=(_abi.HUMAN_LINEAR,))
        _runs[case] = (params, form_lookahead(_env, params, b, **kw), form_lookahead(oracle_env, params, b, **kw))
    return _runs[case]


def check_rule(dev, ref, T, unicycle, tag):
    """(a) for one record -> rows held bit for bit."""
    c, s = frame_of(dev["rot"])
    ec, es, _ = frame_error(dev["robot"], c, s)
    # the probe's report is a frame at all: the bar every row was held to until now (the fine bar is (b)'s)
    assert max(ec, es) <= ROWS_BAR, "%s: the probe row's (c, s) is %.3g / %.3g from cos / sin of the frame" % (tag, ec, es)
    exact = dev.get("exact")
    rows = assert_rows_equal_rule(dev, T, unicycle, tag, select=exact)
    if exact is not None and not exact.all():  # unicycle look-ahead: cos / sin of a heading in the propagation
        np.testing.assert_allclose(dev["rot"][~exact], ref["rot"][~exact], atol=ROWS_BAR, rtol=ROWS_BAR, err_msg=tag)
    return rows


@pytest.mark.parametrize("form,T,unicycle", FORM_CASES, ids=lambda v: str(v))
def test_rows_equal_the_rule(form, T, unicycle):
    """(a) every form: 67 envs of up to 6 humans and 3 static rows, every record (observe: reset and after 3 steps; step:
    3 steps under EXTERNAL and under LINEAR; orca: 3 steps; look-ahead: 81 actions under each policy; one launch: K = 3,
    state_rotated and obs_rotated).  Under unicycle column 2 is (b)'s, and of the look-ahead the frames of rotation 0
    from heading 0 are compared bit for bit, the others with the oracle at 1e-5."""
    params, dev, ref = form_run(form, T, unicycle)
    assert len(dev) == len(ref) >= 3
    rows = {}
    for k, (d, r) in enumerate(zip(dev, ref)):
        assert d["site"] == r["site"]
        rows[d["site"]] = rows.get(d["site"], 0) + check_rule(d, r, T, unicycle, "%s T%d unicycle%d record %d" % (
            form, T, unicycle, k))
    for site, count in rows.items():
        print("rows held bit for bit: %-30s T%d %s %6d" % (site, T, "unicycle " if unicycle else "holonomic", count))
    assert sum(rows.values()) >= 3 * FORM_SHAPE[0] * (FORM_SHAPE[1] + FORM_SHAPE[2])


def _la_device(g, actions_t, case, keys):
    """A device-location look-ahead with every output between canaries, poisoned -> {key: the inside on the host}."""
    import torch
    A, N, S, T, _ = case
    E, R = LA_E, N + S
    spec = dict(reward=((E * A,), torch.float64), done=((E * A,), torch.uint8), info=((E * A,), torch.uint8),
                dmin=((E * A, 3), torch.float64), next_ob=((E * R, 5), torch.float64),
                rows_rotated=((E * A * R, T), torch.float32))  # flat: the canaries are sized by the last axis
    bufs = {k: Guarded(spec[k][0], spec[k][1]) for k in keys}
    g.lookahead_device(actions_t, {k: v.t for k, v in bufs.items()}, human_policy=_abi.HUMAN_LINEAR)
    g.synchronize()
    return {k: v.check() for k, v in bufs.items()}  # canaries intact, every element written


@pytest.mark.parametrize("case", LA_CASES, ids=la_case_id)
def test_lookahead_shapes(case):
    """(a) and (e) at every (A, R, T) of the table, 5 envs: rows_rotated equals the rule in every bit where the flat copy
    has every head, tail and chunk pattern (copy_split), and with the outputs on the device between canaries — the key
    sets rows_rotated, next_ob, reward alone and all six — every requested element is written, nothing beside it, and
    the bytes are the host-location call's."""
    import torch
    A, N, S, T, uni = case
    params, dev, ref = la_run(case)
    assert sum(sp[3] for sp in copy_split(LA_E, A, N + S, T)) == LA_E * A * (N + S)
    rows = check_rule(dev[0], ref[0], T, uni, la_case_id(case))
    print("rows held bit for bit: %-30s %-22s %6d" % ("lookahead_kernel (table)", la_case_id(case), rows))
    b = la_batch(case)
    g = _env(params, LA_E, N, S)
    g.use_torch_stream()
    g.reset(b)
    actions = dev[0]["actions"]
    host = g.lookahead(actions, human_policy=_abi.HUMAN_LINEAR)
    assert host["rows_rotated"].tobytes() == dev[0]["rot"].tobytes()
    actions_t = torch.tensor(actions, dtype=torch.float64, device="cuda")
    for keys in (("rows_rotated",), ("next_ob",), ("reward",), LA_KEYS):
        got = _la_device(g, actions_t, case, keys)
        for k in keys:
            assert got[k].tobytes() == host[k].tobytes(), (la_case_id(case), keys, k)
    _close(g)


def _frame_figures(recs, unicycle):
    """max |c - cos|, |s - sin| and (unicycle) |column 2 - (float32(theta) - atan2)| over the records' frames, frames."""
    worst, n = np.zeros(3), 0
    for rec in recs:
        c, s = frame_of(rec["rot"])
        worst = np.maximum(worst, frame_error(rec["robot"], c, s, rec["rot"][..., 0, 2] if unicycle else None))
        n += c.size
    return worst, n


def test_frames_against_float64():
    """(b) every frame of (a), forms and table: the device's c and s (read from the probe row) against cos / sin of
    theta = atan2 of the float32 (dy, dx) in float64, and under rotate_unicycle column 2 against float32(heading) -
    theta.  The yardstick is the oracle's figure — glibc's atan2f / cosf / sinf, nearly correctly rounded — on the same
    frames, computed here; the bar is 4 x that figure (a few ulp for an OpenCL-grade library), never anything the device
    returned.  The figures are printed (-s); profiles/rotated_rows.txt holds a run's."""
    dev_w, ref_w, frames = np.zeros(3), np.zeros(3), 0
    for key in FORM_CASES + LA_CASES:
        params, dev, ref = form_run(*key) if len(key) == 3 else la_run(key)
        uni = key[-1]
        d, n = _frame_figures(dev, uni)
        r, _ = _frame_figures(ref, uni)
        dev_w, ref_w, frames = np.maximum(dev_w, d), np.maximum(ref_w, r), frames + n
    dev_cs, ref_cs = float(dev_w[:2].max()), float(ref_w[:2].max())
    print("frames: %d" % frames)
    print("max |c - cos theta|, |s - sin theta|: device %.4g, oracle (glibc) %.4g, bar %.4g" % (dev_cs, ref_cs, 4 * ref_cs))
    print("max |column 2 - (float32(heading) - theta)| under rotate_unicycle: device %.4g, oracle (glibc) %.4g, bar %.4g" % (
        dev_w[2], ref_w[2], 4 * ref_w[2]))
    assert 0 < ref_cs < 1e-6 and 0 < ref_w[2] < 2e-6  # the yardstick is a float32 library's, not a broken one's
    assert dev_cs <= 4 * ref_cs, (dev_cs, ref_cs)
    assert dev_w[2] <= 4 * ref_w[2], (float(dev_w[2]), float(ref_w[2]))


@pytest.mark.parametrize("form,T,unicycle", FORM_CASES, ids=lambda v: str(v))
def test_raw_rows(form, T, unicycle):
    """(c) ob / next_ob against the oracle: the same double formula with contraction off on both sides, so the bytes
    under HUMAN_EXTERNAL and HUMAN_ORCA (and at reset); within 1e-9 under HUMAN_LINEAR, whose cos / sin differ."""
    params, dev, ref = form_run(form, T, unicycle)
    for k, (d, r) in enumerate(zip(dev, ref)):
        policy = d.get("policy", _abi.HUMAN_ORCA if form == "one_launch" else _abi.HUMAN_LINEAR)
        tag = "%s (%s) record %d" % (form, POLICY_NAME[policy], k)
        np.testing.assert_allclose(d["raw"], r["raw"], atol=1e-9, rtol=0, err_msg=tag)
        if policy != _abi.HUMAN_LINEAR or (form == "observe" and k == 0):
            bad = np.argwhere(d["raw"] != r["raw"])
            assert d["raw"].tobytes() == r["raw"].tobytes(), "%s: raw rows differ from the oracle's bytes in columns %s" % (
                tag, sorted(set(bad[:, -1].tolist())))
            # and the robot states the frames were built from (holonomic: no cos / sin in the robot's step either)
            if not unicycle:
                assert d["robot"].tobytes() == r["robot"].tobytes(), tag


@pytest.mark.parametrize("unicycle", [0, 1], ids=["holonomic", "unicycle"])
@pytest.mark.parametrize("T", WIDTHS)
def test_forms_agree(T, unicycle):
    """(d) byte for byte: ebc_observe's rows are the rows the step before returned; the one-launch form's obs_rotated[k]
    and state_rotated[k] are the per-step form's; state_rotated[k + 1] is obs_rotated[k]."""
    _, obs, _ = form_run("observe", T, unicycle)
    for rec in obs[1:]:
        assert rec["rot"].tobytes() == rec["returned"]["obs_rotated"].tobytes(), ("observe / step", rec["step"])
        assert rec["raw"].tobytes() == rec["returned"]["ob"].tobytes(), ("observe / step, raw", rec["step"])
    _, one, _ = form_run("one_launch", T, unicycle)
    state = {r["step"]: r for r in one if r["site"].endswith("state_rotated")}
    after = {r["step"]: r for r in one if r["site"].endswith("obs_rotated")}
    assert len(state) == len(after) >= 3
    for k in state:
        assert state[k]["rot"].tobytes() == state[k]["per_step"].tobytes(), ("state_rotated", k)
        assert after[k]["rot"].tobytes() == after[k]["per_step"].tobytes(), ("obs_rotated", k)
        if k + 1 in state:
            assert state[k + 1]["rot"].tobytes() == after[k]["rot"].tobytes(), ("state_rotated[k + 1] / obs_rotated[k]", k)


@pytest.mark.parametrize("unicycle", [0, 1], ids=["holonomic", "unicycle"])
def test_placement(unicycle):
    """(f) one scene at env 0 and at env E - 1 of a batch of different scenes (E = 67; 37 actions x 9 rows: the two
    places start at different residues of the flat copy): the
    look-ahead's rows and the one-launch form's rows of the two places are the same bytes, and no other env's."""
    T, (E, N, S) = 17, FORM_SHAPE
    params = rows_params(T, unicycle)
    b = place(probe_batch(np.random.RandomState(31 + unicycle), E, N, S), 0, E - 1)
    g = _env(params, E, N, S)
    g.reset(b)
    la = g.lookahead(la_actions(37, unicycle), human_policy=_abi.HUMAN_LINEAR)
    for k in ("rows_rotated", "next_ob", "reward", "dmin"):
        assert la[k][0].tobytes() == la[k][E - 1].tobytes(), ("look-ahead", k)
    assert la["rows_rotated"][0].tobytes() != la["rows_rotated"][1].tobytes()
    K = 3
    acts = robot_actions(K, E, unicycle)
    acts[:, E - 1] = acts[:, 0]
    g.reset(b)
    one = g.step_k(K, ("state_rotated", "obs_rotated"), robot_action=acts, human_policy=_abi.HUMAN_ORCA,
                   robot_policy=_abi.ROBOT_EXTERNAL, flags=_abi.FLAG_ONE_LAUNCH)
    for k in ("state_rotated", "obs_rotated"):
        assert one[k][:, 0].tobytes() == one[k][:, E - 1].tobytes(), ("one launch", k)
        assert one[k][:, 0].tobytes() != one[k][:, 1].tobytes()
    _close(g)


@pytest.mark.parametrize("unicycle", [0, 1], ids=["holonomic", "unicycle"])
def test_lookahead_caches_the_linear_velocities(unicycle):
    """(g) phase A of the look-ahead under HUMAN_LINEAR writes the velocities it computed: a HUMAN_CACHED step behind it
    returns the bytes of a HUMAN_LINEAR step from the same state, every output.  The cache is overwritten first with
    other velocities, so a look-ahead that wrote nothing shows."""
    T, (E, N, S) = 17, FORM_SHAPE
    params = rows_params(T, unicycle)
    b = form_batch("step", T, unicycle)
    act = robot_actions(1, E, unicycle)[0]
    g = _env(params, E, N, S)
    g.reset(b)
    want = g.step(robot_action=act, human_policy=_abi.HUMAN_LINEAR)
    g.reset(b)
    g.set_human_actions(np.full((E, N, 2), 0.125))
    g.lookahead(la_actions(37, unicycle), human_policy=_abi.HUMAN_LINEAR)
    got = g.step(robot_action=act, human_policy=_abi.HUMAN_CACHED)
    assert (want["human_action"][:, 0] == (1.0, 0.0)).all()
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k
    _close(g)
