"""Every kernel on the step path with time_step, the ORCA horizon and the humans' safety space off their defaults (-m gpu).

The runs are those of tests/params_cases.py, which tests/test_params_cpu.py shows to differ from the same runs at the
default fields, to restart every env and to meet every info code; here each form of the step is held to what the oracle
computed for them, every step, at the bars of test_gpu_parity._compare_step (masks and codes exact, float64 1e-9, rotated
rows 1e-5) and, on the ORCA path, human_action bit for bit as in test_orca_branches_gpu.py.  Then the Python layer that
reads params.time_step: DeviceSarlPolicy.decide, collect_il and evaluate.  The worst |difference| per output goes to
profiles/param_coverage.txt (the last test)."""
import os

import numpy as np
import pytest
import torch

import params_cases as pc
from ebcsim import _abi
from ebcsim.batched import BatchedEnv
from test_gpu_parity import _compare_step
from test_orca_branches_gpu import _bitwise
from test_step_k_one_launch_gpu import _bytes_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "profiles", "param_coverage.txt")
WORST = {}  # (form, output) -> the largest |device - oracle| seen


def _note(form, key, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore"):  # inf - inf where both hold inf
        d = float(np.abs(np.where(same, 0.0, got - want)).max()) if got.size else 0.0
    WORST[form, key] = max(WORST.get((form, key), 0.0), d)


def _step_bars(form, out, ref, tag, bitwise_humans):
    for k in ("reward", "dmin", "dist_to_goal", "human_action", "ob", "robot_action_out", "obs_rotated"):
        _note(form, k, out[k], ref[k])
    if bitwise_humans:
        _bitwise(out["human_action"], ref["human_action"], tag + " human_action")
    _compare_step(out, ref, tag)


def _state_bars(form, g, want, tag):
    got = g.get_state()
    for k in got:
        _note(form, "state " + k, got[k], want[k])
        np.testing.assert_allclose(got[k], want[k], atol=1e-9, rtol=0, err_msg=tag + " state " + k)


def _device_env(params, sim=None):
    return pc.start(BatchedEnv(params, pc.E, pc.N, pc.S), sim)


sets = pytest.mark.parametrize("ps", pc.SETS)
kinematics = pytest.mark.parametrize("kin", pc.KINEMATICS)


# ------------------------------------------------------------------ ebc_step, ebc_lookahead
@sets
@kinematics
def test_step_linear_humans(ps, kin):
    """step_kernel with HUMAN_LINEAR: the humans' and the robot's advance, closest_dist, the clock, the rows."""
    ref = pc.step_reference(ps, kin, _abi.HUMAN_LINEAR)
    g, act = _device_env(pc.case_params(ps, kin)), pc.robot_actions(kin)
    for t in range(pc.STEPS):
        tag = "%s %s linear step %d" % (ps, kin, t)
        out = g.step(robot_action=act[t], human_policy=_abi.HUMAN_LINEAR, flags=pc.AUTO)
        _step_bars("step linear", out, ref["out"][t], tag, False)
        _state_bars("step linear", g, ref["state"][t], tag)


@sets
@kinematics
def test_step_supplied_velocities(ps, kin):
    """step_kernel with HUMAN_EXTERNAL: the velocities the oracle's ORCA gave, handed in by the host."""
    ref = pc.step_reference(ps, kin, _abi.HUMAN_ORCA)
    g, act = _device_env(pc.case_params(ps, kin)), pc.robot_actions(kin)
    for t in range(pc.STEPS):
        tag = "%s %s supplied step %d" % (ps, kin, t)
        g.set_human_actions(ref["out"][t]["human_action"])
        out = g.step(robot_action=act[t], human_policy=_abi.HUMAN_EXTERNAL, flags=pc.AUTO)
        _step_bars("step supplied", out, ref["out"][t], tag, True)
        _state_bars("step supplied", g, ref["state"][t], tag)


@sets
@kinematics
def test_step_orca_humans(ps, kin):
    """orca_step_kernel, every step."""
    ref = pc.step_reference(ps, kin, _abi.HUMAN_ORCA)
    g, act = _device_env(pc.case_params(ps, kin)), pc.robot_actions(kin)
    for t in range(pc.STEPS):
        tag = "%s %s orca step %d" % (ps, kin, t)
        out = g.step(robot_action=act[t], human_policy=_abi.HUMAN_ORCA, flags=pc.AUTO)
        _step_bars("step orca", out, ref["out"][t], tag, True)
        _state_bars("step orca", g, ref["state"][t], tag)


@sets
@kinematics
def test_lookahead_then_cached_step(ps, kin):
    """ebc_lookahead over the action space before every fifth step (orca_kernel, lookahead_kernel: its dt, the discomfort
    reward, the time-out one step ahead), the step after it on the cached velocities; the other steps on ORCA."""
    ref = pc.step_reference(ps, kin, _abi.HUMAN_ORCA)
    g, act, space = _device_env(pc.case_params(ps, kin)), pc.robot_actions(kin), pc.action_space(kin)
    assert sorted(ref["la"]) == list(range(0, pc.STEPS, pc.LOOKAHEAD_EVERY))
    for t in range(pc.STEPS):
        tag = "%s %s look-ahead step %d" % (ps, kin, t)
        if t in ref["la"]:
            la, want = g.lookahead(space, human_policy=_abi.HUMAN_ORCA), ref["la"][t]
            for k in ("reward", "dmin", "next_ob", "rows_rotated"):
                _note("lookahead", k, la[k], want[k])
            np.testing.assert_array_equal(la["done"], want["done"], err_msg=tag)
            np.testing.assert_array_equal(la["info"], want["info"], err_msg=tag)
            for k in ("reward", "dmin", "next_ob"):
                np.testing.assert_allclose(la[k], want[k], atol=1e-9, rtol=0, err_msg=tag + " " + k)
            np.testing.assert_allclose(la["rows_rotated"], want["rows_rotated"], atol=1e-5, rtol=1e-5, err_msg=tag)
        out = g.step(robot_action=act[t], human_policy=_abi.HUMAN_CACHED if t in ref["la"] else _abi.HUMAN_ORCA, flags=pc.AUTO)
        _step_bars("step cached", out, ref["out"][t], tag, True)
    _state_bars("step cached", g, ref["state"][-1], tag)


# ------------------------------------------------------------------ ebc_step_k, per step and as one launch
@sets
@pytest.mark.parametrize("form", pc.STEP_K_FORMS, ids=pc.form_id)
def test_step_k_both_forms(ps, form):
    """K = 30 steps in one call, per step and with EBC_FLAG_ONE_LAUNCH (rollout_kernel keeps a dt of its own and restates
    the tile record): the two forms byte for byte, as test_step_k_one_launch_gpu.py holds them, and both to K oracle
    steps; the ORCA robot's action bit for bit (its own safety space, 0.15, is never the handle's)."""
    robot, kin, sim = form
    ref = pc.step_k_reference(ps, form)
    keys, kw = pc.step_k_keys(robot), pc.step_k_kw(robot, kin)
    a, b = _device_env(pc.case_params(ps, kin), sim), _device_env(pc.case_params(ps, kin), sim)
    oa = a.step_k(pc.STEPS, keys, flags=pc.AUTO, **kw)
    ob = b.step_k(pc.STEPS, keys, flags=pc.AUTO | pc.ONE, **kw)
    tag = "%s %s" % (ps, pc.form_id(form))
    for k in keys:
        _bytes_equal(oa[k], ob[k], "%s: per step and one launch, output %s" % (tag, k))
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        _bytes_equal(sa[k], sb[k], "%s: per step and one launch, state %s" % (tag, k))
    if sim:
        ma, mb = a.robot_orca_sim_state(), b.robot_orca_sim_state()
        for k in ma:
            _bytes_equal(ma[k], mb[k], "%s: per step and one launch, simulator %s" % (tag, k))
        np.testing.assert_array_equal(ma["rows"], ref["sim"]["rows"], err_msg=tag)
    want = ref["out"]
    for k in ("done", "info", "n_rows"):
        np.testing.assert_array_equal(ob[k], want[k], err_msg=tag + " " + k)
    if robot == "orca":
        _bitwise(ob["robot_action_out"], want["robot_action_out"], tag + " robot_action_out")
    for k in ("reward", "dmin", "dist_to_goal", "robot_action_out"):
        if k in ob:
            _note("step_k " + robot, k, ob[k], want[k])
            np.testing.assert_allclose(ob[k], want[k], atol=1e-9, rtol=0, err_msg=tag + " " + k)
    for k in ("state_rotated", "obs_rotated"):
        _note("step_k " + robot, k, ob[k], want[k])
        np.testing.assert_allclose(ob[k], want[k], atol=1e-5, rtol=1e-5, err_msg=tag + " " + k)
    for k in sb:
        _note("step_k " + robot, "state " + k, sb[k], ref["state"][k])
        np.testing.assert_allclose(sb[k], ref["state"][k], atol=1e-9, rtol=0, err_msg=tag + " state " + k)
    assert want["done"].astype(bool).any(0).all()  # every env restarted inside the call
    b.synchronize()


# ------------------------------------------------------------------ ebc_sail_dagger_k
def test_sail_dagger_under_all():
    """8 steps of ebc_sail_dagger_k under "all" (dagger_label_kernel: the handle's step and horizon, the expert's own safety
    space): every output is the Python composition's of tests/test_sail_dagger_gpu.py, byte for byte, and the expert's
    labels are the oracle's robot_orca on the states the executed actions lead to, bit for bit."""
    from ebcsim.sail import DeviceSailPolicy, SailNet
    from oracle import oracle
    from sail_dagger_cases import OUT
    from test_sail_dagger_gpu import _dagger, _mask_dev, _state_equal, make_env
    c = pc.DAGGER
    K, n, A = c["K"], c["E"], c["A"]
    params, batch, pool, sd, mask = pc.dagger_setup()
    net = SailNet(sd, device=DEV)
    a, b = make_env(params, batch, net, pool), make_env(params, batch, net, pool)
    got = _dagger(a, K, mask, pc.AUTO, safety=c["safety"])
    pol, m = DeviceSailPolicy(net), _mask_dev(mask)
    robot = torch.empty((n, 9), dtype=torch.float64, device=DEV)
    ob = torch.empty((n, A, 5), dtype=torch.float64, device=DEV)
    n_rows = torch.empty((n,), dtype=torch.int64, device=DEV)
    expert = torch.empty((n, 2), dtype=torch.float64, device=DEV)
    so = b.alloc_step_outputs(("reward", "done", "info"))
    o = oracle.OracleEnv(params, batch.n, batch.N, batch.S)
    o.reset(batch)
    o.set_scene_pool(pool)
    for k in range(K):
        b.robot_state_device(robot)
        b.observe_ob_device(ob)
        b.row_counts_device(n_rows)
        learner, _ = pol.decide(b)
        b.robot_orca_device(expert, c["safety"])
        act = torch.where(m[k].bool()[:, None], expert, learner).contiguous()
        b.step_device(so, robot_action=act, human_policy=_abi.HUMAN_ORCA, flags=pc.AUTO)
        b.synchronize()
        want = dict(robot=robot, ob=ob, n_rows=n_rows, learner_action=learner, expert_action=expert, robot_action_out=act, **so)
        for name in OUT:
            _bytes_equal(got[name][k], want[name].cpu().numpy(), "dagger step %d %s" % (k, name))
        _bitwise(got["expert_action"][k], o.robot_orca(c["safety"]), "dagger step %d: the expert's label" % k)
        ref = o.step(robot_action=got["robot_action_out"][k], human_policy=_abi.HUMAN_ORCA, flags=pc.AUTO)
        np.testing.assert_array_equal(got["done"][k], ref["done"])
        np.testing.assert_array_equal(got["info"][k], ref["info"])
        _note("sail_dagger_k", "reward", got["reward"][k], ref["reward"])
        np.testing.assert_allclose(got["reward"][k], ref["reward"], atol=1e-9, rtol=0)
    assert got["done"].astype(bool).any(0).all()
    _state_equal(a, b, "dagger")


# ------------------------------------------------------------------ ebc_step_with_map
def test_step_with_map_unicycle_dt01():
    """local_map_kernel advances the robot itself when the step hands it the action (io.next): with a unicycle robot at
    time_step 0.1 the returned map is ebc_local_map of the state after the step, bit for bit, and that state's robot is
    the oracle's."""
    from oracle import oracle
    c = pc.MAP
    params, batch, act = pc.map_setup()
    g = BatchedEnv(params, batch.n, batch.N, batch.S)
    g.configure_local_map(c["dim"], c["max_range"], -np.pi, np.pi)
    g.reset(batch)
    o = oracle.OracleEnv(params, batch.n, batch.N, batch.S)
    o.reset(batch)
    moved = 0
    for t in range(c["steps"]):
        before = g.local_map()
        out = g.step(act[t], human_policy=_abi.HUMAN_LINEAR, local_map=True)
        ref = o.step(act[t], human_policy=_abi.HUMAN_LINEAR)
        _compare_step(out, ref, "map step %d" % t)
        _state_bars("step_with_map", g, o.get_state(), "map step %d" % t)
        _bytes_equal(out["local_map"], g.local_map(), "map step %d" % t)
        moved += int((out["local_map"] != before).any(1).sum())
    assert (out["local_map"] < 1).any() and moved >= c["E"]
    g.close()


# ------------------------------------------------------------------ the Python layer that reads params.time_step
def _sarl_decision(time_step):
    from ebcsim.sarl import DeviceSarlPolicy, SarlValueNet
    params, batch, space, gamma, weights = pc.sarl_setup(time_step)
    env = BatchedEnv(params, batch.n, batch.N, batch.S)
    env.reset(batch)
    env.use_torch_stream()
    net = SarlValueNet.load(weights, device=DEV)
    pol = DeviceSarlPolicy(net, space, gamma)
    actions, values = pol.decide(env)
    torch.cuda.synchronize()
    return params, batch, space, gamma, net, pol, actions, values


def test_sarl_decide_discounts_by_the_env_s_time_step():
    """values = reward + gamma ** (time_step * v_pref) * V, exactly, in float64, at time_step 0.1: `reward` is the
    look-ahead's (the oracle's at 1e-9), V the network on the policy's own rows — its matrix-core value, or its float32
    value for the candidates action_values re-evaluated.  At 0.25 the values are others."""
    from oracle import oracle
    params, batch, space, gamma, net, pol, actions, values = _sarl_decision(0.1)
    n, A = batch.n, len(space)
    rr, reward = pol._bufs["rows_rotated"], pol._bufs["reward"]
    o = oracle.OracleEnv(params, batch.n, batch.N, batch.S)
    o.reset(batch)
    la = o.lookahead(space, human_policy=_abi.HUMAN_ORCA)
    _note("sarl decide", "reward", reward.cpu().numpy(), la["reward"])
    np.testing.assert_allclose(reward.cpu().numpy(), la["reward"], atol=1e-9, rtol=0)
    np.testing.assert_allclose(rr.cpu().numpy(), la["rows_rotated"], atol=1e-5, rtol=1e-5)
    discount = gamma ** (0.1 * float(batch.robot[0, 7]))
    pairs = rr.reshape(n * A, rr.shape[2], rr.shape[3])
    coarse = reward + discount * net.forward(pairs).to(torch.float64).view(n, A)
    exact = reward + discount * net.forward(pairs, exact=True).to(torch.float64).view(n, A)
    hit = (values == coarse) | (values == exact)
    print("values off both forms: %d of %d; re-evaluated in float32: %d" % (int((~hit).sum()), hit.numel(), int((values != coarse).sum())))
    assert bool(hit.all()), (values - coarse).abs().max()
    other = _sarl_decision(0.25)[-1]
    assert float((other != values).double().mean()) > 0.9
    wrong = reward + gamma ** (0.25 * float(batch.robot[0, 7])) * net.forward(pairs).to(torch.float64).view(n, A)
    assert float((wrong - values).abs().max()) > 1e-4  # the default step's discount on the same rows would show


class _Kept(object):
    """A replay memory that keeps what collect_il pushes as it comes (float64 values)."""

    def push(self, states, values, n_valid=None):
        self.states, self.values = states.clone(), values.clone()


def test_collect_il_discounts_by_the_env_s_time_step():
    """collect_il at time_step 0.1, 16 envs, 20 steps: the values it stores are the host scan of il_value_targets (the
    torch loop) over the ORACLE's rewards with gamma ** (0.1 * v_pref), at the 1e-12 of
    test_il_targets_kernel_equals_the_host_scan; with gamma ** (0.25 * v_pref) they would not be."""
    from ebcsim.train import collect_il, il_value_targets
    c = pc.IL
    params, batch = pc.near_goal_batch(c["seed"], c["E"], 0.1, c["time_limit"])
    env = BatchedEnv(params, batch.n, batch.N, batch.S)
    env.reset(batch)
    env.use_torch_stream()
    mem = _Kept()
    stored, episodes = collect_il(env, mem, c["steps"], c["gamma"], c["safety"])
    ref = pc.il_walk()
    r, d, i = (torch.from_numpy(np.array(ref[k])) for k in ("reward", "done", "info"))
    gamma_bar = c["gamma"] ** (0.1 * float(batch.robot[0, 7]))
    values, keep = il_value_targets(r, d, gamma_bar, i)  # CPU tensors: the torch loop
    assert stored == int(keep.sum()) > 0 and episodes == int(d.sum())
    got, want = mem.values.cpu().numpy(), values.reshape(-1)[keep.reshape(-1)].numpy()
    _note("collect_il", "value", got, want)
    print("collect_il: %d values, worst |difference| %.3e" % (len(want), WORST["collect_il", "value"]))
    np.testing.assert_allclose(got, want, atol=1e-12, rtol=0)
    np.testing.assert_allclose(mem.states.cpu().numpy(), ref["state_rotated"].reshape((-1,) + ref["state_rotated"].shape[2:])
                               [keep.reshape(-1).numpy()], atol=1e-5, rtol=1e-5)
    at_default = il_value_targets(r, d, c["gamma"] ** (0.25 * float(batch.robot[0, 7])), i)[0].reshape(-1)[keep.reshape(-1)].numpy()
    assert np.abs(at_default - want).max() > 1e-3
    env.close()


def test_evaluate_counts_time_in_the_env_s_time_step():
    """evaluate at time_step 0.5, 8 envs, the robot on ORCA: avg_nav_time and the danger frequency are a plain numpy tally
    of the oracle's per-step outputs."""
    from ebcsim.train import evaluate
    c = pc.EVAL
    params, batch = pc.near_goal_batch(c["seed"], c["E"], 0.5, c["time_limit"])
    env = BatchedEnv(params, batch.n, batch.N, batch.S)
    env.reset(batch)
    env.use_torch_stream()
    act = torch.zeros((batch.n, 2), dtype=torch.float64, device=DEV)

    def demo(e):
        e.robot_orca_device(act, c["safety"])
        return act
    m = evaluate(env, demo, c["gamma"])
    p, out = pc.eval_walk()
    want = pc.eval_tally(p, out)
    print("evaluate: avg_nav_time %r (tally %r), danger frequency %r (tally %r)" % (
        m["avg_nav_time"], want["avg_nav_time"], m["Frequency of being in danger"], want["danger"]))
    assert m["success"] == want["success"] and m["timeout"] == int((want["final"] == _abi.INFO_TIMEOUT).sum())
    np.testing.assert_allclose(m["avg_nav_time"], want["avg_nav_time"], atol=1e-12, rtol=0)
    np.testing.assert_allclose(m["Frequency of being in danger"], want["danger"], atol=1e-12, rtol=0)
    env.close()


# ------------------------------------------------------------------ the figures
BEGIN, END = "# BEGIN measured on the device by tests/test_params_gpu.py", "# END measured"


def test_write_the_device_figures():
    """The worst |device - oracle| per form and output, over every set and step of the tests above, into
    profiles/param_coverage.txt between its own markers (written only when it differs; only from a whole run of this file)."""
    forms = sorted({f for f, _ in WORST})
    if not {"step linear", "step supplied", "step orca", "step cached", "lookahead", "step_k external", "step_k linear", "step_k orca",
            "sail_dagger_k", "step_with_map", "collect_il", "sarl decide"} <= set(forms):
        return  # the figures come from a whole run of this file
    lines = [BEGIN, "# worst |device - oracle| over the sets %s, every env and step (bars: float64 1e-9, rotated rows 1e-5)"
             % ", ".join(pc.SETS)]
    for f in forms:
        lines.append("%-16s %s" % (f, "  ".join("%s %.2e" % (k, v) for (ff, k), v in sorted(WORST.items()) if ff == f and v > 0) or "all equal"))
    lines.append(END)
    new = "\n".join(lines) + "\n"
    old = open(TABLE).read() if os.path.exists(TABLE) else ""
    if BEGIN in old and END in old:
        text = old[:old.index(BEGIN)] + new + old[old.index(END) + len(END) + 1:]
    else:
        text = old + new
    if text != old:
        with open(TABLE, "w") as f:
            f.write(text)
