"""The robot's own ORCA solve on more than 32 observation rows (-m gpu): orca_robot_wide_kernel (csrc/ebc_orca_wide.h)
behind ebc_robot_orca, EBC_ROBOT_ORCA of ebc_step_k and collect_il.

(1) Up to 64 rows the oracle solves the full batch: the action bit for bit.  (2) Above 64 rows, and on the hand-built
ties, the oracle solves the REDUCED batch (orca_wide_cases.reduced_batch); tests/test_robot_orca_wide_cpu.py shows on the
oracle that the reduction is exact and what the batches cover.  (3) The persistent simulator through ebc_step_k with
restarts onto scenes of other radii and row counts, against the oracle's step_k.  (4) ebc_step_k against its own
composition, byte for byte, and collect_il on top of it.  (5) The output between canaries.  (6) What is still refused."""
import numpy as np
import pytest

from ebcsim import _abi, _capi
from helpers import Guarded, orca_case_params
from orca_wide_cases import (ORACLE_RUNS, PARAM_SETS, REDUCED_CASES, SAFETIES, TIES_ROWS, full_reference, oracle_robot_orca,
                             reduced_reference, sim_batch, ties_batch, wide_batch)

pytestmark = pytest.mark.gpu

AUTO, ONE = _abi.FLAG_AUTO_RESET, _abi.FLAG_ONE_LAUNCH
KEYS = ("state_rotated", "n_rows", "robot_action_out", "reward", "done", "info", "dmin", "dist_to_goal", "obs_rotated")


def _env(params, E, N, S):
    from ebcsim.batched import BatchedEnv
    return BatchedEnv(params, E, N, S)


def _bitwise(got, want, tag):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, tag
    bad = np.flatnonzero((got.reshape(len(got), -1).view(np.uint8) != want.reshape(len(want), -1).view(np.uint8)).any(-1))
    assert not len(bad), "%s: %d of %d differ, the first at %d: %r / %r" % (tag, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]])


# ------------------------------------------------------------------ 1. the oracle on the full batch
@pytest.mark.parametrize("safety", SAFETIES)
@pytest.mark.parametrize("case,ps", ORACLE_RUNS, ids=lambda v: v if isinstance(v, str) else "N%d-S%d" % v)
def test_full_batch_vs_oracle(case, ps, safety):
    N, S = case
    b, params = wide_batch(N, S), orca_case_params(0, ps)
    want = oracle_robot_orca(b, params, safety) if ps == "all" else full_reference(N, S, ps, safety)
    g = _env(params, b.n, N, S)
    g.reset(b)
    _bitwise(g.robot_orca(safety), want, "N %d S %d %s safety %g" % (N, S, ps, safety))
    g.close()


# ------------------------------------------------------------------ 2. the oracle on the reduced batch
@pytest.mark.parametrize("safety", SAFETIES)
@pytest.mark.parametrize("ps", PARAM_SETS)
@pytest.mark.parametrize("case", REDUCED_CASES, ids=lambda c: "N%d-S%d" % c)
def test_reduced_batch_vs_oracle(case, ps, safety):
    N, S = case
    b, params = wide_batch(N, S), orca_case_params(0, ps)
    g = _env(params, b.n, N, S)
    g.reset(b)
    _bitwise(g.robot_orca(safety), reduced_reference(case, b, ps, safety), "N %d S %d %s safety %g" % (N, S, ps, safety))
    g.close()


@pytest.mark.parametrize("safety", SAFETIES)
@pytest.mark.parametrize("R", TIES_ROWS)
def test_ties_vs_oracle(R, safety):
    b, params = ties_batch(R), orca_case_params(0, "default")
    g = _env(params, b.n, b.N, b.S)
    g.reset(b)
    _bitwise(g.robot_orca(safety), reduced_reference(("ties", R), b, "default", safety), "ties R %d safety %g" % (R, safety))
    g.close()


# ------------------------------------------------------------------ 3. the persistent simulator
def _sim_setup(E=9, N=14, S=30):
    params = orca_case_params(0, "default")
    params.time_limit = 1.0  # four steps: every env restarts three times inside a window of 12
    rs = np.random.RandomState(4410)
    return params, E, N, S, sim_batch(rs, E, N, S), sim_batch(rs, 3 * E, N, S)


def test_persistent_simulator_vs_oracle_step_k():
    """K = 12 steps with the robot on ORCA and auto-reset over a pool whose scenes differ in radii and row counts: a
    restart onto another row count rebuilds the env's simulator, one onto the same count keeps the radii it was built
    with.  The robot's action bit for bit, done / info / n_rows exactly, the rest at the project's tolerances."""
    from oracle import oracle
    params, E, N, S, first, pool = _sim_setup()
    K = 12
    g, o = _env(params, E, N, S), oracle.OracleEnv(params, E, N, S)
    for x in (g, o):
        x.reset(first)
        x.set_scene_pool(pool)
        x.robot_orca_sim(True)
    kw = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA, robot_safety_space=0.15, flags=AUTO)
    og, oo = g.step_k(K, KEYS, **kw), o.step_k(K, KEYS, **kw)
    rows = oo["n_rows"]
    assert (rows > 32).all()
    restarted = oo["done"][:-1].astype(bool)
    rebuilt, kept = restarted & (rows[1:] != rows[:-1]), restarted & (rows[1:] == rows[:-1])
    assert int(rebuilt.sum()) >= 3 and int(kept.sum()) >= 3, (int(rebuilt.sum()), int(kept.sum()))
    for k in ("done", "info", "n_rows"):
        np.testing.assert_array_equal(og[k], oo[k], err_msg=k)
    _bitwise(og["robot_action_out"], oo["robot_action_out"], "robot_action_out")
    for k in ("reward", "dmin", "dist_to_goal"):
        both_inf = np.isinf(og[k]) & np.isinf(oo[k])
        np.testing.assert_allclose(np.where(both_inf, 0, og[k]), np.where(both_inf, 0, oo[k]), atol=1e-9, rtol=0, err_msg=k)
    for k in ("state_rotated", "obs_rotated"):
        np.testing.assert_allclose(og[k], oo[k], atol=1e-5, rtol=1e-5, err_msg=k)
    sg, so = g.get_state(), o.get_state()
    for k in sg:
        np.testing.assert_allclose(sg[k], so[k], atol=1e-9, rtol=0, err_msg=k)
    mg, mo = g.robot_orca_sim_state(), o.robot_orca_sim_state()
    np.testing.assert_array_equal(mg["rows"], mo["rows"])
    _bitwise(mg["self"], mo["self"], "simulator self")
    for e in range(E):  # the rows the simulator holds; what lies behind them is never read
        _bitwise(mg["radius"][e, :mo["rows"][e]], mo["radius"][e, :mo["rows"][e]], "simulator radius of env %d" % e)
    # set / read round trip on the wide handle
    rs = np.random.RandomState(5)
    state = dict(rows=rs.randint(-1, N + S + 1, E).astype(np.int32), radius=rs.uniform(0.1, 1, (E, N + S)).astype(np.float32),
                 self=rs.uniform(0.1, 1, (E, 2)).astype(np.float32))
    g.robot_orca_sim_state(state)
    back = g.robot_orca_sim_state()
    for k in state:
        _bitwise(back[k], state[k], "round trip " + k)
    g.close()


# ------------------------------------------------------------------ 4. step_k and its composition
def _composed(env, K, safety):
    """K times [state, row counts, robot_orca_device, step_device]: the outputs of ebc_step_k, stacked."""
    import torch
    dev = torch.device("cuda", 0)
    out = {k: [] for k in KEYS}
    for _ in range(K):
        s = torch.empty((env.E, env.R, env.T), dtype=torch.float32, device=dev)
        env.observe_device(s)
        n = torch.empty((env.E,), dtype=torch.int64, device=dev)
        env.row_counts_device(n)
        act = torch.empty((env.E, 2), dtype=torch.float64, device=dev)
        env.robot_orca_device(act, safety)
        o = env.alloc_step_outputs(("reward", "done", "info", "dmin", "dist_to_goal", "obs_rotated"))
        env.step_device(o, robot_action=act, human_policy=_abi.HUMAN_ORCA, flags=AUTO)
        o.update(state_rotated=s, n_rows=n, robot_action_out=act)
        for k in KEYS:
            out[k].append(o[k])
    env.synchronize()
    return {k: torch.stack(v) for k, v in out.items()}


@pytest.mark.parametrize("persistent", [True, False])
def test_step_k_equals_its_composition(persistent):
    import torch
    params, E, N, S, first, pool = _sim_setup()
    K = 12
    envs = []
    for _ in range(2):
        g = _env(params, E, N, S)
        g.reset(first)
        g.set_scene_pool(pool)
        g.use_torch_stream()
        g.robot_orca_sim(persistent)
        envs.append(g)
    a, b = envs
    outs = a.alloc_step_k_outputs(K, KEYS)
    a.step_k_device(outs, K, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA, flags=AUTO, robot_safety_space=0.15)
    a.synchronize()
    want = _composed(b, K, 0.15)
    assert int(outs["done"].sum()) >= E
    for k in KEYS:
        assert torch.equal(outs[k].view(torch.uint8), want[k].view(torch.uint8)), k
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        _bitwise(sa[k], sb[k], "state " + k)
    if persistent:
        ma, mb = a.robot_orca_sim_state(), b.robot_orca_sim_state()
        for k in ma:
            _bitwise(ma[k], mb[k], "simulator " + k)
    a.close()
    b.close()


def test_collect_il_fills_the_memory_of_the_composition():
    """collect_il on 4 envs x 6 steps at (14, 30): the replay's states, values and row counts are those of the
    composition of robot_orca_device and step_device on a twin handle."""
    import torch
    from ebcsim.sarl import uniform_v_pref
    from ebcsim.train import DeviceReplay, collect_il, il_value_targets
    params, _, N, S, first, pool = _sim_setup()
    E, steps, gamma, safety = 4, 6, 0.9, 0.15
    from helpers import batch_rows
    first = batch_rows(first, np.arange(E))
    dev = torch.device("cuda", 0)
    envs, mems = [], []
    for _ in range(2):
        g = _env(params, E, N, S)
        g.reset(first)
        g.set_scene_pool(pool)
        g.use_torch_stream()
        envs.append(g)
        mems.append(DeviceReplay(steps * E, g.R, g.T, dev))
    a, b = envs
    stored, ended = collect_il(a, mems[0], steps, gamma, safety)
    b.robot_orca_sim(True)
    c = _composed(b, steps, safety)
    values, keep = il_value_targets(c["reward"], c["done"], gamma ** (params.time_step * uniform_v_pref(b)), c["info"])
    keep = keep.reshape(-1)
    mems[1].push(c["state_rotated"].reshape(steps * E, b.R, b.T)[keep], values.reshape(-1)[keep], c["n_rows"].reshape(-1)[keep])
    assert stored == int(keep.sum()) > 0 and ended > 0 and len(mems[0]) == len(mems[1]) == stored
    n = stored
    assert torch.equal(mems[0].states[:n], mems[1].states[:n])
    assert torch.equal(mems[0].values[:n], mems[1].values[:n])
    assert torch.equal(mems[0].n_valid[:n], mems[1].n_valid[:n])
    assert int(mems[0].n_valid[:n].max()) > 32
    a.close()
    b.close()


# ------------------------------------------------------------------ 5. the output between canaries
@pytest.mark.parametrize("case", [(14, 30), (33, 95)], ids=lambda c: "N%d-S%d" % c)
def test_output_between_canaries(case):
    import torch
    N, S = case
    b, params = wide_batch(N, S), orca_case_params(0, "default")
    g = _env(params, b.n, N, S)
    g.reset(b)
    g.use_torch_stream()
    out = Guarded((b.n, 2), torch.float64)
    g.robot_orca_device(out.t, 0.15)
    g.synchronize()
    got = out.check()  # both canaries intact, every element written
    _bitwise(got, reduced_reference(case, b, "default", 0.15), "N %d S %d" % case)
    g.close()


# ------------------------------------------------------------------ 6. what is still refused
def _refused(call, code, words):
    with pytest.raises(_capi.EbcError) as err:
        call()
    assert err.value.code == code and words in str(err.value), (err.value.code, str(err.value))


def test_refusals():
    import torch
    N, S = 14, 30
    b, params = wide_batch(N, S), orca_case_params(0, "default")
    g = _env(params, b.n, N, S)
    g.reset(b)
    g.use_torch_stream()
    before = g.get_state()
    K = 2
    outs = {k: Guarded((K,) + tuple(v.shape[1:]), v.dtype) for k, v in g.alloc_step_k_outputs(K, ("reward", "done", "robot_action_out")).items()}
    tensors = {k: v.t for k, v in outs.items()}
    kw = dict(human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA, robot_safety_space=0.15)
    _refused(lambda: g.step_k_device(tensors, K, flags=ONE, **kw), _abi.ERR_UNSUPPORTED, "more than 32 observation rows")
    _refused(lambda: g.step_k(K, ("reward",), flags=ONE | AUTO, **kw), _abi.ERR_UNSUPPORTED, "more than 32 observation rows")
    act = Guarded((b.n, 2), torch.float64)
    for bad in (-0.1, float("nan")):
        _refused(lambda: g.robot_orca_device(act.t, bad), _abi.ERR_INVALID, "safety_space")
        _refused(lambda: g.step_k_device(tensors, K, flags=0, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_ORCA,
                                         robot_safety_space=bad), _abi.ERR_INVALID, "safety_space")
    g.synchronize()
    for v in list(outs.values()) + [act]:
        v.check(written=False)  # nothing was enqueued
    after = g.get_state()
    for k in before:
        _bitwise(after[k], before[k], "state after the refusals, " + k)
    # the one-launch form with another robot policy still runs on the wide handle
    lin = g.step_k(K, ("reward", "done"), human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=ONE)
    g2 = _env(params, b.n, N, S)
    g2.reset(b)
    per = g2.step_k(K, ("reward", "done"), human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=0)
    for k in lin:
        _bitwise(lin[k], per[k], "one launch, linear robot, " + k)
    g.close()
    g2.close()
    # a unicycle robot has no ORCA demonstrator, wide or not
    uni = orca_case_params(0, "default")
    uni.robot_kinematics = _abi.UNICYCLE
    u = _env(uni, b.n, N, S)
    u.reset(b)
    _refused(lambda: u.robot_orca(0.15), _abi.ERR_UNSUPPORTED, "holonomic robots only")
    u.close()
