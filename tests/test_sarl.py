"""Robot decisions = look-ahead sweep + SARL value network.  Golden: the
reference's own SARL policy (its shipped weights) driving full episodes, 81 action values per
decision (tests/golden/sarl_*.npz, humans on the oracle-substituted rvo2).  Values are float32
network outputs on O(1) numbers: 5e-5 absolute (observed <= 1.5e-5 with the split-bf16 matrix-core
blocks); EVERY decision must pick the reference's action (counted per episode)."""
import json
import os

import numpy as np
import pytest
import torch

from ebcsim import _abi
from ebcsim.sarl import DeviceSarlPolicy, SarlValueNet, reference_choice
from helpers import GOLDEN, Guarded, batch_from_init, load, params_of, reference_rule

# the last three are the reference's remaining known-answer runs (tests/run_tests.py:23-41): test_basic_simulation on
# two more configs (bicycles; bicycles + a static map) and test_scene_simulation on the frozen 10-obstacle scene
RUNS = ["sarl_a5_baseline", "sarl_n10_ebcadrl", "sarl_a3b3s2_baseline", "sarl_a3b3_baseline",
        "sarl_scene_a3b3s10_baseline"]
TOL = 5e-5


def _check_values(values, z, t):
    """-> 1 when the decision picks the reference's action"""
    ref = z["values"][t]
    np.testing.assert_allclose(values, ref, atol=TOL, rtol=0, err_msg="decision %d" % t)
    best = int(np.argmax(values))
    chosen = int(np.where((z["action_space"] == z["action"][t]).all(1))[0][0])
    return int(best == chosen)


@pytest.mark.parametrize("name", RUNS)
def test_sarl_values_cpu(name):
    """SarlValueNet (torch, CPU) on the oracle's look-ahead rows."""
    from oracle import oracle
    z = load(name)
    meta = json.loads(str(z["meta"]))
    params = params_of(z)
    b = batch_from_init(z)
    env = oracle.OracleEnv(params, 1, b.N, b.S)
    env.reset(b)
    net = SarlValueNet.load(os.path.join(GOLDEN, "weights", meta["weights"]))
    pol = DeviceSarlPolicy(net, z["action_space"], meta["gamma"])
    v_pref = float(b.robot[0, 7])
    steps = len(z["action"]) if name in RUNS[2:] else min(len(z["action"]), 40)  # the known-answer runs: to the goal
    agree = decided = 0
    for t in range(steps):
        la = env.lookahead(z["action_space"], human_policy=_abi.HUMAN_ORCA)
        if not np.isnan(z["values"][t]).any():
            vals = pol.values_from(torch.from_numpy(la["rows_rotated"]), torch.from_numpy(la["reward"]),
                                   None, params.time_step, v_pref)
            agree += _check_values(vals[0].numpy(), z, t)
            decided += 1
        out = env.step(robot_action=z["action"][t][None], human_policy=_abi.HUMAN_CACHED)
        assert int(out["info"][0]) == int(z["info"][t])
    assert agree == decided, (agree, decided)
    if steps == len(z["action"]):  # pass criterion of the reference's test: terminal class ReachGoal
        assert bool(out["done"][0]) and int(out["info"][0]) == _abi.INFO_REACH_GOAL


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUNS)
def test_sarl_decisions_gpu(name):
    """The whole decision on device: ebc_lookahead -> torch GEMMs -> argmax -> cached step."""
    from ebcsim.batched import BatchedEnv
    z = load(name)
    meta = json.loads(str(z["meta"]))
    params = params_of(z)
    E = 5
    b = batch_from_init(z, copies=E)
    env = BatchedEnv(params, E, b.N, b.S)
    env.reset(b)
    env.use_torch_stream()
    net = SarlValueNet.load(os.path.join(GOLDEN, "weights", meta["weights"]), device="cuda:0")
    pol = DeviceSarlPolicy(net, z["action_space"], meta["gamma"])
    outs = env.alloc_step_outputs(("reward", "done", "info"))
    agree = decided = 0
    for t in range(len(z["action"])):
        actions, values = pol.decide(env)
        torch.cuda.synchronize()
        v = values.cpu().numpy()
        assert (np.abs(v - v[0:1]) < 1e-5).all()
        if not np.isnan(z["values"][t]).any():
            agree += _check_values(v[0], z, t)
            decided += 1
        forced = torch.tensor(np.tile(z["action"][t], (E, 1)), dtype=torch.float64, device="cuda:0")
        env.step_device(outs, robot_action=forced, human_policy=_abi.HUMAN_CACHED)
        torch.cuda.synchronize()
        assert int(outs["info"][0]) == int(z["info"][t]), t
        np.testing.assert_allclose(float(outs["reward"][0]), z["reward"][t], atol=1e-9)
    assert int(z["info"][-1]) == _abi.INFO_REACH_GOAL
    assert agree == decided, (agree, decided)  # every decision of the episode picks the reference's action
    # the values above came from the HIP value-network kernels, not from a torch stand-in
    assert net._native_blocks(), "the value network did not run on the MFMA blocks"
    assert getattr(net, "native_forwards", 0) >= decided


def _ragged_pool_decisions(make_env, device, check_rows):
    """A scene pool whose scenes differ in size: after restarts the rows the policy masks with must be the
    CURRENT scene's (read from the device state at every decision), and its values must equal the network
    run on exactly the rows that exist."""
    z = load("sarl_a5_baseline")
    meta = json.loads(str(z["meta"]))
    params = params_of(z)
    params.time_limit = 1  # every env times out at step 4: restarts come quickly
    E = 4
    b = batch_from_init(z, copies=E)
    pool = batch_from_init(z, copies=2 * E)
    for c in range(2 * E):
        pool.n_humans[c] = 5 - (c % 3)       # 5, 4, 3 humans
        pool.px[c, pool.n_humans[c]:] = 0
    env = make_env(params, E, b.N, b.S)
    env.reset(b)
    env.set_scene_pool(pool, stride=E)
    env.use_torch_stream()
    net = SarlValueNet.load(os.path.join(GOLDEN, "weights", meta["weights"]), device=device)
    pol = DeviceSarlPolicy(net, z["action_space"], meta["gamma"])
    outs = env.alloc_step_outputs(("reward", "done", "info"))
    seen = set()
    for t in range(14):
        actions, values = pol.decide(env)
        rows = check_rows(env)
        assert env.ragged and pol.n_valid is not None
        np.testing.assert_array_equal(pol.n_valid.cpu().numpy(), rows)
        seen.update(rows.tolist())
        # the masked batch forward == the network on the rows that exist, env by env
        rr = pol._bufs["rows_rotated"]
        for e in range(E):
            alone = net.forward(rr[e, :, :int(rows[e])].contiguous()).to(torch.float64)
            full = (values[e] - pol._bufs["reward"][e]) / (meta["gamma"] ** (params.time_step * pol._v_pref))
            np.testing.assert_allclose(full.cpu().numpy(), alone.cpu().numpy(), atol=2e-5)
        env.step_device(outs, robot_action=actions.contiguous(), human_policy=_abi.HUMAN_CACHED, flags=_abi.FLAG_AUTO_RESET)
    assert seen == {3, 4, 5}  # the walk went through scenes of every size


def test_ragged_pool_row_counts_follow_restarts_cpu():
    from helpers import CpuDeviceEnv
    _ragged_pool_decisions(CpuDeviceEnv, "cpu", lambda env: env._o.row_counts())


@pytest.mark.gpu
def test_ragged_pool_row_counts_follow_restarts_gpu():
    from ebcsim.batched import BatchedEnv
    _ragged_pool_decisions(lambda p, E, N, S: BatchedEnv(p, E, N, S), "cuda:0", lambda env: env.row_counts())


@pytest.mark.gpu
def test_evaluate_reports_the_reference_metrics():
    """Explorer.run_k_episodes' statistics (explorer.py:202-330) from one batched pass: the shipped SARL
    weights on the golden episode's scene reach the goal in the golden episode's time, with its
    discounted reward; and the imitation-learning demonstrator through the same function."""
    from ebcsim.batched import BatchedEnv
    from ebcsim.train import evaluate
    z = load("sarl_a5_baseline")
    meta = json.loads(str(z["meta"]))
    params = params_of(z)
    E = 6
    b = batch_from_init(z, copies=E)
    env = BatchedEnv(params, E, b.N, b.S)
    env.reset(b)
    env.use_torch_stream()
    net = SarlValueNet.load(os.path.join(GOLDEN, "weights", meta["weights"]), device="cuda:0")
    pol = DeviceSarlPolicy(net, z["action_space"], meta["gamma"])
    m = evaluate(env, lambda e: pol.decide(e)[0], meta["gamma"], human_policy=_abi.HUMAN_CACHED)
    T = len(z["action"])
    assert m["success_rate"] == 1.0 and m["success"] == E and m["timeout"] == 0 and m["num_episodes"] == E
    assert abs(m["avg_nav_time"] - T * params.time_step) <= 2 * params.time_step
    gb = meta["gamma"] ** (params.time_step * float(b.robot[0, 7]))
    ref_total = float(sum(gb ** t * r for t, r in enumerate(z["reward"])))
    assert abs(m["total_reward:"] - ref_total) < 0.05
    danger_steps = int((z["info"] == _abi.INFO_DANGER).sum())
    if abs(m["avg_nav_time"] - T * params.time_step) < 1e-9:
        np.testing.assert_allclose(m["Frequency of being in danger"], danger_steps / T, atol=1e-9)
    # the demonstrator (robot on ORCA): every episode ends, the rates add up to one
    env.reset(b)
    act = torch.zeros((E, 2), dtype=torch.float64, device="cuda:0")

    def demo(e):
        e.robot_orca_device(act, 0.15)
        return act
    d = evaluate(env, demo, meta["gamma"])
    total = (d["success_rate"] + d["collision_rate_adult"] + d["collision_rate_bicycle"] + d["collision_rate_child"]
             + d["collision_rate_obstacle"] + d["timeout"] / E)
    assert abs(total - 1.0) < 1e-12


@pytest.mark.gpu
def test_decisions_are_the_float32_decisions_on_the_bench_workload():
    """Where the split-bf16 error is largest (the shipped eb-cadrl weights: large attention scores) and the batch is the
    bench's: 1024 envs x 81 actions x 18 rows at three points of the episodes.  (a) The matrix-core values stay within
    the bound the refinement is built on (SarlValueNet.COARSE_EPS); (b) after the bound-driven refinement EVERY env
    takes the float32 network's action (multi_human_rl.py:61-80 maximises float32 values) and (c) the refined values
    are float32-GEMM-grade (2e-6 of torch's float32 GEMMs); (d) the refinement ran inside the library
    (ebc_mlp2_forward_f32), not through torch."""
    import bench
    from ebcsim import actions as ebc_actions
    from ebcsim.batched import BatchedEnv
    dev = torch.device("cuda", 0)
    E = 1024
    params, batch = bench.build_batch("metric", E, 0)
    env = BatchedEnv(params, E, batch.N, batch.S)
    env.reset(batch)
    env.use_torch_stream()
    space = ebc_actions.build_action_space(float(batch.robot[0, 7]))
    acts = torch.tensor(space, dtype=torch.float64, device=dev)
    A = len(space)
    outs = env.alloc_step_outputs(("reward", "done"))
    net = SarlValueNet.load(os.path.join(GOLDEN, "weights", "sarl_n10_ebcadrl.pth"), device=str(dev))
    net64 = SarlValueNet.load(os.path.join(GOLDEN, "weights", "sarl_n10_ebcadrl.pth"), device=str(dev), dtype=torch.float64)
    bufs = env.alloc_lookahead_outputs(A, ("reward", "done", "info", "rows_rotated"))
    worst_coarse = worst_refined = worst_native64 = worst_torch64 = 0.0
    for point in range(3):
        for _ in range(10 * point):
            env.step_device(outs, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=_abi.FLAG_AUTO_RESET)
        env.lookahead_device(acts, bufs, human_policy=_abi.HUMAN_ORCA)
        rows, reward = bufs["rows_rotated"], bufs["reward"]
        net.native_exact = False  # the yard-stick: torch's float32 GEMMs
        f32 = torch.empty((E, A), dtype=torch.float32, device=dev)
        for e0 in range(0, E, 128):
            f32[e0:e0 + 128] = net.forward(rows[e0:e0 + 128].reshape(-1, env.R, env.T), exact=True).view(-1, A)
        net.native_exact = True
        want = reward + 0.9 * f32.double()
        coarse = net.action_values(rows, reward, 0.9, refine=0)
        before = getattr(net, "native_exact_forwards", 0)
        got = net.action_values(rows, reward, 0.9)
        torch.cuda.synchronize()
        assert net.native_exact_forwards > before
        worst_coarse = max(worst_coarse, float((coarse - want).abs().max()) / 0.9)
        changed = got != coarse
        worst_refined = max(worst_refined, float((got - want).abs()[changed].max()))
        # the yard-stick of both float32 forms: the same network in float64 on the refined candidates
        ei, ai = torch.nonzero(changed, as_tuple=True)
        truth = reward[ei, ai] + 0.9 * net64.forward(rows[ei, ai]).double()
        worst_native64 = max(worst_native64, float((got[ei, ai] - truth).abs().max()))
        worst_torch64 = max(worst_torch64, float((want[ei, ai] - truth).abs().max()))
        assert int((got.argmax(1) == want.argmax(1)).sum()) == E, point
    assert worst_coarse <= net.coarse_eps, (worst_coarse, net.coarse_eps)  # the measured bound the refinement set is built on
    # float32-GEMM-grade: as close to the float64 network as torch's float32 GEMMs are (two float32 evaluations of this
    # network differ by ~2e-6 from one another: its attention scores are large)
    assert worst_native64 <= max(1.5 * worst_torch64, 2e-6), (worst_native64, worst_torch64)
    assert worst_refined <= 5e-6, worst_refined
    st = net.refine_stats
    assert st["capped"] == 0 and st["decisions"] == 3 * E and st["bound_violations"] == 0
    print("refinement: %.2f candidates per decision, %d of %d decisions with more than 2, largest set %d; coarse error %.2e; "
          "refined vs torch float32 %.2e; vs the float64 network: native %.2e, torch float32 %.2e" % (
              st["candidates"] / st["decisions"], st["over2"], st["decisions"], st["max_set"], worst_coarse, worst_refined,
              worst_native64, worst_torch64))


@pytest.mark.gpu
def test_chunks_on_two_streams_give_the_values_of_one_stream():
    """action_values spreads the chunks of a decision batch over two streams (one chunk's small per-pair kernels beside
    the other's wide ones): every value must be the value of the single-stream pass, bit for bit — a pair's result does
    not depend on where its rows lie in a batch — and the caller's stream must see them complete."""
    import torch
    from ebcsim.sarl import SarlValueNet
    dev = torch.device("cuda", 0)
    net = SarlValueNet.load(os.path.join(GOLDEN, "weights", "sarl_n10_ebcadrl.pth"), device=str(dev))
    g = torch.Generator().manual_seed(21)
    E, A, R, T = 37, 81, 18, 17
    rows = torch.randn(E, A, R, T, generator=g).to(dev)
    rows[..., 13:] = 0
    rows[..., 13] = 1
    reward = torch.randn(E, A, generator=g, dtype=torch.float64).to(dev)
    nv = torch.randint(12, R + 1, (E,), generator=g).to(dev)
    out = {}
    for streams in (1, 2):
        net.CHUNK_STREAMS = streams
        for _ in range(2):  # the second pass re-uses the streams and the allocator's blocks of the first
            out[streams] = net.action_values(rows, reward, 0.9, n_valid=nv, refine=0, chunk_pairs=5 * A)
    assert torch.equal(out[1], out[2])
    assert bool(torch.isfinite(out[2]).all())


def test_batches_whose_robots_differ_in_v_pref_are_refused():
    """One action space and one discount gamma^(dt v_pref) per batch (the reference has them per robot,
    multi_human_rl.py:36-60, 72-76): a batch of robots with different v_pref must not silently take env 0's."""
    from ebcsim.sarl import uniform_v_pref

    class Env:
        def __init__(self, v):
            self.v = v

        def get_state(self):
            robot = np.zeros((len(self.v), 9))
            robot[:, 7] = self.v
            return {"robot": robot}
    assert uniform_v_pref(Env([1.0, 1.0, 1.0])) == 1.0
    with pytest.raises(ValueError, match="v_pref"):
        uniform_v_pref(Env([1.0, 1.2, 1.0]))


def _rank(v, reward, discount, bound, E=None, A=None):
    """ebc_decision_rank into guarded outputs -> (return code, values, order, count) as Guarded buffers.  v / reward:
    tensors, or Guarded ones (whose address is valid also when they are empty)."""
    from ebcsim import _capi
    E, A = v.shape if E is None else (E, A)
    ptr = lambda b: b.ptr if isinstance(b, Guarded) else b.data_ptr()  # noqa: E731
    out = (Guarded((E, A), torch.float64), Guarded((E, A), torch.int32), Guarded((E,), torch.int32))
    rc = _capi.lib().ebc_decision_rank(torch.cuda.current_stream().cuda_stream, ptr(v), ptr(reward), discount, bound, E, A,
                                       out[0].ptr, out[1].ptr, out[2].ptr)
    return (rc,) + out


def _rank_ref(v, reward, discount, bound):
    """ebc_decision_rank's contract in float64 numpy, env by env: the values; the actions by value (equal values: lower
    index first), NaNs last in index order; the near-best count over the non-NaN values, -1 for a row with a NaN or
    no value above -inf."""
    vals = reward.cpu().numpy() + discount * v.cpu().numpy().astype(np.float64)
    E, A = vals.shape
    order = np.zeros((E, A), np.int64)
    count = np.zeros(E, np.int64)
    for e in range(E):
        row = vals[e]
        num = np.nonzero(~np.isnan(row))[0]
        order[e] = np.concatenate([num[np.lexsort((num, -row[num]))], np.nonzero(np.isnan(row))[0]])
        best = row[num].max() if len(num) else -np.inf
        count[e] = -1 if (len(num) < A or not best > -np.inf) else int((row >= best - bound).sum())
    return vals, order, count


@pytest.mark.gpu
def test_decision_rank_kernel_against_torch():
    """ebc_decision_rank (one launch: values, every env's actions by value, the size of the near-best set) against the
    torch expressions it replaces: the same float64 values bit for bit, a permutation per env that sorts them (equal
    values: the lower action first), the same counts — with exact ties in the rows; every output guarded and written."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    for E, A in ((1024, 81), (3, 1), (17, 200), (1, 1024), (33, 17)):
        v = torch.randn(E, A, generator=g)
        v[:, A // 2] = v[:, 0]                      # an exact tie in every row
        reward = torch.randn(E, A, generator=g, dtype=torch.float64) * 0.1
        reward[:, A // 2] = reward[:, 0]
        v, reward = v.to(dev), reward.to(dev)
        discount, bound = 0.9 ** 0.25, 0.05
        rc, gv, go, gc = _rank(v, reward, discount, bound)
        assert rc == 0
        torch.cuda.synchronize()
        for buf in (gv, go, gc):
            buf.check()
        values, order, count = gv.t, go.t, gc.t
        ref = reward + discount * v.to(torch.float64)
        assert torch.equal(values, ref)
        o = order.to(torch.int64)
        assert torch.equal(o.sort(1).values, torch.arange(A, device=dev).expand(E, A))
        ranked = ref.gather(1, o)
        assert bool((ranked[:, 1:] <= ranked[:, :-1]).all())
        tie = ranked[:, 1:] == ranked[:, :-1]
        assert bool((o[:, 1:][tie] > o[:, :-1][tie]).all()) and int(tie.sum()) >= (E if A > 1 else 0)
        assert torch.equal(count.to(torch.int64), (ref >= (ref.max(1, keepdim=True).values - bound)).sum(1))


@pytest.mark.gpu
def test_decision_rank_kernel_edges():
    """ebc_decision_rank on rows with NaN, +inf and -inf (at index 0 too), all-NaN and all -inf rows, A = 1 and 1024,
    E = 0, against its contract restated in float64 numpy: `order` is always a permutation, NaNs rank last in index
    order, the best value and the count are over the non-NaN values, and a row the values cannot rank (a NaN in it, or
    none above -inf) has count -1 — every action a candidate.  A = 1025 is refused and nothing is written."""
    dev = torch.device("cuda", 0)
    nan, inf = float("nan"), float("inf")
    g = torch.Generator().manual_seed(51)
    for E, A in ((64, 81), (6, 1), (4, 1024), (9, 2)):
        v = torch.randn(E, A, generator=g)
        v[torch.rand(E, A, generator=g) < 0.03] = nan
        v[torch.rand(E, A, generator=g) < 0.03] = inf
        v[torch.rand(E, A, generator=g) < 0.03] = -inf
        reward = (torch.randn(E, A, generator=g, dtype=torch.float64) * 0.1)
        specials = [[nan], [inf], [-inf], [nan] * A, [-inf] * A, [inf, 0.5, inf], [-inf, nan, 1.0], [0.25, nan],
                    [-inf, -inf, 2.0, 2.0]]
        for e, row in enumerate(specials[:E]):
            v[e] = 0.0
            v[e, :min(len(row), A)] = torch.tensor(row[:A])
            reward[e] = 0.0
        if E > len(specials):
            v[len(specials), ::3] = v[len(specials), 0]  # exact ties around NaNs
            reward[len(specials), ::3] = reward[len(specials), 0]
            reward[len(specials) + 1, 1] = -inf         # an infinity from the reward
        v, reward = v.to(dev), reward.to(dev)
        for bound in (0.0, 0.05, 3.0):
            rc, gv, go, gc = _rank(v, reward, 0.9, bound)
            assert rc == 0
            torch.cuda.synchronize()
            values, order, count = gv.check(), go.check(), gc.check()
            want_v, want_o, want_c = _rank_ref(v, reward, 0.9, bound)
            assert np.array_equal(values, want_v, equal_nan=True)
            assert (np.sort(order, 1) == np.arange(A)).all()
            assert np.array_equal(order, want_o), (E, A, bound)
            assert np.array_equal(count, want_c), (E, A, bound, count, want_c)
    # E = 0: nothing to do, nothing written; A = 1025 refused, nothing written
    v = Guarded((0, 81), torch.float32, poison=False)
    r = Guarded((0, 81), torch.float64, poison=False)
    rc, gv, go, gc = _rank(v, r, 0.9, 0.1, 0, 81)
    assert rc == 0
    torch.cuda.synchronize()
    for buf in (gv, go, gc):
        buf.check(written=True)  # nothing to write: the canaries are what is checked
    v1025, r1025 = torch.zeros((2, 1025), device=dev), torch.zeros((2, 1025), dtype=torch.float64, device=dev)
    rc, gv, go, gc = _rank(v1025, r1025, 0.9, 0.1)
    assert rc == _abi.ERR_INVALID
    rc_nan, _, _, _ = _rank(v1025[:, :81].contiguous(), r1025[:, :81].contiguous(), 0.9, nan)
    assert rc_nan == _abi.ERR_INVALID  # a NaN bound is refused
    torch.cuda.synchronize()
    for buf in (gv, go, gc):
        buf.check(written=False)


def _apply(exact, v, env_i, act_i, reward, values, discount=0.9):
    """ebc_decision_apply into guarded `values` (a copy of the given ones) and `worst` (zeroed) -> (rc, values, worst).
    env_i / act_i: tensors, or one Guarded empty buffer for both (n = 0 with valid addresses)."""
    from ebcsim import _capi
    E, A = v.shape
    n = 0 if isinstance(env_i, Guarded) else int(env_i.shape[0])
    ptr = lambda b: b.ptr if isinstance(b, Guarded) else b.data_ptr()  # noqa: E731
    gv = Guarded((E, A), torch.float64, poison=False)
    gv.t.copy_(values)
    gw = Guarded((1,), torch.float32, poison=False)
    gw.t.zero_()
    rc = _capi.lib().ebc_decision_apply(torch.cuda.current_stream().cuda_stream, exact.data_ptr(), v.data_ptr(), ptr(env_i),
                                        ptr(act_i), reward.data_ptr(), discount, A, n, gv.ptr, gw.ptr)
    torch.cuda.synchronize()
    return rc, gv.check(), float(gw.check()[0])


@pytest.mark.gpu
def test_decision_apply_kernel_against_torch():
    """ebc_decision_apply against the torch expressions it replaces: the candidates' values written where they belong
    (bit for bit reward + discount * exact), everything else untouched, and the largest |exact - coarse| among them."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(6)
    E, A = 300, 81
    v = torch.randn(E, A, generator=g).to(dev)
    reward = (torch.randn(E, A, generator=g, dtype=torch.float64) * 0.1).to(dev)
    for n in (1, 77, 5000, E * A):
        flat = torch.randperm(E * A, generator=g)[:n].sort().values.to(dev)
        env_i, act_i = flat // A, flat % A
        exact = (v[env_i, act_i] + 1e-3 * torch.randn(n, generator=g).to(dev)).contiguous()
        values = (reward + 0.9 * v.to(torch.float64)).contiguous()
        ref = values.clone()
        ref[env_i, act_i] = reward[env_i, act_i] + 0.9 * exact.to(torch.float64)
        rc, got, worst = _apply(exact, v, env_i, act_i, reward, values)
        assert rc == 0
        assert np.array_equal(got, ref.cpu().numpy())
        assert worst == float((exact - v[env_i, act_i]).abs().max())


@pytest.mark.gpu
def test_decision_apply_kernel_edges():
    """ebc_decision_apply where the values are not finite: a pair that is NaN in both forms, or the same infinity, is no
    error; every other pair with a NaN in it (NaN against a number, either way round) makes `worst` a NaN, above every
    bound; opposite infinities, or an infinity against a number, differ by inf.  n = 0 writes nothing."""
    dev = torch.device("cuda", 0)
    nan, inf = float("nan"), float("inf")
    g = torch.Generator().manual_seed(61)
    E, A = 40, 81
    v = torch.randn(E, A, generator=g)
    reward = torch.randn(E, A, generator=g, dtype=torch.float64) * 0.1
    n = 600
    flat = torch.randperm(E * A, generator=g)[:n]
    env_i, act_i = flat // A, flat % A
    exact = v[env_i, act_i] + 1e-4 * torch.randn(n, generator=g)
    # the first slots: the pairs whose difference is 0 by the rule
    same = [(nan, nan), (inf, inf), (-inf, -inf), (nan, nan)]
    for i, (c, x) in enumerate(same):
        v[env_i[i], act_i[i]], exact[i] = c, x
    finite = float((exact[len(same):] - v[env_i[len(same):], act_i[len(same):]]).abs().max())
    cases = [(None, finite), ((inf, -inf), inf), ((1.0, inf), inf), ((-inf, 2.0), inf), ((nan, 1.0), nan), ((1.0, nan), nan),
             ((nan, inf), nan), ((-inf, nan), nan)]
    for extra, want in cases:
        vv, ex = v.clone(), exact.clone()
        if extra is not None:
            vv[env_i[n - 1], act_i[n - 1]], ex[n - 1] = extra
        vd, xd, ed, ad, rd = vv.to(dev), ex.to(dev), env_i.to(dev), act_i.to(dev), reward.to(dev)
        values = (rd + 0.9 * vd.to(torch.float64)).contiguous()
        ref = values.clone()
        ref[ed, ad] = rd[ed, ad] + 0.9 * xd.to(torch.float64)
        rc, got, worst = _apply(xd, vd, ed, ad, rd, values)
        assert rc == 0
        assert np.array_equal(got, ref.cpu().numpy(), equal_nan=True)
        d = torch.where((ex == vv[env_i, act_i]) | (ex.isnan() & vv[env_i, act_i].isnan()), torch.zeros(n),
                        (ex - vv[env_i, act_i]).abs())
        assert (np.isnan(worst) and np.isnan(want)) or worst == want, (extra, worst, want)
        assert (np.isnan(worst) and bool(d.isnan().any())) or worst == float(d.max())
        if np.isnan(want):
            assert not worst <= 3.0e38  # above any bound the caller can hold it against
    # n = 0: nothing written, worst stays as the caller left it
    vd, rd = v.to(dev), reward.to(dev)
    values = (rd + 0.9 * vd.to(torch.float64)).contiguous()
    none = Guarded((0,), torch.int64, poison=False)  # empty, but a valid device address
    rc, got, worst = _apply(torch.zeros(1, device=dev), vd, none, none, rd, values)
    assert rc == 0 and worst == 0.0
    assert np.array_equal(got, values.cpu().numpy(), equal_nan=True)


NAN, INF = float("nan"), float("inf")
# the reference's rule on hand-written rows: (values, the action it takes or None for its ValueError)
REFERENCE_CASES = [
    ([1.0, 2.0, 2.0, 0.5], 1),                  # a tie: the first maximum
    ([3.0, 3.0, 3.0], 0),
    ([-0.0, 0.0], 0),                           # equal values
    ([2.0, NAN, 1.0], 0),                       # a NaN is never taken
    ([NAN, 1.0, 3.0], 2),                       # ... not even at index 0
    ([NAN, -5.0, NAN], 1),
    ([INF, 1.0, INF], 0),                       # +inf: the first one
    ([1.0, INF], 1),
    ([-INF, -INF, 0.0], 2),
    ([-INF, -1e300], 1),
    ([7.0], 0),
    ([NAN, NAN, NAN], None),                    # all NaN: no value above -inf
    ([-INF, -INF], None),                       # all -inf
    ([-INF, NAN, -INF], None),
    ([NAN], None),
]


def test_reference_rule_on_hand_written_rows_cpu():
    """The restated rule (tests/helpers.py: reference_rule, the loop of multi_human_rl.py:36-80) pinned on rows written
    by hand: ties, NaN, +-inf, all NaN, all -inf."""
    for row, want in REFERENCE_CASES:
        if want is None:
            with pytest.raises(ValueError, match="not well trained"):
                reference_rule(row)
        else:
            assert reference_rule(row) == want, row


def test_reference_choice_is_the_reference_rule_cpu():
    """ebcsim.sarl.reference_choice (what DeviceSarlPolicy.decide and the facade take their action with) against the
    loop, on numpy and torch values: the hand-written rows one by one, a batch of random rows with NaN and infinities,
    and a batch with one env that has no value above -inf (the whole call raises)."""
    for row, want in REFERENCE_CASES:
        for vals in (np.asarray([row], dtype=np.float64), torch.tensor([row], dtype=torch.float64)):
            if want is None:
                with pytest.raises(ValueError, match="not well trained"):
                    reference_choice(vals)
            else:
                assert int(reference_choice(vals)[0]) == want, row
    rs = np.random.RandomState(3)
    vals = np.round(rs.randn(500, 81), 1)  # rounded: many exact ties
    for x, p in ((NAN, 0.2), (INF, 0.01), (-INF, 0.2)):
        vals[rs.rand(*vals.shape) < p] = x
    vals[7] = NAN
    vals[7, 80] = 1.0  # the only number at the last index
    want = np.array([reference_rule(r) for r in vals])
    assert (reference_choice(vals) == want).all()
    assert (reference_choice(torch.from_numpy(vals)).numpy() == want).all()
    vals[11] = -INF
    vals[11, 3] = NAN
    for form in (vals, torch.from_numpy(vals)):
        with pytest.raises(ValueError, match="not well trained"):
            reference_choice(form)


# ---- the bound-driven re-evaluation, deterministic: the real kernels and host selection around a stubbed network ----
# The stub's rows carry, in row 0: the network's coarse (split-bf16) output, its float32 output, and the pair's tag
# (env * A + action), so a test knows which pairs were re-evaluated in float32.
DISCOUNT = 0.9


def _stub_net():
    """The shipped network on the GPU (so the native blocks exist and the native selection runs), its forward replaced
    on this instance by a stub that returns the coarse or (exact=True) the float32 value from the rows."""
    net = SarlValueNet.load(os.path.join(GOLDEN, "weights", "sarl_n10_ebcadrl.pth"), device="cuda:0")
    assert net._native_blocks()
    net.exact_tags = []

    def forward(rows, n_valid=None, want_weights=False, exact=False):
        if exact:
            net.exact_tags.append(rows[:, 0, 2].to(torch.int64).clone())
        return rows[:, 0, 1 if exact else 0].contiguous().clone()
    net.forward = forward
    return net


def _scenario_rows(coarse, f32):
    E, A = coarse.shape
    rows = torch.zeros((E, A, 2, 3), dtype=torch.float32)
    rows[:, :, 0, 0] = torch.from_numpy(coarse)
    rows[:, :, 0, 1] = torch.from_numpy(f32)
    rows[:, :, 0, 2] = torch.arange(E * A, dtype=torch.float32).view(E, A)
    return rows.cuda()


def _run_stubbed(net, coarse, f32, reward, eps, chunk_pairs=None):
    """-> (decisions, values, stats delta, tags re-evaluated in float32) of one shipped decision on the stub's outputs."""
    E, A = coarse.shape
    before = net.refine_stats or {}
    net.exact_tags.clear()
    pol = DeviceSarlPolicy(net, np.zeros((A, 2)), 0.9)
    values = net.action_values(_scenario_rows(coarse, f32), torch.from_numpy(reward).cuda(), DISCOUNT, chunk_pairs=chunk_pairs,
                               eps=eps)
    best = pol.choose(values)
    torch.cuda.synchronize()
    after = net.refine_stats
    delta = {k: after.get(k, 0) - before.get(k, 0) for k in ("decisions", "candidates", "bound_violations", "fallbacks")}
    tags = set(torch.cat(net.exact_tags).cpu().tolist()) if net.exact_tags else set()
    return best.cpu().numpy(), values.cpu().numpy(), delta, tags


def _check_stubbed(net, coarse, f32, reward, eps, violations, fallbacks=0, chunk_pairs=None):
    """(i) every decision is the reference rule on the float32 values; (ii) after the call every action within
    2 * discount * coarse_eps (its final value) of the env's coarse best holds reward + discount * float32 and was
    re-evaluated — in every env with two or more such actions (one alone is decided and keeps its coarse value), in
    every action of an env whose coarse values hold a NaN or nothing above -inf, and everywhere after a fallback — and
    every other action holds its coarse value; (iii) the counters."""
    E, A = coarse.shape
    best, values, delta, tags = _run_stubbed(net, coarse, f32, reward, eps, chunk_pairs)
    want_f = reward + DISCOUNT * f32.astype(np.float64)
    want_c = reward + DISCOUNT * coarse.astype(np.float64)
    assert [int(b) for b in best] == [reference_rule(r) for r in want_f]                                        # (i)
    bound = 2.0 * DISCOUNT * net.coarse_eps
    expect_cand = 0
    for e in range(E):
        row = want_c[e]
        top = np.nanmax(row) if not np.isnan(row).all() else -np.inf
        full = bool(fallbacks) or bool(np.isnan(row).any()) or not top > -np.inf
        within = np.ones(A, bool) if full else row >= top - bound
        reeval = within if (full or within.sum() > 1) else np.zeros(A, bool)
        expect_cand += int(reeval.sum())
        for a in range(A):
            got, want = values[e, a], (want_f[e, a] if reeval[a] else want_c[e, a])
            assert got == want or (np.isnan(got) and np.isnan(want)), (e, a, got, want_f[e, a], want_c[e, a])      # (ii)
            if reeval[a]:
                assert e * A + a in tags, (e, a)
    assert delta == {"decisions": E, "candidates": expect_cand, "bound_violations": violations, "fallbacks": fallbacks}, delta  # (iii)
    return best


def _layout(E, A, pattern_c, pattern_f, seed, filler=0.5):
    """Every env: the pattern's actions at a random place in the row, filler elsewhere (coarse = float32), a constant
    reward per env."""
    rs = np.random.RandomState(seed)
    coarse = np.full((E, A), filler, np.float32)
    f32 = np.full((E, A), filler, np.float32)
    slots = np.zeros((E, len(pattern_c)), np.int64)
    for e in range(E):
        p = rs.permutation(A)[:len(pattern_c)] if E > 1 else np.arange(len(pattern_c))
        coarse[e, p], f32[e, p] = pattern_c, pattern_f
        slots[e] = p
    reward = np.repeat(rs.uniform(-0.5, 0.5, (E, 1)), A, axis=1) if E > 1 else np.zeros((E, A))
    return coarse, f32, reward, slots


SHAPES = [(1, None), (37, 5 * 81)]  # one env; 37 envs in chunks of 5 that alternate between two streams


@pytest.mark.gpu
@pytest.mark.parametrize("E,chunk", SHAPES)
def test_refinement_without_violation(E, chunk):
    """A single candidate (decided on the coarse values), exact ties (the lowest action wins) and a near tie that the
    float32 values turn round: no violation, no fallback."""
    net = _stub_net()
    kinds = [([1.0], [1.00005]),                                   # one action within the bound
             ([1.0, 1.0], [1.00002, 1.00002]),                     # an exact tie in both forms
             ([1.0, 0.99995], [0.99996, 1.00004])]                 # the float32 values take the second
    coarse, f32, reward, slots = _layout(E, 81, [1.0, 1.0, 0.99995], [1.00005, 1.00002, 1.00004], 1)
    for e in range(E):
        kc, kf = kinds[e % 3]
        coarse[e, slots[e]], f32[e, slots[e]] = 0.5, 0.5
        coarse[e, slots[e][:len(kc)]], f32[e, slots[e][:len(kc)]] = kc, kf
    best = _check_stubbed(net, coarse, f32, reward, 1e-4, violations=0, chunk_pairs=chunk)
    for e in range(E):
        assert best[e] == (slots[e][0] if e % 3 == 0 else min(slots[e][:2]) if e % 3 == 1 else slots[e][1])


# item 1 of the decision review, worked by hand: discount 0.9, eps 1e-4.  Attempt 0 re-evaluates {a0, a1} and finds
# an error of 2e-4 (eps -> 4e-4); the widened bound takes in a2 (coarse 0.89935 >= 0.9 - 7.2e-4), whose float32 value is
# the best (an error of 1.7e-3: eps -> 3.4e-3, and the third attempt holds).  Selecting on the float32 value of a0
# (0.90018 - 7.2e-4) drops a2 and takes a0.
ITEM1_C, ITEM1_F = [1.0, 0.99995, 0.999278], [1.0002, 0.99995, 1.001]


@pytest.mark.gpu
@pytest.mark.parametrize("E,chunk", SHAPES)
def test_refinement_reselects_from_the_coarse_values(E, chunk):
    net = _stub_net()
    coarse, f32, reward, slots = _layout(E, 81, ITEM1_C, ITEM1_F, 2)
    best = _check_stubbed(net, coarse, f32, reward, 1e-4, violations=2, chunk_pairs=chunk)
    assert (best == slots[:, 2]).all()
    assert abs(net.coarse_eps - 2.0 * 1.722e-3) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("E,chunk", SHAPES)
def test_refinement_set_does_not_depend_on_the_margin(E, chunk):
    """EPS_MARGIN = 1 and the item-1 outputs with a2 at coarse 0.8997 / 0.9 and no error: the widened bound (eps 2e-4:
    0.9 - 3.6e-4 = 0.89964) holds a2, so a2 is re-evaluated although the decision stays a0."""
    net = _stub_net()
    net.EPS_MARGIN = 1.0
    a2 = np.float32(0.8997 / 0.9)
    coarse, f32, reward, slots = _layout(E, 81, [1.0, 0.99995, a2], [1.0002, 0.99995, a2], 3)
    best = _check_stubbed(net, coarse, f32, reward, 1e-4, violations=1, chunk_pairs=chunk)
    assert (best == slots[:, 0]).all()


# four violations in a row, each below COARSE_EPS_MAX, every widening taking in a larger error: eps 1e-5 -> 4e-5 ->
# 1e-4 -> 2.4e-4 -> 6e-4, and a5 beyond every bound holds the float32 maximum (its error 2.5e-3 is below the maximum)
CHAIN_C = [1.0, 1.0 - 1e-5, 1.0 - 6e-5, 1.0 - 1.5e-4, 1.0 - 4e-4, 1.0 - 2e-3]
CHAIN_F = [1.0, 1.0 - 1e-5 + 2e-5, 1.0 - 6e-5 + 5e-5, 1.0 - 1.5e-4 + 1.2e-4, 1.0 - 4e-4 + 3e-4, 1.0 - 2e-3 + 2.5e-3]


@pytest.mark.gpu
@pytest.mark.parametrize("E,chunk", SHAPES)
def test_refinement_falls_back_to_every_action_after_four_violations(E, chunk):
    net = _stub_net()
    coarse, f32, reward, slots = _layout(E, 81, np.float32(CHAIN_C), np.float32(CHAIN_F), 4)
    best = _check_stubbed(net, coarse, f32, reward, 1e-5, violations=4, fallbacks=1, chunk_pairs=chunk)
    assert (best == slots[:, 5]).all()
    # an error above COARSE_EPS_MAX still refuses the network
    f32[:, :] = coarse
    f32[0, slots[0, 1]] += 2 * SarlValueNet.COARSE_EPS_MAX
    with pytest.raises(RuntimeError, match="not fit"):
        _run_stubbed(net, coarse, f32, reward, 1e-5, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("E,chunk", SHAPES)
def test_refinement_with_nan_in_the_coarse_values(E, chunk):
    """NaN only in the coarse values (at index 0 of the pattern, a whole row of them in some envs), finite float32
    values: the env is re-evaluated in full and decided on its float32 values; envs without NaN beside them as usual."""
    net = _stub_net()
    coarse, f32, reward, slots = _layout(E, 81, [np.nan, 1.0, 0.99995], [1.2, 1.00001, 1.00003], 5)
    for e in range(E):
        if e % 3 == 1:
            coarse[e] = np.nan  # nothing to rank on: the float32 values decide
        elif e % 3 == 2:
            coarse[e, slots[e, 0]] = f32[e, slots[e, 0]] = 0.5  # no NaN: the float32 values of the near-best pair decide
    best = _check_stubbed(net, coarse, f32, reward, 1e-4, violations=0, chunk_pairs=chunk)
    assert all(best[e] == (slots[e, 2] if e % 3 == 2 else slots[e, 0]) for e in range(E))


@pytest.mark.gpu
@pytest.mark.parametrize("E,chunk", SHAPES)
def test_refinement_with_nan_in_both_forms(E, chunk):
    """NaN where both forms have one (no error), the best float32 number wins; -inf and +inf beside them."""
    net = _stub_net()
    coarse, f32, reward, slots = _layout(E, 81, [np.nan, 1.0, 0.99999, np.nan, -np.inf], [np.nan, 0.98, 0.995, np.nan, -np.inf], 6)
    best = _check_stubbed(net, coarse, f32, reward, 1e-4, violations=0, chunk_pairs=chunk)
    assert (best == slots[:, 2]).all()
    # two +inf in both forms: the same infinity is no error, the first of them is taken
    coarse, f32, reward, slots = _layout(E, 81, [np.inf, np.inf, 1.0], [np.inf, np.inf, 1.0], 7)
    best = _check_stubbed(net, coarse, f32, reward, 1e-4, violations=0, chunk_pairs=chunk)
    assert (best == slots[:, :2].min(1)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("E,chunk", SHAPES)
def test_refinement_raises_for_an_env_without_a_value(E, chunk):
    """An env whose values are all NaN (or all -inf) in both forms: the reference's ValueError."""
    net = _stub_net()
    for bad in (np.nan, -np.inf):
        coarse, f32, reward, slots = _layout(E, 81, [1.0, 0.99995], [1.0, 0.99996], 8)
        coarse[E // 2], f32[E // 2] = bad, bad
        with pytest.raises(ValueError, match="not well trained"):
            _run_stubbed(net, coarse, f32, reward, 1e-4, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("E,chunk", [(1, None), (37, 5)])
def test_refinement_with_one_action(E, chunk):
    """A = 1: the one action is the decision (its coarse value kept) unless its coarse value is NaN, which is replaced by
    the float32 value; NaN in both forms raises."""
    net = _stub_net()
    rs = np.random.RandomState(9)
    coarse = rs.uniform(0, 1, (E, 1)).astype(np.float32)
    f32 = coarse + np.float32(1e-5)
    reward = np.zeros((E, 1))
    coarse[::2] = np.nan
    best = _check_stubbed(net, coarse, f32, reward, 1e-4, violations=0, chunk_pairs=chunk)
    assert (best == 0).all()
    f32[0] = np.nan
    with pytest.raises(ValueError, match="not well trained"):
        _run_stubbed(net, coarse, f32, reward, 1e-4, chunk)


@pytest.mark.gpu
def test_decisions_are_the_float32_decisions_with_a_quarter_of_the_bound():
    """The shipped eb-cadrl weights on the bench workload (as test_decisions_are_the_float32_decisions_on_the_bench_workload)
    with eps a quarter of the calibrated one: every env takes the float32 network's action.  A quarter can hold at every
    candidate of these batches (the calibration's sample maximum lies far above the errors of near-best actions), so each
    point is also decided at the largest eps, down from the quarter in steps of 4, at which a candidate's coarse error
    (against torch's float32 GEMMs) exceeds twice the bound: there the bound is violated (the precondition, asserted) and
    widened, and every env must still take the float32 network's action."""
    import bench
    from ebcsim import actions as ebc_actions
    from ebcsim.batched import BatchedEnv
    dev = torch.device("cuda", 0)
    E = 1024
    params, batch = bench.build_batch("metric", E, 0)
    env = BatchedEnv(params, E, batch.N, batch.S)
    env.reset(batch)
    env.use_torch_stream()
    space = ebc_actions.build_action_space(float(batch.robot[0, 7]))
    acts = torch.tensor(space, dtype=torch.float64, device=dev)
    A = len(space)
    outs = env.alloc_step_outputs(("reward", "done"))
    net = SarlValueNet.load(os.path.join(GOLDEN, "weights", "sarl_n10_ebcadrl.pth"), device=str(dev))
    pol = DeviceSarlPolicy(net, space, 0.9)
    bufs = env.alloc_lookahead_outputs(A, ("reward", "done", "info", "rows_rotated"))
    quarter = None
    seen = []
    for point in range(3):
        for _ in range(10 * point):
            env.step_device(outs, human_policy=_abi.HUMAN_ORCA, robot_policy=_abi.ROBOT_LINEAR, flags=_abi.FLAG_AUTO_RESET)
        env.lookahead_device(acts, bufs, human_policy=_abi.HUMAN_ORCA)
        rows, reward = bufs["rows_rotated"], bufs["reward"]
        if quarter is None:
            quarter = net.calibrate_eps(rows.reshape(E * A, env.R, env.T)) / 4
        net.native_exact = False  # the yard-stick: torch's float32 GEMMs
        f32 = torch.empty((E, A), dtype=torch.float32, device=dev)
        for e0 in range(0, E, 128):
            f32[e0:e0 + 128] = net.forward(rows[e0:e0 + 128].reshape(-1, env.R, env.T), exact=True).view(-1, A)
        net.native_exact = True
        want = reward + 0.9 * f32.double()
        coarse = net.action_values(rows, reward, 0.9, refine=0)
        err = (coarse - want).abs() / 0.9
        top = coarse.max(1, keepdim=True).values
        eps = quarter
        while eps > 1e-9:
            cand = coarse >= top - 2.0 * 0.9 * eps
            cand &= (cand.sum(1) > 1)[:, None]
            if float(torch.where(cand, err, torch.zeros_like(err)).max()) > 2.0 * eps:
                break
            eps /= 4
        for e_run in (quarter, eps):
            before = net.refine_stats or {}
            got = net.action_values(rows, reward, 0.9, eps=e_run)
            chosen = pol.choose(got)
            torch.cuda.synchronize()
            wrong = torch.nonzero(chosen != want.argmax(1)).flatten().tolist()
            assert not wrong, [(e_run, e, int(chosen[e]), int(want[e].argmax()), float(want[e].max() - want[e, chosen[e]]))
                               for e in wrong[:5]]
            st = net.refine_stats
            seen.append((point, e_run, st["bound_violations"] - before.get("bound_violations", 0),
                         st["fallbacks"] - before.get("fallbacks", 0), st["candidates"] - before.get("candidates", 0)))
    print("(point, eps, violations, fallbacks, candidates):", seen)
    assert sum(x[2] for x in seen) >= 1, seen  # the precondition: the widening ran on the real network
