"""The value-based robot policy for the single-env facade: rl/policy/sarl.py:85-135 (SARL) with the
decision of rl/policy/multi_human_rl.py:12-87, served by the accelerated path.

The reference's predict() asks the env 81 times (`env.onestep_lookahead(action)`), rotates each answer
and runs the network 81 times.  Here one decision is ONE look-ahead sweep (`env.lookahead_all`:
ebc_lookahead leaves the rotated rows of all candidate actions) and ONE batched network forward
(ebcsim.sarl.SarlValueNet: the MFMA blocks on a HIP device, torch on the CPU).  Same attribute surface as
the reference's policy object (configure / set_phase / set_device / set_epsilon / get_model /
action_values / get_attention_weights / last_state), the same numpy draws for epsilon-greedy, the same
first-maximum tie rule, and its weight files load unchanged (`get_model().load_state_dict(torch.load(p))`)."""
import numpy as np
import torch

from .action import ActionRot, ActionXY
from .actions import build_action_space
from .policy import Policy
from .sarl import reference_choice


def _dims(config, key):
    return [int(x) for x in config.get("sarl", key).split(", ")]


class SARL(Policy):
    def __init__(self):
        Policy.__init__(self)
        self.name = "SARL"
        self.trainable = True
        self.multiagent_training = None
        self.epsilon = self.gamma = None
        self.sampling = self.speed_samples = self.rotation_samples = self.query_env = None
        self.action_space = self.speeds = self.rotations = None
        self.action_values = None
        self.with_om = None
        self.with_agent_type = False
        self.cell_num = self.cell_size = self.om_channel_size = None
        self.self_state_dim, self.agent_state_dim, self.agent_type_state_dim = 6, 7, 0
        self.joint_state_dim = 13
        self._net = None
        self._weights = None

    # ---------------------------------------------------------------- configuration
    def configure(self, config):
        """cadrl.py:72-81 + sarl.py:90-130"""
        from .train import SarlModule
        self.gamma = config.getfloat("rl", "gamma")
        self.kinematics = config.get("action_space", "kinematics")
        self.sampling = config.get("action_space", "sampling")
        self.speed_samples = config.getint("action_space", "speed_samples")
        self.rotation_samples = config.getint("action_space", "rotation_samples")
        self.query_env = config.getboolean("action_space", "query_env")
        self.cell_num = config.getint("om", "cell_num")
        self.cell_size = config.getfloat("om", "cell_size")
        self.om_channel_size = config.getint("om", "om_channel_size")
        self.with_om = config.getboolean("sarl", "with_om")
        if not self.query_env:
            raise NotImplementedError("query_env = false ends in the reference's own NotImplementedError "
                                      "(multi_human_rl.py:89-91)")
        if config.has_option("sarl", "with_agent_type"):
            self.with_agent_type = config.getboolean("sarl", "with_agent_type")
            self.agent_type_state_dim = 4 if self.with_agent_type else 0
            self.joint_state_dim = self.self_state_dim + self.agent_state_dim + self.agent_type_state_dim
        self.model = SarlModule(self.input_dim(), _dims(config, "mlp1_dims"), _dims(config, "mlp2_dims"),
                                _dims(config, "mlp3_dims"), _dims(config, "attention_dims"),
                                config.getboolean("sarl", "with_global_state"), self.self_state_dim)
        self.multiagent_training = config.getboolean("sarl", "multiagent_training")
        if self.with_om:
            self.name = "OM-SARL"

    def input_dim(self):
        """multi_human_rl.py:151-154"""
        return self.joint_state_dim + (self.cell_num ** 2 * self.om_channel_size if self.with_om else 0)

    def om_spec(self):
        """The [om] section as an OccupancySpec, or None without occupancy maps."""
        from .occupancy import OccupancySpec
        return OccupancySpec(self.cell_num, self.cell_size, self.om_channel_size) if self.with_om else None

    def build_occupancy_maps(self, agent_states):
        """multi_human_rl.py:156-227 on a list of observable states -> [rows, W] float32 (ebcsim.occupancy: the same
        cells from an algebraic frame).  A one-row state raises the reference's ValueError: np.concatenate of nothing."""
        from .occupancy import occupancy_maps
        if len(agent_states) == 1:
            raise ValueError("need at least one array to concatenate")
        ob = np.array([[s.px, s.py, s.vx, s.vy] for s in agent_states], dtype=np.float64).reshape(1, -1, 4)
        return torch.from_numpy(occupancy_maps(ob, None, self.om_spec())[0])

    def set_device(self, device):
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        self.model.to(self.device)
        self._net = None

    def set_epsilon(self, epsilon):
        self.epsilon = epsilon

    def get_attention_weights(self):
        """sarl.py:134-135: the weights of the network's LAST forward, i.e. of the last candidate action."""
        return self._weights

    def build_action_space(self, v_pref):
        """cadrl.py:91-116"""
        rows = build_action_space(v_pref, self.kinematics, self.speed_samples, self.rotation_samples)
        make = ActionXY if self.kinematics == "holonomic" else ActionRot
        self.action_space = [make(float(a), float(b)) for a, b in rows]
        self.speeds = sorted({float(np.hypot(a, b)) for a, b in rows[1:]}) if self.kinematics == "holonomic" \
            else sorted({float(a) for a, _ in rows[1:]})
        self.rotations = (np.linspace(0, 2 * np.pi, self.rotation_samples, endpoint=False)
                          if self.kinematics == "holonomic"
                          else np.linspace(-np.pi / 4, np.pi / 4, self.rotation_samples))
        self._action_rows = rows

    def _value_net(self):
        """Inference view of the model's current weights (packed for the matrix cores on a HIP device);
        rebuilt when the weights were replaced (load_state_dict) or moved."""
        version = tuple(p._version for p in self.model.parameters())
        if self._net is None or self._net_version != version:
            from .sarl import SarlValueNet
            self._net = SarlValueNet({k: v.detach() for k, v in self.model.state_dict().items()},
                                     device=str(self.device), with_global_state=self.model.with_global_state,
                                     self_state_dim=self.self_state_dim)
            self._net_version = version
        return self._net

    # ---------------------------------------------------------------- decision
    def predict(self, state, env=None):
        """multi_human_rl.py:12-87"""
        if self.phase is None:
            raise AttributeError("Phase attribute has to be set!")
        if self.device is None:
            raise AttributeError("Device attributes has to be set!")
        if self.phase == "train" and self.epsilon is None:
            raise AttributeError("Epsilon attribute has to be set in training phase")
        if self.reach_destination(state):
            return ActionXY(0, 0) if self.kinematics == "holonomic" else ActionRot(0, 0)
        if self.action_space is None:
            self.build_action_space(state.self_state.v_pref)
        if env is None or not hasattr(env, "lookahead_all"):
            raise ValueError("SARL.predict needs the env it acts in: robot.act(ob, env=env)")
        probability = np.random.random()
        if self.phase == "train" and probability < self.epsilon:
            chosen = self.action_space[np.random.choice(len(self.action_space))]
        else:
            sweep = env.lookahead_all(self._action_rows)
            rows = torch.from_numpy(sweep["rows_rotated"][:, :sweep["n_rows"]]).to(self.device)
            if self.with_om:
                # the maps of the state every action shares (multi_human_rl.py:62-69: built once, from the first action's
                # next_agent_states), appended to every action's rows
                from .occupancy import occupancy_maps, widen
                n = sweep["n_rows"]
                if n == 1:
                    raise ValueError("need at least one array to concatenate")
                om = occupancy_maps(sweep["next_ob"][None, :n], None, self.om_spec())[0]
                rows = widen(rows, torch.from_numpy(om).to(self.device))
            net = self._value_net()
            if net.input_dim != rows.shape[-1]:
                raise ValueError("the value network takes rows %d wide, this policy builds them %d wide" % (net.input_dim, rows.shape[-1]))
            # the attention weights of the network's last forward in the reference = of the last action
            _, w = net.forward(rows[-1:], want_weights=True, exact=True)
            self._weights = w[0].cpu().numpy()
            discount = pow(self.gamma, self.time_step * state.self_state.v_pref)
            reward = torch.from_numpy(np.ascontiguousarray(sweep["reward"], dtype=np.float64)).to(self.device)
            values = net.action_values(rows[None], reward[None], discount)[0].cpu().numpy()
            self.action_values = [float(x) for x in values]
            chosen = self.action_space[int(reference_choice(values[None])[0])]
        if self.phase == "train":
            self.last_state = self.transform(state, env)
        return chosen

    def transform(self, state, env=None):
        """multi_human_rl.py:128-149: the rotated joint state [rows, T].  With the env: the rows the env keeps
        for its current state (the kernels' rotate()).  Without — the reference's one-argument call, e.g.
        Explorer.update_memory's `target_policy.transform(state)` (rl/utils/explorer.py:162) — from `state`
        itself on the host, float32 like the reference's tensors."""
        if env is not None:
            rows = torch.from_numpy(env.observe_rotated()).to(self.device)
        else:
            rows = torch.Tensor([tuple(state.self_state + other) for other in state.agent_states])
            rows = self.rotate(rows).to(self.device)
        if self.with_om:  # multi_human_rl.py:142-146: the maps of the state as it is handed in
            rows = torch.cat([rows, self.build_occupancy_maps(state.agent_states).to(self.device)], dim=1)
        return rows

    def rotate(self, rows):
        """cadrl.py:236-337 on [n, 15] float32 rows (robot FullState 9 | other ObservableState 5 + type): the
        robot-centric frame with the x axis towards the goal."""
        sx, sy, svx, svy, sr, gx, gy, vpref, theta = (rows[:, c] for c in range(9))
        ox, oy, ovx, ovy, orad = (rows[:, c] for c in range(9, 14))
        ex, ey = gx - sx, gy - sy
        ang = torch.atan2(ey, ex)
        c, s_ = torch.cos(ang), torch.sin(ang)
        col = lambda v: v.reshape(-1, 1)  # noqa: E731
        heading = col(theta - ang) if self.kinematics == "unicycle" else torch.zeros_like(col(vpref))
        rx, ry = ox - sx, oy - sy
        parts = [torch.norm(torch.cat([col(ex), col(ey)], 1), 2, dim=1, keepdim=True), col(vpref), heading, col(sr),
                 col(svx * c + svy * s_), col(svy * c - svx * s_),
                 col(rx * c + ry * s_), col(ry * c - rx * s_),
                 col(ovx * c + ovy * s_), col(ovy * c - ovx * s_), col(orad),
                 torch.norm(torch.cat([col(sx - ox), col(sy - oy)], 1), 2, dim=1, keepdim=True), col(sr) + col(orad)]
        if self.with_agent_type:
            parts.append(torch.nn.functional.one_hot(rows[:, 14].long(), num_classes=self.agent_type_state_dim))
        return torch.cat(parts, dim=1)


class LstmRL(Policy):
    """rl/policy/lstm_rl.py:72-124 with the decision of multi_human_rl.py:12-87: one look-ahead sweep and one batched
    forward of the LSTM value network (ebcsim.lstm_rl.LstmValueNet) per decision.  configure() never reads
    with_agent_type (the reference's does not), so the rows are 13 wide and the env runs with with_agent_type = 0.
    The reference sorts state.agent_states by decreasing distance to the robot before it decides, but with query_env
    its network sees the rows env.onestep_lookahead returns, in the env's own order: the decision runs on the sweep's
    rows as they are, and the sort shows in `last_state` (phase "train") alone."""

    def __init__(self):
        Policy.__init__(self)
        self.name = "LSTM-RL"
        self.trainable = True
        self.multiagent_training = None
        self.epsilon = self.gamma = None
        self.sampling = self.speed_samples = self.rotation_samples = self.query_env = None
        self.action_space = self.speeds = self.rotations = None
        self.action_values = None
        self.with_om = None
        self.with_agent_type = False
        self.with_interaction_module = None
        self.interaction_module_dims = None
        self.cell_num = self.cell_size = self.om_channel_size = None
        self.self_state_dim, self.agent_state_dim, self.agent_type_state_dim = 6, 7, 0
        self.joint_state_dim = 13
        self._net = None

    def configure(self, config):
        """cadrl.py:72-81 + lstm_rl.py:79-106"""
        from .lstm_rl import LstmModule
        self.gamma = config.getfloat("rl", "gamma")
        self.kinematics = config.get("action_space", "kinematics")
        self.sampling = config.get("action_space", "sampling")
        self.speed_samples = config.getint("action_space", "speed_samples")
        self.rotation_samples = config.getint("action_space", "rotation_samples")
        self.query_env = config.getboolean("action_space", "query_env")
        self.cell_num = config.getint("om", "cell_num")
        self.cell_size = config.getfloat("om", "cell_size")
        self.om_channel_size = config.getint("om", "om_channel_size")
        dims = lambda key: [int(x) for x in config.get("lstm_rl", key).split(", ")]  # noqa: E731
        self.with_om = config.getboolean("lstm_rl", "with_om")
        if self.with_om:
            raise NotImplementedError("LstmRL is the policy without occupancy maps; [lstm_rl] with_om = true (OM-LSTM) is "
                                      "OmLstmRL, policy=\"om_lstm_rl\"")
        if not self.query_env:
            raise NotImplementedError("query_env = false ends in the reference's own NotImplementedError "
                                      "(multi_human_rl.py:89-91)")
        self.with_interaction_module = config.getboolean("lstm_rl", "with_interaction_module")
        self.model = LstmModule(self.input_dim(), self.self_state_dim, dims("mlp2_dims"),
                                config.getint("lstm_rl", "global_state_dim"),
                                dims("mlp1_dims") if self.with_interaction_module else None)
        self.multiagent_training = config.getboolean("lstm_rl", "multiagent_training")

    input_dim = SARL.input_dim
    set_device = SARL.set_device
    set_epsilon = SARL.set_epsilon
    build_action_space = SARL.build_action_space
    rotate = SARL.rotate

    def _value_net(self):
        """Inference view of the model's current weights; rebuilt when they were replaced (load_state_dict) or moved."""
        version = tuple(p._version for p in self.model.parameters())
        if self._net is None or self._net_version != version:
            from .lstm_rl import LstmValueNet
            self._net = LstmValueNet({k: v.detach() for k, v in self.model.state_dict().items()},
                                     device=str(self.device), self_state_dim=self.self_state_dim)
            self._net_version = version
        return self._net

    @staticmethod
    def sorted_order(state):
        """lstm_rl.py:117-123: the indices of state.agent_states by decreasing float64 distance to the robot; equal
        distances keep their original order (sorted(..., reverse=True) is stable)."""
        me = np.array(state.self_state.position)
        keys = [np.linalg.norm(np.array(a.position) - me) for a in state.agent_states]
        return sorted(range(len(keys)), key=keys.__getitem__, reverse=True)

    def predict(self, state, env=None):
        """lstm_rl.py:108-124 -> multi_human_rl.py:12-87"""
        order = self.sorted_order(state)
        state.agent_states = [state.agent_states[i] for i in order]
        if self.phase is None:
            raise AttributeError("Phase attribute has to be set!")
        if self.device is None:
            raise AttributeError("Device attributes has to be set!")
        if self.phase == "train" and self.epsilon is None:
            raise AttributeError("Epsilon attribute has to be set in training phase")
        if self.reach_destination(state):
            return ActionXY(0, 0) if self.kinematics == "holonomic" else ActionRot(0, 0)
        if self.action_space is None:
            self.build_action_space(state.self_state.v_pref)
        if env is None or not hasattr(env, "lookahead_all"):
            raise ValueError("LstmRL.predict needs the env it acts in: robot.act(ob, env=env)")
        probability = np.random.random()
        if self.phase == "train" and probability < self.epsilon:
            chosen = self.action_space[np.random.choice(len(self.action_space))]
        else:
            sweep = env.lookahead_all(self._action_rows)
            rows = self._sweep_rows(sweep)
            discount = pow(self.gamma, self.time_step * state.self_state.v_pref)
            reward = torch.from_numpy(np.ascontiguousarray(sweep["reward"], dtype=np.float64)).to(self.device)
            values = self._value_net().action_values(rows[None], reward[None], discount)[0].cpu().numpy()
            self.action_values = [float(x) for x in values]
            chosen = self.action_space[int(reference_choice(values[None])[0])]
        if self.phase == "train":
            self.last_state = self.transform(state, env, order)
        return chosen

    def _sweep_rows(self, sweep):
        """The rows the network sees for every candidate action, [A, rows, T], in the env's order."""
        return torch.from_numpy(sweep["rows_rotated"][:, :sweep["n_rows"]]).to(self.device)

    def transform(self, state, env=None, order=None):
        """multi_human_rl.py:128-149 of the (sorted) state: with the env, the rows it keeps for its current state
        re-ordered by `order` (indices into the env's own row order); without, from `state` itself as it stands."""
        if env is not None:
            rows = torch.from_numpy(env.observe_rotated())
            if order is not None:
                rows = rows[torch.as_tensor(order, dtype=torch.int64)]
            return rows.to(self.device)
        rows = torch.Tensor([tuple(state.self_state + other) for other in state.agent_states])
        return self.rotate(rows).to(self.device)


class OmLstmRL(LstmRL):
    """OM-LSTM: rl/policy/lstm_rl.py:72-124 with [lstm_rl] with_om = true.  The occupancy maps of
    multi_human_rl.py:156-227 are appended to every row the LSTM value network sees: in the decision to the sweep's rows,
    built once from the sweep's next_ob in the env's order (multi_human_rl.py:62-69); in `last_state` (phase "train") to
    the rows sorted by decreasing distance, built from the SORTED state (lstm_rl.py:117-123, then transform), so a cell's
    sums run over its occupants in the sorted order (ebcsim.occupancy.wide_state_sorted)."""
    MAX_INPUT_DIM = 64  # csrc/ebc_lstm_cell.h EBC_LSTM_MAX_DIM, csrc/ebc_lstm_grad_rule.h EBC_LSTM_GRAD_MAX_IN

    def __init__(self):
        LstmRL.__init__(self)
        self.name = "OM-LSTM-RL"

    def configure(self, config):
        """cadrl.py:72-81 + lstm_rl.py:79-106 with with_om"""
        from .lstm_rl import LstmModule
        from .occupancy import OccupancySpec
        CADRL.set_common_parameters(self, config)
        dims = lambda key: [int(x) for x in config.get("lstm_rl", key).split(", ")]  # noqa: E731
        self.with_om = config.getboolean("lstm_rl", "with_om")
        if not self.with_om:
            raise ValueError("OmLstmRL is OM-LSTM: [lstm_rl] with_om = false is LstmRL, policy=\"lstm_rl\"")
        if not self.query_env:
            raise NotImplementedError("query_env = false ends in the reference's own NotImplementedError "
                                      "(multi_human_rl.py:89-91)")
        self._spec = OccupancySpec(self.cell_num, self.cell_size, self.om_channel_size)
        if self.input_dim() > self.MAX_INPUT_DIM:
            raise NotImplementedError("OmLstmRL: rows of 13 + %d map columns = %d, the LSTM kernels take rows up to %d wide"
                                      % (self._spec.width, self.input_dim(), self.MAX_INPUT_DIM))
        self.with_interaction_module = config.getboolean("lstm_rl", "with_interaction_module")
        self.model = LstmModule(self.input_dim(), self.self_state_dim, dims("mlp2_dims"),
                                config.getint("lstm_rl", "global_state_dim"),
                                dims("mlp1_dims") if self.with_interaction_module else None)
        self.multiagent_training = config.getboolean("lstm_rl", "multiagent_training")

    def spec(self):
        """The [om] section as an OccupancySpec."""
        return self._spec

    om_spec = spec

    def _sweep_rows(self, sweep):
        from .occupancy import occupancy_maps, widen
        n = sweep["n_rows"]
        if n == 1:
            raise ValueError("need at least one array to concatenate")  # build_occupancy_maps of a one-row state
        rows = LstmRL._sweep_rows(self, sweep)
        om = occupancy_maps(sweep["next_ob"][None, :n], None, self._spec)[0]
        return widen(rows, torch.from_numpy(om).to(self.device))

    def transform(self, state, env=None, order=None):
        """multi_human_rl.py:128-149 of the (sorted) state with its maps: [rows, 13 + W] float32."""
        from .occupancy import wide_state_sorted
        if len(state.agent_states) == 1:
            raise ValueError("need at least one array to concatenate")
        rows = LstmRL.transform(self, state, env, order).cpu().numpy()
        ob = np.array([[a.px, a.py, a.vx, a.vy] for a in state.agent_states], dtype=np.float64)
        return torch.from_numpy(wide_state_sorted(rows[None], ob[None], None, self._spec)[0]).to(self.device)


class CADRL(Policy):
    """rl/policy/cadrl.py:34-234: the value network on every (robot, other) row separately, the minimum over the rows,
    the first action above every earlier one — one look-ahead sweep and one batched forward per decision
    (ebcsim.cadrl.CadrlValueNet).  The reference's own quirks are kept: configure() never reads with_agent_type (rows 13
    wide), predict() never reads query_env and always takes the look-ahead, no value above -inf returns None instead of
    raising, and transform() asserts exactly one other agent, so phase "train" works on one-human scenes only."""

    def __init__(self):
        Policy.__init__(self)
        self.name = "CADRL"
        self.trainable = True
        self.multiagent_training = None
        self.epsilon = self.gamma = None
        self.sampling = self.speed_samples = self.rotation_samples = self.query_env = None
        self.action_space = self.speeds = self.rotations = None
        self.action_values = None
        self.with_om = None
        self.with_agent_type = False
        self.cell_num = self.cell_size = self.om_channel_size = None
        self.self_state_dim, self.agent_state_dim, self.agent_type_state_dim = 6, 7, 0
        self.joint_state_dim = 13
        self._net = None

    def configure(self, config):
        """cadrl.py:66-82"""
        from .cadrl import CadrlModule
        self.set_common_parameters(config)
        self.model = CadrlModule(self.joint_state_dim, [int(x) for x in config.get("cadrl", "mlp_dims").split(", ")])
        self.multiagent_training = config.getboolean("cadrl", "multiagent_training")

    def set_common_parameters(self, config):
        self.gamma = config.getfloat("rl", "gamma")
        self.kinematics = config.get("action_space", "kinematics")
        self.sampling = config.get("action_space", "sampling")
        self.speed_samples = config.getint("action_space", "speed_samples")
        self.rotation_samples = config.getint("action_space", "rotation_samples")
        self.query_env = config.getboolean("action_space", "query_env")
        self.cell_num = config.getint("om", "cell_num")
        self.cell_size = config.getfloat("om", "cell_size")
        self.om_channel_size = config.getint("om", "om_channel_size")

    set_device = SARL.set_device
    set_epsilon = SARL.set_epsilon
    build_action_space = SARL.build_action_space
    rotate = SARL.rotate

    def _value_net(self):
        """Inference view of the model's current weights; rebuilt when they were replaced (load_state_dict) or moved."""
        version = tuple(p._version for p in self.model.parameters())
        if self._net is None or self._net_version != version:
            from .cadrl import CadrlValueNet
            self._net = CadrlValueNet({k: v.detach() for k, v in self.model.state_dict().items()}, device=str(self.device))
            self._net_version = version
        return self._net

    def predict(self, state, env=None):
        """cadrl.py:167-222"""
        if self.phase is None:
            raise AttributeError("Phase attribute has to be set!")
        if self.device is None:
            raise AttributeError("Device attributes has to be set!")
        if self.phase == "train" and self.epsilon is None:
            raise AttributeError("Epsilon attribute has to be set in training phase")
        if self.reach_destination(state):
            return ActionXY(0, 0) if self.kinematics == "holonomic" else ActionRot(0, 0)
        if self.action_space is None:
            self.build_action_space(state.self_state.v_pref)
        if env is None or not hasattr(env, "lookahead_all"):
            raise ValueError("CADRL.predict needs the env it acts in: robot.act(ob, env=env)")
        probability = np.random.random()
        if self.phase == "train" and probability < self.epsilon:
            chosen = self.action_space[np.random.choice(len(self.action_space))]
        else:
            sweep = env.lookahead_all(self._action_rows)
            rows = torch.from_numpy(sweep["rows_rotated"][:, :sweep["n_rows"]]).to(self.device)
            discount = pow(self.gamma, self.time_step * state.self_state.v_pref)
            reward = torch.from_numpy(np.ascontiguousarray(sweep["reward"], dtype=np.float64)).to(self.device)
            net = self._value_net()
            values = net.action_values(rows[None], reward[None], discount)[0].cpu().numpy()
            self.action_values = [float(x) for x in values]
            pick = int(net.last_choice[0])
            chosen = self.action_space[pick] if pick >= 0 else None  # max_action stays None (cadrl.py:193)
        if self.phase == "train":
            self.last_state = self.transform(state)
        return chosen

    def transform(self, state):
        """cadrl.py:224-234: the one (robot, other) row of a two-agent state, rotated -> [13] float32."""
        assert len(state.agent_states) == 1
        row = torch.Tensor([tuple(state.self_state + state.agent_states[0])])
        return self.rotate(row).squeeze(dim=0).to(self.device)


class SAIL(Policy):
    """rl/policy/sail.py:104-156: no look-ahead and no action space; one network (ebcsim.sail.SailModule, the
    reference's ExtendedNetwork) maps the robot's state and the world-frame states of exactly `adult_num` others straight
    to the action — one forward per decision (ebcsim.sail.SailNet: one kernel on a HIP device, torch on the CPU)."""

    def __init__(self):
        Policy.__init__(self)
        self.name = "SAIL"
        self.trainable = True
        self.multiagent_training = None
        self.epsilon = self.gamma = None
        self.sampling = self.speed_samples = self.rotation_samples = self.query_env = None
        self.action_space = self.speeds = self.rotations = None
        self.action_values = None
        self.with_om = None
        self.with_agent_type = False
        self.cell_num = self.cell_size = self.om_channel_size = None
        self.self_state_dim, self.agent_state_dim, self.agent_type_state_dim = 6, 7, 0
        self.joint_state_dim = 13
        self.adult_num = None
        self._net = None

    def configure(self, config):
        """sail.py:109-112"""
        from .sail import SailModule, check_adult_num
        self.set_common_parameters(config)
        self.multiagent_training = config.getboolean("sail", "multiagent_training")
        self.adult_num = config.getint("sail", "adult_num")
        check_adult_num(self.adult_num)
        self.model = SailModule(self.adult_num)

    set_common_parameters = CADRL.set_common_parameters
    set_device = SARL.set_device
    set_epsilon = SARL.set_epsilon
    build_action_space = SARL.build_action_space

    def _value_net(self):
        """Inference view of the model's current weights; rebuilt when they were replaced (load_state_dict) or moved."""
        version = tuple(p._version for p in self.model.parameters())
        if self._net is None or self._net_version != version:
            from .sail import SailNet
            self._net = SailNet({k: v.detach() for k, v in self.model.state_dict().items()}, device=str(self.device))
            self._net_version = version
        return self._net

    def predict(self, state, env=None):
        """sail.py:114-132"""
        if self.phase is None:
            raise AttributeError("Phase attribute has to be set!")
        if self.device is None:
            raise AttributeError("Device attributes has to be set!")
        if self.phase == "train" and self.epsilon is None:
            raise AttributeError("Epsilon attribute has to be set in training phase")
        make = ActionXY if self.kinematics == "holonomic" else ActionRot
        if self.reach_destination(state):
            return make(0, 0)
        self.last_state = self.transform(state)
        net = self._value_net()
        if len(state.agent_states) != net.adult_num:
            raise ValueError("SAIL.predict: %d agents, the network takes exactly adult_num = %d (the reference raises "
                             "there too)" % (len(state.agent_states), net.adult_num))
        s = state.self_state
        robot = torch.tensor([[s.px, s.py, s.vx, s.vy, s.radius, s.gx, s.gy, s.v_pref, s.theta]], dtype=torch.float64)
        ob = torch.tensor([[[a.px, a.py, a.vx, a.vy, a.radius] for a in state.agent_states]], dtype=torch.float64)
        action, self.feat_joint = net.forward(robot.to(self.device), ob.to(self.device))
        return make(float(action[0, 0]), float(action[0, 1]))

    def transform(self, state):
        """sail.py:134-156: [robot (px, py, vx, vy, gx, gy) [6], agents (px, py, vx, vy) [N, 4]], float32"""
        s = state.self_state
        robot = torch.Tensor([s.px, s.py, s.vx, s.vy, s.gx, s.gy])
        agents = torch.empty([len(state.agent_states), 4])
        for k, a in enumerate(state.agent_states):
            agents[k, 0], agents[k, 1], agents[k, 2], agents[k, 3] = a.px, a.py, a.vx, a.vy
        return [robot, agents]
