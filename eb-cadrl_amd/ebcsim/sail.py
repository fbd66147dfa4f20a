"""The SAIL policy's network and its decision (rl/policy/sail.py:9-156), batched.

SAIL has no look-ahead sweep and no action space: one small network (`ExtendedNetwork`) maps the robot's state and the
world-frame states of exactly `adult_num` others straight to a continuous action.

SailModule is the torch module (the reference's state_dict keys: its .pth files load with strict=True).  SailNet is the
inference view: on a HIP device one kernel (ebc_sail_forward, csrc/ebc_sail.h) goes from the env's float64 state to
action [E, 2]; on the CPU it is SailModule plus the same arrival, row-count and cast rules.  DeviceSailPolicy decides for
a whole BatchedEnv from its device state: no host round trip."""
import ctypes as C

import torch

from . import _abi

LOCAL, HIDDEN = 32, 64
MIN_ADULTS, MAX_ADULTS = 2, 32
# the Linear layers in the order of EbcSailWeights (include/ebcsim.h)
LAYERS = ("robot_encoder.0", "robot_encoder.2", "adult_encoder.0", "adult_encoder.2", "adult_head.0", "joint_embedding.0",
          "pairwise.0", "pairwise.2", "attention.0", "attention.2", "task_encoder.0", "task_encoder.2", "joint_encoder.0",
          "planner")


def envs_per_workgroup(adult_num):
    """Envs one workgroup of the kernel owns (csrc/ebc_sail_rule.h: group_envs): whole envs, at most 8 and at most 48
    adult rows, or one env."""
    return max(1, min(8, 48 // int(adult_num)))


def _seq(*dims, last_relu=True):
    layers = []
    for i in range(len(dims) - 1):
        layers.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2 or last_relu:
            layers.append(torch.nn.ReLU())
    return torch.nn.Sequential(*layers)


class SailModule(torch.nn.Module):
    """ExtendedNetwork of rl/policy/sail.py:9-101 with its parameter names and construction order."""

    def __init__(self, num_adult, embedding_dim=HIDDEN, hidden_dim=HIDDEN, local_dim=LOCAL):
        super().__init__()
        self.num_adult = int(num_adult)
        self.robot_encoder = _seq(4, local_dim, local_dim)
        self.adult_encoder = _seq(4 * self.num_adult, hidden_dim, hidden_dim)
        self.adult_head = _seq(hidden_dim, local_dim)
        self.joint_embedding = _seq(local_dim * 2, embedding_dim)
        self.pairwise = _seq(embedding_dim, hidden_dim, hidden_dim, last_relu=False)
        self.attention = _seq(embedding_dim, hidden_dim, 1, last_relu=False)
        self.task_encoder = _seq(4, hidden_dim, hidden_dim)
        self.joint_encoder = _seq(hidden_dim * 2, hidden_dim)
        self.planner = torch.nn.Linear(hidden_dim, 2)

    @classmethod
    def from_state_dict(cls, sd):
        """The module a reference state_dict belongs to (adult_encoder.0's input width gives adult_num)."""
        m = cls(int(sd["adult_encoder.0.weight"].shape[1]) // 4)
        m.load_state_dict(sd, strict=True)
        return m

    def transform_frame(self, frame):
        """rl/utils/transform.py:11-20: frame [B, N, 4] -> [B, N, 4 N]: row i = frame[i], then frame[j] - frame[i] for
        every j != i, j ascending."""
        B, N = frame.shape[0], self.num_adult
        if frame.shape[1] != N:
            raise ValueError("SailModule: %d agents, the network takes exactly adult_num = %d" % (frame.shape[1], N))
        compare = frame.unsqueeze(1) - frame.unsqueeze(2)
        keep = ~torch.eye(N, dtype=torch.bool, device=frame.device)
        return torch.cat([frame, compare[:, keep].reshape(B, N, -1)], dim=2)

    def forward(self, robot_state, crowd_obsv):
        """robot_state [B, 6] (px, py, vx, vy, gx, gy) or [6]; crowd_obsv [B, N, 4] or [N, 4] -> (action [B, 2],
        feat_joint [B, hidden])."""
        if robot_state.dim() < 2:
            robot_state, crowd_obsv = robot_state.unsqueeze(0), crowd_obsv.unsqueeze(0)
        emb_robot = self.robot_encoder(robot_state[:, :4])
        emb_adult = self.adult_head(self.adult_encoder(self.transform_frame(crowd_obsv)))
        emb_pairwise = self.joint_embedding(torch.cat([emb_robot.unsqueeze(1).repeat(1, self.num_adult, 1), emb_adult], dim=2))
        feat_pairwise = self.pairwise(emb_pairwise)
        score_pairwise = torch.nn.functional.softmax(self.attention(emb_pairwise), dim=1)
        feat_crowd = torch.sum(feat_pairwise * score_pairwise, dim=1)
        task = torch.cat([robot_state[:, -2:] - robot_state[:, :2], robot_state[:, 2:4]], dim=1)
        feat_joint = self.joint_encoder(torch.cat([self.task_encoder(task), feat_crowd], dim=1))
        return self.planner(feat_joint), feat_joint


def check_adult_num(n):
    if not MIN_ADULTS <= int(n) <= MAX_ADULTS:
        raise NotImplementedError("SAIL: adult_num = %d is outside %d..%d (at 1 the reference's own transform_frame "
                                  "raises)" % (n, MIN_ADULTS, MAX_ADULTS))


class _NativeSail(object):
    """ebc_sail_create / _destroy around a state_dict's 14 layers."""

    def __init__(self, module, device_index):
        from . import _capi
        self._L = _capi.lib()
        sd = module.state_dict()
        keep = [sd[k + s].detach().to("cpu", torch.float32).contiguous() for s in (".weight", ".bias") for k in LAYERS]
        w = _abi.EbcSailWeights()
        w.struct_size = C.sizeof(w)
        w.adult_num = module.num_adult
        for i in range(_abi.SAIL_LAYERS):
            w.weight[i], w.bias[i] = keep[i].data_ptr(), keep[_abi.SAIL_LAYERS + i].data_ptr()
        h = C.c_void_p()
        _capi.check(self._L.ebc_sail_create(C.addressof(w), int(device_index), C.byref(h)))
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.ebc_sail_destroy(h)


def native_forward(handle, robot, ob, n_rows=None, action=None, feat_joint=None, want_feat=True):
    """ebc_sail_forward on the current stream: robot [E, 9] float64, ob [E, R, 5] float64, n_rows [E] int64 or None
    (device tensors) -> (action [E, 2] float64, feat_joint [E, 64] float32 or None)."""
    from . import _capi
    E, R = int(ob.shape[0]), int(ob.shape[1])
    assert robot.dtype == torch.float64 and ob.dtype == torch.float64 and robot.is_cuda and ob.device == robot.device
    assert tuple(robot.shape) == (E, 9) and ob.shape[2] == 5 and robot.is_contiguous() and ob.is_contiguous()
    if action is None:
        action = torch.empty((E, 2), dtype=torch.float64, device=robot.device)
    if feat_joint is None and want_feat:
        feat_joint = torch.empty((E, HIDDEN), dtype=torch.float32, device=robot.device)
    a = _abi.EbcSailArgs()
    a.struct_size = C.sizeof(a)
    a.E, a.R = E, R
    a.robot, a.ob, a.action = robot.data_ptr(), ob.data_ptr(), action.data_ptr()
    a.feat_joint = None if feat_joint is None else feat_joint.data_ptr()
    if n_rows is not None:
        assert n_rows.dtype == torch.int64 and n_rows.is_contiguous() and tuple(n_rows.shape) == (E,) and n_rows.device == robot.device
        a.n_rows = n_rows.data_ptr()
    _capi.check(_capi.lib().ebc_sail_forward(handle, torch.cuda.current_stream(robot.device).cuda_stream, C.addressof(a)))
    return action, feat_joint


class SailNet(object):
    """Inference view of a SAIL network from the reference's state_dict."""

    def __init__(self, state_dict, device="cpu"):
        self.device = torch.device(device)
        self.module = SailModule.from_state_dict({k: v.detach().to("cpu", torch.float32) for k, v in state_dict.items()}
                                                 ).to(self.device).eval()
        for p in self.module.parameters():
            p.requires_grad_(False)
        self.adult_num = self.module.num_adult
        check_adult_num(self.adult_num)
        self.native_forwards = 0
        self._native = None

    @classmethod
    def load(cls, path, device="cpu", **kw):
        return cls(torch.load(path, map_location="cpu"), device=device, **kw)

    def native(self):
        """The kernel's handle on a HIP device; None on the CPU."""
        if self.device.type != "cuda":
            return None
        if self._native is None:
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self._native = _NativeSail(self.module, idx)
        return self._native

    def forward(self, robot, ob, n_rows=None):
        """robot [E, 9] float64 (FullState order), ob [E, R, 5] float64 (R >= adult_num; rows at or past adult_num are
        never read), n_rows [E] int64 or None = adult_num everywhere -> (action [E, 2] float64, feat_joint [E, 64]
        float32).  An arrived env gets (0, 0) (its feat_joint is still the network's); an env whose row count is not
        adult_num gets a NaN action and zeros (the reference raises there)."""
        N = self.adult_num
        if ob.shape[1] < N:
            raise ValueError("SailNet: %d rows per env, the network takes exactly adult_num = %d" % (ob.shape[1], N))
        nat = self.native() if robot.is_cuda else None
        if nat is not None:
            self.native_forwards += 1
            nr = None if n_rows is None else n_rows.to(device=robot.device, dtype=torch.int64).contiguous()
            return native_forward(nat._h, robot.to(torch.float64).contiguous(), ob.to(torch.float64).contiguous(), nr)
        with torch.no_grad():
            robot, ob = robot.to(self.device, torch.float64), ob.to(self.device, torch.float64)
            arrived = torch.sqrt((robot[:, 1] - robot[:, 6]) ** 2 + (robot[:, 0] - robot[:, 5]) ** 2) < robot[:, 4]
            action, feat = self.module(robot[:, [0, 1, 2, 3, 5, 6]].to(torch.float32), ob[:, :N, :4].to(torch.float32))
            action = torch.where(arrived[:, None], torch.zeros_like(action), action).to(torch.float64)
            if n_rows is not None:
                bad = (n_rows.to(self.device) != N)[:, None]
                action = torch.where(bad, torch.full_like(action, float("nan")), action)
                feat = torch.where(bad, torch.zeros_like(feat), feat)
            return action, feat


class DeviceSailPolicy(object):
    """SAIL decisions for a whole BatchedEnv from its device state: ebc_get_state (robot), ebc_observe (ob) and
    ebc_row_counts into device buffers, then one kernel (decide); or K decisions and steps in one call (rollout)."""

    def __init__(self, net):
        self.net = net
        self._bufs = None

    def decide(self, env, human_policy=_abi.HUMAN_ORCA):
        """env: BatchedEnv on this net's device -> (actions [E, 2] float64 on the device, None): there is no look-ahead,
        so there are no values, and no human velocities are left cached (step with the humans' own policy, which
        `human_policy` names for the callers that pass it).  An env whose row count is not adult_num gets NaN."""
        dev = self.net.device
        key = (id(env), env.E, env.R)
        if self._bufs is None or self._key != key:
            self._key = key
            self._bufs = dict(robot=torch.empty((env.E, 9), dtype=torch.float64, device=dev),
                              ob=torch.empty((env.E, env.R, 5), dtype=torch.float64, device=dev),
                              n_rows=torch.empty((env.E,), dtype=torch.int64, device=dev),
                              action=torch.empty((env.E, 2), dtype=torch.float64, device=dev),
                              feat_joint=torch.empty((env.E, HIDDEN), dtype=torch.float32, device=dev))
        b = self._bufs
        if env.R < self.net.adult_num:
            raise ValueError("DeviceSailPolicy: the env has %d rows, the network takes exactly adult_num = %d" % (env.R, self.net.adult_num))
        env.robot_state_device(b["robot"])
        env.observe_ob_device(b["ob"])
        env.row_counts_device(b["n_rows"])
        nat = self.net.native()
        if nat is None:
            raise NotImplementedError("DeviceSailPolicy needs a SailNet on a HIP device")
        self.net.native_forwards += 1
        native_forward(nat._h, b["robot"], b["ob"], b["n_rows"], b["action"], b["feat_joint"])
        self.feat_joint = b["feat_joint"]
        return b["action"], None

    def rollout(self, env, K, outputs, flags=0, human_policy=_abi.HUMAN_ORCA):
        """K closed-loop steps in ONE call: attaches the net to `env` (BatchedEnv.attach_sail) and enqueues
        step_k_device(robot_policy=ROBOT_SAIL) writing into `outputs` (torch CUDA tensors [K, ...], e.g.
        env.alloc_step_k_outputs).  Step for step what decide() followed by step_device computes, without the host in
        the loop; flags may carry FLAG_AUTO_RESET and FLAG_ONE_LAUNCH (the network inside the rollout kernel).  The keys
        "world_robot" and "world_ob" in `outputs` go through as they are: the world before every step (ebc_step_k_world)."""
        if env.R < self.net.adult_num:
            raise ValueError("DeviceSailPolicy: the env has %d rows, the network takes exactly adult_num = %d" % (env.R, self.net.adult_num))
        env.attach_sail(self.net)
        env.step_k_device(outputs, K, human_policy=human_policy, robot_policy=_abi.ROBOT_SAIL, flags=flags)
