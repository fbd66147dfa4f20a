"""ctypes mirror of include/ebcsim.h (struct layouts and enums only; loads nothing)."""
import ctypes as C

ABI_VERSION = 1

OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_DEVICE, ERR_STATE = 0, -1, -2, -3, -4

# simulator/utils/utils.py:9-14
ADULT, BICYCLE, CHILD, ADULT_STATIC, ROBOT = 0, 1, 2, 3, 4

(INFO_NOTHING, INFO_DANGER, INFO_REACH_GOAL, INFO_COLLISION_OBSTACLE, INFO_COLLISION_ADULT,
 INFO_COLLISION_BICYCLE, INFO_COLLISION_CHILD, INFO_TIMEOUT) = range(8)

HOLONOMIC, UNICYCLE = 0, 1
HOST, DEVICE = 0, 1
HUMAN_EXTERNAL, HUMAN_LINEAR, HUMAN_ORCA, HUMAN_CACHED = 0, 1, 2, 3
HUMAN_BY_TYPE = 4  # every entity type on its own policy (ebc_set_human_policies)
ROBOT_EXTERNAL, ROBOT_LINEAR, ROBOT_ORCA, ROBOT_SAIL = 0, 1, 2, 3
FLAG_AUTO_RESET, FLAG_BORDER = 1, 2
FLAG_ONE_LAUNCH = 4  # ebc_step_k: all K steps in one kernel launch (ORCA humans; strict, never a fall-back)

_pd = C.c_void_p  # every buffer pointer travels as an address


class EbcParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("robot_kinematics", C.c_int32),
        ("robot_visible", C.c_int32),
        ("new_reward", C.c_int32),
        ("time_step", C.c_double),
        ("time_limit", C.c_double),
        ("map_size_m", C.c_double),
        ("map_resolution", C.c_double),
        ("time_max", C.c_double),
        ("time_good", C.c_double),
        ("max_goal_distance", C.c_double),
        ("success_reward", C.c_double),
        ("collision_penalty", C.c_double * 4),
        ("discomfort_dist", C.c_double * 3),
        ("discomfort_factor", C.c_double * 3),
        ("rotation_penalty_factor", C.c_double),
        ("orca_safety_space", C.c_double),
        ("orca_neighbor_dist", C.c_float),
        ("orca_time_horizon", C.c_float),
        ("orca_max_neighbors", C.c_int32),
        ("with_agent_type", C.c_int32),
        ("rotate_unicycle", C.c_int32),
        ("reserved", C.c_int32),
    ]


class EbcScene(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_int32), ("n_humans", _pd)] + [
        (k, _pd) for k in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type",
                           "n_static", "spx", "spy", "sradius", "grid", "robot")
    ]


class EbcSceneGen(C.Structure):
    """include/ebcsim.h: the keys SceneGenerator.__init__ reads, phase resolved (scene.SceneConfig.gen_struct)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("randomize_attributes", C.c_int32),
        ("count", C.c_int32 * 3),
        ("rule", C.c_int32 * 3),
    ] + [(k, C.c_double * 3) for k in ("radius", "v_pref", "radius_min", "radius_max", "v_pref_min", "v_pref_max")] + [
        (k, C.c_double) for k in ("square_width", "circle_radius", "discomfort_dist", "robot_radius", "robot_v_pref",
                                  "map_resolution", "map_size_m")
    ] + [(k, C.c_int32) for k in ("min_wall_length", "max_wall_length", "num_circles", "num_walls")]


class EbcSceneOut(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("location", C.c_int32), ("n_humans", _pd)] + [
        (k, _pd) for k in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type",
                           "n_static", "spx", "spy", "sradius", "grid", "robot")
    ]


RULE_CIRCLE_CROSSING, RULE_SQUARE_CROSSING, RULE_SQUARE_CROSSING_OLD = 0, 1, 2
RULE_MIXED, RULE_MIXED_20, RULE_ONE_STATIC = 3, 4, 5  # the crowd rules: adults only
# adult slots a scene of a crowd rule can take, whatever adult_num says (scene_generator.py:523-589)
CROWD_CAPACITY = {RULE_MIXED: 5, RULE_MIXED_20: 20, RULE_ONE_STATIC: 2}


class EbcStepArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("location", C.c_int32),
        ("human_policy", C.c_int32),
        ("robot_policy", C.c_int32),
        ("flags", C.c_int32),
        ("reserved", C.c_int32),
    ] + [
        (k, _pd) for k in ("robot_action", "border", "reward", "done", "info", "dmin",
                           "dist_to_goal", "robot_action_out", "human_action", "ob", "obs_rotated")
    ]


class EbcLookaheadArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("location", C.c_int32),
        ("human_policy", C.c_int32),
        ("n_actions", C.c_int32),
        ("flags", C.c_int32),
        ("reserved", C.c_int32),
    ] + [
        (k, _pd) for k in ("actions", "border", "reward", "done", "info", "dmin", "next_ob",
                           "rows_rotated")
    ]


class EbcStepKArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("location", C.c_int32),
        ("K", C.c_int32),
        ("human_policy", C.c_int32),
        ("robot_policy", C.c_int32),
        ("flags", C.c_int32),
        ("robot_safety_space", C.c_double),
    ] + [
        (k, _pd) for k in ("robot_action", "state_rotated", "n_rows", "robot_action_out", "reward", "done", "info",
                           "dmin", "dist_to_goal", "obs_rotated")
    ]


class EbcStateView(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("location", C.c_int32)] + [
        (k, _pd) for k in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type",
                           "n_humans", "robot", "global_time", "arrival_time", "done")
    ]


class EbcLocalMapParams(C.Structure):
    """include/ebcsim.h: get_local_map_angular's parameters (simulator/env.py:80-84), angles in radians."""
    _fields_ = [("struct_size", C.c_uint32), ("dim", C.c_int32), ("max_range", C.c_double), ("angle_min", C.c_double),
                ("angle_max", C.c_double), ("normalize", C.c_int32), ("reserved", C.c_int32)]


class EbcObstacles(C.Structure):
    """include/ebcsim.h: n scenes' obstacle polygons, n_poly [n] int32, vertices [n][S][4][2] float64 (host)."""
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_int32), ("n_poly", _pd), ("vertices", _pd)]


LOCAL_MAP_MAX_DIM = 128

MLP_IN_FRAGMENTS = 1
MLP_GENERAL_KERNEL = 1
MLP_WIDE_MAX = 640  # K0, H, O of ebc_mlp2_create_wide


class EbcMlpArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("M", C.c_int32), ("relu_out", C.c_int32), ("group_rows", C.c_int32),
                ("seg_rows", C.c_int32), ("flags", C.c_int32)] + [(k, C.c_void_p) for k in ("x", "frag_in", "row_bias", "row_weight", "y", "partial",
                                                                       "frag_out")]


def default_params():
    """Reference defaults: ORCA constants simulator/policy/orca.py:58-69, reward.py:25."""
    p = EbcParams()
    p.struct_size = C.sizeof(EbcParams)
    p.robot_kinematics = HOLONOMIC
    p.robot_visible = 0
    p.new_reward = 0
    p.time_step = 0.25
    p.time_limit = 25
    p.map_size_m = 9.0
    p.map_resolution = 0.1
    nan = float("nan")
    p.time_max = nan
    p.time_good = 10.0
    p.max_goal_distance = nan
    p.success_reward = 1.0
    for i in range(4):
        p.collision_penalty[i] = nan
    for i in range(3):
        p.discomfort_dist[i] = 0.1
        p.discomfort_factor[i] = 0.5
    p.rotation_penalty_factor = 0.0
    p.orca_safety_space = 0.0
    p.orca_neighbor_dist = 10.0
    p.orca_time_horizon = 5.0
    p.orca_max_neighbors = 10
    p.with_agent_type = 0
    p.rotate_unicycle = 0
    return p


def rot_width(params):
    return 17 if params.with_agent_type else 13


class EbcLstmArgs(C.Structure):
    """include/ebcsim.h: one ebc_lstm_forward (x [B * R][I], n_valid [B] int64 or NULL, h_n to out[b * out_stride + out_offset ..])."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("R", C.c_int32), ("out_offset", C.c_int32),
                ("self_cols", C.c_int32), ("reserved", C.c_int32), ("out_stride", C.c_int64), ("self_stride", C.c_int64)] + [
        (k, C.c_void_p) for k in ("x", "n_valid", "out", "self_src")]


class EbcCadrlArgs(C.Structure):
    """include/ebcsim.h: one ebc_cadrl_decide (v [E][A][R] float32, n_valid [E] int64 or NULL, reward [E][A] -> values [E][A], choice [E])."""
    _fields_ = [("struct_size", C.c_uint32), ("E", C.c_int32), ("A", C.c_int32), ("R", C.c_int32), ("discount", C.c_double)] + [
        (k, C.c_void_p) for k in ("v", "n_valid", "reward", "values", "choice")]


class EbcOmArgs(C.Structure):
    """include/ebcsim.h: one ebc_occupancy_rows (next_ob [E][R][5] float64, n_valid [E] int64 or NULL, rows [E][A][R][T] or NULL
    -> om [E][R][W], rows_wide [E][A][R][T + W])."""
    _fields_ = [("struct_size", C.c_uint32), ("E", C.c_int32), ("A", C.c_int32), ("R", C.c_int32), ("T", C.c_int32),
                ("cell_num", C.c_int32), ("channels", C.c_int32), ("reserved", C.c_int32), ("cell_size", C.c_double)] + [
        (k, C.c_void_p) for k in ("next_ob", "n_valid", "rows", "om", "rows_wide")]


class EbcOmSpec(C.Structure):
    """include/ebcsim.h: [om] cell_num / om_channel_size / cell_size, what ebc_observe_wide, ebc_observe_wide_sorted and
    ebc_step_k_om build the maps with."""
    _fields_ = [("struct_size", C.c_uint32), ("cell_num", C.c_int32), ("channels", C.c_int32), ("reserved", C.c_int32),
                ("cell_size", C.c_double)]


class EbcStepKOm(C.Structure):
    """include/ebcsim.h: what ebc_step_k_om adds to ebc_step_k: the spec and state_wide, device float32 [K][E][R][T + W]."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32), ("spec", EbcOmSpec), ("state_wide", C.c_void_p)]


class EbcStepKWorld(C.Structure):
    """include/ebcsim.h: what ebc_step_k_world adds to ebc_step_k: the robot's FullState [K][E][9] and the world-frame rows
    [K][E][R][5] before every step, float64 where EbcStepKArgs.location says; either may be NULL, not both."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32), ("robot", C.c_void_p), ("ob", C.c_void_p)]


def om_spec(spec):
    """An occupancy.OccupancySpec (cell_num, cell_size, channels) as the struct."""
    s = EbcOmSpec()
    s.struct_size = C.sizeof(s)
    s.cell_num, s.channels, s.cell_size = int(spec.cell_num), int(spec.channels), float(spec.cell_size)
    return s


SAIL_LAYERS = 14


class EbcSailWeights(C.Structure):
    """include/ebcsim.h: the 14 Linear layers of the SAIL network, host pointers in torch's layout [out][in]."""
    _fields_ = [("struct_size", C.c_uint32), ("adult_num", C.c_int32), ("weight", C.c_void_p * SAIL_LAYERS),
                ("bias", C.c_void_p * SAIL_LAYERS)]


class EbcSailArgs(C.Structure):
    """include/ebcsim.h: one ebc_sail_forward (robot [E][9] float64, ob [E][R][5] float64, n_rows [E] int64 or NULL
    -> action [E][2] float64, feat_joint [E][64] float32 or NULL)."""
    _fields_ = [("struct_size", C.c_uint32), ("E", C.c_int32), ("R", C.c_int32), ("reserved", C.c_int32)] + [
        (k, C.c_void_p) for k in ("robot", "ob", "n_rows", "action", "feat_joint")]


class EbcSailGradArgs(C.Structure):
    """include/ebcsim.h: one ebc_sail_grad (robot, ob, n_rows or NULL, target [E][2] float64, sample_mask [E] uint8 or NULL
    -> grad float32 [packed_floats], loss_sum float64 [1], count int64 [1], action [E][2] float64 or NULL)."""
    _fields_ = [("struct_size", C.c_uint32), ("E", C.c_int32), ("R", C.c_int32), ("grad_scale", C.c_float)] + [
        (k, C.c_void_p) for k in ("robot", "ob", "n_rows", "target", "sample_mask", "grad", "loss_sum", "count", "action")]


class EbcSailDaggerArgs(C.Structure):
    """include/ebcsim.h: one ebc_sail_dagger_k (K closed-loop steps of the attached SAIL network, the ORCA robot labelling
    every state; device pointers: take_expert [K][E] uint8 or NULL -> robot [K][E][9], ob [K][E][R][5], n_rows [K][E],
    learner_action / expert_action / robot_action_out [K][E][2], and reward / done / info [K][E] or NULL)."""
    _fields_ = [("struct_size", C.c_uint32), ("K", C.c_int32), ("human_policy", C.c_int32), ("flags", C.c_int32),
                ("expert_safety_space", C.c_double)] + [
        (k, C.c_void_p) for k in ("take_expert", "robot", "ob", "n_rows", "learner_action", "expert_action",
                                  "robot_action_out", "reward", "done", "info")]


CADRL_NET_LAYERS = 4


class EbcCadrlNetWeights(C.Structure):
    """include/ebcsim.h: the four Linear layers of a CADRL value network, host pointers in torch's layout [out][in]; widths =
    the row width, then the layers' units."""
    _fields_ = [("struct_size", C.c_uint32), ("n_layers", C.c_int32), ("widths", C.c_int32 * (CADRL_NET_LAYERS + 1)),
                ("reserved", C.c_int32), ("weight", C.c_void_p * CADRL_NET_LAYERS), ("bias", C.c_void_p * CADRL_NET_LAYERS)]


class EbcCadrlGradArgs(C.Structure):
    """include/ebcsim.h: one ebc_cadrl_grad (rows [B][R][T] float32, n_valid [B] int64 or NULL, target [B] float32, sample_mask
    [B] uint8 or NULL -> grad float32 [packed floats], loss_sum float64 [1], count int64 [1], value [B] float32 or NULL,
    min_row [B] int32 or NULL)."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("R", C.c_int32), ("T", C.c_int32), ("grad_scale", C.c_float),
                ("reserved", C.c_int32)] + [
        (k, C.c_void_p) for k in ("rows", "n_valid", "target", "sample_mask", "grad", "loss_sum", "count", "value", "min_row")]


SARL_NET_MAX_LAYERS = 16


class EbcSarlNetWeights(C.Structure):
    """include/ebcsim.h: the Linear layers of a SARL value network in the order mlp1, mlp2, attention, mlp3 (2 / 2 / 3 / 4 of
    them), host pointers in torch's layout [out][in]; widths = the layers' units."""
    _fields_ = [("struct_size", C.c_uint32), ("n_mlp1", C.c_int32), ("n_mlp2", C.c_int32), ("n_attention", C.c_int32),
                ("n_mlp3", C.c_int32), ("with_global_state", C.c_int32), ("self_state_dim", C.c_int32), ("input_dim", C.c_int32),
                ("widths", C.c_int32 * SARL_NET_MAX_LAYERS), ("weight", C.c_void_p * SARL_NET_MAX_LAYERS),
                ("bias", C.c_void_p * SARL_NET_MAX_LAYERS)]


class EbcSarlGradArgs(C.Structure):
    """include/ebcsim.h: one ebc_sarl_grad (rows [B][R][T] float32, n_valid [B] int64 or NULL, target [B] float32, sample_mask
    [B] uint8 or NULL -> grad float32 [packed floats], loss_sum float64 [1], count int64 [1], value [B] float32 or NULL,
    attention [B][R] float32 or NULL).  states_per_pass: 0 = the whole chunk at once, 4 / 2 / 1 = that many states at a time."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("R", C.c_int32), ("T", C.c_int32), ("grad_scale", C.c_float),
                ("states_per_pass", C.c_int32)] + [
        (k, C.c_void_p) for k in ("rows", "n_valid", "target", "sample_mask", "grad", "loss_sum", "count", "value", "attention")]


LSTM_NET_LAYERS = 8


class EbcLstmNetWeights(C.Structure):
    """include/ebcsim.h: an LSTM-RL value network (rl/policy/lstm_rl.py:9-69): the Linear layers of mlp1 (slots 0 .. 3; n_mlp1
    = 0 for ValueNetwork1) and mlp (slots 4 .. 7) and nn.LSTM's four tensors, host pointers in torch's layout."""
    _fields_ = [("struct_size", C.c_uint32), ("n_mlp1", C.c_int32), ("n_mlp", C.c_int32), ("self_state_dim", C.c_int32),
                ("input_dim", C.c_int32), ("lstm_input_dim", C.c_int32), ("hidden_dim", C.c_int32), ("reserved", C.c_int32),
                ("widths", C.c_int32 * LSTM_NET_LAYERS), ("weight", C.c_void_p * LSTM_NET_LAYERS),
                ("bias", C.c_void_p * LSTM_NET_LAYERS), ("w_ih", C.c_void_p), ("w_hh", C.c_void_p), ("b_ih", C.c_void_p),
                ("b_hh", C.c_void_p)]


class EbcLstmGradArgs(C.Structure):
    """include/ebcsim.h: one ebc_lstm_grad (rows [B][R][T] float32, n_valid [B] int64 or NULL, target [B] float32, sample_mask
    [B] uint8 or NULL -> grad float32 [packed floats], loss_sum float64 [1], count int64 [1], value [B] float32 or NULL,
    joint [B][S + H] float32 or NULL).  states_per_pass: 0 = the whole chunk at once, 4 / 2 / 1 = that many states at a time."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("R", C.c_int32), ("T", C.c_int32), ("grad_scale", C.c_float),
                ("states_per_pass", C.c_int32)] + [
        (k, C.c_void_p) for k in ("rows", "n_valid", "target", "sample_mask", "grad", "loss_sum", "count", "value", "joint")]
