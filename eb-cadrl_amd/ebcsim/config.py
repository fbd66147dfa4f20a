"""INI files -> EbcParams: the keys env.configure(), Reward.__init__ and the policy
config contribute to the hot path (simulator/env.py:58-87, simulator/utils/reward.py:18-75,
rl/policy/cadrl.py:72-81, rl/policy/sarl.py:103-110)."""
import configparser
import ctypes as C

from . import _abi

_NAN = float("nan")


def read_config(path):
    cfg = configparser.RawConfigParser()
    if not cfg.read(path):
        raise FileNotFoundError(path)
    return cfg


def _opt(cfg, section, key, default=_NAN):
    v = cfg.getfloat(section, key, fallback=None)
    return default if v is None else v


_HUMAN_ORCA = {"safety_space": "orca_safety_space", "neighbor_dist": "orca_neighbor_dist",
               "max_neighbors": "orca_max_neighbors", "time_horizon": "orca_time_horizon"}


def params_from_config(env_cfg, policy_cfg=None, robot_kinematics=None, policy="sarl", human_orca=None):
    """env_cfg / policy_cfg: RawConfigParser objects in the reference's schema.  policy: the robot's policy;
    "lstm_rl", "om_lstm_rl", "cadrl" and "sail" never read with_agent_type (rl/policy/lstm_rl.py:79-100, rl/policy/cadrl.py:66-82,
    rl/policy/sail.py:109-112), so their rows are 13 wide whatever [sarl] says.  human_orca: attributes of the humans'
    ORCA policy objects by the reference's names (safety_space, neighbor_dist, max_neighbors, time_horizon), which no
    config file sets (simulator/policy/orca.py:63-80): the defaults are that constructor's."""
    p = _abi.default_params()
    for k, v in (human_orca or {}).items():
        setattr(p, _HUMAN_ORCA[k], v)
    p.time_step = env_cfg.getfloat("env", "time_step")
    p.time_limit = env_cfg.getint("env", "time_limit")
    # env.configure itself raises without a [map] section (env.py:79); Reward alone does not
    p.map_size_m = _opt(env_cfg, "map", "map_size_m", 9.0) if env_cfg.has_section("map") else 9.0
    p.map_resolution = _opt(env_cfg, "map", "map_resolution", 0.1) if env_cfg.has_section("map") else 0.1
    p.robot_visible = int(env_cfg.getboolean("robot", "visible"))
    r = "reward"
    p.new_reward = int(env_cfg.getboolean(r, "new_reward", fallback=False))
    p.time_max = _opt(env_cfg, r, "time_max")
    p.max_goal_distance = _opt(env_cfg, r, "max_goal_distance")
    p.time_good = _opt(env_cfg, r, "time_good", 10.0)
    p.success_reward = env_cfg.getfloat(r, "success_reward")
    for i, k in enumerate(("adult", "bicycle", "child", "obstacle")):
        p.collision_penalty[i] = _opt(env_cfg, r, "collision_penalty_" + k)
    dd = env_cfg.getfloat(r, "discomfort_dist")
    df = env_cfg.getfloat(r, "discomfort_penalty_factor")
    for i, k in enumerate(("adult", "bicycle", "child")):
        p.discomfort_dist[i] = _opt(env_cfg, r, "discomfort_dist_" + k, dd)
        p.discomfort_factor[i] = _opt(env_cfg, r, "discomfort_penalty_factor_" + k, df)
    p.rotation_penalty_factor = env_cfg.getfloat(r, "rotation_penalty_factor")
    kin = robot_kinematics
    if policy_cfg is not None:
        if kin is None and policy_cfg.has_option("action_space", "kinematics"):
            kin = policy_cfg.get("action_space", "kinematics")
        if policy_cfg.has_option("sarl", "with_agent_type"):
            p.with_agent_type = int(policy_cfg.getboolean("sarl", "with_agent_type"))
        if policy in ("lstm_rl", "om_lstm_rl", "cadrl", "sail"):
            p.with_agent_type = 0
    kin = kin or "holonomic"
    # agents treat every non-"holonomic" string as rotational (agent.py:166-169);
    # rotate() keeps theta only for the literal "unicycle" (cadrl.py:261)
    p.robot_kinematics = _abi.HOLONOMIC if kin == "holonomic" else _abi.UNICYCLE
    p.rotate_unicycle = int(kin == "unicycle")
    return p


_HUMAN_POLICY_CODE = {"orca": _abi.HUMAN_ORCA, "linear": _abi.HUMAN_LINEAR}
_HUMAN_SECTIONS = (("adults", "adult_num"), ("bicycles", "bicycle_num"), ("children", "children_num"))


def human_policies_from_config(env_cfg):
    """The humans' policies of an env config -> (code, table).  Every entity type carries its own `policy` key
    (simulator/agents/agent.py:19, simulator/policy/policy_factory.py:10-14) and env.step asks every human's own policy
    (simulator/env.py:392-405); as the reference's env does, only the sections of the types the scene has are read.
    A uniform config returns the plain code (HUMAN_ORCA, also with no human at all, or HUMAN_LINEAR) and a table of three
    of it; a mix of `orca` and `linear` returns HUMAN_BY_TYPE and the table for BatchedEnv.set_human_policies (adult,
    bicycle, child; a type the scene does not have stays on ORCA).  Any other policy name is refused by name."""
    from .scene import SceneConfig
    sc = SceneConfig.from_config(env_cfg)
    names = {}
    for t, (section, count) in enumerate(_HUMAN_SECTIONS):
        if getattr(sc, count) and env_cfg.has_section(section):
            names[t] = env_cfg.get(section, "policy")
    bad = sorted(set(n for n in names.values() if n not in _HUMAN_POLICY_CODE))
    if bad:
        raise NotImplementedError("human policies %s: each entity type takes one of orca / linear" % bad)
    kinds = set(names.values())
    if len(kinds) <= 1:
        code = _HUMAN_POLICY_CODE[kinds.pop()] if kinds else _abi.HUMAN_ORCA
        return code, (code, code, code)
    return _abi.HUMAN_BY_TYPE, tuple(_HUMAN_POLICY_CODE[names[t]] if t in names else _abi.HUMAN_ORCA for t in range(3))


def occupancy_from_config(policy_cfg, policy="sarl"):
    """The occupancy maps a policy config asks for: an ebcsim.occupancy.OccupancySpec for policy "sarl" with [sarl]
    with_om = true (OM-SARL, multi_human_rl.py:151-227) and for policy "om_lstm_rl" with [lstm_rl] with_om = true
    (OM-LSTM), else None.  EbcParams has no field for them: the maps are built from the look-ahead's next_ob by
    ebc_occupancy_rows, outside the env handle.  "lstm_rl" with with_om is refused by its policy object, and the
    reference's CADRL.configure never reads with_om."""
    from .occupancy import OccupancySpec
    if policy == "om_lstm_rl":
        return OccupancySpec.from_config(policy_cfg, section="lstm_rl")
    return OccupancySpec.from_config(policy_cfg) if policy == "sarl" else None


_SCALARS = [n for n, t in _abi.EbcParams._fields_ if not hasattr(t, "_length_")]
_ARRAYS = [n for n, t in _abi.EbcParams._fields_ if hasattr(t, "_length_")]


def params_to_dict(p):
    d = {k: getattr(p, k) for k in _SCALARS}
    d.update({k: list(getattr(p, k)) for k in _ARRAYS})
    return d


def params_from_dict(d):
    p = _abi.default_params()
    for k in _SCALARS:
        if k in d and k != "struct_size":
            setattr(p, k, d[k])
    for k in _ARRAYS:
        if k in d:
            arr = getattr(p, k)
            for i, v in enumerate(d[k]):
                arr[i] = v
    p.struct_size = C.sizeof(_abi.EbcParams)
    return p
