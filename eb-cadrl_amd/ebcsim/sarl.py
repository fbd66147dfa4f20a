"""The robot's decision on device: look-ahead sweep + SARL value network + argmax.

What MultiHumanRL.predict does per decision in the reference (rl/policy/multi_human_rl.py:12-87):
for each of the 81 actions, env.onestep_lookahead -> rotate -> model -> value.  Here the sweep is
one ebc_lookahead launch that leaves rows_rotated[E][A][R][T] in HBM, and the value network
(rl/policy/sarl.py:38-82) runs on those rows as batched torch GEMMs (hipBLASLt on ROCm).  The
network is rebuilt functionally from the reference's state_dict, so its .pth files load as they
are.  Rows beyond an env's n_humans + n_static are masked out of the mean / softmax (the
reference never creates them)."""
import collections
import contextlib

import numpy as np
import torch

from . import _abi, _capi
from .mlp2 import Mlp2Block, pair_attend, pair_combine, pair_mask, pair_mean, pair_weights

_NativeMlp2 = Mlp2Block  # the block's name while it lived in this module


def uniform_v_pref(env):
    """The robots' preferred speed, which the whole batch must share: the reference builds the action space from it and
    discounts by gamma^(dt * v_pref) PER ROBOT (multi_human_rl.py:36-60, 72-76); a batch here has one action space and
    one discount, so robots that differ (a scene pool loaded from files can) are refused instead of silently taking
    env 0's."""
    v = np.asarray(env.get_state()["robot"], dtype=np.float64)[:, 7]
    if float(v.min()) != float(v.max()):
        raise ValueError("the robots of this batch differ in v_pref (%g .. %g): one action space and one discount per "
                         "batch — split the batch by v_pref" % (float(v.min()), float(v.max())))
    return float(v[0])


def reference_choice(values, check=True):
    """The reference's choice over the action values (multi_human_rl.py:36-80: max_value = -inf, then
    `if value > max_value`): values [E, A] float64 (torch or numpy) -> the chosen action of every env [E].  The first
    maximum wins and a NaN is never chosen; an env with no value above -inf raises the reference's ValueError (on a
    device that test is a host round trip; check=False skips it for values known to pass it)."""
    if isinstance(values, np.ndarray):
        v = np.where(np.isnan(values), -np.inf, values)
        if check and not bool((v > -np.inf).any(1).all()):
            raise ValueError("Value network is not well trained. ")
        return v.argmax(1)
    v = values.masked_fill(torch.isnan(values), float("-inf"))
    if check and not bool((v > float("-inf")).any(1).all()):
        raise ValueError("Value network is not well trained. ")
    return torch.argmax(v, dim=1)  # the first maximal index


def _mlp(x, layers, last_relu):
    """Linear (+ ReLU) stack.  On the GPU the bias and the ReLU ride in the GEMM's epilogue
    (torch._addmm_activation -> hipBLASLt): same values, no separate pass over the activations."""
    for i, (w, b) in enumerate(layers):
        relu = i != len(layers) - 1 or last_relu
        if (relu and x.is_cuda and x.dim() == 2 and not torch.is_grad_enabled()
                and hasattr(torch, "_addmm_activation")):  # inference only: the fused op has no derivative
            x = torch._addmm_activation(b, x, w.t(), use_gelu=False)
        else:
            x = torch.nn.functional.linear(x, w, b)
            if relu:
                x = torch.relu(x)
    return x


# What select_path knows of a network.  n_blocks: its libebcsim blocks (0: none — a CPU device, another dtype, shapes the
# blocks do not take, a training view that did not ask for them); gterm, frag: the gterm block / the fragment twins exist
PathFacts = collections.namedtuple("PathFacts", "with_global_state n_blocks mlp1_out mlp2_out mlp1_epilogue mlp2_epilogue gterm frag")
PATHS = ("folded_frag", "folded_rows", "exact_native", "blocks", "exact_mlp1", "torch")


def select_path(net, device_type, frag_handoff, native_exact, R, T, exact, want_weights, grad):
    """Which body SarlValueNet._forward runs -> one of PATHS.  net: PathFacts; device_type: of the rows; frag_handoff,
    native_exact: the network's two switches; R, T: the rows' shape; grad: torch.is_grad_enabled().  No device work."""
    if device_type != "cuda" or grad or not net.n_blocks:
        return "torch"  # every other path is the library's: inference on device rows, on blocks that exist
    if not exact:
        # folded: 16 <= R <= 32 (a 32-row tile touches at most three pairs) and the tile epilogue of both blocks
        if net.with_global_state and 16 <= R <= 32 and not want_weights and net.mlp1_epilogue and net.mlp2_epilogue:
            return "folded_frag" if frag_handoff and net.frag else "folded_rows"
        return "blocks"
    if not native_exact:
        return "torch"
    # every block in its float32 form: what the pair kernels between them take (else torch's float32 GEMMs)
    if (not want_weights and net.with_global_state and net.n_blocks >= 5 and net.gterm and net.mlp1_out % 4 == 0
            and net.mlp2_out % 4 == 0 and net.mlp2_out <= 256):
        return "exact_native"
    return "exact_mlp1" if T > 32 else "torch"  # rows wider than one input tile: mlp1 stays in the library


def block_kind(K0, H, O, wide):
    """How a two-layer stack K0 -> H -> O becomes a libebcsim block: "narrow" (ebc_mlp2_create_ex, wherever it fits that
    entry's limits — also in a network that asks for wide blocks), "wide" (ebc_mlp2_create_wide, only when asked for)
    or None."""
    if Mlp2Block.fits(K0, H, O):
        return "narrow"
    return "wide" if wide and Mlp2Block.fits_wide(K0, H, O) else None


def plan_blocks(mlp1, mlp2, attention, mlp3, wide):
    """The blocks of a network from its layers' shapes alone ((out, in) per layer and stack): None when the blocks do
    not apply, else the kinds (block_kind) of [mlp1, mlp2, attention, mlp3[:2], mlp3[2:4]] — as many of the last two as
    exist as blocks — and of the gterm block (None: torch).  No device work."""
    if not (len(mlp1) == 2 and len(mlp2) == 2 and len(attention) == 3 and attention[2][0] == 1):
        return None
    H1 = mlp1[-1][0]

    def kind(st):
        return block_kind(st[0][1], st[0][0], st[1][0], wide)
    kinds = [kind(mlp1), kind(mlp2), block_kind(H1, attention[0][0], attention[1][0], wide)]
    if None in kinds:
        return None
    if len(mlp3) >= 3 and kind(mlp3[:2]):
        kinds.append(kind(mlp3[:2]))
        if len(mlp3) == 4 and kind(mlp3[2:4]):
            kinds.append(kind(mlp3[2:4]))
    return kinds, block_kind(H1, H1, attention[0][0], wide)


def plan_facts(plan, mlp1, mlp2, with_global_state=True):
    """The PathFacts of a network whose blocks follow `plan` (plan_blocks; None: no blocks) — what _native_blocks reads
    off the blocks it has built.  mlp1, mlp2: the stacks' (out, in) per layer.  No device work."""
    if plan is None:
        return PathFacts(with_global_state, 0, 0, 0, False, False, False, False)
    kinds, gterm_kind = plan
    return PathFacts(with_global_state, len(kinds), mlp1[1][0], mlp2[1][0],
                     Mlp2Block.has_tile_epilogue(mlp1[0][1], mlp1[1][0], kinds[0] == "wide"),
                     Mlp2Block.has_tile_epilogue(mlp2[0][1], mlp2[1][0], kinds[1] == "wide"),
                     gterm_kind is not None, "wide" not in kinds[:3])


def _attention_weights(scores, n_valid):
    """The reference's masked softmax (sarl.py:69-71) over the rows that exist: scores [B, R] -> weights [B, R]."""
    e = torch.exp(scores) * (scores != 0).to(scores.dtype)
    if n_valid is not None:
        e = e * (torch.arange(scores.shape[1], device=scores.device)[None, :] < n_valid[:, None])
    return e / e.sum(dim=1, keepdim=True)


def chunk_values(forward, rows, n_valid, chunk_pairs, side_streams=None):
    """forward(pairs [n, R, T], n_valid [n] or None) -> [n] over rows [E, A, R, T] in chunks of whole envs, at most
    chunk_pairs pairs each (None: one chunk) -> (v [E, A] float32, envs per chunk).  side_streams: asked, when there is
    more than one chunk, for the streams the chunks alternate between (none: the caller's stream)."""
    E, A, R, T = rows.shape
    step = E if not chunk_pairs else max(1, int(chunk_pairs) // A)
    v = torch.empty((E, A), dtype=torch.float32, device=rows.device)
    n_chunks = -(-E // step)
    side = side_streams() if n_chunks > 1 and side_streams is not None else ()
    if side:
        # Chunks are independent, and a third of a chunk's kernels are small (the per-pair blocks: ~110 workgroups on
        # 256 CUs, each as long as its own critical path): chunks alternate between two streams, so one chunk's
        # small kernels run beside the other's wide ones.  An even number of equal chunks, no larger than asked for.
        n_chunks += n_chunks & 1
        step = -(-E // n_chunks)
        main = torch.cuda.current_stream(rows.device)
        ready = torch.cuda.Event()
        ready.record(main)
    for i, e0 in enumerate(range(0, E, step)):
        e1 = min(E, e0 + step)
        if side:
            side[i % len(side)].wait_event(ready)
        with torch.cuda.stream(side[i % len(side)]) if side else contextlib.nullcontext():
            nv = None if n_valid is None else n_valid[e0:e1].repeat_interleave(A)
            v[e0:e1] = forward(rows[e0:e1].reshape(-1, R, T), nv).view(e1 - e0, A)
    for s_ in side:
        main.wait_stream(s_)
    return v, step


class SarlValueNet(object):
    """rl/policy/sarl.py:9-82 (ValueNetwork), weights from its state_dict."""

    def __init__(self, state_dict, device="cpu", with_global_state=True, self_state_dim=6, dtype=torch.float32, wide=False):
        """dtype: torch.float32 reproduces the reference's values (2e-4); torch.bfloat16 runs the
        GEMMs on the bf16 matrix cores: measured on MI355X 2.3x faster per decision, but values move by
        up to 0.2 and only 63 % of the envs keep the fp32 action (positions lose their digits in bf16
        inputs) -- an experiment, not a parity path.
        wide: stacks wider than the two-layer block takes (up to 640 units: the reference's policy_x3 / policy_x4)
        become wide blocks (ebc_mlp2_create_wide) instead of sending the whole network to torch; stacks that fit the
        narrow block stay what they are."""
        def stack(prefix):
            idx = sorted({int(k.split(".")[1]) for k in state_dict if k.startswith(prefix + ".")})
            return [(state_dict["%s.%d.weight" % (prefix, i)].to(device=device, dtype=dtype),
                     state_dict["%s.%d.bias" % (prefix, i)].to(device=device, dtype=dtype))
                    for i in idx]
        # the blocks are built on first use: (mlp1, mlp2, attention[1:], mlp3 halves) as fused two-layer blocks
        self._init(stack("mlp1"), stack("mlp2"), stack("attention"), stack("mlp3"), with_global_state, self_state_dim,
                   torch.device(device), dtype, build_on_first_use=True, wide=wide)

    @classmethod
    def from_stacks(cls, mlp1, mlp2, attention, mlp3, with_global_state, self_state_dim, device, native=False, wide=False):
        """A float32 network on the caller's tensors ([(weight, bias), ...] per stack: a training module's parameters,
        which change under it).  Packed copies only on request: native builds the blocks from the current weights on a
        HIP device (enable_native), refresh_native() re-packs them after the weights have changed."""
        net = cls.__new__(cls)
        net._init(mlp1, mlp2, attention, mlp3, with_global_state, self_state_dim, torch.device(device), torch.float32,
                  build_on_first_use=False, wide=wide)
        if native and net.device.type == "cuda":
            net.enable_native()
        return net

    def _init(self, mlp1, mlp2, attention, mlp3, with_global_state, self_state_dim, device, dtype, build_on_first_use, wide=False):
        self.wide = bool(wide)
        self.mlp1, self.mlp2, self.attention, self.mlp3 = mlp1, mlp2, attention, mlp3
        self.with_global_state, self.self_state_dim = with_global_state, self_state_dim
        self.input_dim = mlp1[0][0].shape[1]
        self.device, self.dtype = device, dtype
        # the libebcsim blocks: none until _native_blocks() has built them, which it does once while _build_pending
        self._build_pending = bool(build_on_first_use)
        self._native, self._native_frag, self._gterm_block = None, (), None
        self._facts = PathFacts(with_global_state, 0, 0, 0, False, False, False, False)
        self.frag_handoff = True  # h1 goes from mlp1 to its consumers as fragments (False: as float32 rows)
        self.native_exact = True  # exact=True runs the library's float32 blocks (False: torch's float32 GEMMs)
        self.coarse_eps = None  # the refinement's bound: measured at the first bound-driven decision
        self.values_decidable = False
        self.native_forwards = self.folded_forwards = self.native_exact_forwards = self.native_exact_mlp1_forwards = 0
        self.native_refreshes = 0
        self._refine_host, self._side_streams = None, {}  # refine_stats' counters, from the first bound-driven decision on

    def _block_specs(self):
        """(layers, final) of every libebcsim block of this network, from its CURRENT tensors, or None when the blocks
        do not apply: [mlp1, mlp2, attention (h1 half of layer 0 + layer 1, layer 2 as the one-output tail),
        mlp3[:2], mlp3[2:4]] and the mean-state half of attention layer 0 as a block of its own."""
        plan = self._block_kinds()
        if plan is None:
            return None
        kinds, gterm_kind = plan
        H = self.mlp1[-1][0].shape[0]
        # attention = layer 0 on cat([h1, g]) | layer 1 | layer 2 (one output): the h1 half of layer 0
        # and layer 1 form the block, g's half enters as a per-pair term, layer 2 is the block's tail
        att = [(self.attention[0][0][:, :H], torch.zeros_like(self.attention[0][1])), self.attention[1]]
        specs = [(self.mlp1, None), (self.mlp2, None), (att, self.attention[2])]
        # mlp3's first two layers (the joint vector's widest ones) as a fourth block; its tail
        # (the reference's 200 -> 200 -> 1) stays with torch unless it is a two-layer block too
        if len(kinds) > 3:
            specs.append((self.mlp3[:2], None))
            if len(kinds) > 4:
                specs.append((self.mlp3[2:4], None))
        # the mean state's half of attention layer 0 (one 200 x 200 layer per PAIR) as a block too: the mean of
        # ReLU outputs is >= 0, so relu(I g) = g and [I | w0[:, H:]] is that layer in the two-layer form
        gterm = None
        if gterm_kind is not None:
            eye = torch.eye(H, dtype=torch.float32, device=self.device)
            gterm = ([(eye, torch.zeros(H, dtype=torch.float32, device=self.device)),
                      (self.attention[0][0][:, H:], self.attention[0][1])], None)
        return specs, gterm

    def _block_kinds(self):
        """plan_blocks of this network (which entry makes each block), or None when the blocks do not apply."""
        if not (self.device.type == "cuda" and self.dtype == torch.float32 and self.with_global_state):
            return None

        def shapes(st):
            return [tuple(w.shape) for w, _ in st]
        return plan_blocks(shapes(self.mlp1), shapes(self.mlp2), shapes(self.attention), shapes(self.mlp3), self.wide)

    def _native_blocks(self):
        """The two-layer stacks of the network as libebcsim blocks (inference on a HIP device,
        float32 weights, the reference's layer counts); None when that does not apply."""
        if self._build_pending:
            spec = self._block_specs()
            if spec is not None:
                idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
                # the shapes were checked above: a failure from here on is a HIP error and is raised, never a silent torch path
                specs, gterm = spec
                kinds, gterm_kind = self._block_kinds()
                self._gterm_block = None if gterm is None else Mlp2Block(gterm[0], idx, wide=gterm_kind == "wide")
                self._native = nat = tuple(Mlp2Block(layers, idx, final=final, wide=kind == "wide")
                                           for (layers, final), kind in zip(specs, kinds))
                # the two consumers of h1 once more, taking it as the fragments mlp1 leaves (no transposition, no splitting
                # in their input phase): mlp2 and the attention stack
                # (the wide block hands on rows only: the twins exist when all three stacks are narrow)
                if "wide" not in kinds[:3]:
                    self._native_frag = tuple(Mlp2Block(layers, idx, final=final, in_fragments=True) for layers, final in specs[1:3])
                self._facts = PathFacts(self.with_global_state, len(nat), nat[0].O, nat[1].O, nat[0].tile_epilogue,
                                        nat[1].tile_epilogue, self._gterm_block is not None, len(self._native_frag) == 2)
            self._build_pending = False
        return self._native

    def enable_native(self):
        """For a network whose tensors are a training module's parameters (SarlModule.as_value_net): build the blocks
        from the current weights; refresh_native() re-packs them after the weights have changed."""
        self._build_pending = True
        return self._native_blocks() is not None

    def refresh_native(self):
        """Re-pack every block from the network's current tensors, on the device (ebc_mlp2_update: no host copy): the
        training loop calls this once per round after its optimizer steps (rl/train.py:239-259), so its rollouts decide
        on the matrix-core blocks like every other decision.  Returns False when the network has no blocks."""
        if self._native is None:
            return False
        specs, gterm = self._block_specs()
        for blk, (layers, final) in zip(self._native + self._native_frag, specs + (specs[1:3] if self._native_frag else [])):
            blk.update(layers, final)
        if self._gterm_block is not None:
            self._gterm_block.update(gterm[0], None)
        self.native_refreshes += 1
        self.coarse_eps = None  # other weights: the refinement measures its bound again at the next decision
        return True

    def refresh_from(self, state_dict_or_trainer):
        """New weights for a network that decides: a state_dict of the reference's keys, or a sarl_train.SarlTrainer (its
        master copy, read in place on the device).  They are copied into the tensors this network was built on, then
        refresh_native() re-packs the blocks from them.  Returns what refresh_native returns."""
        sd = state_dict_or_trainer
        if hasattr(sd, "device_state_dict"):
            sd = sd.device_state_dict()
        with torch.no_grad():
            for name in ("mlp1", "mlp2", "attention", "mlp3"):
                for i, (w, b) in enumerate(getattr(self, name)):
                    w.copy_(sd["%s.%d.weight" % (name, 2 * i)])
                    b.copy_(sd["%s.%d.bias" % (name, 2 * i)])
        return self.refresh_native()

    # the pair kernels under the names they had as methods of this class
    _pair_mean = staticmethod(pair_mean)
    _pair_attend = staticmethod(pair_attend)
    _pair_combine = staticmethod(pair_combine)
    _pair_weights = staticmethod(pair_weights)
    _pair_mask = staticmethod(pair_mask)

    @classmethod
    def load(cls, path, device="cpu", **kw):
        return cls(torch.load(path, map_location="cpu"), device=device, **kw)

    def forward(self, rows, n_valid=None, want_weights=False, exact=False):
        """rows [B, R, T] float32; n_valid [B] (rows that exist) or None = all -> values [B]
        (with want_weights: (values, attention weights [B, R]), sarl.py:69-71).  exact: plain float32
        GEMMs instead of the split-bf16 matrix-core blocks (the arithmetic the reference's torch does)."""
        with torch.no_grad():
            return self._forward(rows, n_valid, want_weights, exact)

    # |value of the split-bf16 blocks - float32 value| of the NETWORK OUTPUT (before reward and discount) depends on the
    # weights: <= 3.3e-4 with the shipped eb-cadrl weights on the bench workload (its attention scores are large: a
    # 2^-16 relative error there is e-4 behind the exponential), <= 1.2e-6 with random-init weights, <= 1.5e-5 on the
    # reference's golden episodes.  The bound the refinement works with is therefore MEASURED per network
    # (calibrate_eps: both forms on a sample of the decision batch, times EPS_MARGIN; again after every
    # refresh_native) and CHECKED at every decision on the candidates that were re-evaluated: one of them off by more
    # than the bound widens it and the decision is taken again.  COARSE_EPS_MAX: a network whose blocks are worse than
    # this is refused (the matrix-core path is not fit to rank its values).
    EPS_MARGIN = 2.0
    EPS_FLOOR = 2e-6
    COARSE_EPS_MAX = 5e-3
    REFINE_CAP = 1 << 30  # no cap by default: every candidate within the bound is re-evaluated (an env near its goal can have dozens)

    def calibrate_eps(self, pairs, n_valid=None, sample=2048):
        """Measure |matrix-core value - float32 value| on a strided sample of `pairs` [n, R, T] and set the bound the
        refinement uses (coarse_eps).  One host sync."""
        n = pairs.shape[0]
        idx = torch.arange(0, n, max(1, n // int(sample)), device=pairs.device)[:int(sample)]
        sel = pairs[idx]
        nv = None if n_valid is None else n_valid[idx]
        err = float((self.forward(sel, nv) - self.forward(sel, nv, exact=True)).abs().max())
        if not err <= self.COARSE_EPS_MAX:
            raise RuntimeError("SarlValueNet: the matrix-core blocks are off by %.2e on this network: not fit to rank its values" % err)
        self.coarse_eps = max(self.EPS_MARGIN * err, self.EPS_FLOOR)
        return self.coarse_eps

    CHUNK_STREAMS = 2  # streams the chunks of a decision batch alternate between (1: the caller's stream only)

    def _chunk_streams(self, device):
        if self.CHUNK_STREAMS < 2:
            return ()
        key = (str(device), self.CHUNK_STREAMS)
        if key not in self._side_streams:
            self._side_streams[key] = tuple(torch.cuda.Stream(device=device) for _ in range(self.CHUNK_STREAMS))
        return self._side_streams[key]

    def action_values(self, rows, reward, discount, n_valid=None, refine=None, chunk_pairs=None, eps=None):
        """reward + discount * V(rows) for every candidate action (multi_human_rl.py:72-76): rows
        [E, A, R, T] float32, reward [E, A] float64, n_valid [E] or None -> values [E, A] float64.
        The matrix-core blocks' values carry a split-bf16 error (coarse_eps, measured per network) and the float32
        network's best two actions can be as close as 4e-7, so the DECISION is made on float32 values: every candidate
        whose coarse value lies within 2 * discount * eps of the env's coarse best — any action whose float32 value could
        be the maximum — is re-evaluated with the float32 form of the same blocks (ebc_mlp2_forward_f32) before the
        caller takes the argmax (an env with a single such candidate is decided already and keeps its matrix-core
        value); the bound is checked on those candidates (a violation widens it and repeats the selection from the
        coarse values; after four violations every action of the batch is re-evaluated).  An env whose coarse values
        hold a NaN, or none above -inf, is re-evaluated in full; one whose float32 values have none above -inf raises
        the reference's ValueError (values_decidable: True when no env needed that; the first maximum is then the choice).
        refine: None = this bound-driven set; an int k = the best k candidates of every env (0 = the
        matrix-core values as they are).  refine_stats counts decisions, re-evaluated candidates, envs with more than two
        of them, the largest set, bound violations and fallbacks to the whole batch."""
        self.values_decidable = False  # set where the float32 selection leaves no NaN and a value above -inf in every env
        native = rows.is_cuda and self._native_blocks() is not None
        v, step = chunk_values(self.forward, rows, n_valid, chunk_pairs, (lambda: self._chunk_streams(rows.device)) if native else None)
        if native and refine is None:
            return self._refine_within_bound(rows, reward, discount, n_valid, v, step, eps)
        values = reward + discount * v.to(torch.float64)
        if native and refine != 0:
            self._refine_top_k(rows, reward, discount, n_valid, values, int(refine))
        return values

    def _refine_top_k(self, rows, reward, discount, n_valid, values, k):
        """The best k candidates of every env by coarse value, re-evaluated in float32 into `values`."""
        E, A = values.shape
        k = min(k, A)
        act_i = torch.topk(values, k, dim=1).indices.reshape(-1)
        env_i = torch.arange(E, device=rows.device)[:, None].expand(E, k).reshape(-1)
        nv = None if n_valid is None else n_valid[env_i]
        values[env_i, act_i] = reward[env_i, act_i] + discount * self.forward(rows[env_i, act_i], nv, exact=True).to(torch.float64)

    def _rank(self, rows, n_valid, reward, discount, v, eps):
        """The bound (given, kept or measured now), then values, every env's actions by value and the size of its
        near-best set in ONE launch (ebc_decision_rank) -> (reward float64, values [E, A], order [E, A], counts [E])."""
        E, A, R, T = rows.shape
        if eps is not None:
            self.coarse_eps = float(eps)
        elif self.coarse_eps is None:
            self.calibrate_eps(rows.reshape(E * A, R, T), None if n_valid is None else n_valid.repeat_interleave(A))
        values = torch.empty((E, A), dtype=torch.float64, device=rows.device)
        order = torch.empty((E, A), dtype=torch.int32, device=rows.device)
        count_dev = torch.empty((E,), dtype=torch.int32, device=rows.device)
        reward = reward.to(torch.float64).contiguous()
        _capi.check(_capi.lib().ebc_decision_rank(torch.cuda.current_stream(rows.device).cuda_stream, v.data_ptr(), reward.data_ptr(),
                                                  float(discount), 2.0 * float(discount) * self.coarse_eps, E, A,
                                                  values.data_ptr(), order.data_ptr(), count_dev.data_ptr()))
        return reward, values, order, count_dev

    def _refine_within_bound(self, rows, reward, discount, n_valid, v, step, eps):
        """The bound-driven refinement of action_values: the candidates that could be the float32 best of their env,
        re-evaluated in float32, with the bound checked on them (a violation widens it and selects again)."""
        E, A = v.shape
        reward, values, order, count_dev = self._rank(rows, n_valid, reward, discount, v, eps)
        if self._refine_host is None:
            self._refine_host = {"decisions": 0, "candidates": 0, "over2": 0, "capped": 0, "max_set": 0,
                                 "bound_violations": 0, "contested": 0, "fallbacks": 0}
        st = self._refine_host
        k = min(self.REFINE_CAP, A)
        discount = float(discount)
        # the candidates that could be the float32 best: a PREFIX of every env's sorted row, so the set is its length.
        # The lengths go to the host in one 8 KB copy — the one host round trip of the selection — and the index lists
        # and the counters are made there: torch.nonzero plus four .item() reads were five round trips with an idle GPU
        # and a dozen launch-bound little kernels behind each.
        count = count_dev.cpu().numpy().astype(np.int64)
        # -1: the coarse values cannot rank the env (a NaN among them, or none above -inf).  All of its actions are
        # re-evaluated, once, and its errors are not held against the bound (a coarse NaN has no error to measure); then
        # the reference's rule decides it, and without a value above -inf it is the reference's ValueError.
        full = count < 0
        n_full = int(full.sum())
        if n_full:
            fe = np.nonzero(full)[0]
            self._apply_exact(rows, n_valid, np.repeat(fe, A), np.tile(np.arange(A), n_full), reward, v, discount, values,
                              torch.zeros(1, dtype=torch.float32, device=rows.device), E)
            fe_dev = torch.from_numpy(fe).to(rows.device)
            if not bool((values[fe_dev] > float("-inf")).any(1).all()):
                raise ValueError("Value network is not well trained. ")
        count, n_cand = self._settle_bound(rows, n_valid, reward, discount, v, values, order, count, full, k)
        if count is None:
            # every widening pulled in a larger error: the bound has not settled, so every action of the batch is
            # re-evaluated in float32 and the decision is the float32 network's; the errors seen widen the bound
            live = np.nonzero(~full)[0]
            worst_dev = torch.zeros(1, dtype=torch.float32, device=rows.device)
            self._apply_exact(rows, n_valid, np.repeat(live, A), np.tile(np.arange(A), len(live)), reward, v, discount, values,
                              worst_dev, step)
            self.coarse_eps = max(self.coarse_eps, self.EPS_MARGIN * self._fit_to_rank(float(worst_dev)))
            st["fallbacks"] += 1
            count = np.full(E, A, dtype=np.int64)
            n_cand = len(live) * A
        st["decisions"] += E
        st["candidates"] += n_cand + n_full * A
        st["contested"] += int((count > 1).sum())
        st["over2"] += int((count > 2).sum())
        st["capped"] += int((count >= k).sum()) if k < A else 0
        st["max_set"] = max(st["max_set"], int(count.max()) if E else 0)
        # no NaN is left and every env has a value above -inf: a NaN in the coarse values flags its env, any other NaN
        # error raised above; the flagged envs' float32 values may hold NaNs (reference_choice masks them)
        self.values_decidable = n_full == 0
        return values

    def _fit_to_rank(self, worst):
        if not worst <= self.COARSE_EPS_MAX:
            raise RuntimeError("SarlValueNet: matrix-core values off by %.2e: not fit to rank this network's values" % worst)
        return worst

    def _settle_bound(self, rows, n_valid, reward, discount, v, values, order, count, full, k):
        """Up to four selections: the candidates of every env (a prefix of `order`, `count` long, at most k) re-evaluated
        in float32 into `values`; the largest error among them within the bound ends it, else the bound is widened and
        the prefixes are taken again.  -> (the sizes used, candidates re-evaluated), or (None, 0) when four were not enough."""
        E, A = values.shape
        ar = np.arange(E)
        ranked = None
        for attempt in range(4):
            if attempt:  # the bound was widened: the sizes again, from the COARSE values by rank (a longer prefix)
                bound = 2.0 * discount * self.coarse_eps
                if ranked is None:
                    ranked = (reward + discount * v.to(torch.float64)).gather(1, order.to(torch.int64))
                count = (ranked >= (ranked[:, :1] - bound)).sum(1).cpu().numpy()
            count = np.where(full, A, np.minimum(count, k))
            # an env with ONE candidate is decided: every other action's float32 value lies below that one's
            sizes = np.where((count > 1) & ~full, count, 0)
            n_cand = int(sizes.sum())
            if n_cand == 0:
                return count, n_cand
            env_h = np.repeat(ar, sizes)
            slot_h = np.arange(n_cand) - np.repeat(np.cumsum(sizes) - sizes, sizes)
            idx = torch.from_numpy(np.stack([env_h, slot_h])).to(rows.device, non_blocking=True)
            act_i = order[idx[0], idx[1]].to(torch.int64)
            # the candidates' float32 values into `values`, and the bound checked where it matters: one launch, one read
            # (a widened bound above selects a longer prefix and applies again)
            worst_dev = torch.zeros(1, dtype=torch.float32, device=rows.device)
            self._apply_exact(rows, n_valid, idx[0], act_i, reward, v, discount, values, worst_dev, E)
            worst = float(worst_dev)
            if worst <= self.coarse_eps:
                return count, n_cand
            self._refine_host["bound_violations"] += 1
            self.coarse_eps = self.EPS_MARGIN * self._fit_to_rank(worst)
        return None, 0

    def _apply_exact(self, rows, n_valid, env_i, act_i, reward, v, discount, values, worst_dev, chunk_envs):
        """The float32 form of the network on the pairs (env_i, act_i) (host arrays or device tensors), written into
        `values` as reward + discount * value with the largest |float32 - coarse| among them into worst_dev
        (ebc_decision_apply; worst_dev is not read here).  At most chunk_envs * A pairs per forward."""
        A = values.shape[1]
        if not torch.is_tensor(env_i):
            env_i, act_i = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.int64)).to(rows.device) for t in (env_i, act_i))
        n, step = int(env_i.shape[0]), max(1, int(chunk_envs)) * A
        for p0 in range(0, n, step):
            e_i, a_i = (env_i, act_i) if step >= n else (env_i[p0:p0 + step].contiguous(), act_i[p0:p0 + step].contiguous())
            nv = None if n_valid is None else n_valid[e_i]
            exact = self.forward(rows[e_i, a_i], nv, exact=True).to(torch.float32).contiguous()
            _capi.check(_capi.lib().ebc_decision_apply(torch.cuda.current_stream(rows.device).cuda_stream, exact.data_ptr(), v.data_ptr(),
                                                       e_i.data_ptr(), a_i.data_ptr(), reward.data_ptr(), discount, A,
                                                       int(e_i.shape[0]), values.data_ptr(), worst_dev.data_ptr()))

    @property
    def refine_stats(self):
        """Counters of the bound-driven re-evaluation since the network was made: decisions, re-evaluated candidates, envs
        with more than one / more than two candidates, sets cut at REFINE_CAP, the largest set, bound violations, and
        decisions whose bound did not settle in four attempts (every action re-evaluated)."""
        return None if self._refine_host is None else dict(self._refine_host)

    def path_for(self, rows, want_weights=False, exact=False):
        """The path of select_path that _forward takes on rows [B, R, T] under the current autograd mode."""
        grad = torch.is_grad_enabled()
        if rows.is_cuda and not grad:
            self._native_blocks()  # built on first use; select_path reads what they are from _facts
        return select_path(self._facts, rows.device.type, self.frag_handoff, self.native_exact, rows.shape[1], rows.shape[2],
                           exact, want_weights, grad)

    def _forward(self, rows, n_valid=None, want_weights=False, exact=False):
        rows = rows.to(self.dtype)
        nv64 = None if n_valid is None else n_valid.to(torch.int64).contiguous()
        return self._BODIES[self.path_for(rows, want_weights, exact)](self, rows, n_valid, nv64, want_weights, exact)

    def _gterm(self, g, entry=None):
        """The mean state's half of attention layer 0, once per pair [B, A1]: through `entry` (the gterm block or its
        float32 form), else torch.  Layer 0 acts on cat([h1, g]) without the concatenation being built."""
        if entry is not None:
            return entry(g, False)
        w0, b0 = self.attention[0]
        return torch.nn.functional.linear(g, w0[:, g.shape[1]:], b0)

    def _value(self, rows, attended, nat, f32=False):
        """mlp3 on cat([self state, attended]) -> values [B]: on the blocks `nat` has for it (f32: their float32 form),
        torch for the layers it has none for."""
        joint = torch.cat([rows[:, 0, :self.self_state_dim], attended], dim=1)
        if nat is not None and len(nat) > 4:
            first, second = (nat[3].f32, nat[4].f32) if f32 else (nat[3], nat[4])
            return second(first(joint, True), False).squeeze(1)
        if nat is not None and len(nat) > 3:
            return _mlp(nat[3](joint, True), self.mlp3[2:], False).squeeze(1).to(torch.float32)
        return _mlp(joint, self.mlp3, False).squeeze(1).to(torch.float32)

    def _glue(self, rows, n_valid, nv64, want_weights, h1, feat, nat, on_library):
        """From h1 [B * R, H] and the features [B, R, F] to the values: the pair mean, the attention scores, the
        weighted feature sum and mlp3.  nat: the blocks for the attention stack and mlp3, or None = torch;
        on_library: the forward is the library's (blocks, or exact on the device without autograd)."""
        B, R, _ = rows.shape
        # the pair glue as two HIP kernels (plain float32 arithmetic: also behind the float32 GEMMs of the exact pass,
        # where they replace a dozen element-wise launches)
        fused = on_library and h1.shape[1] % 4 == 0 and feat.shape[2] % 4 == 0 and feat.shape[2] <= 256
        if not self.with_global_state:
            scores = _mlp(h1, self.attention, False).view(B, R)
        else:
            if fused:
                g = pair_mean(h1, nv64, B, R)
            elif n_valid is None:
                g = h1.view(B, R, -1).sum(1) / float(R)
            else:  # [B, H]: the mean of the pair's rows that exist
                valid = (torch.arange(R, device=rows.device)[None, :] < n_valid[:, None])
                g = (h1.view(B, R, -1) * valid[:, :, None]).sum(1) / n_valid.to(rows.dtype).clamp(min=1)[:, None]
            gterm = self._gterm(g)  # added to every row of the pair
            if nat is not None:
                scores = nat[2](h1, False, row_bias=gterm, group_rows=R).view(B, R)
            else:
                H = h1.shape[1]
                a1 = torch.nn.functional.linear(h1, self.attention[0][0][:, :H]).view(B, R, -1)
                a1 = torch.relu(a1 + gterm[:, None, :]).view(B * R, -1)
                scores = _mlp(a1, self.attention[1:], False).view(B, R)
        if fused:
            attended = pair_attend(scores, feat, nv64, B, R)
        else:
            attended = (_attention_weights(scores, n_valid).unsqueeze(2) * feat).sum(dim=1)
        value = self._value(rows, attended, nat)
        return (value, _attention_weights(scores, n_valid)) if want_weights else value

    # one body per path of select_path
    def _folded_frag(self, rows, n_valid, nv64, want_weights, exact):
        """mlp1 leaves the pair sums of h1 beside h1, the attention stack runs BEFORE mlp2, and mlp2 multiplies its rows
        by the attention weights and leaves only their pair sums — the [B * R][F] features are never written, nothing
        reads h1 a second time for the mean.  h1 never exists as float32 rows: mlp1 leaves it split and in fragment
        order, its consumers load that."""
        (B, R, T), M = rows.shape, rows.shape[0] * rows.shape[1]
        self.native_forwards, self.folded_forwards = self.native_forwards + 1, self.folded_forwards + 1
        nat, natf = self._native, self._native_frag
        mask = None if nv64 is None else pair_mask(nv64, B, R)
        h1f = Mlp2Block.frag_buffer(M, nat[0].O, rows.device)
        _, part = nat[0].forward_ex(M, True, x=rows.reshape(M, T), want_y=False, seg_rows=R, row_weight=mask,
                                    want_partial=True, frag_out=h1f)
        gterm = self._gterm(pair_combine(part, nv64, B, R, True), self._gterm_block)
        scores, _ = natf[1].forward_ex(M, False, frag_in=h1f, row_bias=gterm, group_rows=R)
        w = pair_weights(scores, nv64, B, R)
        _, part = natf[0].forward_ex(M, False, frag_in=h1f, want_y=False, seg_rows=R, row_weight=w, want_partial=True)
        return self._value(rows, pair_combine(part, None, B, R, False), nat)

    def _folded_rows(self, rows, n_valid, nv64, want_weights, exact):
        """The folded path with h1 handed on as float32 rows (ebc_mlp2_forward_reduce)."""
        B, R, T = rows.shape
        self.native_forwards, self.folded_forwards = self.native_forwards + 1, self.folded_forwards + 1
        nat = self._native
        mask = None if nv64 is None else pair_mask(nv64, B, R)
        h1, part = nat[0].reduce(rows.reshape(B * R, T), True, R, mask)
        gterm = self._gterm(pair_combine(part, nv64, B, R, True), self._gterm_block)
        scores = nat[2](h1, False, row_bias=gterm, group_rows=R)
        w = pair_weights(scores, nv64, B, R)
        _, part = nat[1].reduce(h1, False, R, w, store=False)
        return self._value(rows, pair_combine(part, None, B, R, False), nat)

    def _exact_native(self, rows, n_valid, nv64, want_weights, exact):
        """exact on a HIP device: the float32 form of the same blocks (vector ALUs, fmaf into float32 sums) with the pair
        kernels in between — the whole refinement stays inside the library (no hipBLASLt GEMMs, no element-wise launches)."""
        B, R, T = rows.shape
        self.native_exact_forwards += 1
        nat = self._native
        h1 = nat[0].f32(rows.reshape(B * R, T), True)
        feat = nat[1].f32(h1, False).view(B, R, -1)
        gterm = self._gterm(pair_mean(h1, nv64, B, R), self._gterm_block.f32)
        scores = nat[2].f32(h1, False, row_bias=gterm, group_rows=R).view(B, R)
        return self._value(rows, pair_attend(scores, feat, nv64, B, R), nat, f32=True)

    def _blocks(self, rows, n_valid, nv64, want_weights, exact):
        """The general native path: every stack a block, the pair glue as kernels where their widths allow."""
        B, R, T = rows.shape
        self.native_forwards += 1  # tests assert the HIP path ran
        h1 = self._native[0](rows.reshape(B * R, T), True)
        feat = self._native[1](h1, False).view(B, R, -1)
        return self._glue(rows, n_valid, nv64, want_weights, h1, feat, self._native, True)

    def _exact_mlp1(self, rows, n_valid, nv64, want_weights, exact):
        """Rows wider than one input tile (occupancy maps appended) on a network the pair kernels do not take (mlp2 with
        50 outputs): mlp1, the one stack that sees the wide rows, as the library's float32 block, torch for the rest."""
        B, R, T = rows.shape
        self.native_exact_mlp1_forwards += 1
        h1 = self._native[0].f32(rows.reshape(B * R, T), True)
        feat = _mlp(h1, self.mlp2, False).view(B, R, -1)
        return self._glue(rows, n_valid, nv64, want_weights, h1, feat, None, True)

    def _torch(self, rows, n_valid, nv64, want_weights, exact):
        """torch's GEMMs: the CPU, training (autograd), networks without blocks, exact=True where no float32 block applies."""
        B, R, T = rows.shape
        h1 = _mlp(rows.reshape(B * R, T), self.mlp1, True)
        feat = _mlp(h1, self.mlp2, False).view(B, R, -1)
        return self._glue(rows, n_valid, nv64, want_weights, h1, feat, None, exact and rows.is_cuda and not torch.is_grad_enabled())

    _BODIES = {"folded_frag": _folded_frag, "folded_rows": _folded_rows, "exact_native": _exact_native, "blocks": _blocks,
               "exact_mlp1": _exact_mlp1, "torch": _torch}


class DeviceSarlPolicy(object):
    """Greedy SARL decisions for a whole BatchedEnv (phase "test": no epsilon draw)."""

    def __init__(self, net, actions, gamma, chunk_rows=1 << 21, refine=None, om=None):
        """refine: None = every candidate within the matrix-core blocks' error bound of the env's best is recomputed in
        float32 before the argmax (SarlValueNet.action_values); an int k = the best k; 0 = the matrix-core values as
        they are.  om: an ebcsim.occupancy.OccupancySpec = OM-SARL (multi_human_rl.py:62-69): the sweep leaves next_ob
        as well, ebc_occupancy_rows appends every env's maps to the rows of all its actions, and the network (whose
        mlp1 is T + W wide) runs on those; None = no maps."""
        self.refine = None if refine is None else int(refine)
        self.om = om
        self.net = net
        self.actions_np = np.ascontiguousarray(actions, dtype=np.float64)
        self.gamma = float(gamma)
        self.chunk_rows = int(chunk_rows)
        self._bufs = self._env_key = None

    def values_from(self, rows, reward, n_valid, dt, v_pref):
        """rows [E, A, R, T] float32, reward [E, A] float64 -> values [E, A] float64
        (multi_human_rl.py:72-76: reward + gamma^(dt * v_pref) * V)."""
        R = rows.shape[2]
        return self.net.action_values(rows, reward, self.gamma ** (dt * v_pref), n_valid, refine=self.refine,
                                      chunk_pairs=max(1, self.chunk_rows // R))

    def decide(self, env, human_policy=_abi.HUMAN_ORCA):
        """env: BatchedEnv on this net's device.  Returns (actions [E, 2] float64 CUDA tensor,
        values [E, A]); the human velocities stay cached for a following EBC_HUMAN_CACHED step.
        The sweep's buffers are taken when an env batch is first seen (a different batch re-allocates
        them).  The rows that exist per env are read from the DEVICE state at every decision when the
        handle may run scenes of different sizes (`env.ragged`: a ragged reset batch or scene pool), so a
        restart inside the step cannot leave them stale; `self.n_valid` is what the last decision used."""
        dev = self.net.device
        A = len(self.actions_np)
        key = (id(env), env.E, env.R, env.T)
        if self._bufs is None or self._env_key != key:  # buffers are sized for ONE env batch
            self._env_key = key
            self._acts = torch.tensor(self.actions_np, dtype=torch.float64, device=dev)
            self._bufs = env.alloc_lookahead_outputs(A, ("reward", "rows_rotated") + (("next_ob",) if self.om is not None else ()))
            self._n_valid = torch.full((env.E,), env.R, dtype=torch.int64, device=dev)
            self._v_pref = uniform_v_pref(env)
            if self.om is not None:
                wide = env.T + self.om.width
                if self.net.input_dim != wide:
                    raise ValueError("the value network takes rows %d wide, occupancy maps make them %d + %d" % (
                        self.net.input_dim, env.T, self.om.width))
                self._wide = torch.empty((env.E, A, env.R, wide), dtype=torch.float32, device=dev)
        self.n_valid = None
        if getattr(env, "ragged", False):
            env.row_counts_device(self._n_valid)
            self.n_valid = self._n_valid
        env.lookahead_device(self._acts, self._bufs, human_policy=human_policy)
        rows = self._bufs["rows_rotated"]
        if self.om is not None:
            from .occupancy import occupancy_rows_device
            rows = occupancy_rows_device(self._bufs["next_ob"], self.n_valid, self.om, rows=rows, wide_out=self._wide,
                                         want_om=False)[1]
        values = self.values_from(rows, self._bufs["reward"], self.n_valid, env.params.time_step, self._v_pref)
        return self._acts[self.choose(values)], values

    def choose(self, values):
        """The reference's choice over values [E, A] (reference_choice).  Values that action_values' float32 selection
        left without a NaN and with a value above -inf in every env (values_decidable) need neither the NaN mask nor
        the host round trip of the check: the first maximum is the reference's choice."""
        if self.net.values_decidable:
            return torch.argmax(values, dim=1)
        return reference_choice(values)
