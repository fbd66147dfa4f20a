"""ebcsim.grad_train holds once what cadrl_train, sarl_train and lstm_train used to hold three times.  Two things must stay
true however the code is folded: the three modules keep every public name they had (the lists below are dir() of the three
modules before the fold, names without a leading underscore), and the trainers and network objects take the shared
methods from the one base, not from a copy of their own."""
import inspect

import pytest

from ebcsim import cadrl_train, grad_train, lstm_train, sarl_train
from ebcsim.cadrl_train import CadrlNet, CadrlTrainer
from ebcsim.lstm_train import LstmNet, LstmTrainer
from ebcsim.sarl_train import SarlNet, SarlTrainer

PUBLIC = {
    cadrl_train: ['C', 'CadrlModule', 'CadrlNet', 'CadrlTrainer', 'CadrlValueNet', 'DeviceCadrlPolicy', 'LAYER_KEYS', 'MAX_IN', 'MAX_ROWS',
                  'MAX_WIDTH', 'collections', 'live_states', 'optimize_batch', 'optimize_epoch', 'os', 'pack_state_dict', 'packed_floats',
                  'pad4', 'run_cadrl_training', 'torch', 'unpack_to_state_dict', 'widths_of'],
    sarl_train: ['C', 'DeviceSarlPolicy', 'LAYER_KEYS', 'MAX_IN', 'MAX_OM', 'MAX_WIDE', 'MAX_WIDTH', 'PASS_SIZES', 'PassChoice', 'STACKS',
                 'SarlModule', 'SarlNet', 'SarlTrainer', 'SarlValueNet', 'checked_states_per_pass', 'collections', 'layer_inputs',
                 'live_states', 'module_of', 'optimize_batch', 'optimize_epoch', 'os', 'pack_state_dict', 'packed_floats', 'pad4',
                 'pick_states_per_pass', 'run_sarl_training', 'shape_of', 'torch', 'unpack_to_state_dict', 'widths_of'],
    lstm_train: ['C', 'DISTANCE_COLUMN', 'DeviceSarlPolicy', 'LSTM_KEYS', 'LstmModule', 'LstmNet', 'LstmTrainer', 'LstmValueNet', 'MAX_DIM',
                 'MAX_IN', 'MAX_WIDTH', 'MLP1_KEYS', 'MLP_KEYS', 'PASS_SIZES', 'PassChoice', 'checked_states_per_pass', 'collections',
                 'distance_order', 'live_states', 'module_of', 'optimize_batch', 'optimize_epoch', 'os', 'pack_state_dict', 'packed_floats',
                 'pad4', 'pick_states_per_pass', 'run_lstm_training', 'shape_of', 'sort_rows_by_distance', 'torch', 'unpack_to_state_dict'],
}
SHARED = ("pad4", "live_states", "optimize_epoch", "optimize_batch", "_finite", "PASS_SIZES", "checked_states_per_pass",
          "pick_states_per_pass", "PassChoice")
TRAINER_METHODS = ("set_learning_rate", "state_dict", "device_state_dict", "save", "load_state_dict", "push_weights", "step")
NET_METHODS = ("packed_floats", "get_packed", "set_packed", "grad_max_rows", "__del__")


@pytest.mark.parametrize("module", list(PUBLIC), ids=lambda m: m.__name__.split(".")[-1])
def test_the_modules_keep_their_public_names(module):
    have = {n for n in dir(module) if not n.startswith("_")}
    assert not set(PUBLIC[module]) - have, sorted(set(PUBLIC[module]) - have)


def test_what_the_modules_re_export_is_grad_trains():
    from ebcsim.lstm_train import PassChoice, optimize_batch, pad4
    assert PassChoice is grad_train.PassChoice and optimize_batch is grad_train.optimize_batch and pad4 is grad_train.pad4
    for module in PUBLIC:
        for name in SHARED:
            if name in PUBLIC[module] or name == "_finite":
                assert getattr(module, name) is getattr(grad_train, name), (module.__name__, name)


@pytest.mark.parametrize("cls", [CadrlTrainer, SarlTrainer, LstmTrainer], ids=lambda c: c.__name__)
def test_the_trainers_take_the_shared_methods_from_the_base(cls):
    assert issubclass(cls, grad_train.GradTrainer)
    for name in TRAINER_METHODS + ("_loss_and_grad",):
        assert name not in vars(cls), name
        assert getattr(cls, name) is getattr(grad_train.GradTrainer, name), name
    # the one body of loss_and_grad is the base's: the class's own is its signature and docstring around one call
    assert cls.loss_and_grad.__code__.co_names == ("_loss_and_grad",)


@pytest.mark.parametrize("cls", [CadrlNet, SarlNet, LstmNet], ids=lambda c: c.__name__)
def test_the_network_objects_take_the_shared_methods_from_the_base(cls):
    assert issubclass(cls, grad_train.GradNet)
    for name in NET_METHODS + ("_grad",):
        assert name not in vars(cls), name
        assert getattr(cls, name) is getattr(grad_train.GradNet, name), name
    assert cls.KIND in ("cadrl", "sarl", "lstm") and cls.ARGS.__name__ == "Ebc%sGradArgs" % cls.KIND.capitalize()


def test_the_signatures_are_what_they_were():
    sig = lambda f: str(inspect.signature(f))  # noqa: E731
    schedule = ("il_steps=0, il_epochs=0, il_learning_rate=0.01, il_safety_space=0.15, rl_learning_rate=0.001, train_iterations=0, "
                "steps_per_iteration=1, train_batches=100, batch_size=100, capacity=100000, epsilon_start=0.5, epsilon_end=0.1, "
                "epsilon_decay=4000, target_update_interval=50, generator=None, log=None, output_dir=None, checkpoint_interval=0, rank=0, "
                "after_il=None")
    assert sig(cadrl_train.run_cadrl_training) == "(env, trainer, actions, gamma, %s)" % schedule
    assert sig(sarl_train.run_sarl_training) == "(env, trainer, actions, gamma, %s, om=None)" % schedule
    assert sig(lstm_train.run_lstm_training) == "(env, trainer, actions, gamma, %s, om=None)" % schedule
    init = "(self, module_or_state_dict, device='cpu', optimizer='sgd', lr=0.01, native=None%s)"
    assert sig(CadrlTrainer.__init__) == init % ""
    assert sig(SarlTrainer.__init__) == init % ", om_width=0, states_per_pass=None"
    assert sig(LstmTrainer.__init__) == init % ", states_per_pass=None"
    lag = "(self, rows, target, n_valid=None, mask=None, grad_scale=None, value=None, %s=None)"
    assert [sig(c.loss_and_grad) for c in (CadrlTrainer, SarlTrainer, LstmTrainer)] == [lag % "min_row", lag % "attention", lag % "joint"]
    grad = "(self, rows, target, grad, loss_sum, count, grad_scale, n_valid=None, mask=None, value=None, %s)"
    assert sig(CadrlNet.grad) == grad % "min_row=None"
    assert sig(SarlNet.grad) == grad % "attention=None, T=None, states_per_pass=0"
    assert sig(LstmNet.grad) == grad % "joint=None, T=None, states_per_pass=0"
