#!/usr/bin/env python3
"""The dynamic-LDS limit of the two forms of a gradient kernel (sarl_grad_kernel<true> / <false>, lstm_grad_kernel<true> /
<false>), on the GPU, in a process of its own: the limit is a function attribute the library raises once per kernel form
and device and remembers for the life of the process, so only a process that has launched neither form can show that each
form gets its own.  argv[1]: "sarl" or "lstm".  On ONE new network object at the reference widths, B = 1:
states_per_pass = 1 at R = grad_max_rows(1), then the default call at R = grad_max_rows(), then states_per_pass = 2 at
R = grad_max_rows(2), each against the host build of the rule header, byte for byte.  A call that does not return EBC_OK
ends the process with status 1 at once (a limit that one form wrongly shares with the other shows as a refused launch,
EBC_ERR_DEVICE); nothing is started after it.  Run by tests/test_grad_lds_limit_gpu.py; prints a JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "eb-cadrl_amd"), ROOT, HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"


def main(kind):
    if kind == "sarl":
        import sarl_grad_cases as cases
        from ebcsim.sarl_train import SarlNet as Net
        net = cases.REFERENCE_NET
    else:
        import lstm_grad_cases as cases
        from ebcsim.lstm_train import LstmNet as Net
        net = cases.REFERENCE_NET2
    sd = cases.random_state_dict(net)
    P, dn = cases.host_pack(sd), Net(sd, 0)
    calls = []
    for S in (1, 0, 2):
        R = dn.grad_max_rows(S)
        rows, target = cases.plain_batch(net, 1, R)
        extra_shape = (1, R) if kind == "sarl" else (1, dn.joint_dim)
        grad = torch.full((dn.packed_floats(),), -7.0, dtype=torch.float32, device=DEV)
        loss, count = torch.full((), -7.0, dtype=torch.float64, device=DEV), torch.full((), -7, dtype=torch.int64, device=DEV)
        value, extra = torch.full((1,), -7.0, dtype=torch.float32, device=DEV), torch.full(extra_shape, -7.0, dtype=torch.float32, device=DEV)
        call = {"states_per_pass": S, "R": R, "ok": False, "same": False}
        calls.append(call)
        try:  # _capi.check raises on every code but EBC_OK, with ebc_last_error()'s text
            dn.grad(torch.from_numpy(rows).to(DEV), torch.from_numpy(target).to(DEV), grad, loss, count, 2.0, None, None, value, extra,
                    states_per_pass=S)
            torch.cuda.synchronize()
        except Exception as e:
            call["error"] = "%s: %s" % (type(e).__name__, e)
            print(json.dumps({"kind": kind, "calls": calls}))
            return 1
        call["ok"] = True
        want = cases.host_grad(P, net, rows, target, None, None, 2.0)
        got = (grad.cpu().numpy(), float(loss), int(count), value.cpu().numpy(), extra.cpu().numpy())
        call["same"] = bool(cases.same_bytes(got[0], want[0]) and np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes()
                            and got[2] == want[2] and cases.same_bytes(got[3], want[3]) and cases.same_bytes(got[4], want[4]))
    print(json.dumps({"kind": kind, "calls": calls}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
