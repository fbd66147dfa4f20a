// ebc_sarl_net.h — the SARL network object behind ebc_sarl_net_* and ebc_sarl_grad, shared by the two units that create
// one: ebcsim_sarl_grad.hip (the chunk form, ebc_sarl_net_create / _create_om) and ebcsim_sarl_grad_layers.hip (the layer
// form, ebc_sarl_net_create_layers).  The packed image, the scratch and the entries' bodies are GradNet's for both.
#pragma once

#include "../../include/ebcsim.h"
#include "ebc_grad_host.h"
#include "ebc_sarl_grad_rule.h"

namespace ebc_host {

struct SarlNet : GradNet, GradPasses {
  ebc_sarl::GradDims D;
  // the layer form's ebc_sarl_grad on this network (args and their struct_size checked); null: the chunk form
  int (*layers_grad)(SarlNet *net, void *stream, const EbcSarlGradArgs *args) = nullptr;
};

}  // namespace ebc_host
