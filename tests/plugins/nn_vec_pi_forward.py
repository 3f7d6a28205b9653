"""Model plugin for vector observations whose policy has a `forward` of its own (the stock stacks, logits scaled).
Plugin API only."""
import torch

import algorithm.nn_models as m

ModelRep = m.ModelSimpleRep
ModelQ = m.ModelQ


class ModelPolicy(m.ModelPolicy):
    def forward(self, state, obs_list):
        d_policy = m.JointOneHotCategorical([
            torch.distributions.OneHotCategorical(logits=0.5 * head(state), validate_args=False)
            for head in self.d_dense_list])
        return d_policy, None
