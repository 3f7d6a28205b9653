"""`nn_rnn.py`'s 2-layer GRU(8) representation over [obs ‖ previous action] with the stock RND model added (`use_rnd=True`
asks the plugin for `ModelRND`).  Written against the plugin API only, so the same file loads under the reference package
(golden minting) and under this repository's package."""
import torch

import algorithm.nn_models as m


class ModelRep(m.ModelBaseRep):
    def _build_model(self):
        in_size = self.obs_shapes[0][0] + sum(self.d_action_sizes) + self.c_action_size
        self.rnn = m.GRU(in_size, 8, 2)

    def forward(self, obs_list, pre_action, pre_seq_hidden_state, padding_mask=None):
        h0 = None if pre_seq_hidden_state is None else pre_seq_hidden_state[:, 0]
        return self.rnn(torch.cat([obs_list[0], pre_action], dim=-1), h0)


ModelQ = m.ModelQ
ModelPolicy = m.ModelPolicy
ModelRND = m.ModelRND
