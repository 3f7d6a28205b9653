"""Model plugin with `nn_rnn`'s 2-layer GRU(8) representation over [obs ‖ previous action] and `nn_vec_d32`'s 32-wide
discrete heads.  Plugin API only: it loads under the reference package too (tests/golden/make_discrete_golden.py)."""
import torch

import algorithm.nn_models as m


class ModelRep(m.ModelBaseRep):
    def _build_model(self):
        in_size = self.obs_shapes[0][0] + sum(self.d_action_sizes) + self.c_action_size
        self.rnn = m.GRU(in_size, 8, 2)

    def forward(self, obs_list, pre_action, pre_seq_hidden_state, padding_mask=None):
        h0 = None if pre_seq_hidden_state is None else pre_seq_hidden_state[:, 0]
        return self.rnn(torch.cat([obs_list[0], pre_action], dim=-1), h0)


class ModelQ(m.ModelQ):
    def _build_model(self):
        super()._build_model(d_dense_n=32)


class ModelPolicy(m.ModelPolicy):
    def _build_model(self):
        super()._build_model(d_dense_n=32)
