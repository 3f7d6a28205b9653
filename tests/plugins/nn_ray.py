"""Model plugin for ray(61, 2) + vector(6) observations: the `default` Conv1d stack over the rays -> 64 features,
concatenated with the vector (the composition of the reference's ray-sensor plugins, `envs/usv/usv_escort/nn.py`:
`m.Conv1dLayers(RAY_SIZE, 2, 'default', out_dense_n=64, out_dense_depth=2)` with RAY_SIZE = 61)."""
import torch

import algorithm.nn_models as m

RAY_SIZE = 61      # (tools/ray_bench.py sets 400, the ugv environments' rays, before it builds a learner)


class ModelRep(m.ModelBaseRep):
    def _build_model(self):
        self.ray_conv = m.Conv1dLayers(RAY_SIZE, 2, 'default', out_dense_n=64, out_dense_depth=2)

    def forward(self, obs_list, pre_action, pre_seq_hidden_state, padding_mask=None):
        ray, vec = obs_list
        state = torch.cat([self.ray_conv(ray), vec], dim=-1)
        return state, self._get_empty_seq_hidden_state(state)


ModelQ = m.ModelQ
ModelPolicy = m.ModelPolicy
ModelForwardDynamic = m.ModelForwardDynamic
ModelRND = m.ModelRND
ModelRepProjection = m.ModelRepProjection
ModelRepPrediction = m.ModelRepPrediction
