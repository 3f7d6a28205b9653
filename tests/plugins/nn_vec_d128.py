"""Model plugin for vector observations with the discrete head widths the reference's own plugins build (`envs/uav/*`,
`envs/gym/toy_*`): critics `d_dense_n=128, d_dense_depth=2`, policy `d_dense_n=128, d_dense_depth=1`.  Plugin API only."""
import algorithm.nn_models as m

ModelRep = m.ModelSimpleRep


class ModelQ(m.ModelQ):
    def _build_model(self):
        super()._build_model(d_dense_n=128, d_dense_depth=2)


class ModelPolicy(m.ModelPolicy):
    def _build_model(self):
        super()._build_model(d_dense_n=128, d_dense_depth=1)
