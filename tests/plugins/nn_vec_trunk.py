"""Model plugin for vector observations whose critics and policy put one shared ResBlock (`dense_depth=1`) in front of
their heads: a trunk that is not the identity.  Plugin API only."""
import algorithm.nn_models as m

ModelRep = m.ModelSimpleRep


class ModelQ(m.ModelQ):
    def _build_model(self):
        super()._build_model(dense_depth=1)


class ModelPolicy(m.ModelPolicy):
    def _build_model(self):
        super()._build_model(dense_depth=1)
