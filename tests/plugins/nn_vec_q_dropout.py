"""Model plugin for vector observations whose critics carry a live dropout (the reference's `envs/ugv/ugv_parking`
builds `ModelQ(dropout=0.2)`): the stacks are no head bank.  Plugin API only."""
import algorithm.nn_models as m

ModelRep = m.ModelSimpleRep
ModelPolicy = m.ModelPolicy


class ModelQ(m.ModelQ):
    def _build_model(self):
        super()._build_model(dropout=0.2)
