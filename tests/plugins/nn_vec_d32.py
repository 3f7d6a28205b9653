"""Model plugin for vector observations with 32-wide discrete heads: `nn_vec`'s composition (concatenated-vector state,
stock Q / policy) with narrower per-branch heads, so that a recorded step of an ensemble of multi-branch critics stays a
small fixture.  Plugin API only: it loads under the reference package too (tests/golden/make_discrete_golden.py)."""
import algorithm.nn_models as m

ModelRep = m.ModelSimpleRep


class ModelQ(m.ModelQ):
    def _build_model(self):
        super()._build_model(d_dense_n=32)


class ModelPolicy(m.ModelPolicy):
    def _build_model(self):
        super()._build_model(d_dense_n=32)
