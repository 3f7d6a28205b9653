"""Model plugin of one option with narrow critics (32 wide, two layers per head): the hybrid and discrete option fixtures,
whose critics carry a discrete and a continuous head each, stay under the size limit of a committed fixture with it.
Written against the plugin API only, so it loads under the reference package too (tests/golden/make_option_golden.py)."""
import algorithm.nn_models as m

ModelRep = m.ModelSimpleRep


class ModelQ(m.ModelQ):
    def _build_model(self):
        super()._build_model(d_dense_n=32, d_dense_depth=2, c_dense_n=32, c_dense_depth=2)


ModelPolicy = m.ModelPolicy
ModelTermination = m.ModelTermination
