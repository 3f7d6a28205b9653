"""Model plugin of one option: `nn_vec` plus the termination head (the option-side names of the reference's
`envs/test/nn_oc.py`)."""
import algorithm.nn_models as m

from .nn_vec import ModelPolicy, ModelQ, ModelRep  # noqa: F401

ModelTermination = m.ModelTermination
